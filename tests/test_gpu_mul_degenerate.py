"""msm_hip_mul_each / msm_hip_mul_base where tests/test_gpu_mul.py is thin: the BASES and the SIZES.

  a, b  bases of small prime order (3 .. 10177, tests/small_order.py) on the three curves with a cofactor, through both entry points, the
        fixed-base table (most of whose records are then identities) and the MSM modes that are exact outside the subgroup of order r;
  c     n = 2^20 + 300 on BN254: every path of mul_impl that takes the tile offset, elementwise;
  d     the six other curves past one block of the normalisation (4096 outputs), identity bases and MONT256 scalars included;
  e     mul_base over each curve's own generator, whose coordinates are tiny.

Every comparison is bit for bit.  The expected values are the oracle's g1_scalar_mul + to_affine64 (or the big-integer model's repeated
addition for the small-order bases, with the oracle pinned to the same bytes), computed once per curve over a short POOL of (point, scalar)
pairs; the large cases tile the pool, so that no test multiplies more than a few hundred points on the CPU."""
import functools

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import bn254_ref, cpu
from tests import small_order
from tests.test_gpu_mul import (ERR_NONCANONICAL, OTHER_CURVES, PATH_ENDO, PATH_PLAIN, PATH_TABLE_BUILT, PATH_TABLE_HELD, PRIME_ORDER, b32, dev_u8,
                                expected, oracle_module, ref_module, scalar_vector, subgroup_points_bls12_381, to_mont256)

pytestmark = pytest.mark.gpu
ALL_CURVES = ["bn254"] + OTHER_CURVES
MSM_MODES = {"plain": dict(endomorphism=False), "tables": dict(precompute=True), "wide": dict(precompute="wide")}  # exact for any point of the curve
R = bn254_ref.R


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def rows(b, width):
    return np.frombuffer(b, dtype=np.uint8).reshape(-1, width)


def tiled(pool_bytes, width, n):
    """n rows: row i is row i mod K of the pool (host)"""
    a = rows(pool_bytes, width)
    return np.tile(a, (-(-n // a.shape[0]), 1))[:n]


def tiled_dev(pool_bytes, width, n):
    """the same on the device, by repeat: only the pool crosses the bus"""
    a = dev_u8(pool_bytes, width)
    return a.repeat(-(-n // a.shape[0]), 1)[:n].contiguous()


def bad_rows_dev(out, pool_want, zero_rows=()):
    """the first rows of the device tensor `out` that differ from row i mod K of `pool_want` (rows `zero_rows`: from the all-zero record),
    compared on the device a slab at a time.  Overwrites the zero_rows of `out`."""
    n, k = out.shape[0], pool_want.shape[0]
    bad = []
    if len(zero_rows):
        z = torch.as_tensor(np.asarray(zero_rows, dtype=np.int64), device=out.device)
        bad += z[(out[z] != 0).any(dim=1)].tolist()
        out[z] = pool_want[z % k]
    step = 1 << 17
    for a in range(0, n, step):
        b = min(a + step, n)
        idx = torch.arange(a, b, device=out.device) % k
        diff = (out[a:b] != pool_want[idx]).any(dim=1)
        if bool(diff.any()):
            bad += (diff.nonzero().flatten()[:4] + a).tolist()
    return bad[:8]


def device_memory_in_use():
    free, total = torch.cuda.mem_get_info()
    return total - free


def report_device_memory(what, before):
    """printed, not asserted (the figure is the whole device's, which others may share): what a 2^20 test holds when it ends -- the context's
    bases and scratch and torch's tensors -- is meant to stay near 300 MB"""
    print("%s: %d MiB of device memory taken since the test began" % (what, (device_memory_in_use() - before) >> 20))


def bad_rows_host(got, want_rows):
    g = rows(got, want_rows.shape[1])
    if g.shape == want_rows.shape and np.array_equal(g, want_rows):
        return []
    return np.flatnonzero((g != want_rows).any(axis=1))[:8].tolist() if g.shape == want_rows.shape else ["shape", g.shape]


# ================================================================================================ a, b: bases of small order
class SmallOrderSet:
    """The degenerate base set of one cofactor curve: every torsion point T found and -T, (0, 2) of order 3 on BLS12-381 G1, and 8 sampler
    points; the edge scalars around each order; and k B for every (scalar, base) pair -- by repeated addition in the big-integer model for
    the torsion bases, by the oracle for the sampler's, and the oracle pinned to the same bytes on all of them."""

    def __init__(self, curve):
        self.curve = curve
        self.ref, self.orc = ref, orc = ref_module(curve), oracle_module(curve)
        self.pb = pb = 2 * orc.coord_bytes()
        self.tors = []  # (index in the set, order f, [0 B, 1 B, ..., (f - 1) B])
        pts = []
        for f in small_order.ORDERS[curve]:
            t = small_order.torsion_point(curve, f)
            for pt in (t, ref.neg(t)):
                self.tors.append((len(pts), f, small_order.multiples(ref, f, pt)))
                pts.append(pt)
        if curve == "bls12_381":
            self.t3 = len(pts)
            self.tors.append((len(pts), 3, small_order.multiples(ref, 3, (0, 2))))
            pts.append((0, 2))
        self.raw = b"".join(small_order.enc(ref, pt) for pt in pts) + orc.sample_points(5100, 8)
        self.pts = pts + ref.bytes_to_points(orc.sample_points(5100, 8))
        self.nb = nb = len(self.pts)
        rnd = np.random.default_rng(5101)
        r_ = ref.R
        ks = []
        for f in small_order.ORDERS[curve]:
            ks += [0, 1, 2, 3, f - 1, f, f + 1, 2 * f, r_ - 1, r_ - 2, (r_ - 1) // 2, 0x8000, 0xFFFF, 0x7FFF8000]
        ks += [int.from_bytes(rnd.bytes(32), "little") % r_ for _ in range(6)]
        assert all(0 <= k < r_ for k in ks)
        self.ks = ks
        # mul_each pairs scalar i with base i: every scalar against every base, row j nb + b = ks[j] * base b
        self.each_points = self.raw * len(ks)
        self.each_scalars = b"".join(b32(k) * nb for k in ks)
        want = rows(expected(orc, self.each_points, self.each_scalars), pb).copy()
        for b, f, mult in self.tors:
            for j, k in enumerate(ks):
                model = small_order.enc(ref, mult[k % f])
                assert want[j * nb + b].tobytes() == model, (curve, f, hex(k), "the oracle against the big-integer model")
        self.each_want = want.tobytes()

    def base_want(self, b):
        """[k * base b for k in ks]"""
        return rows(self.each_want, self.pb)[b::self.nb].tobytes()

    def msm_want(self, scalars):
        """sum_b scalars[b] * base b: the oracle's MSM, cross-checked against the big-integer sum with (k mod f) T for the torsion bases"""
        ref, orc = self.ref, self.orc
        got = orc.to_affine64(orc.cpu_msm(self.raw, b"".join(b32(k) for k in scalars), n_threads=4))
        acc = None
        tors = {b: (f, mult) for b, f, mult in self.tors}
        for b, k in enumerate(scalars):
            acc = ref.add(acc, tors[b][1][k % tors[b][0]] if b in tors else small_order.imul(ref, k, self.pts[b]))
        assert got == small_order.enc(ref, acc), (self.curve, "the oracle's MSM against the big-integer sum")
        return got


@functools.lru_cache(maxsize=None)
def small_order_set(curve):
    return SmallOrderSet(curve)


@pytest.mark.parametrize("curve", small_order.COFACTOR_CURVES)
def test_small_order_bases_through_mul_each(gpu, curve):
    s = small_order_set(curve)
    ref, pb, nb, ks = s.ref, s.pb, s.nb, s.ks
    n = nb * len(ks)
    want = rows(s.each_want, pb)
    # what the expected values themselves must show: k = 0 mod f gives the all-zero record, and on BLS12-381 G1 +-(0, 2) has x = 0 and is not one
    for b, f, _ in s.tors:
        for j, k in enumerate(ks):
            assert (not want[j * nb + b].any()) == (k % f == 0)
    if curve == "bls12_381":
        two, minus_two = (2).to_bytes(48, "little"), (ref.P - 2).to_bytes(48, "little")
        for j, k in enumerate(ks):
            rec = want[j * nb + s.t3].tobytes()
            assert rec == {0: bytes(96), 1: bytes(48) + two, 2: bytes(48) + minus_two}[k % 3]
    a, b2 = m.MsmContext(0, curve=curve), m.MsmContext(0, curve=curve)
    try:
        a.set_bases(s.each_points, check_on_curve=True)
        got = a.mul_each(s.each_scalars)
        assert a.mul_last()[0] == PATH_PLAIN  # (no bases_order_r on these bases: the caller would be lying)
        assert not bad_rows_host(got, want), (curve, "host", bad_rows_host(got, want))
        q = a.mul_each(dev_u8(s.each_scalars, 32))
        assert not bad_rows_host(q.cpu().numpy().tobytes(), want), (curve, "device")
        a.set_scalar_format(mont256=True)
        sm = to_mont256(s.each_scalars, ref.R)
        assert a.mul_each(sm) == s.each_want, (curve, "mont256 host")
        assert a.mul_each(dev_u8(sm, 32)).cpu().numpy().tobytes() == s.each_want, (curve, "mont256 device")
        a.set_scalar_format()
        # the device output, identity records and all, as the bases of an MSM: sum_i c_i Q_i, by the oracle over the rows that are not the
        # identity, and as the big-integer sum_b (sum_j c_(j, b) k_j) B_b with integer coefficients (exact outside the subgroup too)
        rnd = np.random.default_rng(5102)
        cc = [int.from_bytes(rnd.bytes(32), "little") % ref.R for _ in range(n)]
        keep = want.any(axis=1)
        orc = s.orc
        w = orc.to_affine64(orc.cpu_msm(want[keep].tobytes(), b"".join(b32(v) for v, kp in zip(cc, keep) if kp), n_threads=4))
        acc = None
        tors = {b: (f, mult) for b, f, mult in s.tors}
        for b in range(nb):
            coeff = sum(cc[j * nb + b] * ks[j] for j in range(len(ks)))
            acc = ref.add(acc, tors[b][1][coeff % tors[b][0]] if b in tors else small_order.imul(ref, coeff, s.pts[b]))
        assert w == small_order.enc(ref, acc)
        b2.set_bases(q, zero_is_identity=True)
        assert b2.msm(b"".join(b32(v) for v in cc)).to_affine_bytes() == w
    finally:
        a.close()
        b2.close()


@pytest.mark.parametrize("curve", small_order.COFACTOR_CURVES)
def test_small_order_bases_through_mul_base(gpu, curve):
    # one torsion base for every scalar: the broadcast ladder, and the fixed-base table at C = 8 and 12, whose entries j 2^(C w) T are
    # identity records whenever f divides j (for f = 3: a third of the table)
    s = small_order_set(curve)
    sc = b"".join(b32(k) for k in s.ks)
    sm = to_mont256(sc, s.ref.R)
    c = m.MsmContext(0, curve=curve)
    try:
        c.set_bases(s.raw, check_on_curve=True)
        for b, f, _ in s.tors:
            w = s.base_want(b)
            c.mul_policy("never")
            assert c.mul_base(b, sc) == w, (curve, f, b, "ladder, host")
            assert c.mul_last()[:2] == (PATH_PLAIN, 0)
            assert c.mul_base(b, dev_u8(sc, 32)).cpu().numpy().tobytes() == w, (curve, f, b, "ladder, device")
            c.set_scalar_format(mont256=True)
            assert c.mul_base(b, dev_u8(sm, 32)).cpu().numpy().tobytes() == w, (curve, f, b, "ladder, mont256")
            c.set_scalar_format()
            # (an entry j 2^(C w) T is the identity when f divides j <= 2^(C-1): at C = 15 the orders above 2^11 get theirs too, and the
            # scalar k = f is the digit that gathers it)
            for bits in (8, 12) + ((15,) if f > 1 << 11 else ()):
                c.mul_policy(1, bits)
                assert c.mul_base(b, sc) == w, (curve, f, b, bits, "table, host")
                assert c.mul_last()[:2] == (PATH_TABLE_BUILT, bits)
                assert c.mul_base(b, dev_u8(sc, 32)).cpu().numpy().tobytes() == w, (curve, f, b, bits, "table, device")
                assert c.mul_last()[:2] == (PATH_TABLE_HELD, bits)
                c.set_scalar_format(mont256=True)
                assert c.mul_base(b, sm) == w, (curve, f, b, bits, "table, mont256")
                assert c.mul_last()[:2] == (PATH_TABLE_HELD, bits)
                c.set_scalar_format()
        c.mul_policy(0, 0)
        # a regular base of the same set, after all those tables
        b = s.nb - 1
        assert c.mul_base(b, sc) == s.base_want(b) and c.mul_last()[:2] == (PATH_PLAIN, 0)
    finally:
        c.close()


@pytest.mark.parametrize("curve", small_order.COFACTOR_CURVES)
def test_small_order_bases_through_the_msm(gpu, curve):
    # n = the set's size.  All scalars equal: one bucket per window receives T, -T (their sum is the identity, in whatever order they meet)
    # and, on BLS12-381 G1, (0, 2) twice; all scalars equal to f: every torsion base contributes the identity
    s = small_order_set(curve)
    r_ = s.ref.R
    rnd = np.random.default_rng(5103)
    vectors = {"uniform": [int.from_bytes(rnd.bytes(32), "little") % r_ for _ in range(s.nb)],
               "equal": [int.from_bytes(rnd.bytes(32), "little") % r_] * s.nb}
    for f in small_order.ORDERS[curve]:
        vectors["all %d" % f] = [f] * s.nb
    wants = {name: s.msm_want(v) for name, v in vectors.items()}
    c = m.MsmContext(0, curve=curve)
    try:
        for mode, flags in MSM_MODES.items():
            c.set_bases(s.raw, check_on_curve=True, **flags)
            for name, v in vectors.items():
                sc = b"".join(b32(k) for k in v)
                assert c.msm(sc).to_affine_bytes() == wants[name], (curve, mode, name, "host")
                assert c.msm(dev_u8(sc, 32)).to_affine_bytes() == wants[name], (curve, mode, name, "device")
    finally:
        c.close()


# ================================================================================================ c: past one tile, BN254
# mul_impl walks n in tiles of 2^20 outputs and applies the tile's offset to the scalars, the outputs, the base index, the identity bitmap
# and the host staging area.  A pool of K = 509 (point, scalar) pairs is tiled to n = 2^20 + 300, so the expected output is the pool's 509
# oracle products tiled.  509 is prime and 2^20 mod 509 = 36: an offset that is wrong by 2^20, by 256, by 16, or by any multiple of these
# that is not also a multiple of 509, pairs a scalar with another base or lands on another row and shows.  LIMITATION: an offset wrong by a
# multiple of 509 rows is invisible to the periodic part; the identities and the scalar >= r below sit at absolute positions for that.
K_TILE = 509
N_TILE = (1 << 20) + 300
SEAM = [(1 << 20) - 2, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 2, N_TILE - 1]


@pytest.fixture(scope="module")
def tile_pool(gpu):
    points = cpu.sample_points(5200, K_TILE)
    scalars = scalar_vector(cpu, bn254_ref, K_TILE, 5201)  # (the edge scalars of tests/test_gpu_mul.py planted from pair 0 on)
    base36 = points[64 * 36:64 * 37]
    return {"points": points, "scalars": scalars, "mont": to_mont256(scalars, R), "want": expected(cpu, points, scalars),
            "want36": expected(cpu, base36 * K_TILE, scalars)}


def test_second_tile_device_forms(gpu, tile_pool):
    n = N_TILE
    before = device_memory_in_use()
    c = m.MsmContext(0)
    try:
        pts = tiled_dev(tile_pool["points"], 64, n)
        c.set_bases(pts)
        del pts
        torch.cuda.empty_cache()
        want = dev_u8(tile_pool["want"], 64)
        s = tiled_dev(tile_pool["scalars"], 32, n)
        # first: one scalar equal to r, in the second tile only -- the error word is read once, after the last tile
        good = s[(1 << 20) + 5].clone()
        s[(1 << 20) + 5] = torch.from_numpy(np.frombuffer(b32(R), dtype=np.uint8).copy()).cuda()
        with pytest.raises(m.MsmHipError) as e:
            c.mul_each(s)
        assert e.value.code == ERR_NONCANONICAL
        s[(1 << 20) + 5] = good
        out = c.mul_each(s)  # (the next call on the same context is correct)
        assert c.mul_last() == (PATH_ENDO, 0, 16)
        assert not bad_rows_dev(out, want), ("device", bad_rows_dev(out, want))
        out.fill_(0xA5)
        assert c.mul_each(s, out=out) is out
        assert not bad_rows_dev(out, want), ("out=", bad_rows_dev(out, want))
        del s
        torch.cuda.empty_cache()
        sm = tiled_dev(tile_pool["mont"], 32, n)  # MONT256: every tile's canonical copies go through the same scratch
        out.fill_(0x5A)
        c.set_scalar_format(mont256=True)
        c.mul_each(sm, out=out)
        c.set_scalar_format()
        assert not bad_rows_dev(out, want), ("mont256", bad_rows_dev(out, want))
        report_device_memory("test_second_tile_device_forms", before)
    finally:
        c.close()


def test_second_tile_host_forms(gpu, tile_pool):
    # the host forms stage scalars and outputs tile by tile
    n = N_TILE
    want = tiled(tile_pool["want"], 64, n)
    before = device_memory_in_use()
    c = m.MsmContext(0)
    try:
        pts = tiled_dev(tile_pool["points"], 64, n)
        c.set_bases(pts)
        del pts
        torch.cuda.empty_cache()
        s = tiled(tile_pool["scalars"], 32, n).copy()
        s[(1 << 20) + 5] = rows(b32(R), 32)[0]
        with pytest.raises(m.MsmHipError) as e:
            c.mul_each(s.tobytes())
        assert e.value.code == ERR_NONCANONICAL
        s[(1 << 20) + 5] = s[((1 << 20) + 5) % K_TILE]
        got = c.mul_each(s.tobytes())
        assert not bad_rows_host(got, want), ("host", bad_rows_host(got, want))
        c.set_scalar_format(mont256=True)
        got = c.mul_each(tiled(tile_pool["mont"], 32, n).tobytes())
        c.set_scalar_format()
        assert not bad_rows_host(got, want), ("mont256 host", bad_rows_host(got, want))
        report_device_memory("test_second_tile_host_forms", before)
    finally:
        c.close()


def test_second_tile_identity_bases(gpu, tile_pool):
    # identity records on both sides of the seam between the tiles and at the very end; beside them 2^256 - 1 (canonical form: not below r,
    # and not to be looked at) or, in MONT256 form, words that are no residue at all.  Those rows come out zero, every other row as before
    n = N_TILE
    before = device_memory_in_use()
    c = m.MsmContext(0)
    try:
        seam = torch.as_tensor(SEAM, device="cuda")
        pts = tiled_dev(tile_pool["points"], 64, n)
        pts[seam] = 0
        c.set_bases(pts, zero_is_identity=True)
        del pts
        torch.cuda.empty_cache()
        want = dev_u8(tile_pool["want"], 64)
        s = tiled_dev(tile_pool["scalars"], 32, n)
        s[seam] = 0xFF
        out = c.mul_each(s)  # (raises on ERR_NONCANONICAL)
        assert not bad_rows_dev(out, want, SEAM), ("device", bad_rows_dev(out, want, SEAM))
        host_scalars = s.cpu().numpy().tobytes()
        del s
        torch.cuda.empty_cache()
        sm = tiled_dev(tile_pool["mont"], 32, n)
        sm[seam] = 0xFF
        out.fill_(0x5A)
        c.set_scalar_format(mont256=True)
        c.mul_each(sm, out=out)
        c.set_scalar_format()
        assert not bad_rows_dev(out, want, SEAM), ("mont256", bad_rows_dev(out, want, SEAM))
        del sm, out
        torch.cuda.empty_cache()
        want_host = tiled(tile_pool["want"], 64, n).copy()
        want_host[SEAM] = 0
        got = c.mul_each(host_scalars)
        assert not bad_rows_host(got, want_host), ("host", bad_rows_host(got, want_host))
        report_device_memory("test_second_tile_identity_bases", before)
    finally:
        c.close()


def test_second_tile_mul_base(gpu, tile_pool):
    # one base (index 36 of the pool) for n scalars: the broadcast ladders, which must NOT add the tile's offset to the base index, and
    # k_mul_fixed on a second tile
    n = N_TILE
    want = dev_u8(tile_pool["want36"], 64)
    want_host = tiled(tile_pool["want36"], 64, n)
    before = device_memory_in_use()
    c = m.MsmContext(0)
    try:
        c.set_bases(tile_pool["points"])
        s = tiled_dev(tile_pool["scalars"], 32, n)
        host_scalars = tiled(tile_pool["scalars"], 32, n).tobytes()
        c.mul_policy("never")
        out = c.mul_base(36, s)
        assert c.mul_last()[:2] == (PATH_ENDO, 0)
        assert not bad_rows_dev(out, want), ("ladder, device", bad_rows_dev(out, want))
        got = c.mul_base(36, host_scalars)
        assert c.mul_last()[:2] == (PATH_ENDO, 0)
        assert not bad_rows_host(got, want_host), ("ladder, host", bad_rows_host(got, want_host))
        c.mul_force_ladder(1)
        out.fill_(0xA5)
        c.mul_base(36, s, out=out)
        assert c.mul_last()[:2] == (PATH_PLAIN, 0)
        assert not bad_rows_dev(out, want), ("plain ladder, device", bad_rows_dev(out, want))
        c.mul_force_ladder(0)
        c.mul_policy(0, 0)  # the policy's own choice at this n: a table of 12-bit digits
        got = c.mul_base(36, host_scalars)
        assert c.mul_last()[:2] == (PATH_TABLE_BUILT, 12)
        assert not bad_rows_host(got, want_host), ("table built, host", bad_rows_host(got, want_host))
        got = c.mul_base(36, host_scalars)
        assert c.mul_last()[:2] == (PATH_TABLE_HELD, 12)
        assert not bad_rows_host(got, want_host), ("table held, host", bad_rows_host(got, want_host))
        out.fill_(0x5A)
        c.mul_base(36, s, out=out)
        assert c.mul_last()[:2] == (PATH_TABLE_HELD, 12)
        assert not bad_rows_dev(out, want), ("table held, device", bad_rows_dev(out, want))
        report_device_memory("test_second_tile_mul_base", before)
    finally:
        c.close()


# ================================================================================================ d: the other curves past one normalisation block
K_BLOCK = 257  # prime: the pool's period shares no factor with the 256 lanes or the 4096 outputs of a normalisation block


@functools.lru_cache(maxsize=None)
def block_pool(curve):
    orc, ref = oracle_module(curve), ref_module(curve)
    seed = 5300 + 10 * OTHER_CURVES.index(curve)
    # of order r, so that bases_order_r=True is the truth: multiples of the generator on BLS12-381 G1; the G2 samplers draw from the subgroup
    points = subgroup_points_bls12_381(seed, K_BLOCK) if curve == "bls12_381" else orc.sample_points(seed, K_BLOCK)
    scalars = scalar_vector(orc, ref, K_BLOCK, seed + 1)
    pb = 2 * orc.coord_bytes()
    return {"points": points, "scalars": scalars, "want": expected(orc, points, scalars), "want5": expected(orc, points[5 * pb:6 * pb] * K_BLOCK, scalars)}


@pytest.mark.parametrize("curve", OTHER_CURVES)
def test_other_curves_past_one_normalisation_block(gpu, curve):
    pool = block_pool(curve)
    ref = ref_module(curve)
    c = m.MsmContext(0, curve=curve)
    try:
        pb = c.pb
        for n in (4099, 8197):
            points, scalars, want = tiled(pool["points"], pb, n), tiled(pool["scalars"], 32, n), tiled(pool["want"], pb, n)
            sc = scalars.tobytes()
            c.set_bases(points.tobytes(), endomorphism=None if curve in PRIME_ORDER else False)
            for order_r in (False, True):
                path = PATH_ENDO if (curve in PRIME_ORDER or order_r) else PATH_PLAIN
                got = c.mul_each(sc, bases_order_r=order_r)
                assert c.mul_last()[0] == path
                assert not bad_rows_host(got, want), (curve, n, order_r, "host", bad_rows_host(got, want))
                got = c.mul_each(dev_u8(sc, 32), bases_order_r=order_r).cpu().numpy().tobytes()
                assert c.mul_last()[0] == path
                assert not bad_rows_host(got, want), (curve, n, order_r, "device", bad_rows_host(got, want))
            c.set_scalar_format(mont256=True)
            got = c.mul_each(dev_u8(to_mont256(sc, ref.R), 32)).cpu().numpy().tobytes()
            c.set_scalar_format()
            assert not bad_rows_host(got, want), (curve, n, "mont256", bad_rows_host(got, want))
            # identity records at the ends, across a workgroup of the ladder and across a block of the normalisation; 2^256 - 1 (canonical
            # form) and non-residues (MONT256 form) beside every other one of them
            ids = np.array([0, 255, 256, 257, 4095, 4096, 4097, n - 1])
            pi, si, wi = points.copy(), scalars.copy(), want.copy()
            pi[ids] = 0
            si[ids[::2]] = 0xFF
            wi[ids] = 0
            c.set_bases(pi.tobytes(), zero_is_identity=True, endomorphism=None if curve in PRIME_ORDER else False)
            for order_r in (False, True):
                got = c.mul_each(si.tobytes(), bases_order_r=order_r)
                assert not bad_rows_host(got, wi), (curve, n, order_r, "identities, host", bad_rows_host(got, wi))
                got = c.mul_each(dev_u8(si.tobytes(), 32), bases_order_r=order_r).cpu().numpy().tobytes()
                assert not bad_rows_host(got, wi), (curve, n, order_r, "identities, device", bad_rows_host(got, wi))
            sm = rows(to_mont256(sc, ref.R), 32).copy()
            sm[ids[::2]] = 0xFF
            c.set_scalar_format(mont256=True)
            got = c.mul_each(dev_u8(sm.tobytes(), 32)).cpu().numpy().tobytes()
            c.set_scalar_format()
            assert not bad_rows_host(got, wi), (curve, n, "identities, mont256", bad_rows_host(got, wi))
        # one base for 4099 scalars: the broadcast ladder, then the table at C = 8
        n = 4099
        sc, want5 = tiled(pool["scalars"], 32, n).tobytes(), tiled(pool["want5"], pb, n)
        c.set_bases(pool["points"], endomorphism=None if curve in PRIME_ORDER else False)
        for order_r in (False, True):
            path = PATH_ENDO if (curve in PRIME_ORDER or order_r) else PATH_PLAIN
            c.mul_policy("never")
            got = c.mul_base(5, sc, bases_order_r=order_r)
            assert c.mul_last()[:2] == (path, 0)
            assert not bad_rows_host(got, want5), (curve, order_r, "mul_base, ladder", bad_rows_host(got, want5))
            c.mul_policy(1, 8)
            got = c.mul_base(5, dev_u8(sc, 32), bases_order_r=order_r).cpu().numpy().tobytes()
            # (a table is kept per ladder: on a curve of prime order the flag changes nothing, and the second round finds the first one's)
            assert c.mul_last()[:2] == (PATH_TABLE_HELD if order_r and curve in PRIME_ORDER else PATH_TABLE_BUILT, 8)
            assert not bad_rows_host(got, want5), (curve, order_r, "mul_base, table", bad_rows_host(got, want5))
            got = c.mul_base(5, sc, bases_order_r=order_r)
            assert c.mul_last()[:2] == (PATH_TABLE_HELD, 8)
            assert not bad_rows_host(got, want5), (curve, order_r, "mul_base, table held", bad_rows_host(got, want5))
        c.mul_policy(0, 0)
    finally:
        c.close()


# ================================================================================================ e: the standard generators
@pytest.mark.parametrize("curve", ALL_CURVES)
def test_mul_base_over_the_generator(gpu, curve):
    # s_i * G for the curve's own generator: coordinates as small as (1, 2) on BN254 G1, almost every limb of the base zero
    orc, ref = oracle_module(curve), ref_module(curve)
    n = 600
    g = ref.points_to_bytes([ref.G])
    assert orc.points_on_curve(g)
    scalars = scalar_vector(orc, ref, n, 5400 + ALL_CURVES.index(curve))
    want = rows(expected(orc, g * n, scalars), len(g))
    assert want[1].tobytes() == g  # (scalar 1 of the planted edges is 1)
    c = m.MsmContext(0, curve=curve)
    try:
        c.set_bases(g, check_on_curve=True, endomorphism=None if curve in PRIME_ORDER else False)
        for order_r in (False, True):
            path = PATH_ENDO if (curve in PRIME_ORDER or order_r) else PATH_PLAIN
            c.mul_policy("never")
            got = c.mul_base(0, scalars, bases_order_r=order_r)
            assert c.mul_last()[:2] == (path, 0)
            assert not bad_rows_host(got, want), (curve, order_r, "ladder, host", bad_rows_host(got, want))
            got = c.mul_base(0, dev_u8(scalars, 32), bases_order_r=order_r).cpu().numpy().tobytes()
            assert not bad_rows_host(got, want), (curve, order_r, "ladder, device", bad_rows_host(got, want))
            for bits in (8, 12):
                c.mul_policy(1, bits)
                got = c.mul_base(0, scalars, bases_order_r=order_r)
                assert c.mul_last()[:2] == (PATH_TABLE_BUILT, bits)
                assert not bad_rows_host(got, want), (curve, order_r, bits, "table, host", bad_rows_host(got, want))
                got = c.mul_base(0, dev_u8(scalars, 32), bases_order_r=order_r).cpu().numpy().tobytes()
                assert c.mul_last()[:2] == (PATH_TABLE_HELD, bits)
                assert not bad_rows_host(got, want), (curve, order_r, bits, "table, device", bad_rows_host(got, want))
        c.mul_policy(0, 0)
    finally:
        c.close()
