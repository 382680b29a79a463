"""CPU build (g++ -DFQ_CHECK) of csrc/scalar_mul.h -- the endomorphism ladder, the plain ladder and the shared-inversion normalisation that
k_mul_each / k_mul_normalize inline -- for all seven curves, every limb bound and every Montgomery result asserted, against the oracle's
g1_scalar_mul + to_affine64.  Host logic only."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

from tests import small_order
from tests.edge_scalars import edge_values
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msm-webgpu_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_harness", "scalar_mul_harness.cpp")

# curve -> (g++ defines, oracle binding, big-integer model)
CURVES = {
    "bn254": ([], "oracle.cpu", "oracle.bn254_ref"),
    "grumpkin": (["-DMSM_FIELD_NS=grumpkin", "-DMSM_KERNEL_NS=msmk_grumpkin", '-DMSM_CURVE_CONSTANTS="grumpkin_constants.h"', "-DHARNESS_FIELD_NS=grumpkin"],
                 "oracle.cpu_grumpkin", "oracle.grumpkin_ref"),
    "pallas": (["-DMSM_FIELD_NS=pallas", "-DMSM_KERNEL_NS=msmk_pallas", '-DMSM_CURVE_CONSTANTS="pallas_constants.h"', "-DHARNESS_FIELD_NS=pallas"],
               "oracle.cpu_pallas", "oracle.pallas_ref"),
    "vesta": (["-DMSM_FIELD_NS=vesta", "-DMSM_KERNEL_NS=msmk_vesta", '-DMSM_CURVE_CONSTANTS="vesta_constants.h"', "-DHARNESS_FIELD_NS=vesta"],
              "oracle.cpu_vesta", "oracle.vesta_ref"),
    "bls12_381": (["-DMSM_FIELD_NS=bls12_381", "-DMSM_KERNEL_NS=msmk_bls12_381", '-DMSM_CURVE_CONSTANTS="bls12_381_constants.h"', "-DHARNESS_FIELD_NS=bls12_381"],
                  "oracle.cpu_bls12_381", "oracle.bls12_381_ref"),
    "bn254_g2": (["-DHARNESS_G2"], "oracle.cpu_bn254_g2", "oracle.bn254_g2_ref"),
    "bls12_381_g2": (["-DHARNESS_G2", "-DHARNESS_G2_BLS12_381"], "oracle.cpu_bls12_381_g2", "oracle.bls12_381_g2_ref"),
}
_built = {}


def harness(tmp_path_factory, curve):
    if curve not in _built:
        so = str(tmp_path_factory.mktemp("smul_" + curve) / "scalar_mul_harness.so")
        san = ["-fsanitize=undefined", "-fno-sanitize-recover=all"] if os.environ.get("MSM_TEST_SANITIZE") == "1" else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-fPIC", "-shared"] + san + CURVES[curve][0] + ["-I", CSRC, SRC, "-o", so])
        H = C.CDLL(so)
        H.h_smul.restype = C.c_size_t
        H.h_smul.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p]
        H.h_smul_fixed.restype = C.c_size_t
        H.h_smul_fixed.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p]
        H.h_smul_normalize.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p]
        _built[curve] = H
    return _built[curve], importlib.import_module(CURVES[curve][1]), importlib.import_module(CURVES[curve][2])


def b32(v):
    return int(v).to_bytes(32, "little")


def scalar_set(m, seed, uniform):
    """the scalars the ladders must get right: small ones, the ends of [0, r), lambda and its neighbours, the 127 / 128-bit boundary of the
    split's halves, splits with a zero half or equal / opposite halves, the recode edges of tests/edge_scalars.py, and seeded uniform ones"""
    r_, lam = m.R, m.glv_params()["lam"]
    rnd = rng(seed)
    ks = [0, 1, 2, r_ - 1, r_ - 2, (r_ + 1) // 2, (r_ - 1) // 2, lam, lam + 1, lam - 1, r_ - lam, (1 << 127) + 1, (1 << 127) - 1, 1 << 128]
    for t in (1, 2, 3, 0xFFFF, rnd.randrange(1 << 100), rnd.randrange(1 << 126)):
        ks += [t, t * lam % r_, t * (1 + lam) % r_, t * (1 - lam) % r_, (r_ - t) % r_, (r_ - t) * lam % r_]  # k2 = 0, k1 = 0, k1 = k2, k1 = -k2, and negated
    ks += [v for _, v, _ in edge_values(r_.bit_length(), 16, r_)]
    ks += [rnd.randrange(r_) for _ in range(uniform)]
    return [k % r_ for k in ks]


def expected(cx, points, scalars):
    jb = 3 * cx.coord_bytes()
    jac = cx.g1_scalar_mul(points, scalars)
    return b"".join(cx.to_affine64(jac[i:i + jb]) for i in range(0, len(jac), jb))


def order_r_points(cx, m, seed, n):
    """n points of order r: the sampler's on the curves where it draws from the subgroup, else multiples of the generator"""
    pb = 2 * cx.coord_bytes()
    if m.__name__ in COFACTOR_SAMPLERS:
        g = m.points_to_bytes([m.G])
        ks = b"".join(b32(rng(seed + i).randrange(1, m.R)) for i in range(n))
        return expected(cx, g * n, ks)
    return cx.sample_points(seed, n)[:pb * n]


COFACTOR_SAMPLERS = ("oracle.bls12_381_ref",)  # BLS12-381 G1: the sampler's points lie on the curve, not necessarily in the subgroup


@pytest.mark.parametrize("curve", list(CURVES))
def test_ladders_against_the_oracle(tmp_path_factory, curve):
    H, cx, m = harness(tmp_path_factory, curve)
    pb = 2 * cx.coord_bytes()
    ks = scalar_set(m, 50, 200 if cx.coord_bytes() <= 48 else 60)
    n = len(ks)
    npts = 24
    pool = order_r_points(cx, m, 61, npts)
    pts = b"".join(pool[pb * (i % npts):pb * (i % npts) + pb] for i in range(n))
    sc = b"".join(b32(k) for k in ks)
    want = expected(cx, pts, sc)
    assert want[:pb] == bytes(pb)  # (k = 0: the identity is the all-zero record)
    for mode in (0, 1):
        out = C.create_string_buffer(pb * n)
        assert H.h_smul(mode, pts, sc, n, 3, out) == 0
        bad = [hex(ks[i]) for i in range(n) if out.raw[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
        assert not bad, (curve, mode, bad[:4])


def test_plain_ladder_gives_the_integer_multiple_outside_the_subgroup(tmp_path_factory):
    # BLS12-381 G1: the sampler's points are on the curve but carry cofactor components; k P is then the integer multiple (k < r here)
    H, cx, m = harness(tmp_path_factory, "bls12_381")
    pts_list = m.bytes_to_points(cx.sample_points(62, 6))
    assert any(m.add(m.mul(m.R - 1, pt), pt) is not None for pt in pts_list)  # r P != 0: at least one is outside the subgroup of order r
    ks = [1, 2, m.R - 1, (1 << 200) + 12345, rng(7).randrange(m.R), rng(8).randrange(m.R)]
    pts = m.points_to_bytes(pts_list)
    out = C.create_string_buffer(96 * 6)
    assert H.h_smul(0, pts, b"".join(b32(k) for k in ks), 6, 1, out) == 0
    assert out.raw == b"".join(m.affine_to_bytes64(m.mul(k, pt)) for k, pt in zip(ks, pts_list))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_scalars_not_below_r_are_counted_not_multiplied(tmp_path_factory, curve):
    H, cx, m = harness(tmp_path_factory, curve)
    pb = 2 * cx.coord_bytes()
    pts = order_r_points(cx, m, 63, 4)
    ks = [m.R, 5, (1 << 256) - 1, m.R + 1]
    out = C.create_string_buffer(pb * 4)
    for mode in (0, 1):
        assert H.h_smul(mode, pts, b"".join(b32(k) for k in ks), 4, 1, out) == 3
        assert out.raw[pb:2 * pb] == expected(cx, pts[pb:2 * pb], b32(5))


@pytest.mark.parametrize("curve", list(CURVES))
def test_shared_inversion_at_every_chunk_boundary(tmp_path_factory, curve):
    # Jacobian records with random Z through the normalisation alone: batch lengths around the chunk size, identities first, last, at every
    # position of one chunk, a chunk of identities only; lane strides 1 (a chunk is consecutive) and 3 (interleaved, a ragged last group)
    H, cx, m = harness(tmp_path_factory, curve)
    cb = cx.coord_bytes()
    chunk = H.h_smul_chunk()
    rnd = rng(70)
    g2 = hasattr(m, "f2_mul")
    npts = 2 * chunk + 3
    pts = m.bytes_to_points(cx.sample_points(64, npts))

    def jac(pt):
        if pt is None:
            return bytes(3 * cb)
        if g2:
            z = (rnd.randrange(1, m.P), rnd.randrange(m.P))
            z2 = m.f2_sqr(z)
            return m.f2_to_bytes(m.f2_mul(pt[0], z2)) + m.f2_to_bytes(m.f2_mul(pt[1], m.f2_mul(z2, z))) + m.f2_to_bytes(z)
        z = rnd.randrange(1, m.P)
        return b"".join(int(v).to_bytes(cb, "little") for v in (pt[0] * z * z % m.P, pt[1] * z * z * z % m.P, z))

    def run(seq, lanes):
        raw = b"".join(jac(pt) for pt in seq)
        out = C.create_string_buffer(2 * cb * len(seq))
        H.h_smul_normalize(raw, len(seq), lanes, out)
        want = b"".join(bytes(2 * cb) if pt is None else m.points_to_bytes([pt]) for pt in seq)
        assert out.raw == want, (curve, len(seq), lanes, [pt is None for pt in seq])

    for lanes in (1, 3):
        for n in (1, chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
            seq = [pts[i] for i in range(n)]
            run(seq, lanes)
            run([None] + seq[1:], lanes)           # identity first
            run(seq[:-1] + [None], lanes)          # ... last
            run([None] * n, lanes)                 # nothing to invert at all
        for pos in range(chunk):                   # every position of the second chunk
            seq = [pts[i] for i in range(2 * chunk + 3)]
            seq[chunk + pos] = None
            run(seq, lanes)
        seq = [pts[i] for i in range(2 * chunk + 3)]
        for pos in range(chunk):                   # one chunk of identities between two regular ones
            seq[chunk + pos] = None
        run(seq, 1)
        seq = [pts[i] for i in range(2 * chunk + 3)]
        for j in range(chunk):                     # ... the same for the interleaved layout: lane 1 of the first group
            if 1 + 3 * j < len(seq):
                seq[1 + 3 * j] = None
        run(seq, 3)


@pytest.mark.parametrize("curve", list(CURVES))
def test_fixed_base_digit_recode_and_table_lookup(tmp_path_factory, curve):
    # mul_base's table path: T_w[j] = j 2^(C w) P built by either ladder, the signed C-bit recode of every edge scalar, W gathered additions.
    # Small digit widths keep the host build short (the widths the device uses, 8 .. 16, differ only in the table's size); an odd width and
    # one that divides neither 254 nor 255 put the top window's partial chunk and the last carry in different places.
    H, cx, m = harness(tmp_path_factory, curve)
    pb = 2 * cx.coord_bytes()
    big = cx.coord_bytes() > 48
    ks = scalar_set(m, 80, 20 if big else 100)
    n = len(ks)
    p = order_r_points(cx, m, 81, 1)
    sc = b"".join(b32(k) for k in ks)
    want = expected(cx, p * n, sc)
    for mode, c in ((1, 4), (0, 5)) if big else ((1, 7), (0, 5), (1, 4)) + (((1, 8),) if curve == "bn254" else ()):
        out = C.create_string_buffer(pb * n)
        assert H.h_smul_fixed(mode, c, p, sc, n, out) == 0
        bad = [hex(ks[i]) for i in range(n) if out.raw[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
        assert not bad, (curve, mode, c, bad[:4])
    out = C.create_string_buffer(pb * 3)
    assert H.h_smul_fixed(1, 4, p, b32(m.R) + b32(7) + b32((1 << 256) - 1), 3, out) == 2
    assert out.raw[pb:2 * pb] == expected(cx, p, b32(7))


@pytest.mark.parametrize("curve", list(small_order.COFACTOR_CURVES))
def test_bases_of_small_order(tmp_path_factory, curve):
    # A base T of prime order f = 3 .. 10177 (tests/small_order.py) is a legal input on a curve with a cofactor: k T is the integer multiple,
    # (k mod f) T.  The plain ladder's accumulator then runs through +-T and the identity all the time, and most records of a fixed-base table
    # (j 2^(C w) T, j up to 2^(C-1)) are identities when f is small.  On BLS12-381 G1 the point of order 3 is (0, +-2): x = 0 in a record that
    # is NOT the identity.  Expected values: repeated addition in the big-integer model; the C oracle is pinned to the same bytes.
    H, cx, m = harness(tmp_path_factory, curve)
    pb = 2 * cx.coord_bytes()
    big = cx.coord_bytes() > 48
    r_ = m.R
    for f in small_order.ORDERS[curve]:
        t = small_order.torsion_point(curve, f)
        if curve == "bls12_381" and f == 3:
            assert t in ((0, 2), (0, m.P - 2))
            t = (0, 2)
        mult = small_order.multiples(m, f, t)
        rnd = rng(90 + f)
        ks = [0, 1, 2, 3, f - 1, f, f + 1, 2 * f, r_ - 1, r_ - 2, (r_ - 1) // 2, 0x8000, 0xFFFF, 0x7FFF8000] + [rnd.randrange(r_) for _ in range(20)]
        n = len(ks)
        p = small_order.enc(m, t)
        sc = b"".join(b32(k) for k in ks)
        want = b"".join(small_order.enc(m, mult[k % f]) for k in ks)
        assert want[:pb] == bytes(pb) and want[5 * pb:6 * pb] == bytes(pb) and want[pb:2 * pb] == p
        assert expected(cx, p * n, sc) == want, (curve, f, "the C oracle")
        out = C.create_string_buffer(pb * n)
        assert H.h_smul(0, p * n, sc, n, 3, out) == 0
        bad = [hex(ks[i]) for i in range(n) if out.raw[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
        assert not bad, (curve, f, "plain ladder", bad[:4])
        for c in (4, 5) if big else (4, 5, 7):
            out = C.create_string_buffer(pb * n)
            assert H.h_smul_fixed(0, c, p, sc, n, out) == 0
            bad = [hex(ks[i]) for i in range(n) if out.raw[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
            assert not bad, (curve, f, "table", c, bad[:4])


def test_fixed_base_table_outside_the_subgroup(tmp_path_factory):
    # BLS12-381 G1, a point that is not of order r: the table built by the plain ladder holds integer multiples, and so does the product
    H, cx, m = harness(tmp_path_factory, "bls12_381")
    pt = next(q for q in m.bytes_to_points(cx.sample_points(62, 6)) if m.add(m.mul(m.R - 1, q), q) is not None)
    ks = [1, 2, m.R - 1, m.R - 2, (1 << 254) + 5, rng(9).randrange(m.R)]
    out = C.create_string_buffer(96 * len(ks))
    assert H.h_smul_fixed(0, 5, m.points_to_bytes([pt]), b"".join(b32(k) for k in ks), len(ks), out) == 0
    assert out.raw == b"".join(m.affine_to_bytes64(m.mul(k, pt)) for k in ks)
