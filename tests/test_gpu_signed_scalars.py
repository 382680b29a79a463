"""Signed and 128-bit narrow scalar formats (include/msm_hip.h: MSM_HIP_SCALAR_SIGNED on U8 .. U64 / MSM_HIP_SCALAR_U128: I8 .. I64, U128, I128).
A signed value v contributes v * P as an integer multiple -- a negative one -(|v| * P) --, which for bases of order r is what the 32-byte scalar
v mod r gives.  Every result is compared bit-exactly, as affine bytes, with the curve's CPU oracle fed v mod r as 32-byte scalars, and with the
same context's 32-byte canonical run on those bytes.  The values plant 0, +1, -1, the maximum, the minimum (whose magnitude does not fit the
signed type), 2^127, the edges of the C-bit recode of the magnitude in both signs, and a pair (v, -v) on two copies of one base, which cancels."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import cpu
from tests import signed_scalar_model as model
from tests.edge_scalars import edge_vector
from tests.launch_model import narrow_nwin_of, pick_window_bits
from tests.test_gpu_launch_matrix import oracle_module, scalar_order, subgroup_points_bls12_381

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG = -2
FORMATS = ["i8", "i16", "i32", "i64", "u128", "i128"]
MODES = ["plain", "endomorphism", "tables", "wide"]
WINDOWS = [0, 12, 14, 16]
MAXLW, BYTE_MAXLW, BYTE_WBITS = 64, 32, 12
SIGNED_DTYPES = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
OTHER_CURVES = ["grumpkin", "pallas", "vesta", "bls12_381", "bn254_g2", "bls12_381_g2"]
PAIR = 7  # bases PAIR and PAIR + 1 are the same point: the values there are (v, -v)


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


# ---------------------------------------------------------------------------------------------------------------- inputs and rules
def base_flags(mode):
    return dict(endomorphism=mode == "endomorphism", precompute="wide" if mode == "wide" else mode == "tables")


def set_format(c, fmt):
    if fmt == "canonical":
        c.set_scalar_format(width=32)
    else:
        width, signed = model.FORMATS[fmt]
        c.set_scalar_format(width=width, signed=signed)


def run_bits(fmt, fixed, n, nvec=1):
    """the window width the documented rules give a launch of nvec vectors of n values: byte windows run on the 12-bit grid, the others pick
    the width as 32-byte scalars do, widened until the launch's windows fit"""
    width, _ = model.FORMATS[fmt]
    return BYTE_WBITS if model.byte_windows(width) else pick_window_bits(fixed, n, nvec, nb=width)


def batch_groups(fmt, fixed, n, batch):
    width, _ = model.FORMATS[fmt]
    fit = BYTE_MAXLW // width if model.byte_windows(width) else MAXLW // narrow_nwin_of(pick_window_bits(fixed, n, 2, nb=width), width)
    g = max(1, min((1 << 20) // n, fit, batch))
    return [min(g, batch - first) for first in range(0, batch, g)]


def values(fmt, c, n, seed, kind="edges"):
    """n integers of the format.  "edges": the format's own edges, the recode edges of the magnitude at C bits in both signs, then uniform
    values; positions PAIR, PAIR + 1 hold (v, -v).  n = 1: the minimum (signed) or the maximum.  "reversed" / "negated": the same, reordered
    or with every sign flipped where the format has the opposite value."""
    width, signed = model.FORMATS[fmt]
    lo, hi = model.value_range(width, signed)
    if n == 1:
        return [lo if signed else hi]
    mags = edge_vector(8 * width, 8 if model.byte_windows(width) else c, n, seed)
    rng = np.random.default_rng(seed + 1)
    flip = rng.random(n) < 0.5
    out = list(model.edge_values(width, signed))
    for k, mag in enumerate(mags):
        if len(out) >= n:
            break
        if not signed:
            out.append(mag)
            continue
        mag &= (1 << (8 * width - 1)) - 1  # both signs of it are values of the format
        out += [mag, -mag][:n - len(out)] if k < 40 else [-mag if flip[k] else mag]
    out = out[:n]
    if n > PAIR + 1:
        v = out[PAIR] if out[PAIR] not in (0, lo) else 3
        out[PAIR], out[PAIR + 1] = (v, -v) if signed else (v, v)
    if kind == "reversed":
        out = out[::-1]
    elif kind == "negated":
        out = [-v if signed and v != lo else v for v in out]
    return out


def dev_rows(host):
    """host bytes -> a CUDA uint8 tensor (fresh allocations are aligned far beyond 16 bytes)"""
    if not host:
        return torch.zeros(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()


def dev_typed(fmt, host):
    """the signed torch dtype of the width, where torch has one"""
    width, signed = model.FORMATS[fmt]
    return dev_rows(host).view(SIGNED_DTYPES[width]) if signed and width in SIGNED_DTYPES else None


def with_pair(points, pb):
    """bases PAIR and PAIR + 1 made the same point"""
    a = np.frombuffer(points, dtype=np.uint8).reshape(-1, pb).copy()
    if a.shape[0] > PAIR + 1:
        a[PAIR + 1] = a[PAIR]
    return a.tobytes()


class Runner:
    """One context and its points; oracle answers are computed once per input; failures are collected so that one run names every cell."""

    def __init__(self, c, curve, points):
        self.c, self.curve, self.points = c, curve, points
        self.orc, self.r = oracle_module(curve), scalar_order(curve)
        self.answers, self.failures = {}, []
        self.slot = 0

    def want(self, key, ints, idx=None, drop=()):
        """the oracle's sum_j (ints[j] mod r) * P[idx[j]] (idx None: the first len(ints) points), without the entries whose base is in `drop`"""
        if key not in self.answers:
            pb = self.c.pb
            idx = np.arange(len(ints)) if idx is None else np.asarray(idx, dtype=np.int64)
            keep = ~np.isin(idx, np.asarray(list(drop), dtype=np.int64))
            pts = np.frombuffer(self.points, dtype=np.uint8).reshape(-1, pb)[idx[keep]].tobytes()
            s32 = model.scalars32([v for v, k in zip(ints, keep) if k], self.r)
            self.answers[key] = self.orc.to_affine64(self.orc.cpu_msm(pts, s32, n_threads=16)) if keep.any() else None
        return self.answers[key]

    def check(self, where, call, want, bits=None):
        try:
            got = call()
        except (m.MsmHipError, ValueError, TypeError) as e:
            self.failures.append("%s: raised %r" % (where, e))
            return
        many = isinstance(got, list)
        for g, w in zip(got if many else [got], want if many else [want]):
            if (g.is_identity() if w is None else g.to_affine_bytes() == w) is not True:
                self.failures.append("%s: differs from the oracle" % where)
        if bits is not None and self.c.last_window_bits() != bits:
            self.failures.append("%s: ran at %d bits, the rules say %d" % (where, self.c.last_window_bits(), bits))

    def canonical(self, ints, idx=None):
        """the same context's 32-byte canonical run on v mod r"""
        s32 = model.scalars32(ints, self.r)
        set_format(self.c, "canonical")
        return self.c.msm(s32) if idx is None else self.c.msm_sparse(idx, s32)

    def report(self):
        assert not self.failures, "%d failures:\n%s" % (len(self.failures), "\n".join(self.failures[:60]))

    # -- a dense cell: every entry point
    def dense(self, fmt, mode, fixed, n, batch=3):
        c = self.c
        width, signed = model.FORMATS[fmt]
        cb = run_bits(fmt, fixed, n)
        seed = zlib.crc32(repr((self.curve, fmt, cb, n)).encode())
        ints = values(fmt, cb, n, seed)
        want = self.want(("dense", fmt, cb, n, "edges"), ints)
        host = model.encode(ints, width, signed)
        where = "%s %s/%s/%d dense n=%d" % (self.curve, fmt, mode, fixed, n)
        self.check(where + " canonical 32-byte run", lambda: self.canonical(ints), want)
        set_format(c, fmt)
        self.check(where + " host", lambda: c.msm(host), want, cb)
        self.check(where + " device rows", lambda: c.msm(dev_rows(host)), want, cb)
        typed = dev_typed(fmt, host)
        if typed is not None:
            self.check(where + " device dtype", lambda: c.msm(typed), want, cb)
        # launch / finish in two slots at once: the second vector is the first with its signs flipped
        other = values(fmt, cb, n, seed, "negated")
        want2 = self.want(("dense", fmt, cb, n, "negated"), other)
        a, b = self.slot % 3 + 1, (self.slot + 1) % 3 + 1
        self.slot += 2

        def two_slots():
            ta, tb = dev_rows(host), dev_rows(model.encode(other, width, signed))
            c.launch(ta, slot=a)
            c.launch(tb if typed is None else tb.view(SIGNED_DTYPES[width]), slot=b)
            return [c.finish(a), c.finish(b)]

        self.check(where + " slots %d, %d" % (a, b), two_slots, [want, want2], cb)
        if batch:
            kinds = ["edges", "negated", "reversed"][:batch]
            vecs = [values(fmt, cb, n, seed, k) for k in kinds]
            wants = [self.want(("dense", fmt, cb, n, k), v) for k, v in zip(kinds, vecs)]
            blob = b"".join(model.encode(v, width, signed) for v in vecs)
            bbits = run_bits(fmt, fixed, n, batch_groups(fmt, fixed, n, batch)[-1])
            self.check(where + " batch host", lambda: c.msm_batch(blob, n), wants, bbits)
            self.check(where + " batch device", lambda: c.msm_batch(dev_rows(blob), n), wants, bbits)

    # -- a sparse cell
    def sparse(self, fmt, mode, fixed, nnz, n_bases):
        c = self.c
        width, signed = model.FORMATS[fmt]
        cb = run_bits(fmt, fixed, max(nnz, 1))
        seed = zlib.crc32(repr((self.curve, fmt, cb, nnz, n_bases, "sparse")).encode())
        ints = values(fmt, cb, nnz, seed) if nnz else []
        idx = np.random.default_rng(seed).integers(0, n_bases, size=nnz, dtype=np.int64)
        if nnz >= 6:  # repeats: base j with +k and -k (they cancel), and the last base three times
            lo, _ = model.value_range(width, signed)
            k = ints[2] if ints[2] not in (0, lo) else 5
            idx[2] = idx[3] = idx[0]
            ints[2], ints[3] = (k, -k) if signed else (k, k)
            idx[-3:] = n_bases - 1
        want = self.want(("sparse", fmt, cb, nnz, n_bases), ints, idx)
        host = model.encode(ints, width, signed)
        where = "%s %s/%s/%d sparse nnz=%d over %d" % (self.curve, fmt, mode, fixed, nnz, n_bases)
        di = torch.from_numpy(idx).to(torch.int32 if nnz % 2 else torch.int64).cuda()
        if nnz:
            self.check(where + " canonical 32-byte run", lambda: self.canonical(ints, idx), want)
        set_format(c, fmt)
        bits = cb if nnz else None  # (nothing to compute: the plain 16-bit request, whatever the format)
        self.check(where + " host", lambda: c.msm_sparse(idx, host), want, bits)
        self.check(where + " device", lambda: c.msm_sparse(di, dev_rows(host)), want, bits)
        slot = self.slot % 3 + 1
        self.slot += 1
        self.check(where + " slot %d" % slot, lambda: (c.launch_sparse(di, dev_rows(host), slot=slot), c.finish(slot))[1], want, bits)


# ---------------------------------------------------------------------------------------------------------------- dense, BN254
N_BASES = 33001  # > 2^15: the largest oracle-checked n (the existing narrow tests go to 65541)
DENSE_N = [1, 4096, 4097, N_BASES]  # both sides of the automatic 12 / 16-bit threshold, and one n > 2^15


@pytest.fixture(scope="module")
def bn254(gpu):
    c = m.MsmContext(0)
    points = with_pair(cpu.sample_points(701, N_BASES), c.pb)
    R = Runner(c, "bn254", points)
    yield R
    c.close()


@pytest.mark.parametrize("mode", MODES)
def test_dense_bn254(bn254, mode):
    R, c = bn254, bn254.c
    R.failures = []
    c.set_bases(R.points, **base_flags(mode))
    try:
        for fmt in FORMATS:
            for fixed in WINDOWS:
                c.set_window_bits(fixed)
                for n in DENSE_N:
                    R.dense(fmt, mode, fixed, n)
    finally:
        c.set_window_bits(0)
        set_format(c, "canonical")
    R.report()


def test_the_pair_cancels(bn254):
    """(v, -v) on two copies of one base add nothing: the vector that holds only that pair is the identity, in every signed format"""
    R, c = bn254, bn254.c
    c.set_bases(R.points, endomorphism=False)
    try:
        for fmt in FORMATS:
            width, signed = model.FORMATS[fmt]
            if not signed:
                continue
            _, hi = model.value_range(width, signed)
            for v in (1, hi, 0x55 if width == 1 else 0x7F80):
                ints = [0] * (PAIR + 2)
                ints[PAIR], ints[PAIR + 1] = v, -v
                set_format(c, fmt)
                assert c.msm(model.encode(ints, width, signed)).is_identity(), (fmt, v)
    finally:
        set_format(c, "canonical")


# ---------------------------------------------------------------------------------------------------------------- sparse
@pytest.mark.parametrize("mode", ["plain", "endomorphism"])
def test_sparse_bn254(bn254, mode):
    R, c = bn254, bn254.c
    R.failures = []
    n_bases = 5000
    c.set_bases(R.points[:n_bases * c.pb], **base_flags(mode))
    try:
        for fmt in FORMATS:
            for fixed in (0, 14):
                c.set_window_bits(fixed)
                for nnz in (0, 1, 4097, 2 * n_bases + 1):
                    R.sparse(fmt, mode, fixed, nnz, n_bases)
            c.set_window_bits(0)
            # one bad device index: the launch fails, and the context stays usable
            width, signed = model.FORMATS[fmt]
            ints = values(fmt, 12, 100, 5)
            idx = np.arange(100, dtype=np.int64)
            bad = idx.copy()
            bad[50] = n_bases
            set_format(c, fmt)
            with pytest.raises(m.MsmHipError) as e:
                c.msm_sparse(torch.from_numpy(bad).cuda(), dev_rows(model.encode(ints, width, signed)))
            assert e.value.code == ERR_INVALID_ARG
            R.check("%s after a bad index" % fmt, lambda: c.msm_sparse(torch.from_numpy(idx).cuda(), dev_rows(model.encode(ints, width, signed))),
                    R.want(("sparse-after-bad", fmt), ints, idx))
    finally:
        c.set_window_bits(0)
        set_format(c, "canonical")
    R.report()


def test_sparse_on_wide_tables_stays_rejected(bn254):
    R, c = bn254, bn254.c
    n_bases = 2000
    c.set_bases(R.points[:n_bases * c.pb], precompute="wide")
    try:
        for fmt in FORMATS:
            width, signed = model.FORMATS[fmt]
            host = model.encode(values(fmt, 12, 64, 9), width, signed)
            idx = np.arange(64, dtype=np.int64)
            set_format(c, fmt)
            for call in (lambda: c.msm_sparse(idx, host), lambda: c.msm_sparse(torch.from_numpy(idx).cuda(), dev_rows(host)),
                         lambda: c.launch_sparse(torch.from_numpy(idx).cuda(), dev_rows(host), slot=1)):
                with pytest.raises(m.MsmHipError) as e:
                    call()
                assert e.value.code == ERR_INVALID_ARG, fmt
    finally:
        set_format(c, "canonical")


# ---------------------------------------------------------------------------------------------------------------- identity bases
@pytest.mark.parametrize("fmt", ["i16", "i64", "i128"])  # a byte-window, a truncated-window and a 128-bit format
def test_identity_bases_under_negative_scalars(bn254, fmt):
    R, c = bn254, bn254.c
    R.failures = []
    n = 4097
    width, signed = model.FORMATS[fmt]
    ids = [0, 1, 3, 63, 64, 255, 256, 1000, n - 1]
    bases = np.frombuffer(R.points[:n * c.pb], dtype=np.uint8).reshape(n, c.pb).copy()
    bases[ids] = 0
    lo, hi = model.value_range(width, signed)
    try:
        for mode in ("plain", "endomorphism"):
            c.set_bases(bases.tobytes(), zero_is_identity=True, **base_flags(mode))
            ints = values(fmt, 12, n, 31)
            for k, i in enumerate(ids):  # negative scalars on the identities, the minimum and -1 among them
                ints[i] = [lo, -1, -hi, -(12345 % (hi + 1))][k % 4]
            host = model.encode(ints, width, signed)
            want = R.want(("identity", fmt, n), ints, drop=ids)
            set_format(c, fmt)
            R.check("%s %s dense host" % (fmt, mode), lambda: c.msm(host), want)
            R.check("%s %s dense device" % (fmt, mode), lambda: c.msm(dev_rows(host)), want)
            assert c.env_report()["last_identity_mask"] == 1
            idx = np.random.default_rng(41).integers(0, n, size=3000, dtype=np.int64)
            idx[:len(ids)] = ids
            sp = values(fmt, 12, 3000, 32)
            for k in range(len(ids)):
                sp[k] = lo if k % 2 else -1
            R.check("%s %s sparse" % (fmt, mode), lambda: c.msm_sparse(torch.from_numpy(idx).cuda(), dev_rows(model.encode(sp, width, signed))),
                    R.want(("identity-sparse", fmt, n), sp, idx, drop=ids))
    finally:
        set_format(c, "canonical")
    R.report()


# ---------------------------------------------------------------------------------------------------------------- the other curves
SLICE = {"grumpkin": ("i8", "u128"), "pallas": ("i32", "i128"), "vesta": ("i64", "u128"), "bls12_381": ("i16", "i128"),
         "bn254_g2": ("i64", "u128"), "bls12_381_g2": ("i32", "i128")}


@pytest.mark.parametrize("curve", OTHER_CURVES)
def test_other_curves(gpu, curve):
    """one signed and one 128-bit format on every other curve, dense and sparse, plain and endomorphism bases.  BLS12-381's points are drawn
    from the order-r subgroup: outside it -(|v| P) and (r - |v|) P differ, and the oracle is fed v mod r."""
    n_bases = 600 if curve.endswith("_g2") else 1024
    c = m.MsmContext(0, curve=curve)
    try:
        points = subgroup_points_bls12_381(9202, n_bases) if curve == "bls12_381" else c.sample_points(n_bases, 9202).cpu().numpy().tobytes()
        R = Runner(c, curve, with_pair(points, c.pb))
        for mode in ("plain", "endomorphism"):
            c.set_bases(R.points, **base_flags(mode))
            for fmt in SLICE[curve]:
                for n in (1, n_bases):
                    R.dense(fmt, mode, 0, n, batch=2)
                R.sparse(fmt, mode, 0, 2 * n_bases + 1, n_bases)
            set_format(c, "canonical")
        R.report()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- rejections
def test_rejections(bn254):
    R, c = bn254, bn254.c
    L = m.lib()
    c.set_bases(R.points[:2000 * c.pb], endomorphism=None)
    n = 1000
    t = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
    out = torch.zeros(16, 96, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for value in (6, 7, 16, 17, 22, 23, 25, 9, 15, 26, 32 | 18, 0x100 | 24):
        assert L.msm_hip_set_scalar_format(c._h, value) == ERR_INVALID_ARG, value
    for value in (18, 19, 20, 21, 8, 24):
        assert L.msm_hip_set_scalar_format(c._h, value) == 0, value
    assert L.msm_hip_set_scalar_format(c._h, 0) == 0
    try:
        for fmt in FORMATS:
            set_format(c, fmt)
            # the window-sharding entry points do not read 32-byte rows under a narrow format
            assert L.msm_hip_run_windows_device(c._h, C.c_void_p(t.data_ptr()), n, 0, 4, C.c_void_p(out.data_ptr())) == ERR_INVALID_ARG
            assert L.msm_hip_launch_windows_batch_device(c._h, C.c_void_p(t.data_ptr()), n, 1, 0, 2, 0, C.c_void_p(out.data_ptr())) == ERR_INVALID_ARG
            assert L.msm_hip_launch_half_windows_batch_device(c._h, C.c_void_p(t.data_ptr()), n, 1, 0, 8, 0, None) == ERR_INVALID_ARG
            assert L.msm_hip_launch_vwindows_batch_device(c._h, C.c_void_p(t.data_ptr()), n, 1, 0, 1, 0, None) == ERR_INVALID_ARG
        with pytest.raises(ValueError):
            c.set_scalar_format(width=32, signed=True)
        with pytest.raises(ValueError):
            c.set_scalar_format(mont256=True, signed=True)
        with pytest.raises(ValueError):
            c.set_scalar_format(mont256=True, width=8, signed=True)
        with pytest.raises(ValueError):
            c.set_scalar_format(mont256=True, width=16)
        with pytest.raises(ValueError):
            c.set_scalar_format(width=3, signed=True)
        c.set_scalar_format(width=4, signed=True)
        with pytest.raises(TypeError):
            c.msm(torch.zeros(10, dtype=torch.uint32, device="cuda"))  # an unsigned wider dtype under I32
        with pytest.raises(ValueError):
            c.msm(torch.zeros(10, dtype=torch.int16, device="cuda"))  # a signed dtype of another width
        with pytest.raises(ValueError):
            c.msm(bytes(4 * 10 + 2))
        assert c.msm(torch.zeros(10, dtype=torch.int32, device="cuda")).is_identity()
        c.set_scalar_format(width=4)  # ... and under the unsigned format the signed dtype is still refused
        with pytest.raises(TypeError):
            c.msm(torch.zeros(10, dtype=torch.int32, device="cuda"))
        for signed in (False, True):
            c.set_scalar_format(width=16, signed=signed)
            buf = torch.zeros(16 * 11, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            assert c.msm(buf[:160]).is_identity()
            with pytest.raises(ValueError):
                c.msm(buf[8:168])  # rows that are not 16-byte aligned
            with pytest.raises(ValueError):
                c.msm(buf[:150])  # not a whole number of rows
            with pytest.raises((TypeError, ValueError)):
                c.msm(torch.zeros(20, dtype=torch.int64, device="cuda"))  # torch has no 128-bit dtype: uint8 rows only
            assert L.msm_hip_run_device(c._h, C.c_void_p(buf.data_ptr() + 8), 10, C.create_string_buffer(96)) == ERR_INVALID_ARG
    finally:
        set_format(c, "canonical")


# ---------------------------------------------------------------------------------------------------------------- no leak into 32-byte MSMs
def test_no_leak_into_later_32_byte_msms(gpu):
    """A launch in a new format neither arms nor consumes the skew credit that follows skewed 32-byte launches, and the 32-byte launch after it
    gives the 32-byte oracle result."""
    n = 1 << 16  # > FINE_BIG entries in one coarse bin
    points = cpu.sample_points(705, n)
    c = m.MsmContext(0)
    try:
        c.set_bases(points, endomorphism=None)
        s = cpu.sample_scalars(91, n)
        want32 = cpu.to_affine64(cpu.cpu_msm(points, s, n_threads=16))

        def minus_ones(fmt):  # all-equal values: one huge bin in every window that has entries
            width, signed = model.FORMATS[fmt]
            return dev_rows(model.encode([-1 if signed else 1] * n, width, signed))

        assert c.skew_credit() == 0
        for fmt in FORMATS:
            set_format(c, fmt)
            for _ in range(2):
                c.msm(minus_ones(fmt))
            assert c.skew_credit() == 0, fmt
            set_format(c, "canonical")
            assert c.msm(s).to_affine_bytes() == want32, fmt  # the 32-byte launch after a signed one
            assert c.skew_credit() == 0
        c.msm(dev_rows(model.scalars32([1] * n, scalar_order("bn254"))))  # positive control: equal values in 32-byte form arm it
        armed = c.skew_credit()
        assert armed > 0
        for fmt in FORMATS:
            width, signed = model.FORMATS[fmt]
            set_format(c, fmt)
            c.msm(minus_ones(fmt))
            c.msm(dev_rows(model.encode(values(fmt, 16, n, 93), width, signed)))
            assert c.skew_credit() == armed, fmt  # neither used nor re-armed
        set_format(c, "canonical")
        assert c.msm(s).to_affine_bytes() == want32
        assert c.skew_credit() == armed - 1  # a 32-byte launch uses one
    finally:
        set_format(c, "canonical")
        c.close()


# ---------------------------------------------------------------------------------------------------------------- stage parity
@pytest.mark.parametrize("bits", [16, 14, 12])
@pytest.mark.parametrize("fmt", ["i64", "i128", "i32", "u128"])
def test_digit_planes_match_the_model(bn254, fmt, bits):
    """the recode's digit planes (msm_hip_set_debug / msm_hip_read_digits) of a vector in the format equal the Python model's digits of the
    magnitude with the sign applied (tests/signed_scalar_model.py), value by value and window by window"""
    R, c = bn254, bn254.c
    n = 3000
    width, signed = model.FORMATS[fmt]
    ints = values(fmt, bits, n, 1234 + bits)
    c.set_bases(R.points[:n * c.pb], endomorphism=None)
    c.set_debug(True)
    c.set_window_bits(bits)
    set_format(c, fmt)
    try:
        got = c.msm(model.encode(ints, width, signed))
        assert c.last_window_bits() == bits
        nwin = model.windows(width, bits)
        planes = c.read_digits(n, nwin)
    finally:
        c.set_debug(False)
        c.set_window_bits(0)
        set_format(c, "canonical")
    want = np.array([[model.plane_digit(d, bits) for d in model.digits(v, width, signed, bits)] for v in ints], dtype=np.int64).T
    dec = np.array([[model.decode_plane(int(code), bits) for code in row] for row in planes], dtype=np.int64)
    assert dec.shape == want.shape == (nwin, n)
    bad = np.argwhere(dec != want)
    assert bad.size == 0, "window %d, value %d (%d): plane %d, model %d" % (bad[0][0], bad[0][1], ints[bad[0][1]], dec[tuple(bad[0])], want[tuple(bad[0])])
    assert got.to_affine_bytes() == R.want(("planes", fmt, bits), ints)
