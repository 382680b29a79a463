"""Batch scalar multiplication on the device (include/msm_hip.h: msm_hip_mul_each, msm_hip_mul_base): out[i] = s_i * P_i and s_i * P_base.
Every small case is compared bit for bit with the oracle's g1_scalar_mul followed by to_affine64, computed once per (curve, inputs) and reused
across entry points, base modes and scalar formats.  At 2^20 points, where an elementwise oracle would take minutes, the outputs are checked
through a random linear combination (see test_real_size_through_a_random_combination)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import bn254_ref, cpu
from tests.edge_scalars import edge_values

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_NONCANONICAL, ERR_NO_BASES = -2, -4, -6
MODES = {"plain": dict(endomorphism=False), "endomorphism": dict(endomorphism=True), "tables": dict(precompute=True), "wide": dict(precompute="wide")}
OTHER_CURVES = ["grumpkin", "pallas", "vesta", "bls12_381", "bn254_g2", "bls12_381_g2"]
PRIME_ORDER = ("bn254", "grumpkin", "pallas", "vesta")
R = bn254_ref.R
PATH_PLAIN, PATH_ENDO, PATH_TABLE_HELD, PATH_TABLE_BUILT = 1, 2, 3, 4


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def oracle_module(curve):
    return cpu if curve == "bn254" else importlib.import_module("oracle.cpu_" + curve)


def ref_module(curve):
    return importlib.import_module("oracle.%s_ref" % curve)


def b32(v):
    return int(v).to_bytes(32, "little")


def dev_u8(b, row):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda().reshape(-1, row)


def expected(orc, points, scalars):
    """[s_i * P_i] as affine records, the identity as zeros: the oracle's scalar multiplication and its affine conversion"""
    jb = 3 * orc.coord_bytes()
    jac = orc.g1_scalar_mul(points, scalars)
    return b"".join(orc.to_affine64(jac[i:i + jb]) for i in range(0, len(jac), jb))


def edge_scalars(ref):
    """the scalars planted in every vector: small ones, the ends of [0, r), lambda and its neighbours, the 127 / 128-bit boundary of the split's
    halves, splits with a zero half or equal / opposite halves, and the recode edges of tests/edge_scalars.py"""
    r_, lam = ref.R, ref.glv_params()["lam"]
    ks = [0, 1, 2, r_ - 1, r_ - 2, (r_ + 1) // 2, (r_ - 1) // 2, lam, lam + 1, lam - 1, r_ - lam, (1 << 127) + 1, (1 << 127) - 1, 1 << 128]
    for t in (1, 3, 0xFFFF, (1 << 100) + 77):
        ks += [t * lam % r_, t * (1 + lam) % r_, t * (1 - lam) % r_, (r_ - t) * lam % r_]
    ks += [v for _, v, _ in edge_values(r_.bit_length(), 16, r_)]
    return [k % r_ for k in ks]


def scalar_vector(orc, ref, n, seed):
    """n scalars: uniform ones with the edge scalars planted from position 0 on (as many as fit)"""
    a = np.frombuffer(orc.sample_scalars(seed, n), dtype=np.uint8).reshape(n, 32).copy()
    for i, k in enumerate(edge_scalars(ref)[:n]):
        a[i] = np.frombuffer(b32(k), dtype=np.uint8)
    return a.tobytes()


def to_mont256(scalars, r_):
    return b"".join(b32((int.from_bytes(scalars[i:i + 32], "little") << 256) % r_) for i in range(0, len(scalars), 32))


def subgroup_points_bls12_381(seed, n):
    ref = ref_module("bls12_381")
    orc = oracle_module("bls12_381")
    return expected(orc, ref.points_to_bytes([ref.G]) * n, orc.sample_scalars(seed, n))


# ---------------------------------------------------------------------------------------------------------------- mul_each on BN254
@pytest.fixture(scope="module")
def bn254_inputs(gpu):
    """points, scalars and the oracle's products for the largest n; a smaller n uses their prefix (out[i] depends on pair i alone)"""
    n = 8191
    points = cpu.sample_points(2001, n)
    scalars = scalar_vector(cpu, bn254_ref, n, 2002)
    return points, scalars, expected(cpu, points, scalars)


@pytest.mark.parametrize("mode", list(MODES))
def test_mul_each_in_every_base_mode_from_every_input_form(gpu, bn254_inputs, mode):
    points, scalars, want = bn254_inputs
    c = m.MsmContext(0)
    try:
        c.set_bases(points, **MODES[mode])
        for n in (1, 255, 256, 257, 8191):
            s, w = scalars[:32 * n], want[:64 * n]
            assert c.mul_each(s) == w, (mode, n, "host")
            assert c.mul_last() == (PATH_ENDO, 0, 16)
            out = c.mul_each(dev_u8(s, 32))
            assert tuple(out.shape) == (n, 64) and out.dtype == torch.uint8 and out.is_cuda
            assert out.cpu().numpy().tobytes() == w, (mode, n, "device")
            pre = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
            assert c.mul_each(dev_u8(s, 32), out=pre) is pre and pre.cpu().numpy().tobytes() == w, (mode, n, "out=")
            c.set_scalar_format(mont256=True)
            sm = to_mont256(s, R)
            assert c.mul_each(sm) == w, (mode, n, "mont256 host")
            assert c.mul_each(dev_u8(sm, 32)).cpu().numpy().tobytes() == w, (mode, n, "mont256 device")
            c.set_scalar_format()
        with pytest.raises(ValueError):
            c.mul_each(dev_u8(scalars[:64], 32), out=torch.empty((3, 64), dtype=torch.uint8, device="cuda"))
        with pytest.raises(TypeError):
            c.mul_each(dev_u8(scalars[:64], 32), out=bytearray(128))
    finally:
        c.close()


@pytest.mark.parametrize("mode", ["plain", "endomorphism", "tables", "wide"])
def test_identity_bases_give_identity_outputs_whatever_their_scalars(gpu, bn254_inputs, mode):
    points, scalars, want = bn254_inputs
    n = 8191
    # first, last, a run across a workgroup of the ladder kernel, a run across a block of the normalisation (16 x 256 outputs) and a whole chunk
    # of one normalisation lane (outputs 5, 5 + 256, ...)
    ids = np.unique(np.concatenate([[0, n - 1], np.arange(250, 262), np.arange(4090, 4103), 5 + 256 * np.arange(16), 4096 + 7 + 256 * np.arange(16)]))
    pa = np.frombuffer(points, dtype=np.uint8).reshape(n, 64).copy()
    pa[ids] = 0
    sa = np.frombuffer(scalars, dtype=np.uint8).reshape(n, 32).copy()
    sa[ids[::2]] = 0xFF  # 2^256 - 1 beside an identity base: ignored, also by the comparison with r
    wa = np.frombuffer(want, dtype=np.uint8).reshape(n, 64).copy()
    wa[ids] = 0
    c = m.MsmContext(0)
    try:
        c.set_bases(pa.tobytes(), zero_is_identity=True, **MODES[mode])
        assert c.mul_each(sa.tobytes()) == wa.tobytes()
        assert c.mul_each(dev_u8(sa.tobytes(), 32)).cpu().numpy().tobytes() == wa.tobytes()
        # Montgomery-form scalars: the words beside an identity base are not a residue at all
        sm = np.frombuffer(to_mont256(scalars, R), dtype=np.uint8).reshape(n, 32).copy()
        sm[ids[::2]] = 0xFF
        c.set_scalar_format(mont256=True)
        assert c.mul_each(dev_u8(sm.tobytes(), 32)).cpu().numpy().tobytes() == wa.tobytes()
        c.set_scalar_format()
        # one base for all: an identity record, and a regular one of the same set
        assert c.mul_base(int(ids[3]), sa[:300].tobytes()) == bytes(64 * 300)
        assert c.mul_base(int(ids[3]), dev_u8(sa[:300].tobytes(), 32)).cpu().numpy().tobytes() == bytes(64 * 300)
        assert c.mul_base(1, scalars[32:64]) == want[64:128]
        c.mul_policy(1, 8)  # the same with the table forced: an identity base never reaches the policy, a regular one builds its table
        assert c.mul_base(int(ids[3]), sa[:300].tobytes()) == bytes(64 * 300) and c.mul_last()[:2] == (0, 0)
        assert c.mul_base(1, scalars[32:64]) == want[64:128] and c.mul_last()[:2] == (PATH_TABLE_BUILT, 8)
        c.mul_policy(0, 0)
    finally:
        c.close()


def test_all_identities_and_all_zero_scalars(gpu, bn254_inputs):
    points, scalars, _ = bn254_inputs
    n = 4099
    c = m.MsmContext(0)
    try:
        c.set_bases(bytes(64 * n), zero_is_identity=True)
        assert c.mul_each(scalars[:32 * n]) == bytes(64 * n)
        c.set_bases(points[:64 * n])
        assert c.mul_each(bytes(32 * n)) == bytes(64 * n)
        assert c.mul_each(dev_u8(bytes(32 * n), 32)).cpu().numpy().tobytes() == bytes(64 * n)
        assert c.mul_base(0, bytes(32 * n)) == bytes(64 * n)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- rejections
def test_scalars_not_below_r_are_rejected_and_the_context_stays_usable(gpu, bn254_inputs):
    points, scalars, want = bn254_inputs
    n = 600
    c = m.MsmContext(0)
    try:
        c.set_bases(points[:64 * n])
        for bad in (R, (1 << 256) - 1):
            for pos in (0, 257, n - 1):
                sa = bytearray(scalars[:32 * n])
                sa[32 * pos:32 * pos + 32] = b32(bad)
                for call in (lambda s: c.mul_each(s), lambda s: c.mul_each(dev_u8(s, 32)), lambda s: c.mul_base(3, s)):
                    with pytest.raises(m.MsmHipError) as e:
                        call(bytes(sa))
                    assert e.value.code == ERR_NONCANONICAL
                    assert c.mul_each(scalars[:32 * n]) == want[:64 * n]  # the next call on the same context is correct
    finally:
        c.close()


def test_invalid_arguments(gpu, bn254_inputs):
    points, scalars, want = bn254_inputs
    n = 64
    L = m.lib()
    c = m.MsmContext(0)
    try:
        h = c._h
        out = C.create_string_buffer(64 * (n + 1))
        s = scalars[:32 * (n + 1)]
        d_s, d_out = dev_u8(s, 32), torch.empty((n + 1, 64), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        # before set_bases
        assert L.msm_hip_mul_each(h, s, n, out, 0) == ERR_NO_BASES
        assert L.msm_hip_mul_base(h, 0, s, n, out, 0) == ERR_NO_BASES
        assert L.msm_hip_mul_each_device(h, d_s.data_ptr(), n, d_out.data_ptr(), 0) == ERR_NO_BASES
        c.set_bases(points[:64 * n])
        # n == 0: nothing written
        out.raw = b"\x5a" * len(out.raw)
        assert L.msm_hip_mul_each(h, s, 0, out, 0) == 0 and L.msm_hip_mul_base(h, 0, None, 0, None, 0) == 0
        assert out.raw == b"\x5a" * len(out.raw)
        # null pointers with n > 0
        assert L.msm_hip_mul_each(h, None, n, out, 0) == ERR_INVALID_ARG
        assert L.msm_hip_mul_each(h, s, n, None, 0) == ERR_INVALID_ARG
        assert L.msm_hip_mul_base_device(h, 0, None, n, d_out.data_ptr(), 0) == ERR_INVALID_ARG
        assert L.msm_hip_mul_each_device(h, d_s.data_ptr(), n, None, 0) == ERR_INVALID_ARG
        # more outputs than bases (mul_each only), a base index beyond the set
        assert L.msm_hip_mul_each(h, s, n + 1, out, 0) == ERR_INVALID_ARG
        assert L.msm_hip_mul_base(h, 0, s, n + 1, out, 0) == 0
        assert out.raw[:64 * (n + 1)] == expected(cpu, points[:64] * (n + 1), s)
        assert L.msm_hip_mul_base(h, n, s, n, out, 0) == ERR_INVALID_ARG
        assert L.msm_hip_mul_base_device(h, n, d_s.data_ptr(), n, d_out.data_ptr(), 0) == ERR_INVALID_ARG
        # an unknown flag bit
        assert L.msm_hip_mul_each(h, s, n, out, 2) == ERR_INVALID_ARG
        assert L.msm_hip_mul_base(h, 0, s, n, out, 0x80000000) == ERR_INVALID_ARG
        # output and scalar ranges that overlap: the output starts inside the scalars, and the scalars inside the output
        both = torch.zeros(96 * n + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.msm_hip_mul_each_device(h, both.data_ptr(), n, both.data_ptr() + 32 * n - 16, 0) == ERR_INVALID_ARG
        assert L.msm_hip_mul_each_device(h, both.data_ptr() + 64 * n - 16, n, both.data_ptr(), 0) == ERR_INVALID_ARG
        assert L.msm_hip_mul_each_device(h, both.data_ptr(), n, both.data_ptr() + 32 * n, 0) == 0  # back to back is fine
        hb = C.create_string_buffer(96 * n)
        base = C.addressof(hb)
        assert L.msm_hip_mul_each(h, C.cast(base, C.c_char_p), n, C.cast(base + 32 * n - 1, C.c_char_p), 0) == ERR_INVALID_ARG
        # the flag of the cofactor curves is accepted and ignored on a curve of prime order
        assert L.msm_hip_mul_each(h, s, n, out, 1) == 0 and out.raw[:64 * n] == want[:64 * n]
        assert c.mul_each(scalars[:32 * n], bases_order_r=True) == want[:64 * n] and c.mul_last()[0] == PATH_ENDO
        # narrow, signed and 128-bit formats: the Python layer refuses, and so does the library
        for width, signed in ((1, False), (2, False), (4, True), (8, False), (16, False), (16, True)):
            c.set_scalar_format(width=width, signed=signed)
            with pytest.raises(ValueError):
                c.mul_each(scalars[:32 * n])
            assert L.msm_hip_mul_each(h, s, n, out, 0) == ERR_INVALID_ARG
            assert L.msm_hip_mul_base_device(h, 0, d_s.data_ptr(), n, d_out.data_ptr(), 0) == ERR_INVALID_ARG
        c.set_scalar_format()
        assert c.mul_each(scalars[:32 * n]) == want[:64 * n]
    finally:
        c.close()


def test_the_plain_ladder_on_a_curve_of_prime_order(gpu, bn254_inputs):
    # BN254's policy always picks the endomorphism; the test hook runs the plain ladder over the same inputs, edge scalars included
    points, scalars, want = bn254_inputs
    n = 2049
    c = m.MsmContext(0)
    try:
        c.set_bases(points[:64 * n])
        c.mul_force_ladder(1)
        assert c.mul_each(dev_u8(scalars[:32 * n], 32)).cpu().numpy().tobytes() == want[:64 * n]
        assert c.mul_last()[0] == PATH_PLAIN
        c.mul_force_ladder(0)
        assert c.mul_each(scalars[:32 * n]) == want[:64 * n] and c.mul_last()[0] == PATH_ENDO
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- mul_base
def test_mul_base_ladder_and_table_at_every_digit_width(gpu, bn254_inputs):
    # the first base, the last base; the table forbidden (the broadcast ladder) and forced at C = 8, 12, 16; n = 1, 4097, 20 000
    points, scalars, _ = bn254_inputs
    nb = 100
    big = scalar_vector(cpu, bn254_ref, 20000, 2003)
    c = m.MsmContext(0)
    try:
        c.set_bases(points[:64 * nb], endomorphism=True)
        for index, sizes in ((0, (1, 4097, 20000)), (nb - 1, (1, 4097))):
            p = points[64 * index:64 * index + 64]
            w_all = expected(cpu, p * sizes[-1], big[:32 * sizes[-1]])
            for n in sizes:
                w = w_all[:64 * n]
                c.mul_policy("never")
                assert c.mul_base(index, big[:32 * n]) == w, (index, n, "ladder, host")
                assert c.mul_last() == (PATH_ENDO, 0, 16)
                assert c.mul_base(index, dev_u8(big[:32 * n], 32)).cpu().numpy().tobytes() == w, (index, n, "ladder, device")
                for bits in (8, 12, 16):
                    c.mul_policy(1, bits)
                    assert c.mul_base(index, big[:32 * n]) == w, (index, n, bits, "table, host")
                    assert c.mul_last()[1] == bits and c.mul_last()[0] in (PATH_TABLE_HELD, PATH_TABLE_BUILT)
                    assert c.mul_base(index, dev_u8(big[:32 * n], 32)).cpu().numpy().tobytes() == w, (index, n, bits, "table, device")
                    assert c.mul_last() == (PATH_TABLE_HELD, bits, 16)
                c.set_scalar_format(mont256=True)
                assert c.mul_base(index, dev_u8(to_mont256(big[:32 * n], R), 32)).cpu().numpy().tobytes() == w, (index, n, "table, mont256")
                c.set_scalar_format()
        # a scalar >= r through the table path, and the context afterwards
        c.mul_policy(1, 8)
        with pytest.raises(m.MsmHipError) as e:
            c.mul_base(0, big[:64] + b32(R) + big[64:128])
        assert e.value.code == ERR_NONCANONICAL
        assert c.mul_base(0, big[:64]) == expected(cpu, points[:64] * 2, big[:64])
        c.mul_policy(0, 0)
    finally:
        c.close()


def test_mul_base_table_cache_and_policy(gpu, bn254_inputs):
    points, scalars, _ = bn254_inputs
    nb, n = 10, 300
    s = scalars[:32 * n]
    want = [expected(cpu, points[64 * i:64 * i + 64] * n, s) for i in (0, 1)]
    c = m.MsmContext(0)
    try:
        c.set_bases(points[:64 * nb])
        c.mul_policy(1, 8)
        assert c.mul_base(0, s) == want[0] and c.mul_last()[:2] == (PATH_TABLE_BUILT, 8)
        assert c.mul_base(0, s) == want[0] and c.mul_last()[:2] == (PATH_TABLE_HELD, 8)     # the same key: the table is reused
        assert c.mul_base(1, s) == want[1] and c.mul_last()[:2] == (PATH_TABLE_BUILT, 8)    # another base: rebuilt
        assert c.mul_base(1, s) == want[1] and c.mul_last()[:2] == (PATH_TABLE_HELD, 8)
        c.mul_policy(1, 9)
        assert c.mul_base(1, s) == want[1] and c.mul_last()[:2] == (PATH_TABLE_BUILT, 9)    # another digit width: rebuilt
        assert c.mul_each(scalars[:32 * nb]) == expected(cpu, points[:64 * nb], scalars[:32 * nb])  # mul_each leaves the table alone
        assert c.mul_base(1, s) == want[1] and c.mul_last()[:2] == (PATH_TABLE_HELD, 9)
        c.set_bases(points[64:64 * nb])                                                       # a new base set drops it: base 0 is now the old base 1
        assert c.mul_base(0, s) == want[1] and c.mul_last()[:2] == (PATH_TABLE_BUILT, 9)
        # the policy itself: a few outputs run the ladder, many run a table, and a held table is reused even for a few
        c.mul_policy(0, 0)
        c.set_bases(points[:64 * nb])
        assert c.mul_base(0, s) == want[0] and c.mul_last()[:2] == (PATH_ENDO, 0)
        nmany = (1 << 17) + 5  # from 2^17 outputs on the policy builds a table, of 12-bit digits
        many = scalar_vector(cpu, bn254_ref, nmany, 2003)
        assert c.mul_base(0, dev_u8(many[:32 * (nmany - 6)], 32)) is not None and c.mul_last()[:2] == (PATH_ENDO, 0)  # (2^17 - 1: still the ladder)
        got = c.mul_base(0, dev_u8(many, 32))
        assert c.mul_last()[:2] == (PATH_TABLE_BUILT, 12)
        got = got.cpu().numpy().tobytes()
        assert got[:64 * 2000] == expected(cpu, points[:64] * 2000, many[:32 * 2000])
        assert got[-64 * 200:] == expected(cpu, points[:64] * 200, many[-32 * 200:])
        assert c.mul_base(0, s) == want[0] and c.mul_last()[:2] == (PATH_TABLE_HELD, 12)   # a held table serves a few outputs too
        # hook arguments
        assert m.lib().msm_hip_test_mul_policy(c._h, 1, 3) == ERR_INVALID_ARG and m.lib().msm_hip_test_mul_policy(c._h, 1, 17) == ERR_INVALID_ARG
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- the other curves
@pytest.mark.parametrize("curve", OTHER_CURVES)
def test_other_curves(gpu, curve):
    orc, ref = oracle_module(curve), ref_module(curve)
    n = {"bls12_381_g2": 300, "bn254_g2": 600, "bls12_381": 1000}.get(curve, 2000)
    nbase = n // 4
    c = m.MsmContext(0, curve=curve)
    try:
        pb = c.pb
        sampled = c.sample_points(n, 3000 + OTHER_CURVES.index(curve)).cpu().numpy().tobytes()  # (BLS12-381 G1: on the curve; G2: in the subgroup)
        scalars = scalar_vector(orc, ref, n, 3010 + OTHER_CURVES.index(curve))
        w_sampled = expected(orc, sampled, scalars)
        # with the flag the caller vouches for the order of the bases: multiples of the generator on BLS12-381 G1, whose sampler does not promise it
        sub = subgroup_points_bls12_381(3020, n) if curve == "bls12_381" else sampled
        cases = [(sampled, w_sampled, False), (sub, w_sampled if sub is sampled else expected(orc, sub, scalars), True)]
        for points, w, order_r in cases:
            path = PATH_ENDO if (curve in PRIME_ORDER or order_r) else PATH_PLAIN
            c.set_bases(points, endomorphism=None if curve in PRIME_ORDER else False)
            assert c.mul_each(scalars, bases_order_r=order_r) == w, (curve, order_r, "host")
            assert c.mul_last()[0] == path
            assert c.mul_each(dev_u8(scalars, 32), bases_order_r=order_r).cpu().numpy().tobytes() == w, (curve, order_r, "device")
            for index in (0, n - 1):
                wb = expected(orc, points[pb * index:pb * index + pb] * nbase, scalars[:32 * nbase])
                assert c.mul_base(index, scalars[:32 * nbase], bases_order_r=order_r) == wb, (curve, order_r, index)
                assert c.mul_last()[0] == path
                c.mul_policy(1, 8)   # ... and through the fixed-base table (built by the ladder of this case)
                assert c.mul_base(index, dev_u8(scalars[:32 * nbase], 32), bases_order_r=order_r).cpu().numpy().tobytes() == wb, (curve, order_r, index, "table")
                assert c.mul_last()[:2] == (PATH_TABLE_BUILT, 8)
                c.mul_policy(0, 0)
        # the outputs parse as points of the curve's wire format, the zero scalar's as None
        got = m.bytes_to_points(w[:4 * pb], curve)
        assert got[0] is None and all(pt is not None for pt in got[1:])
    finally:
        c.close()


def test_bls12_381_default_ladder_outside_the_subgroup(gpu):
    # a point on the curve whose order is not r: the default (plain) ladder gives the integer multiple, as the oracle's double-and-add does
    orc, ref = oracle_module("bls12_381"), ref_module("bls12_381")
    c = m.MsmContext(0, curve="bls12_381")
    try:
        pts = ref.bytes_to_points(c.sample_points(8, 3100).cpu().numpy().tobytes())
        outside = [pt for pt in pts if ref.add(ref.mul(ref.R - 1, pt), pt) is not None]
        assert outside
        p = ref.points_to_bytes([outside[0]])
        ks = [1, 2, 3, ref.R - 1, ref.R - 2, (1 << 254) + 5, 0x1234567 << 200]
        sc = b"".join(b32(k) for k in ks)
        want = b"".join(ref.affine_to_bytes64(ref.mul(k, outside[0])) for k in ks)  # (k < r: ref.mul is the integer multiple)
        assert want == expected(orc, p * len(ks), sc)
        c.set_bases(p)
        assert c.mul_base(0, sc) == want and c.mul_last()[0] == PATH_PLAIN
        c.mul_policy(1, 10)  # the table built by the plain ladder holds integer multiples too
        assert c.mul_base(0, sc) == want and c.mul_last()[:2] == (PATH_TABLE_BUILT, 10)
        c.mul_policy(0, 0)
        c.set_bases(p * len(ks))
        assert c.mul_each(dev_u8(sc, 32)).cpu().numpy().tobytes() == want
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- into set_bases and back
def test_device_output_feeds_set_bases(gpu, bn254_inputs):
    points, scalars, _ = bn254_inputs
    n = 4097
    rng = np.random.default_rng(5)
    s = [int.from_bytes(scalars[32 * i:32 * i + 32], "little") for i in range(n)]
    cc = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    a, b = m.MsmContext(0), m.MsmContext(0)
    try:
        a.set_bases(points[:64 * n], endomorphism=True)
        q = a.mul_each(dev_u8(scalars[:32 * n], 32))
        assert not q[0].any()  # (scalar 0 of the planted edges is 0: an identity record among the new bases)
        b.set_bases(q, zero_is_identity=True, endomorphism=True)
        got = b.msm(b"".join(b32(v) for v in cc))
        assert got == a.msm(b"".join(b32(x * y % R) for x, y in zip(cc, s)))
    finally:
        a.close()
        b.close()


def test_real_size_through_a_random_combination(gpu):
    """n = 2^20 + 3 on BN254: an elementwise oracle would need five minutes, so the n outputs Q_i are checked through sum_i c_i Q_i for seeded
    uniform 254-bit c_i, against sum_i (c_i s_i mod r) P_i (mul_each) and (sum_i c_i s_i mod r) G (mul_base).  If some Q_i is wrong, the
    difference of the two sides is a nonzero combination of the c_i of the wrong outputs: it vanishes for a fraction of about 1 / r ~ 2^-254 of
    the choices of c.  Both MSMs run through the library's existing MSM path, which the other suites pin against the oracle; the second is also
    compared with the oracle itself on a slice of 2^16."""
    n = (1 << 20) + 3
    a, b = m.MsmContext(0), m.MsmContext(0)
    try:
        pts = a.sample_points(n, 4001)
        s_dev = a.sample_scalars(n, 4002)
        s_dev[::1000] = 0  # every 1000th scalar is zero: identity outputs among the rest
        c_dev = a.sample_scalars(n, 4003)
        s_np, c_np = s_dev.cpu().numpy(), c_dev.cpu().numpy()
        s = [int.from_bytes(row.tobytes(), "little") for row in s_np]
        cc = [int.from_bytes(row.tobytes(), "little") for row in c_np]
        cs = b"".join(b32(x * y % R) for x, y in zip(cc, s))
        a.set_bases(pts, endomorphism=True)
        q = a.mul_each(s_dev)
        zero_rows = (q.view(torch.int64).reshape(n, 8) == 0).all(dim=1)
        assert int(zero_rows.sum()) == len(range(0, n, 1000)) and bool(zero_rows[::1000].all())
        b.set_bases(q, zero_is_identity=True, endomorphism=True)
        direct = a.msm(cs)
        assert b.msm(c_dev) == direct
        k = 1 << 16
        pts_host = pts[:k].cpu().numpy().tobytes()
        a.set_bases(pts[:k].contiguous(), endomorphism=True)
        assert a.msm(cs[:32 * k]).to_affine_bytes() == cpu.to_affine64(cpu.cpu_msm(pts_host, cs[:32 * k], n_threads=16))
        # mul_base: every output a multiple of one base
        g = pts_host[:64]
        a.set_bases(g)
        qb = a.mul_base(0, s_dev)
        assert a.mul_last()[0] == PATH_TABLE_BUILT  # (2^20 outputs of one base: the policy's table)
        b.set_bases(qb, zero_is_identity=True, endomorphism=True)
        total = sum(x * y for x, y in zip(cc, s)) % R
        assert b.msm(c_dev).to_affine_bytes() == expected(cpu, g, b32(total))
    finally:
        a.close()
        b.close()
