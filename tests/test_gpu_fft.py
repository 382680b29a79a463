"""Group FFT over the resident bases on the device (include/msm_hip.h: msm_hip_bases_fft): out[i] = c * sum_j omega^(i j) P_j.
Two independent references, both bit for bit.  The exponent model: with P_j = c_j G the transform is the number-theoretic transform of the c_j in
the exponent, out[i] = NTT(c)[i] G -- a Python-integer NTT, then the oracle's g1_scalar_mul and to_affine64.  The definition itself on points
with no known relation: every output against the oracle's MSM over the powers of omega.  The bases of the exponent model are computed once (the
largest size; a smaller size takes their prefix as its own base set)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from oracle import bn254_ref, cpu
from tests.util import rng

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_NO_BASES = -2, -6
MODES = {"plain": dict(endomorphism=False), "endomorphism": dict(endomorphism=True), "tables": dict(precompute=True), "wide": dict(precompute="wide")}
R = bn254_ref.R
LADDER_NONE, LADDER_PLAIN, LADDER_ENDO = 0, 1, 2
MAX_LOG_N = 13


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


def dev_bytes(t):
    return t.cpu().numpy().tobytes()


def multiples_of_g(curve, ks):
    """[k G] as affine records, the identity (k = 0 mod r) as zeros: the oracle's scalar multiplication and its affine conversion"""
    orc, ref = oracle_module(curve), ref_module(curve)
    jb = 3 * orc.coord_bytes()
    jac = orc.g1_scalar_mul(ref.points_to_bytes([ref.G]) * len(ks), b"".join(b32(k) for k in ks))
    return b"".join(orc.to_affine64(jac[i:i + jb]) for i in range(0, len(jac), jb))


def ntt(c, omega, r):
    """[sum_j c_j omega^(i j) mod r] over Python integers (recursive radix 2; len(c) a power of two)"""
    n = len(c)
    if n == 1:
        return [c[0] % r]
    even, odd = ntt(c[0::2], omega * omega % r, r), ntt(c[1::2], omega * omega % r, r)
    out, w = [0] * n, 1
    for i in range(n // 2):
        t = w * odd[i] % r
        out[i], out[i + n // 2] = (even[i] + t) % r, (even[i] - t) % r
        w = w * omega % r
    return out


def intt(c, omega, r):
    n_inv = pow(len(c), r - 2, r)
    return [v * n_inv % r for v in ntt(c, pow(omega, r - 2, r), r)]


def test_the_python_ntt_is_the_definition():
    w = api.root_of_unity("bn254", 3)
    c = [rng(1).randrange(R) for _ in range(8)]
    assert ntt(c, w, R) == [sum(c[j] * pow(w, i * j, R) for j in range(8)) % R for i in range(8)]
    assert intt(ntt(c, w, R), w, R) == c


# ---------------------------------------------------------------------------------------------------------------- the exponent model on BN254
@pytest.fixture(scope="module")
def bn254_exponents(gpu):
    """coefficients c_j (nonzero) and the bases c_j G for the largest size"""
    rnd = rng(4001)
    c = [rnd.randrange(1, R) for _ in range(1 << MAX_LOG_N)]
    return c, multiples_of_g("bn254", c)


# every stage count up to the first with a non-trivial twiddle (0 .. 4), one and two workgroups of butterflies (9, 10)
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 9, 10])
def test_exponent_model_forward_and_inverse_from_every_output_form(gpu, bn254_exponents, log_n):
    c, bases = bn254_exponents
    n = 1 << log_n
    w = api.root_of_unity("bn254", log_n)
    want_fwd = multiples_of_g("bn254", ntt(c[:n], w, R))
    want_inv = multiples_of_g("bn254", intt(c[:n], w, R))
    ctx = m.MsmContext(0)
    try:
        ctx.set_bases(bases[:64 * n])
        assert ctx.bases_fft(w, log_n) == want_fwd, (log_n, "forward, host")
        assert ctx.fft_last() == (log_n, LADDER_ENDO if log_n >= 2 else LADDER_NONE)
        assert ctx.bases_fft(b32(w)) == want_fwd, (log_n, "omega as bytes, log_n from the bases")
        out = ctx.bases_fft(w, log_n, device=True)
        assert tuple(out.shape) == (n, 64) and out.dtype == torch.uint8 and out.is_cuda
        assert dev_bytes(out) == want_fwd, (log_n, "forward, device")
        pre = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        assert ctx.bases_fft(w, log_n, out=pre) is pre and dev_bytes(pre) == want_fwd, (log_n, "forward, out=")
        w_inv = api.root_of_unity("bn254", log_n, inverse=True)
        assert ctx.bases_fft(w_inv, log_n, scale=True) == want_inv, (log_n, "inverse with the scale, host")
        assert ctx.fft_last() == (log_n, LADDER_ENDO if log_n >= 1 else LADDER_NONE)
        assert ctx.lagrange_bases() == want_inv
        pre.fill_(0x5A)
        assert ctx.lagrange_bases(log_n, out=pre) is pre and dev_bytes(pre) == want_inv, (log_n, "inverse with the scale, out=")
        assert dev_bytes(ctx.bases_fft(w_inv, log_n, scale=True, device=True)) == want_inv
        # the scale alone (forward transform, 1 / n) and the forced plain ladder
        if log_n <= 4:
            n_inv = pow(n, R - 2, R)
            assert ctx.bases_fft(w, log_n, scale=True) == multiples_of_g("bn254", [v * n_inv % R for v in ntt(c[:n], w, R)]), (log_n, "forward with the scale")
        if log_n in (3, 9):
            ctx.mul_force_ladder(1)
            assert ctx.bases_fft(w_inv, log_n, scale=True) == want_inv, (log_n, "plain ladder")
            assert ctx.fft_last() == (log_n, LADDER_PLAIN)
            ctx.mul_force_ladder(0)
        with pytest.raises(ValueError):
            ctx.bases_fft(w, log_n, out=torch.empty((n + 1, 64), dtype=torch.uint8, device="cuda"))
        assert ctx.mul_each(b32(1) * n) == bases[:64 * n]  # the resident bases are not modified
    finally:
        ctx.close()


def test_past_one_normalisation_block_and_the_round_trips(gpu, bn254_exponents):
    # 2^13 records go past one 4096-record block of the normalisation.  Forward against the exponent model; then the output as the next base
    # set, the inverse with the scale gives the bases back -- here and at 2^10
    c, bases = bn254_exponents
    ctx = m.MsmContext(0)
    try:
        for log_n in (MAX_LOG_N, 10):
            n = 1 << log_n
            w = api.root_of_unity("bn254", log_n)
            ctx.set_bases(bases[:64 * n])
            out = ctx.bases_fft(w, log_n, device=True)
            if log_n == MAX_LOG_N:
                assert dev_bytes(out) == multiples_of_g("bn254", ntt(c, w, R))
            ctx.set_bases(out, zero_is_identity=True)
            back = ctx.bases_fft(api.root_of_unity("bn254", log_n, inverse=True), log_n, scale=True, device=True)
            assert dev_bytes(back) == bases[:64 * n], log_n
    finally:
        ctx.close()


def test_a_prefix_of_the_bases(gpu, bn254_exponents):
    c, bases = bn254_exponents
    ctx = m.MsmContext(0)
    try:
        ctx.set_bases(bases[:64 * 1000])  # (not a power of two)
        for log_n in (4, 9):
            w = api.root_of_unity("bn254", log_n)
            assert ctx.bases_fft(w, log_n) == multiples_of_g("bn254", ntt(c[:1 << log_n], w, R)), log_n
        with pytest.raises(ValueError):
            ctx.bases_fft(api.root_of_unity("bn254", 9))  # log_n=None: all the bases
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the definition itself
@pytest.fixture(scope="module")
def unrelated(gpu):
    """16 sampled points and, per log_n <= 4 and direction, [sum_j omega^(i j) P_j] from the oracle's MSM"""
    points = cpu.sample_points(4101, 16)
    want = {}
    for log_n in range(5):
        n = 1 << log_n
        w = api.root_of_unity("bn254", log_n)
        want[log_n] = b"".join(cpu.to_affine64(cpu.cpu_msm(points[:64 * n], b"".join(b32(pow(w, i * j, R)) for j in range(n)))) for i in range(n))
    return points, want


@pytest.mark.parametrize("mode", list(MODES))
def test_definition_on_unrelated_points_in_every_base_mode(gpu, unrelated, mode):
    points, want = unrelated
    ctx = m.MsmContext(0)
    try:
        ctx.set_bases(points, **MODES[mode])  # 16 bases: every size below is a prefix except the last
        for log_n in range(5):
            w = api.root_of_unity("bn254", log_n)
            assert ctx.bases_fft(w, log_n) == want[log_n], (mode, log_n)
            assert dev_bytes(ctx.bases_fft(w, log_n, device=True)) == want[log_n], (mode, log_n, "device")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- degenerate inputs
@pytest.mark.parametrize("log_n", [1, 2, 3])
def test_degenerate_inputs(gpu, log_n):
    n = 1 << log_n
    w = api.root_of_unity("bn254", log_n)
    rnd = rng(4200 + log_n)
    ctx = m.MsmContext(0)
    try:
        # all bases equal: (n P, 0, ..., 0) -- a doubling in stage 0, then identity operands into the later ladders
        k = rnd.randrange(1, R)
        p = multiples_of_g("bn254", [k])
        ctx.set_bases(p * n)
        out = ctx.bases_fft(w, log_n)
        assert out == multiples_of_g("bn254", [n * k % R]) + bytes(64 * (n - 1))
        # ... and that output as a base set: the identity records carry no weight in an MSM
        ctx.set_bases(out, zero_is_identity=True)
        s = [rnd.randrange(R) for _ in range(n)]
        assert ctx.msm(b"".join(b32(v) for v in s)) == m.G1(cpu.g1_scalar_mul(out[:64], b32(s[0])))
        # (X - omega^k) q(X) for random q: every coefficient nonzero, output k the identity -- met in the last stage as a == -t (k < n / 2) or
        # a == t (k >= n / 2) through the twiddle omega^(k mod n/2), its partner a doubling
        for kk in range(n):
            q = [rnd.randrange(1, R) for _ in range(n - 1)]
            root = pow(w, kk, R)
            coeffs = [(-root * q[0]) % R] + [(q[j - 1] - root * q[j]) % R for j in range(1, n - 1)] + [q[n - 2]]
            assert len(coeffs) == n and all(coeffs)
            evals = ntt(coeffs, w, R)
            assert evals[kk] == 0 and sum(1 for v in evals if v == 0) == 1
            ctx.set_bases(multiples_of_g("bn254", coeffs))
            want = multiples_of_g("bn254", evals)
            assert want[64 * kk:64 * kk + 64] == bytes(64)
            assert ctx.bases_fft(w, log_n) == want, (log_n, kk)
            assert dev_bytes(ctx.bases_fft(w, log_n, device=True)) == want, (log_n, kk, "device")
        # identity records among the input (MSM_HIP_BASES_ZERO_IS_IDENTITY): every subset of positions at n = 2, 4; seeded ones at n = 8
        subsets = range(1, 1 << n) if n <= 4 else [rnd.randrange(1, 1 << n) for _ in range(12)] + [(1 << n) - 1, 0x55, 0xAA, 0x0F, 0xF0]
        coeffs = [rnd.randrange(1, R) for _ in range(n)]
        recs = multiples_of_g("bn254", coeffs)
        for mask in subsets:
            cz = [0 if (mask >> j) & 1 else coeffs[j] for j in range(n)]
            ctx.set_bases(b"".join(bytes(64) if (mask >> j) & 1 else recs[64 * j:64 * j + 64] for j in range(n)), zero_is_identity=True)
            want = multiples_of_g("bn254", ntt(cz, w, R))
            assert ctx.bases_fft(w, log_n) == want, (log_n, bin(mask))
            assert ctx.bases_fft(pow(w, R - 2, R), log_n, scale=True) == multiples_of_g("bn254", intt(cz, w, R)), (log_n, bin(mask), "inverse")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the use it is for
def test_commitment_from_evaluations_over_the_lagrange_bases(gpu):
    # the monomial SRS tau^j G from mul_base, its Lagrange form from lagrange_bases, both as base sets on the device:
    # msm(lagrange, evaluations of f) == msm(monomial, coefficients of f) == f(tau) G
    log_n = 10
    n = 1 << log_n
    rnd = rng(4300)
    tau = rnd.randrange(2, R)
    coeffs = [rnd.randrange(R) for _ in range(n)]
    evals = ntt(coeffs, api.root_of_unity("bn254", log_n), R)
    ctx = m.MsmContext(0)
    try:
        ctx.set_bases(multiples_of_g("bn254", [1]))
        powers = torch.from_numpy(np.frombuffer(b"".join(b32(pow(tau, j, R)) for j in range(n)), dtype=np.uint8).copy()).cuda().reshape(n, 32)
        srs = ctx.mul_base(0, powers)
        ctx.set_bases(srs, zero_is_identity=True)
        by_coeffs = ctx.msm(b"".join(b32(v) for v in coeffs))
        lagrange = ctx.lagrange_bases(device=True)
        assert ctx.fft_last() == (log_n, LADDER_ENDO)
        ctx.set_bases(lagrange, zero_is_identity=True)
        by_evals = ctx.msm(b"".join(b32(v) for v in evals))
        f_tau = sum(cf * pow(tau, j, R) for j, cf in enumerate(coeffs)) % R
        want = m.G1(cpu.g1_scalar_mul(multiples_of_g("bn254", [1]), b32(f_tau)))
        assert by_coeffs == want and by_evals == want
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the other curves
@pytest.mark.parametrize("curve,log_n,order_r", [("pallas", 5, False), ("vesta", 5, False), ("bls12_381", 5, False), ("bls12_381", 5, True), ("grumpkin", 1, False)])
def test_other_curves_against_the_exponent_model(gpu, curve, log_n, order_r):
    ref = ref_module(curve)
    r = ref.R
    n = 1 << log_n
    rnd = rng(4400)
    c = [rnd.randrange(1, r) for _ in range(n)]
    w = api.root_of_unity(curve, log_n)
    ctx = m.MsmContext(0, curve)
    try:
        ctx.set_bases(multiples_of_g(curve, c))  # (points of the subgroup of order r)
        assert ctx.bases_fft(w, log_n, bases_order_r=order_r) == multiples_of_g(curve, ntt(c, w, r)), (curve, "forward")
        ladder = LADDER_ENDO if order_r or curve != "bls12_381" else LADDER_PLAIN
        assert ctx.fft_last() == (log_n, ladder if log_n >= 2 else LADDER_NONE)
        out = ctx.lagrange_bases(bases_order_r=order_r, device=True)
        assert dev_bytes(out) == multiples_of_g(curve, intt(c, w, r)), (curve, "inverse with the scale")
        assert ctx.fft_last() == (log_n, ladder)
        if curve == "grumpkin":  # 2-adicity 1: nothing passes for omega at n = 4
            ctx.set_bases(multiples_of_g(curve, c + c))
            for omega in (1, r - 1, 2, rnd.randrange(r)):
                with pytest.raises(m.MsmHipError) as e:
                    ctx.bases_fft(omega, 2)
                assert e.value.code == ERR_INVALID_ARG
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", ["bn254_g2", "bls12_381_g2"])
def test_g2_contexts_are_refused(gpu, curve):
    orc = oracle_module(curve)
    ctx = m.MsmContext(0, curve)
    try:
        for with_bases in (False, True):
            if with_bases:
                ctx.set_bases(orc.sample_points(4500, 2))
            with pytest.raises(m.MsmHipError) as e:
                ctx.bases_fft(api.SCALAR_FIELDS[curve[:-3]] - 1, 1)
            assert e.value.code == ERR_INVALID_ARG
            with pytest.raises(m.MsmHipError) as e:
                ctx.bases_fft(1, 0, device=True)
            assert e.value.code == ERR_INVALID_ARG
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_output_untouched(gpu, bn254_exponents):
    c, bases = bn254_exponents
    L = m.lib()
    ctx = m.MsmContext(0)
    try:
        w3 = api.root_of_unity("bn254", 3)
        host = C.create_string_buffer(b"\xa5" * (64 * 16), 64 * 16)
        dev = torch.full((16, 64), 0xA5, dtype=torch.uint8, device="cuda")

        def both(omega, log_n, flags, want):
            wb = omega if isinstance(omega, bytes) else b32(omega)
            assert L.msm_hip_bases_fft(ctx._h, wb, log_n, host, flags) == want, (omega, log_n, flags)
            assert L.msm_hip_bases_fft_device(ctx._h, wb, log_n, dev.data_ptr(), flags) == want, (omega, log_n, flags, "device")
            torch.cuda.synchronize()
            assert host.raw == b"\xa5" * (64 * 16) and dev_bytes(dev) == b"\xa5" * (64 * 16)

        both(w3, 3, 0, ERR_NO_BASES)                         # no bases yet
        ctx.set_bases(bases[:64 * 8])
        both(w3 * w3 % R, 3, 0, ERR_INVALID_ARG)             # order 4, not 8
        both(1, 3, 0, ERR_INVALID_ARG)                       # omega = 1 for n >= 2
        both(R - 1, 0, 0, ERR_INVALID_ARG)                   # n = 1: omega must be 1
        both(api.root_of_unity("bn254", 4), 3, 0, ERR_INVALID_ARG)   # order 16
        both(rng(4600).randrange(2, R), 3, 0, ERR_INVALID_ARG)       # no root of unity of that order at all
        both(w3 + R, 3, 0, ERR_INVALID_ARG)                  # omega >= r, although it is a primitive root mod r
        both(R, 0, 0, ERR_INVALID_ARG)
        both(b"\xff" * 32, 3, 0, ERR_INVALID_ARG)
        both(api.root_of_unity("bn254", 4), 4, 0, ERR_INVALID_ARG)   # 2^log_n > n_bases
        both(w3, -1, 0, ERR_INVALID_ARG)                     # log_n < 0
        both(api.root_of_unity("bn254", 28), 29, 0, ERR_INVALID_ARG)
        for flags in (4, 8, 0x80000000, 7):                  # unknown flag bits
            both(w3, 3, flags, ERR_INVALID_ARG)
        assert L.msm_hip_bases_fft(ctx._h, b32(w3), 3, None, 0) == ERR_INVALID_ARG               # a null output ...
        assert L.msm_hip_bases_fft_device(ctx._h, b32(w3), 3, None, 0) == ERR_INVALID_ARG
        assert L.msm_hip_bases_fft_device(ctx._h, b32(w3), 3, dev.data_ptr() + 4, 0) == ERR_INVALID_ARG   # ... and a misaligned one
        assert L.msm_hip_bases_fft(ctx._h, None, 3, host, 0) == ERR_INVALID_ARG                  # a null omega
        torch.cuda.synchronize()
        assert host.raw == b"\xa5" * (64 * 16) and dev_bytes(dev) == b"\xa5" * (64 * 16)
        # the context stays usable, and the Python mirror raises the same code
        with pytest.raises(m.MsmHipError) as e:
            ctx.bases_fft(1, 3)
        assert e.value.code == ERR_INVALID_ARG
        assert ctx.bases_fft(w3, 3) == multiples_of_g("bn254", ntt(c[:8], w3, R))
        for flags in (1, 3):  # MSM_HIP_MUL_BASES_ORDER_R is accepted (and ignored on a curve of prime order), alone and with the scale
            assert L.msm_hip_bases_fft(ctx._h, b32(w3), 3, host, flags) == 0
    finally:
        ctx.close()
