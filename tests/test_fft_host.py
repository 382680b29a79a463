"""CPU build (g++ -DFQ_CHECK) of what the group FFT over the resident bases (msm_hip_bases_fft) adds to csrc/scalar_mul.h -- the butterfly that
k_fft_stage inlines and the normalisation that keeps Montgomery records -- on the five G1 curves, every limb bound and every Montgomery result
asserted, against the oracle's g1_scalar_mul and g1_op; and of csrc/host_fr.h, the host's twiddle arithmetic, against Python's pow.  Host logic only."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msm-webgpu_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_harness", "fft_harness.cpp")

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
}
LADDER_NONE, LADDER_PLAIN, LADDER_ENDO = 0, 1, 2
_built = {}


def harness(tmp_path_factory, curve):
    if curve not in _built:
        so = str(tmp_path_factory.mktemp("fft_" + curve) / "fft_harness.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-fPIC", "-shared"] + CURVES[curve][0] + ["-I", CSRC, SRC, "-o", so])
        H = C.CDLL(so)
        H.h_fft_butterfly.restype = None
        H.h_fft_butterfly.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p]
        H.h_fft_normalize.restype = None
        H.h_fft_normalize.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p]
        H.h_fr_is_primitive_root.argtypes = [C.c_char_p, C.c_int]
        H.h_fr_twiddles.restype = None
        H.h_fr_twiddles.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
        H.h_fr_inverse_of_n.restype = None
        H.h_fr_inverse_of_n.argtypes = [C.c_int, C.c_char_p]
        _built[curve] = H
    return _built[curve], importlib.import_module(CURVES[curve][1]), importlib.import_module(CURVES[curve][2])


def b32(v):
    return int(v).to_bytes(32, "little")


def affine(cx, jac):
    jb = 3 * cx.coord_bytes()
    return b"".join(cx.to_affine64(jac[i:i + jb]) for i in range(0, len(jac), jb))


def order_r_points(cx, m, seed, n):
    """n affine points of order r: seeded multiples of the generator (BLS12-381's sampler leaves the subgroup)"""
    ks = b"".join(b32(rng(seed + i).randrange(1, m.R)) for i in range(n))
    return affine(cx, cx.g1_scalar_mul(m.points_to_bytes([m.G]) * n, ks))


def as_jacobian(cx, xy):
    """affine records (all-zero: the identity) -> the oracle's Jacobian records (x, y, 1), Z = 0 for the identity"""
    cb = cx.coord_bytes()
    one = (1).to_bytes(cb, "little")
    return b"".join(bytes(3 * cb) if xy[i:i + 2 * cb] == bytes(2 * cb) else xy[i:i + 2 * cb] + one for i in range(0, len(xy), 2 * cb))


def expected_butterflies(cx, a, b, w):
    """(a_i + w_i b_i, a_i - w_i b_i) interleaved, as affine records: the oracle's scalar multiplication, negation and addition"""
    cb = cx.coord_bytes()
    pb, jb = 2 * cb, 3 * cb
    n = len(w) // 32
    # the oracle's scalar multiplication takes curve points: an identity b is multiplied as some other point and its product replaced by Z = 0
    zero_b = [b[pb * i:pb * i + pb] == bytes(pb) for i in range(n)]
    some = next(b[pb * i:pb * i + pb] for i in range(n) if not zero_b[i])
    b_safe = b"".join(some if zero_b[i] else b[pb * i:pb * i + pb] for i in range(n))
    t = cx.g1_scalar_mul(b_safe, w)
    t = b"".join(bytes(jb) if zero_b[i] else t[jb * i:jb * i + jb] for i in range(n))
    aj = as_jacobian(cx, a)
    s = affine(cx, cx.g1_op("add", aj, t))
    d = affine(cx, cx.g1_op("add", aj, cx.g1_op("negate", t)))
    return b"".join(s[pb * i:pb * i + pb] + d[pb * i:pb * i + pb] for i in range(n))


@pytest.mark.parametrize("curve", list(CURVES))
def test_butterfly_against_the_oracle_with_both_ladders(tmp_path_factory, curve):
    H, cx, m = harness(tmp_path_factory, curve)
    pb = 2 * cx.coord_bytes()
    r_, lam = m.R, m.glv_params()["lam"]
    rnd = rng(300)
    twiddles = [1, r_ - 1, lam, rnd.randrange(2, r_), rnd.randrange(2, r_)]
    pool = order_r_points(cx, m, 310, 12)
    pt = lambda i: pool[pb * (i % 12):pb * (i % 12) + pb]
    ident = bytes(pb)
    a, b, w = [], [], []
    for ti, k in enumerate(twiddles):
        wb = affine(cx, cx.g1_scalar_mul(pt(ti + 5), b32(k)))                                 # w * b
        nwb = affine(cx, cx.g1_op("negate", cx.g1_scalar_mul(pt(ti + 5), b32(k))))            # -w * b
        for ai, bi in ((pt(ti), pt(ti + 5)), (pt(ti + 1), pt(ti + 6)),                        # a, b random
                       (ident, pt(ti + 5)), (pt(ti), ident), (ident, ident),                  # a / b / both the identity
                       (wb, pt(ti + 5)), (nwb, pt(ti + 5))):                                  # a == w b, a == -w b
            a.append(ai), b.append(bi), w.append(b32(k))
    n = len(w)
    a, b, w = b"".join(a), b"".join(b), b"".join(w)
    want = expected_butterflies(cx, a, b, w)
    # the cases the butterfly must meet are really there: per twiddle, a doubling beside an identity in both orders, and identities from identities
    per = 7 * 2 * pb
    for ti in range(len(twiddles)):
        blk = want[per * ti:per * ti + per]
        rec = lambda j: blk[pb * j:pb * j + pb]
        assert rec(8) == ident and rec(9) == ident                       # both the identity
        assert rec(4) != ident and rec(5) != ident and rec(6) == rec(7)  # a the identity: t and -t; b the identity: a and a
        assert rec(10) != ident and rec(11) == ident                     # a == t: doubling, identity
        assert rec(12) == ident and rec(13) != ident                     # a == -t: identity, doubling
    for ladder in (LADDER_PLAIN, LADDER_ENDO):
        for lanes in (1, 3):
            out = C.create_string_buffer(2 * n * pb)
            H.h_fft_butterfly(ladder, a, b, w, n, lanes, out)
            bad = [i for i in range(2 * n) if out.raw[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
            assert not bad, (curve, ladder, lanes, bad[:6])
    # the add-only form of the first stage: the cases with the twiddle 1
    out = C.create_string_buffer(2 * 7 * pb)
    H.h_fft_butterfly(LADDER_NONE, a[:7 * pb], b[:7 * pb], w[:7 * 32], 7, 3, out)
    assert out.raw == want[:2 * 7 * pb], curve


@pytest.mark.parametrize("curve", list(CURVES))
def test_montgomery_keeping_normalisation_against_the_existing_one(tmp_path_factory, curve):
    # Jacobian records with random Z: lengths around the chunk size, identities first, last and as a whole chunk, both lane strides.  The kept
    # records are x R, y R mod p (R = the limb representation's Montgomery radix, recovered from the pair of outputs of the first record) of
    # exactly what the existing normalisation writes, and the identity is the all-zero record in both.
    H, cx, m = harness(tmp_path_factory, curve)
    cb = cx.coord_bytes()
    pb = 2 * cb
    rnd = rng(320)
    chunk = 16
    pts = m.bytes_to_points(cx.sample_points(321, 2 * chunk + 3))

    def jac(pt):
        if pt is None:
            return bytes(3 * cb)
        z = rnd.randrange(1, m.P)
        return b"".join(int(v).to_bytes(cb, "little") for v in (pt[0] * z * z % m.P, pt[1] * z * z * z % m.P, z))

    radix = None
    for lanes in (1, 3):
        for n in (1, chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
            for variant in range(4):
                seq = [pts[i] for i in range(n)]
                if variant == 1:
                    seq[0] = None
                elif variant == 2:
                    seq[-1] = None
                elif variant == 3:
                    seq = [None if chunk <= i < 2 * chunk or i == 0 else q for i, q in enumerate(seq)]
                raw = b"".join(jac(q) for q in seq)
                wire, kept = C.create_string_buffer(pb * n), C.create_string_buffer(pb * n)
                H.h_fft_normalize(0, raw, n, lanes, wire)
                H.h_fft_normalize(1, raw, n, lanes, kept)
                assert wire.raw == b"".join(bytes(pb) if q is None else m.points_to_bytes([q]) for q in seq), (curve, n, lanes, variant)
                for i, q in enumerate(seq):
                    wx, kx = (int.from_bytes(buf.raw[pb * i:pb * i + cb], "little") for buf in (wire, kept))
                    wy, ky = (int.from_bytes(buf.raw[pb * i + cb:pb * i + pb], "little") for buf in (wire, kept))
                    if q is None:
                        assert (kx, ky) == (0, 0)
                        continue
                    if radix is None:
                        radix = kx * pow(wx, m.P - 2, m.P) % m.P
                        assert radix != 1  # (the records really are in Montgomery form)
                    assert kx == wx * radix % m.P and ky == wy * radix % m.P and kx < m.P and ky < m.P, (curve, n, lanes, variant, i)


@pytest.mark.parametrize("curve", list(CURVES))
def test_host_fr_twiddles_inverse_of_n_and_the_check_of_omega(tmp_path_factory, curve):
    H, cx, m = harness(tmp_path_factory, curve)
    r_ = m.R
    two_adicity = ((r_ - 1) & -(r_ - 1)).bit_length() - 1
    g = 2
    while pow(g, (r_ - 1) // 2, r_) != r_ - 1:
        g += 1
    for log_n in (1, 2, 5, 10):
        n = 1 << log_n
        if log_n > two_adicity:  # Grumpkin beyond n = 2: no element of that order at all; an element of smaller order is rejected
            assert H.h_fr_is_primitive_root(b32(r_ - 1), log_n) == 0
            continue
        w = pow(g, (r_ - 1) >> log_n, r_)
        assert H.h_fr_is_primitive_root(b32(w), log_n) == 1
        out = C.create_string_buffer(32 * (n // 2))
        for omega in (w, pow(w, r_ - 2, r_)):
            H.h_fr_twiddles(b32(omega), log_n, out)
            assert out.raw == b"".join(b32(pow(omega, j, r_)) for j in range(n // 2)), (curve, log_n)
        inv = C.create_string_buffer(32)
        H.h_fr_inverse_of_n(log_n, inv)
        assert int.from_bytes(inv.raw, "little") == pow(n, r_ - 2, r_)
        assert H.h_fr_is_primitive_root(b32(1), log_n) == 0                      # omega = 1 for n >= 2
        assert H.h_fr_is_primitive_root(b32(w * w % r_), log_n) == (1 if log_n == 0 else 0)   # order n / 2
        assert H.h_fr_is_primitive_root(b32(w + r_), log_n) == 0                 # omega >= r, although a root of unity mod r
        assert H.h_fr_is_primitive_root(b32(r_), log_n) == 0
        assert H.h_fr_is_primitive_root(b32((1 << 256) - 1), log_n) == 0
    assert H.h_fr_is_primitive_root(b32(1), 0) == 1 and H.h_fr_is_primitive_root(b32(r_ - 1), 0) == 0
    assert H.h_fr_is_primitive_root(b32(r_ - 1), 1) == 1
