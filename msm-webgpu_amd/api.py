"""ctypes binding of libmsm_hip.so and the Python mirror of the reference's Rust API for the MSM path.

Reference surface mirrored here (paths relative to /root/reference):
    run_webgpu_msm(g, v) -> C::Curve          src/lib.rs:76-82
    compute_msm(points, scalars) -> C::Curve  src/cuzk/msm.rs:75-417
    points_to_bytes / scalars_to_bytes        src/lib.rs:50-65
    sample_points / sample_scalars            src/lib.rs:20-42   (seeded here; the reference uses thread_rng)
Error behaviour: the reference panics (gpu.rs:22,51; lib.rs:58; msm.rs:399; utils.rs:20); here every failure raises
MsmHipError carrying the C-ABI error code.
"""
import ctypes as C
import functools
import os

import numpy as np
import torch

from . import build as _build

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583  # src/cuzk/msm.rs:39
R_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254's scalar field = Grumpkin's base field
# curve of a context (include/msm_hip.h: MSM_HIP_CURVE_*): id and base-field modulus
PALLAS_P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001  # Pallas' base field = Vesta's scalar field
VESTA_P = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001   # Vesta's base field = Pallas' scalar field
BLS12_381_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
CURVES = {"bn254": (0, P), "grumpkin": (1, R_BN254), "pallas": (2, PALLAS_P), "vesta": (3, VESTA_P), "bls12_381": (4, BLS12_381_P),
          "bn254_g2": (5, P), "bls12_381_g2": (6, BLS12_381_P)}  # G2: coordinates in Fq2 = Fq[u] / (u^2 + 1), an element on the wire is c0 || c1


# group order r (the scalar field) of the G1 curves: what msm_hip_bases_fft's omega lives in
BLS12_381_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SCALAR_FIELDS = {"bn254": R_BN254, "grumpkin": P, "pallas": VESTA_P, "vesta": PALLAS_P, "bls12_381": BLS12_381_R,
                 "bn254_g2": R_BN254, "bls12_381_g2": BLS12_381_R}  # (a G2 group has its G1's order)
# largest log_n of a scalar-field transform (include/msm_fr.h): min(2-adicity of r - 1, 26)
FR_MAX_LOG_N = 26


def root_of_unity(curve, log_n, inverse=False):
    """A primitive 2^log_n-th root of unity of a G1 curve's scalar field (its inverse with inverse=True), as an integer: the smallest quadratic
    non-residue raised to (r - 1) / 2^log_n.  Raises ValueError where 2^log_n does not divide r - 1 (Grumpkin: log_n > 1)."""
    return _root_of_unity(curve, int(log_n), bool(inverse))


@functools.lru_cache(maxsize=None)
def _root_of_unity(curve, log_n, inverse):
    # (two 254-bit modular exponentiations, a quarter of a millisecond: remembered, since scalars_fft asks on every call)
    r = SCALAR_FIELDS[curve]
    if log_n < 0 or (r - 1) % (1 << log_n):
        raise ValueError("the scalar field of %s has no root of unity of order 2^%d" % (curve, log_n))
    g = 2
    while pow(g, (r - 1) // 2, r) != r - 1:
        g += 1
    w = pow(g, (r - 1) >> log_n, r)
    return pow(w, r - 2, r) if inverse else w


def coord_bytes(curve):
    """Bytes of a coordinate on a curve's wire: 32; 48 for BLS12-381; 64 / 96 for BN254 / BLS12-381 G2 (an Fq2 element) -- points 2 x, Jacobian
    records 3 x that."""
    return {"bls12_381": 48, "bn254_g2": 64, "bls12_381_g2": 96}.get(curve, 32)
NUM_WINDOWS = 16
WINDOW_BITS = 16
BUCKETS_PER_WINDOW = 1 << 15

_lib = None


class MsmHipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib().msm_hip_strerror(code).decode() if _lib is not None else "error"
        super().__init__("%s failed: %s (%d)" % (where, msg, code))


def lib():
    """Load libmsm_hip.so (in-tree).  Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        so = _build.SO
        if not os.path.exists(so):
            raise ImportError("libmsm_hip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % so)
        L = C.CDLL(so)
        vp, u8p, sz, i = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int
        L.msm_hip_strerror.restype = C.c_char_p
        L.msm_hip_strerror.argtypes = [i]
        L.msm_hip_abi_version.restype = i
        L.msm_hip_ctx_create.argtypes = [C.POINTER(vp), i]
        L.msm_hip_ctx_create_curve.argtypes = [C.POINTER(vp), i, i]
        L.msm_hip_ctx_curve.argtypes = [vp]
        L.msm_hip_combine_windows_curve.argtypes = [i, u8p, i, u8p]
        L.msm_hip_g1_to_affine_curve.argtypes = [i, u8p, u8p]
        L.msm_hip_ctx_destroy.argtypes = [vp]
        L.msm_hip_ctx_destroy.restype = None
        L.msm_hip_set_bases.argtypes = [vp, u8p, sz, C.c_uint32]
        L.msm_hip_set_bases_device.argtypes = [vp, vp, sz, C.c_uint32]
        L.msm_hip_run.argtypes = [vp, u8p, sz, u8p]
        L.msm_hip_run_device.argtypes = [vp, vp, sz, u8p]
        L.msm_hip_run_batch.argtypes = [vp, u8p, sz, sz, u8p]
        L.msm_hip_launch_windows_batch_device.argtypes = [vp, vp, sz, i, i, i, i, vp]
        L.msm_hip_finish_batch.argtypes = [vp, i, u8p]
        L.msm_hip_launch_half_windows_batch_device.argtypes = [vp, vp, sz, i, i, i, i, vp]
        L.msm_hip_combine_windows_batch_curve.argtypes = [i, vp, i, i, u8p]
        L.msm_hip_launch_vwindows_batch_device.argtypes = [vp, vp, sz, i, i, i, i, vp]
        L.msm_hip_combine_vwindows_batch_curve.argtypes = [i, vp, i, i, u8p]
        L.msm_hip_mgpu_set_wide_bits.argtypes = [vp, i]
        L.msm_hip_run_batch_device.argtypes = [vp, vp, sz, sz, u8p]
        L.msm_hip_launch_device.argtypes = [vp, vp, sz, i]
        L.msm_hip_launch.argtypes = [vp, u8p, sz, i]
        L.msm_hip_run_sparse.argtypes = [vp, vp, u8p, sz, u8p]
        L.msm_hip_run_sparse_device.argtypes = [vp, vp, vp, sz, u8p]
        L.msm_hip_launch_sparse_device.argtypes = [vp, vp, vp, sz, i]
        L.msm_hip_mul_each.argtypes = [vp, u8p, sz, u8p, C.c_uint32]
        L.msm_hip_mul_each_device.argtypes = [vp, vp, sz, vp, C.c_uint32]
        L.msm_hip_mul_base.argtypes = [vp, sz, u8p, sz, u8p, C.c_uint32]
        L.msm_hip_mul_base_device.argtypes = [vp, sz, vp, sz, vp, C.c_uint32]
        L.msm_hip_test_mul_last.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
        L.msm_hip_test_mul_ladder.argtypes = [vp, i]
        L.msm_hip_test_mul_policy.argtypes = [vp, sz, i]
        L.msm_hip_bases_fft.argtypes = [vp, u8p, i, u8p, C.c_uint32]
        L.msm_hip_bases_fft_device.argtypes = [vp, u8p, i, vp, C.c_uint32]
        L.msm_hip_test_fft_last.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
        L.msm_hip_wait_stream.argtypes = [vp, vp]
        L.msm_hip_finish.argtypes = [vp, i, u8p]
        L.msm_hip_run_windows_device.argtypes = [vp, vp, sz, i, i, vp]
        L.msm_hip_launch_windows_device.argtypes = [vp, vp, sz, i, i, i, vp]
        L.msm_hip_slot_wait_stream.argtypes = [vp, i, vp]
        L.msm_hip_slot_sync.argtypes = [vp, i]
        L.msm_hip_combine_windows_bn254.argtypes = [u8p, i, u8p]
        L.msm_hip_msm_bn254_g1.argtypes = [u8p, u8p, sz, u8p]
        L.msm_hip_msm_curve.argtypes = [i, u8p, u8p, sz, u8p]
        L.msm_hip_test_oneshot_parts.argtypes = [i, sz]
        L.msm_hip_oneshot_release.argtypes = []
        L.msm_hip_oneshot_release.restype = None
        L.msm_hip_sample_scalars_device.argtypes = [vp, C.c_uint64, sz, vp]
        L.msm_hip_sample_points_device.argtypes = [vp, C.c_uint64, sz, vp]
        L.msm_hip_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float), i]
        L.msm_hip_stream.argtypes = [vp]
        L.msm_hip_stream.restype = vp
        L.msm_hip_set_debug.argtypes = [vp, i]
        L.msm_hip_set_fine_hist_min_n.argtypes = [vp, sz]
        L.msm_hip_test_skew_credit.argtypes = [vp]
        L.msm_hip_test_env_report.argtypes = [vp, C.c_char_p, sz]
        L.msm_hip_set_scalar_format.argtypes = [vp, C.c_uint32]
        L.msm_hip_set_stage_timing.argtypes = [vp, i]
        L.msm_hip_set_window_bits.argtypes = [vp, i]
        L.msm_hip_set_wide_bits.argtypes = [vp, i]
        L.msm_hip_wide_bits.argtypes = [vp]
        L.msm_hip_wide_config.argtypes = [i, i, C.c_size_t] + [C.POINTER(C.c_int)] * 4
        L.msm_hip_window_config.argtypes = [i, C.POINTER(i), C.POINTER(i)]
        L.msm_hip_last_window_bits.argtypes = [vp]
        L.msm_hip_endomorphism_window_count.argtypes = [i]
        L.msm_hip_uses_endomorphism.argtypes = [vp]
        L.msm_hip_batch_group_size.argtypes = [vp, sz]
        L.msm_hip_read_digits.argtypes = [vp, vp, sz]
        L.msm_hip_read_col_ptr.argtypes = [vp, vp, sz]
        L.msm_hip_read_val_idxs.argtypes = [vp, vp, sz]
        L.msm_hip_read_buckets.argtypes = [vp, vp, sz]
        L.msm_hip_read_window_sums.argtypes = [vp, vp, sz]
        L.msm_hip_test_fq_op.argtypes = [vp, i, u8p, u8p, u8p, sz]
        L.msm_hip_test_g1_op.argtypes = [vp, i, u8p, u8p, u8p, sz]
        L.msm_hip_test_g1_mul_u32.argtypes = [vp, u8p, vp, u8p, sz]
        L.msm_hip_last_hip_error.argtypes = [vp]
        L.msm_hip_mgpu_create.argtypes = [C.POINTER(vp), C.POINTER(i), i, C.c_uint32]
        L.msm_hip_mgpu_create_curve.argtypes = [C.POINTER(vp), C.POINTER(i), i, C.c_uint32, i]
        L.msm_hip_mgpu_destroy.argtypes = [vp]
        L.msm_hip_mgpu_destroy.restype = None
        L.msm_hip_mgpu_device_count.argtypes = [vp]
        L.msm_hip_mgpu_uses_rccl.argtypes = [vp]
        L.msm_hip_mgpu_set_bases.argtypes = [vp, u8p, sz, C.c_uint32]
        L.msm_hip_mgpu_run.argtypes = [vp, u8p, sz, u8p]
        L.msm_hip_mgpu_run_batch.argtypes = [vp, u8p, sz, sz, u8p]
        L.msm_hip_mgpu_launch_batch.argtypes = [vp, u8p, sz, i, i]
        L.msm_hip_mgpu_launch_batch_device.argtypes = [vp, C.POINTER(vp), sz, i, i]
        L.msm_hip_mgpu_finish_batch.argtypes = [vp, i, u8p]
        L.msm_hip_mgpu_group_size.argtypes = [vp]
        L.msm_hip_mgpu_inject_fault.argtypes = [vp, i, i]
        L.msm_hip_window_range.argtypes = [i, i, i, C.POINTER(i), C.POINTER(i)]
        _lib = L
    return _lib


_fr_libs = {}  # the scalar-field libraries loaded so far, by their name in msm-webgpu_amd/build.py's FR_LIBRARIES


def _load_fr(name, what):
    """Load libmsm_<name>.so (in-tree), once.  what: the argument types of its functions, by their name behind msm_<name>_ (release and destroy
    return nothing, the others an int).  Raises if the library has not been built -- there is no fallback path."""
    if name not in _fr_libs:
        so = _build.FR_LIBRARIES[name].so
        if not os.path.exists(so):
            raise ImportError("libmsm_%s.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % (name, so))
        L = C.CDLL(so)
        getattr(L, "msm_%s_abi_version" % name).restype = C.c_int
        for fn, argtypes in what.items():
            f = getattr(L, "msm_%s_%s" % (name, fn))
            f.argtypes = argtypes
            if fn in ("release", "destroy"):
                f.restype = None
        _fr_libs[name] = L
    return _fr_libs[name]


def fr_lib():
    """Load libmsm_fr.so (in-tree; include/msm_fr.h): the scalar-field NTT.  Raises if it has not been built -- there is no fallback path."""
    if "fr" in _fr_libs:
        return _fr_libs["fr"]
    vp, u8p, sz, i = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int
    return _load_fr("fr", {
        "ntt_device": [i, i, vp, vp, i, sz, u8p, u8p, u8p, C.c_uint32],
        "ntt": [i, i, vp, i, sz, u8p, u8p, u8p, C.c_uint32],
        "release": [],
        "test_pass_bits": [i],
        "test_last": [C.POINTER(i), C.POINTER(i)],
    })


def fr_test_pass_bits(bits=0):
    """test hook msm_fr_test_pass_bits: cap the radix-2 levels of a pass of the scalar-field NTT at `bits` (0: the design's 10)"""
    _check(fr_lib().msm_fr_test_pass_bits(int(bits)), "msm_fr_test_pass_bits")


def fr_last():
    """(passes, widest pass's levels) of the last scalar-field NTT of this process (test hook msm_fr_test_last)"""
    v = [C.c_int(), C.c_int()]
    _check(fr_lib().msm_fr_test_last(*[C.byref(x) for x in v]), "msm_fr_test_last")
    return tuple(x.value for x in v)


def fr_release():
    """msm_fr_release: free the scalar-field NTT's cached twiddles and scratch (they come back with the next call)"""
    fr_lib().msm_fr_release()


def frvec_lib():
    """Load libmsm_frvec.so (in-tree; include/msm_frvec.h): vector arithmetic over the scalar field.  Raises if it has not been built -- there is no
    fallback path."""
    if "frvec" in _fr_libs:
        return _fr_libs["frvec"]
    vp, u8p, sz, i, u32 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32
    return _load_fr("frvec", {
        "map_device": [i, i, vp, vp, vp, vp, vp, sz, i, u8p, u8p, u32],
        "inverse_device": [i, i, vp, vp, vp, sz, u32],
        "scan_device": [i, i, vp, vp, vp, sz, sz, i, u32, vp],
        "map": [i, i, vp, vp, vp, vp, sz, i, u8p, u8p, u32],
        "inverse": [i, i, vp, vp, sz, u32],
        "scan": [i, i, vp, vp, sz, sz, i, u32, vp],
        "release": [],
        "test_tile": [i],
        "test_last": [C.POINTER(i), C.POINTER(i)],
    })


def frvec_test_tile(elements=0):
    """test hook msm_frvec_test_tile: shrink the tile of scalars_inverse and scalars_scan to `elements` (0: the design's 1024)"""
    _check(frvec_lib().msm_frvec_test_tile(int(elements)), "msm_frvec_test_tile")


def frvec_last():
    """(kernel launches, levels) of the last vector call of this process (test hook msm_frvec_test_last)"""
    v = [C.c_int(), C.c_int()]
    _check(frvec_lib().msm_frvec_test_last(*[C.byref(x) for x in v]), "msm_frvec_test_last")
    return tuple(x.value for x in v)


def frvec_release():
    """msm_frvec_release: free the vector library's scratch and staging buffers (they come back with the next call)"""
    frvec_lib().msm_frvec_release()


def frpoly_lib():
    """Load libmsm_frpoly.so (in-tree; include/msm_frpoly.h): polynomial opening over the scalar field.  Raises if it has not been built -- there is
    no fallback path."""
    if "frpoly" in _fr_libs:
        return _fr_libs["frpoly"]
    vp, u8p, sz, i, u32 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32
    return _load_fr("frpoly", {
        "eval_device": [i, i, vp, vp, sz, sz, u8p, u32, vp],
        "divide_device": [i, i, vp, vp, vp, sz, sz, u8p, u32, vp],
        "dot_device": [i, i, vp, vp, vp, sz, sz, u32, vp],
        "combine_device": [i, i, vp, vp, vp, sz, sz, u8p, u32],
        "powers_device": [i, i, vp, vp, sz, u8p, u8p, u32],
        "eval": [i, i, vp, sz, sz, u8p, u32, vp],
        "divide": [i, i, vp, vp, sz, sz, u8p, u32, vp],
        "dot": [i, i, vp, vp, sz, sz, u32, vp],
        "combine": [i, i, vp, vp, sz, sz, u8p, u32],
        "powers": [i, i, vp, sz, u8p, u8p, u32],
        "release": [],
        "test_tile": [i],
        "test_last": [C.POINTER(i), C.POINTER(i)],
    })


def frpoly_test_tile(elements=0):
    """test hook msm_frpoly_test_tile: shrink the tile of scalars_eval, scalars_divide and scalars_dot to `elements` (0: the design's 1024)"""
    _check(frpoly_lib().msm_frpoly_test_tile(int(elements)), "msm_frpoly_test_tile")


def frpoly_last():
    """(kernel launches, levels) of the last opening call of this process (test hook msm_frpoly_test_last)"""
    v = [C.c_int(), C.c_int()]
    _check(frpoly_lib().msm_frpoly_test_last(*[C.byref(x) for x in v]), "msm_frpoly_test_last")
    return tuple(x.value for x in v)


def frpoly_release():
    """msm_frpoly_release: free the opening library's scratch, constants and staging buffers (they come back with the next call)"""
    frpoly_lib().msm_frpoly_release()


class FrmleTerm(C.Structure):
    """msm_frmle_term (include/msm_frmle.h): coeff * prod_{f < degree} row[rows[f]]"""
    _fields_ = [("coeff", C.c_uint8 * 32), ("degree", C.c_uint32), ("rows", C.c_uint32 * 4)]


def frmle_lib():
    """Load libmsm_frmle.so (in-tree; include/msm_frmle.h): the sumcheck over multilinear tables of the scalar field.  Raises if it has not been built
    -- there is no fallback path."""
    if "frmle" in _fr_libs:
        return _fr_libs["frmle"]
    vp, u8p, sz, i, u32, tp = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(FrmleTerm)
    return _load_fr("frmle", {
        "fold_device": [i, i, vp, vp, vp, sz, sz, sz, u8p, u32],
        "eval_device": [i, i, vp, vp, sz, sz, sz, u8p, u32, vp],
        "eq_device": [i, i, vp, vp, sz, u8p, u8p, u32],
        "round_device": [i, i, vp, vp, sz, sz, sz, tp, sz, u8p, u32, vp],
        "fold": [i, i, vp, vp, sz, sz, sz, u8p, u32],
        "eval": [i, i, vp, sz, sz, sz, u8p, u32, vp],
        "eq": [i, i, vp, sz, u8p, u8p, u32],
        "round": [i, i, vp, sz, sz, sz, tp, sz, u8p, u32, vp],
        "release": [],
        "test_tile": [i],
        "test_last": [C.POINTER(i), C.POINTER(i)],
    })


def frmle_test_tile(elements=0):
    """test hook msm_frmle_test_tile: shrink the tile of scalars_mle_eval and scalars_sumcheck_round to `elements` (0: the design's 1024)"""
    _check(frmle_lib().msm_frmle_test_tile(int(elements)), "msm_frmle_test_tile")


def frmle_last():
    """(kernel launches, levels) of the last sumcheck call of this process (test hook msm_frmle_test_last)"""
    v = [C.c_int(), C.c_int()]
    _check(frmle_lib().msm_frmle_test_last(*[C.byref(x) for x in v]), "msm_frmle_test_last")
    return tuple(x.value for x in v)


def frmle_release():
    """msm_frmle_release: free the sumcheck library's scratch, constants and staging buffers (they come back with the next call)"""
    frmle_lib().msm_frmle_release()


def frmat_lib():
    """Load libmsm_frmat.so (in-tree; include/msm_frmat.h): sparse matrix-vector products over the scalar field.  Raises if it has not been built
    (msm-webgpu_amd/build.py builds it beside the other five)."""
    if "frmat" in _fr_libs:
        return _fr_libs["frmat"]
    i, sz, vp, u32 = C.c_int, C.c_size_t, C.c_void_p, C.c_uint32
    return _load_fr("frmat", {
        "create": [i, i, sz, sz, sz, vp, vp, vp, u32, C.POINTER(vp)],
        "info": [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(u32)],
        "destroy": [vp],
        "mul_device": [vp, vp, vp, sz, vp, sz, u32],
        "mul": [vp, vp, sz, vp, sz, u32],
        "release": [],
        "test_tile": [i],
        "test_last": [C.POINTER(i), C.POINTER(i)],
    })


def frmat_test_tile(entries=0):
    """test hook msm_frmat_test_tile: the matrices created from now on use tiles of `entries` entries (0: the design's 1024)"""
    _check(frmat_lib().msm_frmat_test_tile(int(entries)), "msm_frmat_test_tile")


def frmat_last():
    """(kernel launches, levels) of the last sparse product of this process (test hook msm_frmat_test_last)"""
    v = [C.c_int(), C.c_int()]
    _check(frmat_lib().msm_frmat_test_last(*[C.byref(x) for x in v]), "msm_frmat_test_last")
    return tuple(x.value for x in v)


def frmat_release():
    """msm_frmat_release: free the sparse-product library's staging buffers (they come back with the next call); the matrices stay"""
    frmat_lib().msm_frmat_release()


class FrgateTerm(C.Structure):
    """msm_frgate_term (include/msm_frgate.h): coeff * prod_{f < degree} row[rows[f]] at the rotation rots[f]"""
    _fields_ = [("coeff", C.c_uint8 * 32), ("degree", C.c_uint32), ("rows", C.c_uint32 * 8), ("rots", C.c_int32 * 8)]


def frgate_lib():
    """Load libmsm_frgate.so (in-tree; include/msm_frgate.h): constraint evaluation over rotated rows of the scalar field.  Raises if it has not been
    built (msm-webgpu_amd/build.py builds it beside the other six)."""
    if "frgate" in _fr_libs:
        return _fr_libs["frgate"]
    vp, sz, i, u32, tp = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(FrgateTerm)
    return _load_fr("frgate", {
        "apply_device": [i, i, vp, vp, vp, sz, sz, sz, tp, sz, sz, vp, sz, u32],
        "apply": [i, i, vp, vp, sz, sz, sz, tp, sz, sz, vp, sz, u32],
        "release": [],
    })


def frgate_release():
    """msm_frgate_release: free the constraint-evaluation library's constants and staging buffers (they come back with the next call)"""
    frgate_lib().msm_frgate_release()


def frlook_lib():
    """Load libmsm_frlook.so (in-tree; include/msm_frlook.h): lookup arguments over the scalar field -- multiplicities and table indices.  Raises
    if it has not been built (msm-webgpu_amd/build.py builds it beside the other seven)."""
    if "frlook" in _fr_libs:
        return _fr_libs["frlook"]
    vp, sz, i, u32, u64p = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)
    return _load_fr("frlook", {
        "create_device": [i, i, vp, vp, sz, u32, C.POINTER(vp)],
        "create": [i, i, vp, sz, u32, C.POINTER(vp)],
        "info": [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(u32)],
        "destroy": [vp],
        "count_device": [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, u64p, u64p],
        "count": [vp, vp, vp, vp, vp, sz, sz, sz, u32, u64p, u64p],
        "release": [],
        "test_hash_bits": [i],
    })


lib_frlook = frlook_lib


def frlook_test_hash_bits(bits=0):
    """test hook msm_frlook_test_hash_bits: the tables created from now on keep only the low `bits` of the hash (0: the design's 32)"""
    _check(frlook_lib().msm_frlook_test_hash_bits(int(bits)), "msm_frlook_test_hash_bits")


def frlook_release():
    """msm_frlook_release: free the lookup library's staging buffers (they come back with the next call); the tables stay"""
    frlook_lib().msm_frlook_release()


class FrLookup:
    """A lookup table over a scalar field, resident on one device (msm_frlook_create_device, include/msm_frlook.h): MsmContext.lookup_table makes
    it, MsmContext.scalars_multiplicities and MsmContext.logup count into it.  n: its entries; distinct: how many different values they hold;
    mont256: the form its keys were stored in.  close() frees it; so does collecting it or leaving a `with` block."""

    def __init__(self, handle, curve, device, n, distinct, mont256):
        self._h, self.curve, self.device = handle, curve, device
        self.n, self.distinct, self.mont256 = n, distinct, mont256

    def close(self):
        if self._h:
            frlook_lib().msm_frlook_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frhash_lib():
    """Load libmsm_frhash.so (in-tree; include/msm_frhash.h): Poseidon and Poseidon2 over the scalar field -- batch permutations, sponges, Merkle trees.  Raises
    if it has not been built (msm-webgpu_amd/build.py builds it beside the other eight)."""
    if "frhash" in _fr_libs:
        return _fr_libs["frhash"]
    vp, sz, i, u32, u32p = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)
    return _load_fr("frhash", {
        "create": [i, i, u32, u32, u32, u32, vp, vp, u32, C.POINTER(vp)],
        "info": [vp, u32p, u32p, u32p],
        "destroy": [vp],
        "permute_device": [vp, vp, vp, vp, sz, u32],
        "permute": [vp, vp, vp, sz, u32],
        "hash_device": [vp, vp, vp, vp, sz, sz, sz, vp, u32, u32, u32],
        "hash": [vp, vp, vp, sz, sz, sz, vp, u32, u32, u32],
        "merkle_device": [vp, vp, vp, vp, sz, vp, u32, u32, u32],
        "merkle": [vp, vp, vp, sz, vp, u32, u32, u32],
        "release": [],
        "test_tile": [i],
    })


lib_frhash = frhash_lib


def frhash_test_tile(lanes=0):
    """test hook msm_frhash_test_tile: only the first `lanes` lanes of a workgroup take a permutation (0: the design's 64)"""
    _check(frhash_lib().msm_frhash_test_tile(int(lanes)), "msm_frhash_test_tile")


def frhash_release():
    """msm_frhash_release: free the hashing library's staging buffers (they come back with the next call); the handles stay"""
    frhash_lib().msm_frhash_release()


# the partial rounds of the alpha = 5, 128-bit column of the Poseidon paper's round-number table for R_F = 8, t = 2 .. 12 (circomlib's)
POSEIDON_PARTIAL_ROUNDS = {2: 56, 3: 57, 4: 56, 5: 60, 6: 60, 7: 63, 8: 64, 9: 63, 10: 60, 11: 66, 12: 60}


def poseidon_parameters(curve, t, full_rounds=8, partial_rounds=None):
    """(round_constants, mds) of a Poseidon permutation of width t over a curve's scalar field, as lists of integers: (full_rounds +
    partial_rounds) * t round constants and the t rows of the matrix, by the Poseidon paper's generator -- an 80-bit Grain LFSR seeded with
    the field's bit length, t and the round numbers; round constants rejected where they are not below r; the matrix 1 / (x_i + y_j) of
    2 t values reduced mod r.  partial_rounds=None: POSEIDON_PARTIAL_ROUNDS[t].  For BN254 these are circomlib's constants.  It does NOT
    run the paper's subspace-trail checks on the matrix (the reference script redraws a matrix that fails them): the caller vouches for
    parameters outside the published sets.  Pure Python, remembered."""
    t, full_rounds = int(t), int(full_rounds)
    if curve not in SCALAR_FIELDS:
        raise ValueError("no scalar field for %s" % (curve,))
    if not 2 <= t <= 12 or full_rounds % 2 or not 2 <= full_rounds <= 16:
        raise ValueError("a permutation has 2 <= t <= 12 and an even 2 <= full_rounds <= 16")
    partial_rounds = POSEIDON_PARTIAL_ROUNDS[t] if partial_rounds is None else int(partial_rounds)
    if not 0 <= partial_rounds <= 128:
        raise ValueError("a permutation has 0 .. 128 partial rounds")
    rc, mds = _poseidon_parameters(SCALAR_FIELDS[curve], t, full_rounds, partial_rounds)
    return list(rc), [list(row) for row in mds]


@functools.lru_cache(maxsize=None)
def _poseidon_parameters(r, t, full_rounds, partial_rounds):
    n = r.bit_length()
    state = 0  # bit 79 is b[0], the oldest
    for value, width in ((1, 2), (0, 4), (n, 12), (t, 12), (full_rounds, 10), (partial_rounds, 10), ((1 << 30) - 1, 30)):
        state = state << width | value

    def step():
        nonlocal state
        b = (state >> 17 ^ state >> 28 ^ state >> 41 ^ state >> 56 ^ state >> 66 ^ state >> 79) & 1  # b[62] ^ b[51] ^ b[38] ^ b[23] ^ b[13] ^ b[0]
        state = (state << 1 | b) & ((1 << 80) - 1)
        return b

    for _ in range(160):
        step()

    def draw():
        v = got = 0
        while got < n:
            if step():  # of every pair, the second bit where the first is 1
                v = v << 1 | step()
                got += 1
            else:
                step()
        return v

    rc = []
    while len(rc) < (full_rounds + partial_rounds) * t:
        v = draw()
        if v < r:
            rc.append(v)
    while True:
        xy = [draw() % r for _ in range(2 * t)]
        if len(set(xy)) == 2 * t:
            break
    return tuple(rc), tuple(tuple(pow(xy[i] + xy[t + j], r - 2, r) for j in range(t)) for i in range(t))


class FrHash:
    """A Poseidon or Poseidon2 permutation over a scalar field (msm_frhash_create, include/msm_frhash.h): MsmContext.poseidon or
    MsmContext.poseidon2 makes it, MsmContext.scalars_permute, scalars_hash, merkle_tree and merkle_path use it.  kind: "poseidon" or
    "poseidon2"; t, full_rounds, partial_rounds: its shape; arity = t - 1; capacity, capacity_at, out_at: the sponge's convention, remembered
    for the calls.  close() frees it; so does collecting it or leaving a `with` block."""

    def __init__(self, handle, curve, device, t, full_rounds, partial_rounds, capacity, capacity_at, out_at, kind="poseidon"):
        self._h, self.curve, self.device, self.kind = handle, curve, device, kind
        self.t, self.full_rounds, self.partial_rounds, self.arity = t, full_rounds, partial_rounds, t - 1
        self.capacity, self.capacity_at, self.out_at = capacity, capacity_at, out_at

    def close(self):
        if self._h:
            frhash_lib().msm_frhash_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrMatrix:
    """A sparse matrix over a scalar field, resident on one device (msm_frmat_create, include/msm_frmat.h): MsmContext.scalars_matrix makes it,
    MsmContext.scalars_matvec multiplies by it.  close() frees it; so does collecting it."""

    def __init__(self, handle, curve, device, rows, cols, nnz, has_transpose):
        self._h, self.curve, self.device = handle, curve, device
        self.rows, self.cols, self.nnz, self.has_transpose = rows, cols, nnz, has_transpose

    def close(self):
        if self._h:
            frmat_lib().msm_frmat_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check(code, where):
    if code != 0:
        raise MsmHipError(code, where)


# ------------------------------------------------------------------------------------------------ wire format
# MSM_HIP_BASES_ZERO_IS_IDENTITY (include/msm_hip.h): an all-zero base record is the point at infinity
BASES_ZERO_IS_IDENTITY = 128


def points_to_bytes(points, zero_is_identity=False):
    """[(x, y), ...] canonical integers -> n x 64 B, x || y little-endian (src/lib.rs:55-65).
    The point at infinity (None) is not representable: the reference panics at lib.rs:58, this raises -- unless zero_is_identity, which
    writes it as 64 zero bytes (x = y = 0, for a base set set with zero_is_identity=True)."""
    out = bytearray()
    for pt in points:
        if pt is None:
            if zero_is_identity:
                out += bytes(64)
                continue
            raise ValueError("point at infinity has no coordinates (src/lib.rs:58)")
        x, y = pt
        if not (0 <= x < P and 0 <= y < P):
            raise ValueError("coordinate out of range")
        out += int(x).to_bytes(32, "little") + int(y).to_bytes(32, "little")
    return bytes(out)


def bytes_to_points(b, curve="bn254"):
    """n records x || y of a curve's wire format -> [(x, y) | None, ...]: canonical integers (pairs (c0, c1) on a G2 curve), None for an
    all-zero record (the identity, as mul_each / mul_base write it).  The inverse of points_to_bytes(..., zero_is_identity=True) on BN254."""
    b = bytes(b)
    cb = coord_bytes(curve)
    if len(b) % (2 * cb):
        raise ValueError("points must be n x %d bytes" % (2 * cb))
    h = cb // 2 if curve in ("bn254_g2", "bls12_381_g2") else cb
    out = []
    for k in range(0, len(b), 2 * cb):
        rec = b[k:k + 2 * cb]
        if not any(rec):
            out.append(None)
            continue
        v = [int.from_bytes(rec[j:j + h], "little") for j in range(0, 2 * cb, h)]
        out.append((v[0], v[1]) if h == cb else ((v[0], v[1]), (v[2], v[3])))
    return out


def scalars_to_bytes(scalars):
    """[s, ...] integers in [0, r) -> n x 32 B little-endian (src/lib.rs:50-52)."""
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


class G1:
    """Result of an MSM: a Jacobian point (x, y, z), canonical integers, z = 0 <=> identity (≙ C::Curve)."""

    __slots__ = ("xyz", "p")

    def __init__(self, xyz, p=P):
        self.xyz = bytes(xyz)
        self.p = p  # base-field modulus of the point's curve
        assert len(self.xyz) in (96, 144, 192, 288)  # 3 coordinates of 32 bytes (48: BLS12-381; 64 / 96: BN254 / BLS12-381 G2, coordinates in Fq2)

    @property
    def quadratic(self):
        """The coordinates are Fq2 elements (c0, c1) (a G2 point: 192-byte record; 288 bytes on BLS12-381)."""
        return len(self.xyz) in (192, 288)

    def coords(self):
        b, cb = self.xyz, len(self.xyz) // 3
        if self.quadratic:
            h = cb // 2
            return tuple((int.from_bytes(b[k:k + h], "little"), int.from_bytes(b[k + h:k + cb], "little")) for k in (0, cb, 2 * cb))
        return tuple(int.from_bytes(b[k:k + cb], "little") for k in (0, cb, 2 * cb))

    def is_identity(self):
        return self.coords()[2] in (0, (0, 0))

    def to_affine(self):
        """(x, y) canonical integers (pairs (c0, c1) for a G2 point), or None for the identity (≙ Curve::to_affine, tests/cuzk.rs:88-94)."""
        x, y, z = self.coords()
        p = self.p
        if self.quadratic:
            if z == (0, 0):
                return None
            mul = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)
            n = pow(z[0] * z[0] + z[1] * z[1], -1, p)
            zi = (z[0] * n % p, -z[1] * n % p)
            zi2 = mul(zi, zi)
            return (mul(x, zi2), mul(y, mul(zi2, zi)))
        if z == 0:
            return None
        zi = pow(z, -1, p)
        return (x * zi * zi % p, y * zi * zi * zi % p)

    def to_affine_bytes(self):
        """The canonical affine encoding x || y used for bit-exact comparison (64 bytes; 96 for BLS12-381, 128 for G2); zero bytes for the identity."""
        a, cb = self.to_affine(), len(self.xyz) // 3
        if a is None:
            return bytes(2 * cb)
        if self.quadratic:
            return b"".join(c.to_bytes(cb // 2, "little") for c in (a[0][0], a[0][1], a[1][0], a[1][1]))
        return a[0].to_bytes(cb, "little") + a[1].to_bytes(cb, "little")

    def __eq__(self, other):  # projective equality, as G1's PartialEq (src/lib.rs:166)
        return isinstance(other, G1) and self.to_affine() == other.to_affine()

    def __hash__(self):
        return hash(self.to_affine())

    def __repr__(self):
        return "G1(%s)" % (self.to_affine(),)


# ------------------------------------------------------------------------------------------------ context
def _as_device_u8(t, row, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError("%s must be a CUDA(HIP) uint8 tensor" % what)
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() % row:
        raise ValueError("%s must be contiguous uint8 with a multiple of %d bytes" % (what, row))
    return t, t.numel() // row


# narrow scalar formats (include/msm_hip.h: MSM_HIP_SCALARS_U8 .. U64): bytes per scalar -> format value, and the unsigned dtype of that width
SCALAR_WIDTHS = {1: 2, 2: 3, 4: 4, 8: 5}
_UNSIGNED_OF_WIDTH = {1: "uint8", 2: "uint16", 4: "uint32", 8: "uint64"}
# signed and 128-bit narrow formats (MSM_HIP_SCALAR_SIGNED, MSM_HIP_SCALAR_U128): the flag, the 16-byte format, and every (width, signed) -> format value
SCALAR_SIGNED = 16
SCALAR_U128 = 8
SCALAR_FORMATS = {(w, sg): (SCALAR_U128 if w == 16 else SCALAR_WIDTHS[w]) | (SCALAR_SIGNED if sg else 0) for w in (1, 2, 4, 8, 16) for sg in (False, True)}
_SIGNED_OF_WIDTH = {1: "int8", 2: "int16", 4: "int32", 8: "int64"}


def _as_device_scalars(t, width, what="scalars", signed=False):
    """A CUDA tensor of scalars of `width` bytes -> (uint8 view, number of scalars).  32: the 32-byte forms (uint8 only, as always); a narrow
    width: uint8 (a multiple of `width` bytes) or the integer dtype of that width and of the format's signedness, read as its little-endian
    bytes.  16 bytes: uint8 only (torch has no 128-bit dtype)."""
    if width == 32:
        return _as_device_u8(t, 32, what)
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError("%s must be a CUDA(HIP) tensor" % what)
    if t.dtype != torch.uint8:
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise TypeError("%s: %s is not an integer dtype" % (what, t.dtype))
        if not signed and t.dtype.is_signed:
            raise TypeError("%s: %s is not an unsigned integer dtype (narrow scalars are unsigned)" % (what, t.dtype))
        if signed and not t.dtype.is_signed:
            raise TypeError("%s: %s is not a signed integer dtype (the scalar format is signed; uint8 rows are taken as bytes)" % (what, t.dtype))
        if t.dtype != getattr(torch, (_SIGNED_OF_WIDTH if signed else _UNSIGNED_OF_WIDTH).get(width, "uint8")):
            raise ValueError("%s: dtype %s does not hold %d-byte scalars" % (what, t.dtype, width))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % what)
        t = t.reshape(-1).view(torch.uint8)
    t, n = _as_device_u8(t, width, what)
    if t.data_ptr() % width:
        raise ValueError("%s must be aligned to %d bytes" % (what, width))
    return t, n


def _host_indices(indices, n_bases):
    """Host base indices of a sparse MSM (a numpy array or anything numpy takes) -> contiguous uint32, every one checked against n_bases."""
    a = np.asarray(indices).reshape(-1)
    if a.dtype.kind not in "iu":
        raise TypeError("indices must be integers, not %s" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n_bases):
        raise ValueError("indices must lie in [0, %d): found %d .. %d" % (n_bases, int(a.min()), int(a.max())))
    return np.ascontiguousarray(a, dtype=np.uint32)


def _device_indices(t):
    """Device base indices of a sparse MSM (a CUDA int64 / int32 / uint32 tensor) -> contiguous 32-bit words holding the uint32 indices.  Values
    outside the uint32 range become 0xffffffff (a negative int32 already reads as a huge uint32): the kernels reject them like any index beyond
    the bases, and finish raises."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError("device scalars take device indices (a CUDA integer tensor)")
    t = t.reshape(-1)
    if t.dtype == torch.int64:
        t = torch.where((t < 0) | (t > 0xFFFFFFFF), torch.full_like(t, 0xFFFFFFFF), t)
        return torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32)
    if t.dtype == torch.int32 or t.dtype == getattr(torch, "uint32", None):
        return t.contiguous()
    raise TypeError("indices must be int64, int32 or uint32, not %s" % t.dtype)


class MsmContext:
    """Persistent engine on one GPU: stream, pooled buffers, resident bases (include/msm_hip.h)."""

    def __init__(self, device=0, curve="bn254"):
        self._h = C.c_void_p()
        self.curve = curve
        self.curve_id, self.modulus = CURVES[curve]
        self.cb = coord_bytes(curve)  # bytes per coordinate; a point is pb = 2 cb, a Jacobian record jb = 3 cb
        self.pb, self.jb = 2 * self.cb, 3 * self.cb
        _check(lib().msm_hip_ctx_create_curve(C.byref(self._h), int(device), self.curve_id), "msm_hip_ctx_create_curve")
        self.device = int(device)
        self.n_bases = 0
        self.wide_bits_choice = 0
        self.scalar_width = 32  # bytes per scalar of the following runs (set_scalar_format) ...
        self.scalar_signed = False  # ... and whether they are two's-complement integers
        self.scalar_mont256 = False  # ... or, at 32 bytes, s * 2^256 mod r
        self._keepalive = {}  # slot -> tensors the slot's launch still reads / writes; released when the slot is collected

    def _order_after_torch(self, *tensors):
        """The engine's streams are not ordered with torch's: make its main stream wait (on the device) for everything
        enqueued so far on the torch stream that produced the inputs (include/msm_hip.h, ordering contract)."""
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                _check(lib().msm_hip_wait_stream(self._h, torch.cuda.current_stream(t.device).cuda_stream), "msm_hip_wait_stream")
                return

    def close(self):
        if self._h:
            lib().msm_hip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- bases
    def set_bases(self, points, check_on_curve=False, mont256=False, precompute=False, endomorphism=False, zero_is_identity=False):
        """points: bytes (host, n x 64 B wire format) or a CUDA uint8 tensor holding the same bytes.
        mont256: the coordinates are x * 2^256 mod p (4 x 64-bit Montgomery limbs, R = 2^256) instead of canonical integers.
        precompute: fixed-base tables 2^(16 w) P_i (16 x the memory): whole MSMs then use one bucket set for all windows.  "wide":
        MSM_HIP_BASES_PRECOMPUTE_WIDE -- tables 2^(C w) P_i for digits of C = 17 (more than 2^20 bases: 20; up to 2^16: 16) bits: 15 (13) bucket additions per
        point instead of 16, one bucket set (large MSMs; set_wide_bits overrides C).
        endomorphism: True: also store phi(P_i) (2 x the memory): whole MSMs split every scalar into two 127-bit halves and need
        half the windows.  False (this wrapper's default: the stage-level parity tests read the reference's 16-window shape):
        MSM_HIP_BASES_PLAIN.  None: the C ABI's own default (flags = 0) -- the fastest mode the curve has, which is what the
        reference-shaped calls (compute_msm / run_webgpu_msm below, msm_hip_msm_bn254_g1) use.
        zero_is_identity: MSM_HIP_BASES_ZERO_IS_IDENTITY -- an all-zero record is the point at infinity, and the scalars paired with it are
        ignored (points_to_bytes(..., zero_is_identity=True) writes None that way)."""
        flags = (1 if check_on_curve else 0) | (2 if mont256 else 0) | (32 if precompute == "wide" else 4 if precompute else 0) | (8 if endomorphism else 0)
        flags |= BASES_ZERO_IS_IDENTITY if zero_is_identity else 0
        if endomorphism is False and not precompute:
            flags |= 16
        if isinstance(points, torch.Tensor) and points.is_cuda:
            t, n = _as_device_u8(points, self.pb, "points")
            self._order_after_torch(t)
            _check(lib().msm_hip_set_bases_device(self._h, t.data_ptr(), n, flags), "msm_hip_set_bases_device")
        else:
            b = bytes(points)
            if len(b) % self.pb:
                raise ValueError("points must be n x 64 bytes")
            n = len(b) // self.pb
            _check(lib().msm_hip_set_bases(self._h, b, n, flags), "msm_hip_set_bases")
        self.n_bases = n
        return n

    # -- whole MSM
    def _host_scalars(self, scalars):
        b = bytes(scalars)
        w = self.scalar_width
        if len(b) % w:
            raise ValueError("scalars must be n x %d bytes" % w)
        return b, len(b) // w

    def msm(self, scalars):
        """sum_i scalars[i] * bases[i] -> G1.  scalars: bytes (n x 32 B; n x width B under a narrow format) or a CUDA tensor (uint8; under a
        narrow format also the integer dtype of its width: unsigned, or signed under a signed format)."""
        out = C.create_string_buffer(self.jb)
        if isinstance(scalars, torch.Tensor) and scalars.is_cuda:
            t, n = _as_device_scalars(scalars, self.scalar_width, signed=self.scalar_signed)
            self._order_after_torch(t)
            _check(lib().msm_hip_run_device(self._h, t.data_ptr(), n, out), "msm_hip_run_device")
        else:
            b, n = self._host_scalars(scalars)
            _check(lib().msm_hip_run(self._h, b, n, out), "msm_hip_run")
        return G1(out.raw, self.modulus)

    # -- batch scalar multiplication: n points out
    MUL_BASES_ORDER_R = 1  # MSM_HIP_MUL_BASES_ORDER_R

    def _mul(self, index, scalars, bases_order_r, out):
        if self.scalar_width != 32:
            raise ValueError("mul_each / mul_base take 32-byte scalars (canonical or mont256), not the %d-byte format set on the context" % self.scalar_width)
        flags = self.MUL_BASES_ORDER_R if bases_order_r else 0
        if isinstance(scalars, torch.Tensor) and scalars.is_cuda:
            t, n = _as_device_u8(scalars, 32, "scalars")
            if out is None:
                out = torch.empty((n, self.pb), dtype=torch.uint8, device=t.device)
            elif not (isinstance(out, torch.Tensor) and out.is_cuda):
                raise TypeError("out must be a CUDA(HIP) uint8 tensor, as the scalars are")
            elif out.dtype != torch.uint8 or tuple(out.shape) != (n, self.pb) or not out.is_contiguous() or out.device != t.device:
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d, %d) on %s" % (n, self.pb, t.device))
            self._order_after_torch(t)
            if index is None:
                _check(lib().msm_hip_mul_each_device(self._h, t.data_ptr(), n, out.data_ptr(), flags), "msm_hip_mul_each_device")
            else:
                _check(lib().msm_hip_mul_base_device(self._h, index, t.data_ptr(), n, out.data_ptr(), flags), "msm_hip_mul_base_device")
            return out
        if out is not None:
            raise TypeError("out is for device scalars; host scalars return bytes")
        b, n = self._host_scalars(scalars)
        buf = C.create_string_buffer(self.pb * n)
        if index is None:
            _check(lib().msm_hip_mul_each(self._h, b, n, buf, flags), "msm_hip_mul_each")
        else:
            _check(lib().msm_hip_mul_base(self._h, index, b, n, buf, flags), "msm_hip_mul_base")
        return buf.raw

    def mul_each(self, scalars, bases_order_r=False, out=None):
        """[scalars[i] * bases[i]] for the first n resident bases (msm_hip_mul_each): n affine records x || y, the identity as the all-zero
        record (bytes_to_points reads them; a device result can go straight into set_bases(..., zero_is_identity=True)).  Host bytes in give
        bytes out; a CUDA uint8 tensor in gives a CUDA uint8 tensor [n, pb] out (`out`: a preallocated one).  32-byte scalar formats only.
        bases_order_r: on BLS12-381 and the G2 curves, vouch that the bases have order r, so that the endomorphism's ladder may run."""
        return self._mul(None, scalars, bases_order_r, out)

    def mul_base(self, index, scalars, bases_order_r=False, out=None):
        """[scalars[i] * bases[index]] (msm_hip_mul_base): as mul_each with one resident base for every scalar; n is free of n_bases."""
        index = int(index)
        if index < 0:
            raise ValueError("base index %d is negative" % index)
        return self._mul(index, scalars, bases_order_r, out)

    def mul_last(self):
        """(path, table_bits, chunk) of the last mul_each / mul_base call (test hook msm_hip_test_mul_last): path 0 none, 1 plain ladder, 2 endomorphism, 3 table held, 4 table built"""
        v = [C.c_int(), C.c_int(), C.c_int()]
        _check(lib().msm_hip_test_mul_last(self._h, *[C.byref(x) for x in v]), "msm_hip_test_mul_last")
        return tuple(x.value for x in v)

    def mul_policy(self, table_min_n=0, table_bits=0):
        """test hook msm_hip_test_mul_policy: mul_base's table runs exactly when n >= table_min_n (1 forces it, "never" forbids it), with digit
        width table_bits (0: the cost model's); 0, 0 restores the policy"""
        if table_min_n == "never":
            table_min_n = C.c_size_t(-1).value
        _check(lib().msm_hip_test_mul_policy(self._h, int(table_min_n), int(table_bits)), "msm_hip_test_mul_policy")

    def mul_force_ladder(self, ladder):
        """test hook msm_hip_test_mul_ladder: 0 the policy, 1 always the plain ladder, 2 always the endomorphism's"""
        _check(lib().msm_hip_test_mul_ladder(self._h, int(ladder)), "msm_hip_test_mul_ladder")

    # -- group FFT over the resident bases: monomial SRS -> Lagrange basis
    FFT_SCALE_INV_N = 2  # MSM_HIP_FFT_SCALE_INV_N

    def bases_fft(self, omega, log_n=None, scale=False, bases_order_r=False, out=None, device=False):
        """[c * sum_j omega^(i j) * bases[j]] for i < n = 2^log_n over the first n resident bases (msm_hip_bases_fft): n affine records as mul_each
        writes them, in natural order.  omega: an integer (or its 32 little-endian bytes), a primitive n-th root of unity of the scalar field
        (root_of_unity).  log_n: None takes all the bases, whose number must then be a power of two.  scale: c = 1 / n instead of 1.
        bases_order_r: as for mul_each.  Returns bytes; with device=True a new CUDA uint8 tensor [n, pb]; with `out`, that preallocated tensor."""
        if log_n is None:
            if self.n_bases == 0 or self.n_bases & (self.n_bases - 1):
                raise ValueError("log_n=None needs a power-of-two number of resident bases, not %d" % self.n_bases)
            log_n = self.n_bases.bit_length() - 1
        log_n = int(log_n)
        w = bytes(omega) if isinstance(omega, (bytes, bytearray)) else int(omega).to_bytes(32, "little")
        if len(w) != 32:
            raise ValueError("omega must be an integer or 32 bytes")
        flags = (self.FFT_SCALE_INV_N if scale else 0) | (self.MUL_BASES_ORDER_R if bases_order_r else 0)
        n = 1 << log_n if 0 <= log_n <= 28 else 0
        if out is not None or device:
            if out is None:
                out = torch.empty((n, self.pb), dtype=torch.uint8, device="cuda:%d" % self.device)
            elif not (isinstance(out, torch.Tensor) and out.is_cuda):
                raise TypeError("out must be a CUDA(HIP) uint8 tensor")
            elif out.dtype != torch.uint8 or tuple(out.shape) != (n, self.pb) or not out.is_contiguous():
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d, %d)" % (n, self.pb))
            self._order_after_torch(out)
            _check(lib().msm_hip_bases_fft_device(self._h, w, log_n, out.data_ptr() if n else None, flags), "msm_hip_bases_fft_device")
            return out
        buf = C.create_string_buffer(self.pb * max(n, 1))
        _check(lib().msm_hip_bases_fft(self._h, w, log_n, buf, flags), "msm_hip_bases_fft")
        return buf.raw[:self.pb * n]

    def lagrange_bases(self, log_n=None, bases_order_r=False, out=None, device=False):
        """The resident monomial SRS [tau^j G] in the Lagrange basis of the 2^log_n-th roots of unity: L_i(tau) G = (1 / n) sum_j omega^(-i j) tau^j G
        for omega = root_of_unity(curve, log_n) -- bases_fft(omega^-1, scale=True)."""
        if log_n is None:
            if self.n_bases == 0 or self.n_bases & (self.n_bases - 1):
                raise ValueError("log_n=None needs a power-of-two number of resident bases, not %d" % self.n_bases)
            log_n = self.n_bases.bit_length() - 1
        return self.bases_fft(root_of_unity(self.curve, log_n, inverse=True), log_n, scale=True, bases_order_r=bases_order_r, out=out, device=device)

    def fft_last(self):
        """(stages, ladder) of the last bases_fft call (test hook msm_hip_test_fft_last): ladder 0 none, 1 plain, 2 endomorphism"""
        v = [C.c_int(), C.c_int()]
        _check(lib().msm_hip_test_fft_last(self._h, *[C.byref(x) for x in v]), "msm_hip_test_fft_last")
        return tuple(x.value for x in v)

    # -- scalar-field NTT (libmsm_fr.so): coefficients <-> evaluations of the vectors this context commits to
    FR_SCALE_INV_N, FR_MONT256 = 1, 2  # MSM_FR_SCALE_INV_N, MSM_FR_MONT256

    def scalars_fft(self, scalars, log_n=None, omega=None, inverse=False, shift=None, batch=1):
        """The transform of `batch` vectors of n = 2^log_n scalars (msm_fr_ntt_device, include/msm_fr.h), in natural order:
        out[i] = sum_j omega^(i j) (shift^j a[j]) -- the evaluations of the polynomial with coefficients a on the n-th roots of unity (on the coset
        shift * H with `shift`); inverse=True undoes it: omega^-1, 1 / n, and shift^-i afterwards.  scalars: a CUDA uint8 tensor of batch * n * 32
        bytes, transformed IN PLACE on this context's stream and returned -- it can go straight into msm() --, or host bytes (bytes come back).
        log_n: None takes it from the size.  omega: None takes root_of_unity(curve, log_n); an integer or 32 bytes otherwise, a primitive n-th root.
        The scalars are in this context's 32-byte scalar format (set_scalar_format: canonical, or mont256) and must be below r."""
        if self.curve not in SCALAR_FIELDS or self.curve == "grumpkin":
            raise ValueError("the scalar field of %s has no transform (2-adicity 1)" % self.curve)
        if getattr(self, "scalar_width", 32) != 32:
            raise ValueError("scalars_fft takes 32-byte scalars; the context's scalar format is %d bytes wide" % self.scalar_width)
        r = SCALAR_FIELDS[self.curve]
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be at least 1")
        on_device = isinstance(scalars, torch.Tensor) and scalars.is_cuda
        if on_device:
            t, total = _as_device_u8(scalars, 32, "scalars")
        else:
            buf = bytes(scalars)
            if len(buf) % 32:
                raise ValueError("scalars must be n x 32 bytes")
            total = len(buf) // 32
        if log_n is None:
            n = total // batch
            if total % batch or n == 0 or n & (n - 1):
                raise ValueError("%d scalars are not %d vectors of a power-of-two length" % (total, batch))
            log_n = n.bit_length() - 1
        log_n = int(log_n)
        two_adicity = ((r - 1) & -(r - 1)).bit_length() - 1
        if not 0 <= log_n <= min(two_adicity, FR_MAX_LOG_N):
            raise ValueError("log_n must lie in [0, %d] on %s, not %d" % (min(two_adicity, FR_MAX_LOG_N), self.curve, log_n))
        if total != batch << log_n:
            raise ValueError("%d scalars are not %d vectors of 2^%d" % (total, batch, log_n))
        if omega is None:
            w = root_of_unity(self.curve, log_n)
        else:
            w = int.from_bytes(omega, "little") if isinstance(omega, (bytes, bytearray)) else int(omega)
            if isinstance(omega, (bytes, bytearray)) and len(omega) != 32:
                raise ValueError("omega must be an integer or 32 bytes")
            if not 0 < w < r or (w != 1 if log_n == 0 else pow(w, 1 << (log_n - 1), r) != r - 1):
                raise ValueError("omega is not a primitive 2^%d-th root of unity of the scalar field" % log_n)
        g = None
        if shift is not None:
            g = (int.from_bytes(shift, "little") if isinstance(shift, (bytes, bytearray)) else int(shift)) % r
            if g == 0:
                raise ValueError("shift must be invertible")
        flags = self.FR_MONT256 if getattr(self, "scalar_mont256", False) else 0
        pre = post = None
        if inverse:
            w = root_of_unity(self.curve, log_n, inverse=True) if omega is None else pow(w, r - 2, r)
            flags |= self.FR_SCALE_INV_N
            post = pow(g, r - 2, r).to_bytes(32, "little") if g is not None else None
        else:
            pre = g.to_bytes(32, "little") if g is not None else None
        wb = w.to_bytes(32, "little")
        if on_device:
            self._order_after_torch(t)
            stream = lib().msm_hip_stream(self._h)
            _check(fr_lib().msm_fr_ntt_device(self.curve_id, self.device, stream, t.data_ptr(), log_n, batch, wb, pre, post, flags), "msm_fr_ntt_device")
            return scalars
        out = C.create_string_buffer(buf, max(len(buf), 1))
        _check(fr_lib().msm_fr_ntt(self.curve_id, self.device, C.cast(out, C.c_void_p), log_n, batch, wb, pre, post, flags), "msm_fr_ntt")
        return out.raw[:len(buf)]

    # -- vector arithmetic over the scalar field (libmsm_frvec.so): what lies between a transform and the next commitment
    FRVEC_EXCLUSIVE, FRVEC_MONT256 = 1, 2  # MSM_FRVEC_EXCLUSIVE, MSM_FRVEC_MONT256
    FRVEC_MAX_ELEMENTS = 1 << 26
    _FRVEC_MAPS = {"add": 0, "sub": 1, "mul": 2, "mul_add": 3, "mul_sub": 4}  # MSM_FRVEC_ADD ..
    _FRVEC_SCANS = {"sum": 0, "product": 1}  # MSM_FRVEC_SUM, MSM_FRVEC_PRODUCT

    def _frvec_field(self, what):
        if self.curve not in SCALAR_FIELDS or self.curve == "grumpkin":
            raise ValueError("%s is not offered on the scalar field of %s" % (what, self.curve))
        if getattr(self, "scalar_width", 32) != 32:
            raise ValueError("%s takes 32-byte scalars; the context's scalar format is %d bytes wide" % (what, self.scalar_width))
        return SCALAR_FIELDS[self.curve]

    def _frvec_vector(self, v, name):
        """-> (tensor or None, bytes or None, number of scalars)"""
        if isinstance(v, torch.Tensor) and v.is_cuda:
            t, n = _as_device_u8(v, 32, name)
            return t, None, n
        b = bytes(v)
        if len(b) % 32:
            raise ValueError("%s must be n x 32 bytes" % name)
        return None, b, len(b) // 32

    def _frvec_out(self, out, t, n, on_device):
        if out is None:
            return None
        if not on_device:
            raise TypeError("out is for device vectors; host bytes return bytes")
        if not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * n or not out.is_contiguous() or out.device != t.device:
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes on %s" % (n, t.device))
        return out

    def _frvec_map(self, op, a, b, c, out):
        r = self._frvec_field("scalars_" + op)
        if op not in self._FRVEC_MAPS:
            raise ValueError("unknown op %r" % (op,))
        ta, ba, n = self._frvec_vector(a, "a")
        on_device = ta is not None
        if n < 1 or n > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("a vector holds 1 .. 2^26 scalars, not %d" % n)
        vecs, consts = [], []
        for name, v in (("b", b), ("c", c)):
            if v is None:  # (an op of two operands has no c)
                vecs.append(None), consts.append(None)
            elif isinstance(v, int) or (isinstance(v, (bytes, bytearray)) and len(v) == 32 and (on_device or n != 1)):
                k = int.from_bytes(v, "little") if isinstance(v, (bytes, bytearray)) else int(v)
                if not 0 <= k < r:
                    raise ValueError("the constant %s must lie in [0, r)" % name)
                vecs.append(None), consts.append(k.to_bytes(32, "little"))
            else:
                tv, bv, m = self._frvec_vector(v, name)
                if (tv is not None) != on_device:
                    raise TypeError("%s must be on the device exactly when a is" % name)
                if m != n:
                    raise ValueError("%s holds %d scalars, a holds %d" % (name, m, n))
                vecs.append(tv if on_device else bv), consts.append(None)
        out = self._frvec_out(out, ta, n, on_device)
        flags = self.FRVEC_MONT256 if getattr(self, "scalar_mont256", False) else 0
        code = self._FRVEC_MAPS[op]
        if on_device:
            self._order_after_torch(ta)
            stream = lib().msm_hip_stream(self._h)
            dst = a if out is None else out
            ptr = [v.data_ptr() if v is not None else None for v in vecs]
            _check(frvec_lib().msm_frvec_map_device(self.curve_id, self.device, stream, (ta if out is None else out).data_ptr(), ta.data_ptr(), ptr[0], ptr[1], n, code,
                                                    consts[0], consts[1], flags), "msm_frvec_map_device")
            return dst
        buf = C.create_string_buffer(32 * n)
        host = [C.cast(C.c_char_p(v), C.c_void_p) if v is not None else None for v in vecs]
        _check(frvec_lib().msm_frvec_map(self.curve_id, self.device, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), host[0], host[1], n, code, consts[0],
                                         consts[1], flags), "msm_frvec_map")
        return buf.raw

    def scalars_add(self, a, b, out=None):
        """a + b, element by element, over this context's scalar field (msm_frvec_map_device, include/msm_frvec.h).  a: a CUDA uint8 tensor of n x 32
        bytes -- the result is written over it (out=None) or into `out`, on this context's stream, and that tensor is returned -- or host bytes
        (bytes come back).  b: a vector like a, or an integer / its 32 little-endian bytes in [0, r), which is broadcast.  The vectors are in this
        context's 32-byte scalar format (canonical, or mont256) and must be below r; a constant is always a plain integer.  (Beside a host vector of ONE scalar, 32 bytes
        are a vector too.)"""
        return self._frvec_map("add", a, b, None, out)

    def scalars_sub(self, a, b, out=None):
        """a - b (as scalars_add)"""
        return self._frvec_map("sub", a, b, None, out)

    def scalars_mul(self, a, b, out=None):
        """a * b (as scalars_add)"""
        return self._frvec_map("mul", a, b, None, out)

    def scalars_mul_add(self, a, b, c, out=None):
        """a * b + c (as scalars_add; c: a vector or a constant, like b)"""
        if c is None:
            raise ValueError("scalars_mul_add needs c")
        return self._frvec_map("mul_add", a, b, c, out)

    def scalars_mul_sub(self, a, b, c, out=None):
        """a * b - c (as scalars_mul_add)"""
        if c is None:
            raise ValueError("scalars_mul_sub needs c")
        return self._frvec_map("mul_sub", a, b, c, out)

    def scalars_inverse(self, a, out=None):
        """1 / a element by element, 1 / 0 = 0 (msm_frvec_inverse_device): Montgomery's trick on the device, with one Fermat inversion per call.
        a, out: as scalars_add."""
        self._frvec_field("scalars_inverse")
        ta, ba, n = self._frvec_vector(a, "a")
        on_device = ta is not None
        if n < 1 or n > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("a vector holds 1 .. 2^26 scalars, not %d" % n)
        out = self._frvec_out(out, ta, n, on_device)
        flags = self.FRVEC_MONT256 if getattr(self, "scalar_mont256", False) else 0
        if on_device:
            self._order_after_torch(ta)
            stream = lib().msm_hip_stream(self._h)
            _check(frvec_lib().msm_frvec_inverse_device(self.curve_id, self.device, stream, (ta if out is None else out).data_ptr(), ta.data_ptr(), n, flags),
                   "msm_frvec_inverse_device")
            return a if out is None else out
        buf = C.create_string_buffer(32 * n)
        _check(frvec_lib().msm_frvec_inverse(self.curve_id, self.device, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), n, flags), "msm_frvec_inverse")
        return buf.raw

    def scalars_scan(self, a, op="product", exclusive=False, batch=1, out=None, totals=False):
        """Running products (op="product") or sums (op="sum") along each of `batch` rows of a (msm_frvec_scan_device): out[i] = a[0] o .. o a[i];
        exclusive=True: a[0] o .. o a[i - 1], and out[0] is 1 (0 for sums).  a, out: as scalars_add.  totals=True: returns (result, totals) with
        every row's total -- what an exclusive scan does not store, e.g. the closing value of a grand product -- as batch x 32 host bytes."""
        self._frvec_field("scalars_scan")
        if op not in self._FRVEC_SCANS:
            raise ValueError("op must be \"sum\" or \"product\", not %r" % (op,))
        batch = int(batch)
        ta, ba, total = self._frvec_vector(a, "a")
        on_device = ta is not None
        if batch < 1 or total < 1 or total % batch or total > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        n = total // batch
        out = self._frvec_out(out, ta, total, on_device)
        flags = (self.FRVEC_MONT256 if getattr(self, "scalar_mont256", False) else 0) | (self.FRVEC_EXCLUSIVE if exclusive else 0)
        tot = C.create_string_buffer(32 * batch) if totals else None
        tot_ptr = C.cast(tot, C.c_void_p) if totals else None
        code = self._FRVEC_SCANS[op]
        if on_device:
            self._order_after_torch(ta)
            stream = lib().msm_hip_stream(self._h)
            _check(frvec_lib().msm_frvec_scan_device(self.curve_id, self.device, stream, (ta if out is None else out).data_ptr(), ta.data_ptr(), n, batch, code, flags,
                                                     tot_ptr), "msm_frvec_scan_device")
            res = a if out is None else out
        else:
            buf = C.create_string_buffer(32 * total)
            _check(frvec_lib().msm_frvec_scan(self.curve_id, self.device, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), n, batch, code, flags, tot_ptr),
                   "msm_frvec_scan")
            res = buf.raw
        return (res, tot.raw) if totals else res

    # -- polynomial opening over the scalar field (libmsm_frpoly.so): what follows the last commitment
    FRPOLY_SHARED_B, FRPOLY_MONT256, FRPOLY_MAX_ROWS = 1, 2, 256  # MSM_FRPOLY_SHARED_B, MSM_FRPOLY_MONT256, MSM_FRPOLY_MAX_ROWS

    def _frpoly_const(self, v, r, name):
        k = int.from_bytes(v, "little") if isinstance(v, (bytes, bytearray)) else int(v)
        if isinstance(v, (bytes, bytearray)) and len(v) != 32:
            raise ValueError("%s must be an integer or its 32 little-endian bytes" % name)
        if not 0 <= k < r:
            raise ValueError("%s must lie in [0, r)" % name)
        return k.to_bytes(32, "little")

    def _frpoly_rows(self, a, batch, name="a"):
        """-> (tensor or None, bytes or None, scalars per row)"""
        batch = int(batch)
        ta, ba, total = self._frvec_vector(a, name)
        if batch < 1 or total < 1 or total % batch or total > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        return ta, ba, total // batch

    def _frpoly_flags(self):
        return self.FRPOLY_MONT256 if getattr(self, "scalar_mont256", False) else 0

    def scalars_eval(self, a, z, batch=1):
        """The values a(z) = sum_j a[j] z^j of `batch` polynomials given by their coefficients, one row of a each (msm_frpoly_eval_device,
        include/msm_frpoly.h) -> batch x 32 host bytes in the data's form.  a: a CUDA uint8 tensor of batch x n x 32 bytes, or host bytes, in this
        context's 32-byte scalar format; z: an integer in [0, r) or its 32 little-endian bytes, always a plain integer."""
        r = self._frvec_field("scalars_eval")
        ta, ba, n = self._frpoly_rows(a, batch)
        zb = self._frpoly_const(z, r, "z")
        values = C.create_string_buffer(32 * int(batch))
        if ta is not None:
            self._order_after_torch(ta)
            _check(frpoly_lib().msm_frpoly_eval_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), ta.data_ptr(), n, int(batch), zb, self._frpoly_flags(),
                                                       C.cast(values, C.c_void_p)), "msm_frpoly_eval_device")
        else:
            _check(frpoly_lib().msm_frpoly_eval(self.curve_id, self.device, C.cast(C.c_char_p(ba), C.c_void_p), n, int(batch), zb, self._frpoly_flags(),
                                                C.cast(values, C.c_void_p)), "msm_frpoly_eval")
        return values.raw

    def scalars_divide(self, a, z, batch=1, out=None, values=False):
        """(a(X) - a(z)) / (X - z) for every row of a, by synthetic division (msm_frpoly_divide_device): out[i] = sum_{j > i} a[j] z^(j - i - 1), kept
        at the length of a (the last coefficient is 0).  a, out: as scalars_add -- in place on a device tensor unless `out` is given; z, batch: as
        scalars_eval.  values=True: returns (quotients, values) with every a(z) as batch x 32 host bytes."""
        r = self._frvec_field("scalars_divide")
        ta, ba, n = self._frpoly_rows(a, batch)
        batch = int(batch)
        zb = self._frpoly_const(z, r, "z")
        on_device = ta is not None
        out = self._frvec_out(out, ta, n * batch, on_device)
        vals = C.create_string_buffer(32 * batch) if values else None
        vals_ptr = C.cast(vals, C.c_void_p) if values else None
        if on_device:
            self._order_after_torch(ta)
            _check(frpoly_lib().msm_frpoly_divide_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), (ta if out is None else out).data_ptr(), ta.data_ptr(), n,
                                                         batch, zb, self._frpoly_flags(), vals_ptr), "msm_frpoly_divide_device")
            res = a if out is None else out
        else:
            buf = C.create_string_buffer(32 * n * batch)
            _check(frpoly_lib().msm_frpoly_divide(self.curve_id, self.device, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), n, batch, zb, self._frpoly_flags(),
                                                  vals_ptr), "msm_frpoly_divide")
            res = buf.raw
        return (res, vals.raw) if values else res

    def scalars_dot(self, a, b, batch=1):
        """sum_j a[row][j] b[row][j] for every row of a (msm_frpoly_dot_device) -> batch x 32 host bytes in the data's form.  b: as many scalars as
        a, or -- beside batch > 1 -- one row of n scalars that is used for every row of a.  a and b are both device tensors or both host bytes."""
        self._frvec_field("scalars_dot")
        ta, ba, n = self._frpoly_rows(a, batch)
        batch = int(batch)
        tb, bb, m = self._frvec_vector(b, "b")
        if (tb is not None) != (ta is not None):
            raise TypeError("b must be on the device exactly when a is")
        if m != n * batch and m != n:
            raise ValueError("b holds %d scalars; a holds %d rows of %d" % (m, batch, n))
        flags = self._frpoly_flags() | (self.FRPOLY_SHARED_B if m == n and batch > 1 else 0)
        values = C.create_string_buffer(32 * batch)
        if ta is not None:
            self._order_after_torch(ta)
            _check(frpoly_lib().msm_frpoly_dot_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), ta.data_ptr(), tb.data_ptr(), n, batch, flags,
                                                      C.cast(values, C.c_void_p)), "msm_frpoly_dot_device")
        else:
            _check(frpoly_lib().msm_frpoly_dot(self.curve_id, self.device, C.cast(C.c_char_p(ba), C.c_void_p), C.cast(C.c_char_p(bb), C.c_void_p), n, batch, flags,
                                               C.cast(values, C.c_void_p)), "msm_frpoly_dot")
        return values.raw

    def scalars_combine(self, a, coeffs, out=None):
        """out[i] = sum_k coeffs[k] a[k][i]: the linear combination of the len(coeffs) rows of a (msm_frpoly_combine_device), e.g. the fold of the
        polynomials of a batched opening with powers of a challenge.  coeffs: 1 .. 256 integers in [0, r) (or their 32-byte encodings).  a: a CUDA
        uint8 tensor of len(coeffs) x n x 32 bytes -- the n scalars of the result go into `out` (a CUDA uint8 tensor, which may be row 0 of a) or
        a new tensor -- or host bytes (bytes come back)."""
        r = self._frvec_field("scalars_combine")
        coeffs = list(coeffs)
        if not 1 <= len(coeffs) <= self.FRPOLY_MAX_ROWS:
            raise ValueError("a combination takes 1 .. %d rows, not %d" % (self.FRPOLY_MAX_ROWS, len(coeffs)))
        ta, ba, n = self._frpoly_rows(a, len(coeffs))
        cb = b"".join(self._frpoly_const(c, r, "a coefficient") for c in coeffs)
        on_device = ta is not None
        out = self._frvec_out(out, ta, n, on_device)
        if on_device:
            if out is None:
                out = torch.empty((n, 32), dtype=torch.uint8, device=ta.device)
            self._order_after_torch(ta)
            _check(frpoly_lib().msm_frpoly_combine_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), out.data_ptr(), ta.data_ptr(), n, len(coeffs), cb,
                                                          self._frpoly_flags()), "msm_frpoly_combine_device")
            return out
        buf = C.create_string_buffer(32 * n)
        _check(frpoly_lib().msm_frpoly_combine(self.curve_id, self.device, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), n, len(coeffs), cb,
                                               self._frpoly_flags()), "msm_frpoly_combine")
        return buf.raw

    def scalars_powers(self, g, n, scale=1, out=None):
        """scale * g^i for i < n as a CUDA uint8 tensor of n x 32 bytes in this context's scalar format (msm_frpoly_powers_device): the powers of a
        challenge, or the evaluation domain from a root of unity.  g, scale: integers in [0, r) or their 32 little-endian bytes."""
        r = self._frvec_field("scalars_powers")
        n = int(n)
        if n < 1 or n > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("a vector holds 1 .. 2^26 scalars, not %d" % n)
        gb, cb = self._frpoly_const(g, r, "g"), self._frpoly_const(scale, r, "scale")
        if out is None:
            out = torch.empty((n, 32), dtype=torch.uint8, device="cuda:%d" % self.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * n or not out.is_contiguous():
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes" % n)
        self._order_after_torch(out)
        _check(frpoly_lib().msm_frpoly_powers_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), out.data_ptr(), n, gb, cb, self._frpoly_flags()),
               "msm_frpoly_powers_device")
        return out

    def kzg_open(self, coeffs, z):
        """A KZG opening of the polynomial with the coefficients `coeffs` (a CUDA uint8 tensor of n x 32 bytes, n <= the resident bases, or host
        bytes) at z over the resident monomial bases tau^j G: -> (y, W) with y = f(z) as 32 bytes in the data's form and W the commitment (G1) to
        (f - y) / (X - z).  scalars_divide into a fresh tensor, then msm."""
        if isinstance(coeffs, torch.Tensor) and coeffs.is_cuda:
            q, y = self.scalars_divide(coeffs, z, out=torch.empty_like(coeffs), values=True)
        else:
            q, y = self.scalars_divide(coeffs, z, values=True)
        return y, self.msm(q)

    # -- the sumcheck over multilinear tables of the scalar field (libmsm_frmle.so): the loop between the commitments of a Nova / Spartan /
    # HyperPlonk-style prover.  The FIRST variable of a table is the TOP bit of its index (include/msm_frmle.h).
    FRMLE_MONT256, FRMLE_MAX_DEGREE, FRMLE_MAX_TERMS, FRMLE_MAX_ROWS = 2, 4, 8, 16  # MSM_FRMLE_MONT256, MSM_FRMLE_MAX_DEGREE, ..

    def _frmle_field(self, what):
        """every curve's scalar field, Grumpkin's included (a G2 context takes its G1's)"""
        if self.curve not in SCALAR_FIELDS:
            raise ValueError("%s is not offered on the scalar field of %s" % (what, self.curve))
        if getattr(self, "scalar_width", 32) != 32:
            raise ValueError("%s takes 32-byte scalars; the context's scalar format is %d bytes wide" % (what, self.scalar_width))
        return SCALAR_FIELDS[self.curve]

    def _frmle_flags(self):
        return self.FRMLE_MONT256 if getattr(self, "scalar_mont256", False) else 0

    def _frmle_rows(self, a, batch, n, least):
        """-> (tensor or None, bytes or None, n, stride): `batch` rows, stride = scalars / batch apart, of which the first n (default: all) are the table"""
        batch = int(batch)
        ta, ba, total = self._frvec_vector(a, "a")
        if batch < 1 or total < 1 or total % batch or total > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        stride = total // batch
        n = stride if n is None else int(n)
        if n < least or n > stride or n & (n - 1):
            raise ValueError("a table holds a power of two of scalars, at least %d and at most the %d of a row, not %d" % (least, stride, n))
        return ta, ba, n, stride

    def scalars_mle_fold(self, a, c, batch=1, n=None, out=None):
        """Bind the top variable of `batch` multilinear tables to c (msm_frmle_fold_device, include/msm_frmle.h): row[i] = row[i] + c (row[i + n/2] -
        row[i]) for i < n / 2.  a: a CUDA uint8 tensor of batch x N x 32 bytes -- folded in place, or into `out` (same size; only the first n / 2
        scalars of every row are written) -- or host bytes (bytes of the same layout come back).  n: the table's length, a power of two <= N
        (default N): a sumcheck keeps halving n in one buffer.  c: an integer in [0, r) or its 32 little-endian bytes, always a plain integer."""
        r = self._frmle_field("scalars_mle_fold")
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 2)
        batch = int(batch)
        cb = self._frpoly_const(c, r, "c")
        on_device = ta is not None
        out = self._frvec_out(out, ta, stride * batch, on_device)
        if on_device:
            self._order_after_torch(ta)
            _check(frmle_lib().msm_frmle_fold_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), (ta if out is None else out).data_ptr(), ta.data_ptr(), n,
                                                     batch, stride, cb, self._frmle_flags()), "msm_frmle_fold_device")
            return a if out is None else out
        buf = C.create_string_buffer(ba, len(ba))
        _check(frmle_lib().msm_frmle_fold(self.curve_id, self.device, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), n, batch, stride, cb,
                                          self._frmle_flags()), "msm_frmle_fold")
        return buf.raw

    def scalars_mle_eval(self, a, point, batch=1, n=None):
        """The multilinear extensions of `batch` tables at `point` (msm_frmle_eval_device) -> batch x 32 host bytes in the data's form.  point:
        log2(n) integers in [0, r) (or their 32-byte encodings); point[0] is the variable at the TOP bit of the index -- a table indexed with x_0 at
        the lowest bit passes its point reversed.  a, batch, n: as scalars_mle_fold; nothing is written."""
        r = self._frmle_field("scalars_mle_eval")
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 1)
        batch = int(batch)
        point = list(point)
        if len(point) != n.bit_length() - 1:
            raise ValueError("a table of %d scalars has %d variables, the point %d" % (n, n.bit_length() - 1, len(point)))
        pb = b"".join(self._frpoly_const(z, r, "a coordinate of the point") for z in point)
        values = C.create_string_buffer(32 * batch)
        if ta is not None:
            self._order_after_torch(ta)
            _check(frmle_lib().msm_frmle_eval_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), ta.data_ptr(), n, batch, stride, pb, self._frmle_flags(),
                                                     C.cast(values, C.c_void_p)), "msm_frmle_eval_device")
        else:
            _check(frmle_lib().msm_frmle_eval(self.curve_id, self.device, C.cast(C.c_char_p(ba), C.c_void_p), n, batch, stride, pb, self._frmle_flags(),
                                              C.cast(values, C.c_void_p)), "msm_frmle_eval")
        return values.raw

    def scalars_eq(self, point, scale=1, out=None):
        """The table of scale * eq(point, .) over {0, 1}^k, k = len(point), as a CUDA uint8 tensor of 2^k x 32 bytes in this context's scalar format
        (msm_frmle_eq_device): out[i] = scale prod_j (bit_(k-1-j)(i) ? point[j] : 1 - point[j]).  point, scale: integers in [0, r) or their 32
        little-endian bytes."""
        r = self._frmle_field("scalars_eq")
        point = list(point)
        if len(point) > 26:
            raise ValueError("a table holds at most 2^26 scalars, not 2^%d" % len(point))
        n = 1 << len(point)
        pb = b"".join(self._frpoly_const(z, r, "a coordinate of the point") for z in point)
        cb = self._frpoly_const(scale, r, "scale")
        if out is None:
            out = torch.empty((n, 32), dtype=torch.uint8, device="cuda:%d" % self.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * n or not out.is_contiguous():
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes" % n)
        self._order_after_torch(out)
        _check(frmle_lib().msm_frmle_eq_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), out.data_ptr(), n, pb, cb, self._frmle_flags()),
               "msm_frmle_eq_device")
        return out

    def _frmle_terms(self, terms, batch, r):
        """[(coeff, (row, ..)), ..] -> (array of msm_frmle_term, the largest degree)"""
        terms = list(terms)
        if not 1 <= len(terms) <= self.FRMLE_MAX_TERMS:
            raise ValueError("a round takes 1 .. %d terms, not %d" % (self.FRMLE_MAX_TERMS, len(terms)))
        arr = (FrmleTerm * len(terms))()
        top = 0
        for t, (coeff, rows) in zip(arr, terms):
            rows = [int(x) for x in rows]
            if not 1 <= len(rows) <= self.FRMLE_MAX_DEGREE:
                raise ValueError("a term has 1 .. %d factors, not %d" % (self.FRMLE_MAX_DEGREE, len(rows)))
            if any(not 0 <= x < batch for x in rows):
                raise ValueError("a term names a row outside the %d rows" % batch)
            t.coeff[:] = self._frpoly_const(coeff, r, "a coefficient")
            t.degree = len(rows)
            t.rows[:len(rows)] = rows
            top = max(top, len(rows))
        return arr, top

    def scalars_sumcheck_round(self, a, terms, batch=1, n=None, fold=None):
        """The values g(0) .. g(D) of a sumcheck round polynomial over `batch` multilinear tables (msm_frmle_round_device) -> (D + 1) x 32 host bytes
        in the data's form: g(t) = sum_{i < n/2} sum_terms coeff prod_f (row_f[i] + t (row_f[i + n/2] - row_f[i])), D the largest degree.  terms:
        1 .. 8 pairs (coeff, (row, ..)) of a plain integer coefficient and 1 .. 4 row numbers (a row may repeat); batch <= 16.  fold: None, or the
        previous round's challenge -- the call then first binds the top variable of ALL rows to it, in place (as scalars_mle_fold, n >= 4), and
        returns the round values of the folded tables, of n / 2 scalars: one pass over the data per round.  a, n: as scalars_mle_fold; host bytes
        with fold return (values, the folded bytes)."""
        r = self._frmle_field("scalars_sumcheck_round")
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 2 if fold is None else 4)
        batch = int(batch)
        if batch > self.FRMLE_MAX_ROWS:
            raise ValueError("a round takes at most %d rows, not %d" % (self.FRMLE_MAX_ROWS, batch))
        arr, top = self._frmle_terms(terms, batch, r)
        fb = None if fold is None else self._frpoly_const(fold, r, "fold")
        values = C.create_string_buffer(32 * (self.FRMLE_MAX_DEGREE + 1))
        if ta is not None:
            self._order_after_torch(ta)
            _check(frmle_lib().msm_frmle_round_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), ta.data_ptr(), n, batch, stride, arr, len(arr), fb,
                                                      self._frmle_flags(), C.cast(values, C.c_void_p)), "msm_frmle_round_device")
            return values.raw[:32 * (top + 1)]
        buf = C.create_string_buffer(ba, len(ba))
        _check(frmle_lib().msm_frmle_round(self.curve_id, self.device, C.cast(buf, C.c_void_p), n, batch, stride, arr, len(arr), fb, self._frmle_flags(),
                                           C.cast(values, C.c_void_p)), "msm_frmle_round")
        return values.raw[:32 * (top + 1)] if fold is None else (values.raw[:32 * (top + 1)], buf.raw)

    def sumcheck_prove(self, a, terms, batch, challenge):
        """The prover's side of a sumcheck of sum_x sum_terms coeff prod_f row_f[x] over `batch` tables of N = 2^k scalars (a: a CUDA uint8 tensor of
        batch x N x 32 bytes, DESTROYED: the rounds run in place), the counterpart of kzg_open: round j's values go to challenge(j, values) -- values:
        (D + 1) x 32 bytes in the data's form --, which returns the verifier's challenge, an integer in [0, r); every round after the first binds
        the previous challenge in the same pass (scalars_sumcheck_round with fold).  -> (the k rounds' values, the k challenges, every row's value
        at that point as batch x 32 bytes)."""
        r = self._frmle_field("sumcheck_prove")
        if not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise TypeError("sumcheck_prove runs in place on a CUDA(HIP) uint8 tensor")
        _, _, n, _ = self._frmle_rows(a, batch, None, 1)
        rounds, point = [], []
        while n >> len(point) > 1:
            j = len(point)
            values = self.scalars_sumcheck_round(a, terms, batch, n >> max(j - 1, 0), fold=point[-1] if j else None)
            c = int(challenge(j, values))
            if not 0 <= c < r:
                raise ValueError("challenge %d is not in [0, r)" % j)
            rounds.append(values)
            point.append(c)
        # the last challenge binds what is left of every row: two scalars, or -- N = 1 -- the row itself
        finals = self.scalars_mle_eval(a, point[-1:], batch, 2 if point else 1)
        return rounds, point, finals

    # -- sparse matrix-vector products over the scalar field (libmsm_frmat.so): the rows Az, Bz, Cz of an R1CS, between the commitment to the
    # witness (msm) and the sumcheck (sumcheck_prove)
    FRMAT_MONT256, FRMAT_WITH_TRANSPOSE, FRMAT_TRANSPOSE = 2, 4, 8  # MSM_FRMAT_MONT256, ..
    FRMAT_MAX_DIM, FRMAT_MAX_NNZ = 1 << 26, 1 << 28

    @staticmethod
    def _frmat_indices(v, name, bound):
        """any integer sequence, numpy array or CPU tensor -> a contiguous uint32 array; a negative or too large index raises"""
        if isinstance(v, torch.Tensor):
            if v.is_cuda:
                raise TypeError("%s comes from host memory" % name)
            v = v.numpy()
        a = np.asarray(v)
        if a.size == 0:
            return np.zeros(0, dtype=np.uint32)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError("%s must be a flat sequence of integers" % name)
        if int(a.min()) < 0 or int(a.max()) > bound:
            raise ValueError("%s holds an index outside [0, %d]" % (name, bound))
        return np.ascontiguousarray(a, dtype=np.uint32)

    def scalars_matrix(self, rows, cols, row_ptr, col_idx, values, transpose=False):
        """A rows x cols sparse matrix over this context's scalar field in CSR form -> FrMatrix (msm_frmat_create, include/msm_frmat.h), checked
        here on the host and resident on this context's device from its first product on.  row_ptr: rows + 1 integers from 0 to nnz, never
        decreasing; col_idx: nnz columns below cols, in any order within a row, repeats adding up; values: nnz integers in [0, r) or nnz x 32
        canonical little-endian bytes -- always plain integers, whatever the context's scalar format.  Indices: any integer sequence, a numpy array
        or a CPU tensor.  transpose=True also keeps the transposed structure, for scalars_matvec(..., transpose=True).  Every curve's scalar
        field, Grumpkin's included; a G2 context takes its G1's."""
        r = self._frmle_field("scalars_matrix")
        rows, cols = int(rows), int(cols)
        if not (1 <= rows <= self.FRMAT_MAX_DIM and 1 <= cols <= self.FRMAT_MAX_DIM):
            raise ValueError("a matrix has 1 .. 2^26 rows and columns, not %d x %d" % (rows, cols))
        ptr = self._frmat_indices(row_ptr, "row_ptr", self.FRMAT_MAX_NNZ)
        idx = self._frmat_indices(col_idx, "col_idx", cols - 1)
        nnz = int(idx.size)
        if ptr.size != rows + 1 or int(ptr[0]) != 0 or int(ptr[-1]) != nnz or (rows and bool((ptr[1:] < ptr[:-1]).any())):
            raise ValueError("row_ptr must hold rows + 1 integers from 0 to nnz = %d that never decrease" % nnz)
        if isinstance(values, (bytes, bytearray)):
            vb = bytes(values)
        elif isinstance(values, np.ndarray) and values.dtype == np.uint8:
            vb = values.tobytes()
        else:
            values = [int(v) for v in values]
            if any(not 0 <= v < r for v in values):
                raise ValueError("the values must lie in [0, r)")
            vb = b"".join(v.to_bytes(32, "little") for v in values)
        if len(vb) != 32 * nnz:
            raise ValueError("%d values for %d columns" % (len(vb) // 32, nnz))
        h = C.c_void_p()
        _check(frmat_lib().msm_frmat_create(self.curve_id, self.device, rows, cols, nnz, ptr.ctypes.data, idx.ctypes.data if nnz else None,
                                            C.cast(C.c_char_p(vb), C.c_void_p) if nnz else None, self.FRMAT_WITH_TRANSPOSE if transpose else 0, C.byref(h)), "msm_frmat_create")
        return FrMatrix(h, self.curve, self.device, rows, cols, nnz, bool(transpose))

    def scalars_matvec(self, mat, x, out=None, transpose=False, pad_to=None):
        """y = M x -- transpose=True: M^T x, for a matrix made with transpose=True -- over the scalar field (msm_frmat_mul_device): y[i] = sum_j
        M[i][j] x[j].  x: a CUDA uint8 tensor of cols x 32 bytes (rows x 32 with transpose) in this context's 32-byte scalar format, or host bytes
        (bytes come back).  -> a CUDA uint8 tensor of pad_to x 32 bytes, or `out` (contiguous, that size; a row of a larger buffer will do):
        pad_to defaults to the exact length, and y[length .. pad_to) is zero whatever out held.  An element of x that is not below r raises
        MsmHipError (code -4) where an entry of the matrix references it; a column nobody references is not read."""
        self._frmle_field("scalars_matvec")
        if not isinstance(mat, FrMatrix) or not mat._h:
            raise TypeError("mat must be an open FrMatrix (scalars_matrix)")
        if mat.curve != self.curve or mat.device != self.device:
            raise ValueError("the matrix belongs to %s on device %d" % (mat.curve, mat.device))
        if transpose and not mat.has_transpose:
            raise ValueError("the matrix was made without transpose=True")
        in_len, out_len = (mat.rows, mat.cols) if transpose else (mat.cols, mat.rows)
        tx, bx, n = self._frvec_vector(x, "x")
        if n != in_len:
            raise ValueError("x holds %d scalars, the matrix takes %d" % (n, in_len))
        y_len = out_len if pad_to is None else int(pad_to)
        if not out_len <= y_len <= self.FRMAT_MAX_DIM:
            raise ValueError("pad_to must lie in [%d, 2^26], not %d" % (out_len, y_len))
        flags = (self.FRMAT_MONT256 if getattr(self, "scalar_mont256", False) else 0) | (self.FRMAT_TRANSPOSE if transpose else 0)
        if tx is None:
            if out is not None:
                raise TypeError("out is for device vectors; host bytes return bytes")
            buf = C.create_string_buffer(32 * y_len)
            _check(frmat_lib().msm_frmat_mul(mat._h, C.cast(buf, C.c_void_p), y_len, C.cast(C.c_char_p(bx), C.c_void_p), n, flags), "msm_frmat_mul")
            return buf.raw
        if out is None:
            out = torch.empty((y_len, 32), dtype=torch.uint8, device=tx.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * y_len or not out.is_contiguous() or out.device != tx.device:
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes on %s" % (y_len, tx.device))
        self._order_after_torch(tx)
        _check(frmat_lib().msm_frmat_mul_device(mat._h, lib().msm_hip_stream(self._h), out.data_ptr(), y_len, tx.data_ptr(), n, flags), "msm_frmat_mul_device")
        return out

    def r1cs_tables(self, a, b, c, z, n=None, out=None, first_row=0):
        """The tables Az, Bz, Cz of an R1CS as the rows first_row .. first_row + 2 of a batch x N x 32 byte CUDA buffer: three scalars_matvec calls
        over one z (a CUDA uint8 tensor of cols x 32 bytes).  N = n, or the next power of two >= the matrices' rows; the tail of every row is zero.
        out: None -- a new buffer of (first_row + 3) x N, whose other rows are NOT initialised -- or a contiguous buffer of batch x N x 32 bytes,
        whose other rows are left as they are: with scalars_eq(point, out=out[0]) and first_row=1 it is one sumcheck_prove input for eq A B - eq C."""
        mats = (a, b, c)
        if any(not isinstance(m, FrMatrix) for m in mats) or len({(m.rows, m.cols) for m in mats}) != 1:
            raise ValueError("a, b, c must be three FrMatrix of one shape")
        first_row = int(first_row)
        if n is None:
            n = 1
            while n < a.rows:
                n *= 2
        n = int(n)
        if n < a.rows or n & (n - 1) or first_row < 0:
            raise ValueError("n must be a power of two >= %d rows, first_row >= 0" % a.rows)
        if out is None:
            if not (isinstance(z, torch.Tensor) and z.is_cuda):
                raise TypeError("z must be a CUDA(HIP) uint8 tensor")
            out = torch.empty((first_row + 3, n, 32), dtype=torch.uint8, device=z.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() % (32 * n) or \
                out.numel() < 32 * n * (first_row + 3):
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of batch x %d x 32 bytes with batch >= %d" % (n, first_row + 3))
        table = out.view(-1, n, 32)
        for k, m in enumerate(mats):
            self.scalars_matvec(m, z, out=table[first_row + k], pad_to=n)
        return out

    # -- constraint evaluation over the scalar field (libmsm_frgate.so): sums of products of rotated rows, the numerator of a PLONK / halo2-style
    # quotient over the extended coset domain, between two scalars_fft
    FRGATE_MONT256, FRGATE_ACCUMULATE = 2, 4  # MSM_FRGATE_MONT256, MSM_FRGATE_ACCUMULATE
    FRGATE_MAX_DEGREE, FRGATE_MAX_TERMS, FRGATE_MAX_ROWS = 8, 64, 32  # MSM_FRGATE_MAX_DEGREE, ..

    def _frgate_terms(self, terms, batch, r):
        """[(coeff, (factor, ..)), ..], a factor a row number or (row, rotation) -> (array of msm_frgate_term, the largest degree)"""
        terms = list(terms)
        if not 1 <= len(terms) <= self.FRGATE_MAX_TERMS:
            raise ValueError("a gate takes 1 .. %d terms, not %d" % (self.FRGATE_MAX_TERMS, len(terms)))
        arr = (FrgateTerm * len(terms))()
        top = 0
        for t, (coeff, factors) in zip(arr, terms):
            factors = [(int(f), 0) if isinstance(f, (int, np.integer)) else (int(f[0]), int(f[1])) for f in factors]
            if not 1 <= len(factors) <= self.FRGATE_MAX_DEGREE:
                raise ValueError("a term has 1 .. %d factors, not %d" % (self.FRGATE_MAX_DEGREE, len(factors)))
            if any(not 0 <= row < batch for row, _ in factors):
                raise ValueError("a term names a row outside the %d rows" % batch)
            if any(not -2 ** 31 <= rot < 2 ** 31 for _, rot in factors):
                raise ValueError("a rotation is a signed 32-bit integer")
            t.coeff[:] = self._frpoly_const(coeff, r, "a coefficient")
            t.degree = len(factors)
            t.rows[:len(factors)] = [row for row, _ in factors]
            t.rots[:len(factors)] = [rot for _, rot in factors]
            top = max(top, len(factors))
        return arr, top

    def scalars_gate(self, a, terms, batch=1, n=None, step=1, scale=None, out=None, accumulate=False):
        """out[i] = (out[i] if accumulate else 0) + scale[i mod len(scale)] * sum_terms coeff prod_f row_f[(i + rotation_f * step) mod n], i < n
        (msm_frgate_apply_device, include/msm_frgate.h): a constraint system evaluated element by element in one pass.  terms: 1 .. 64 pairs
        (coeff, factors) of a plain integer coefficient and 1 .. 8 factors, each a row number or (row, rotation) -- a rotation of any sign and
        size, in units of `step` elements, wrapping round the n elements.  a, batch, n: as scalars_mle_fold (batch <= 32 rows, n a power of two);
        a CUDA tensor runs on this context's stream, behind torch's; host bytes return bytes.  scale: None, or a vector like a of a power of two
        <= n of scalars.  out: a contiguous CUDA uint8 tensor of n x 32 bytes that overlaps neither a nor scale (a new one by default; with host
        bytes and accumulate, the n x 32 bytes to add onto).  The vectors are in this context's 32-byte scalar format and must be below r
        where they are read: the rows a term names, scale, and out with accumulate."""
        r = self._frmle_field("scalars_gate")
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 1)
        batch, step = int(batch), int(step)
        if batch > self.FRGATE_MAX_ROWS:
            raise ValueError("a gate takes at most %d rows, not %d" % (self.FRGATE_MAX_ROWS, batch))
        if not 1 <= step <= n:
            raise ValueError("step must lie in [1, n = %d], not %d" % (n, step))
        arr, _ = self._frgate_terms(terms, batch, r)
        on_device = ta is not None
        ts = bs = None
        scale_len = 0
        if scale is not None:
            ts, bs, scale_len = self._frvec_vector(scale, "scale")
            if (ts is not None) != on_device:
                raise TypeError("scale must be on the device exactly when a is")
            if scale_len < 1 or scale_len > n or scale_len & (scale_len - 1):
                raise ValueError("scale holds a power of two of scalars, at most n = %d, not %d" % (n, scale_len))
        flags = (self.FRGATE_MONT256 if getattr(self, "scalar_mont256", False) else 0) | (self.FRGATE_ACCUMULATE if accumulate else 0)
        if not on_device:
            if accumulate:
                ob = bytes(out) if out is not None else b""
                if len(ob) != 32 * n:
                    raise ValueError("with host bytes, accumulate adds onto out: %d x 32 bytes" % n)
                buf = C.create_string_buffer(ob, len(ob))
            elif out is not None:
                raise TypeError("out is for device vectors; host bytes return bytes")
            else:
                buf = C.create_string_buffer(32 * n)
            _check(frgate_lib().msm_frgate_apply(self.curve_id, self.device, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), n, batch, stride, arr, len(arr),
                                                 step, C.cast(C.c_char_p(bs), C.c_void_p) if bs is not None else None, scale_len, flags), "msm_frgate_apply")
            return buf.raw
        if out is None:
            if accumulate:
                raise ValueError("accumulate adds onto out")
            out = torch.empty((n, 32), dtype=torch.uint8, device=ta.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * n or not out.is_contiguous() or out.device != ta.device:
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes on %s" % (n, ta.device))
        if ts is not None and ts.device != ta.device:
            raise ValueError("scale must be on %s" % (ta.device,))
        lo, hi = out.data_ptr(), out.data_ptr() + 32 * n
        for t, size in ((ta, 32 * batch * stride), (ts, 32 * scale_len)):
            if t is not None and lo < t.data_ptr() + size and t.data_ptr() < hi:
                raise ValueError("out overlaps an input: a lane reads what its neighbours write to, the call is never in place")
        self._order_after_torch(ta)
        _check(frgate_lib().msm_frgate_apply_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), out.data_ptr(), ta.data_ptr(), n, batch, stride, arr, len(arr),
                                                    step, ts.data_ptr() if ts is not None else None, scale_len, flags), "msm_frgate_apply_device")
        return out

    def vanishing_inverse(self, log_n, log_ext, shift):
        """The 2^log_ext values 1 / (shift^n w^(n i) - 1), i < 2^log_ext, w = root_of_unity(curve, log_n + log_ext), n = 2^log_n, as a CUDA uint8 tensor
        of 2^log_ext x 32 bytes in this context's scalar format: 1 / Z_H on the coset shift <w>, which has period 2^log_ext -- the `scale` of
        scalars_gate on the extended domain.  Computed with Python integers on the host.  Raises ValueError where shift^n = 1 (the coset meets H)."""
        r = self._frvec_field("vanishing_inverse")
        log_n, log_ext = int(log_n), int(log_ext)
        if log_n < 0 or log_ext < 0:
            raise ValueError("log_n and log_ext are not negative")
        w = root_of_unity(self.curve, log_n + log_ext)
        g = pow((int.from_bytes(shift, "little") if isinstance(shift, (bytes, bytearray)) else int(shift)) % r, 1 << log_n, r)
        wn = pow(w, 1 << log_n, r)  # a primitive 2^log_ext-th root
        vals, x = [], g
        for _ in range(1 << log_ext):
            if x in (0, 1):
                raise ValueError("Z_H vanishes on the coset: shift^n = %d" % x)
            vals.append(pow(x - 1, r - 2, r))
            x = x * wn % r
        if getattr(self, "scalar_mont256", False):
            vals = [v * pow(2, 256, r) % r for v in vals]
        host = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()
        return torch.from_numpy(host).to("cuda:%d" % self.device)

    def quotient(self, coeffs, terms, batch, log_n, log_ext, shift):
        """The N = n 2^log_ext coefficients of t(X) = E(X) / Z_H(X), n = 2^log_n, as a CUDA uint8 tensor of N x 32 bytes:
        E(X) = sum_terms coeff prod_f column_f(omega^rotation_f X), omega = root_of_unity(curve, log_n) -- a rotation by +1 is the next row of H.
        coeffs: a CUDA uint8 tensor of batch x n x 32 bytes, the columns in coefficient form, left untouched.  Nothing leaves the device: a
        zero-padded copy of batch x N, scalars_fft onto the coset shift <root_of_unity(curve, log_n + log_ext)>, scalars_gate with step = 2^log_ext
        and scale = vanishing_inverse, scalars_fft back.  Needs 2^log_ext >= D - 1, D the largest degree among the terms: E / Z_H then has fewer
        than N coefficients, and where the constraints hold on H those from (D - 1) n upward are zero."""
        r = self._frvec_field("quotient")
        if not (isinstance(coeffs, torch.Tensor) and coeffs.is_cuda):
            raise TypeError("quotient takes a CUDA(HIP) uint8 tensor")
        batch, log_n, log_ext = int(batch), int(log_n), int(log_ext)
        t, total = _as_device_u8(coeffs, 32, "coeffs")
        if log_n < 0 or log_ext < 0 or batch < 1 or total != batch << log_n:
            raise ValueError("%d scalars are not %d columns of 2^%d" % (total, batch, log_n))
        if batch > self.FRGATE_MAX_ROWS or (batch << (log_n + log_ext)) > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("the extended columns are at most %d rows and 2^26 scalars" % self.FRGATE_MAX_ROWS)
        _, top = self._frgate_terms(terms, batch, r)
        if (1 << log_ext) < top - 1:
            raise ValueError("terms of degree %d need log_ext with 2^log_ext >= %d" % (top, top - 1))
        n, big = 1 << log_n, 1 << (log_n + log_ext)
        scale = self.vanishing_inverse(log_n, log_ext, shift)
        ext = torch.zeros((batch, big, 32), dtype=torch.uint8, device=t.device)
        ext[:, :n] = t.view(batch, n, 32)
        self.scalars_fft(ext, log_n + log_ext, shift=shift, batch=batch)
        out = self.scalars_gate(ext, terms, batch=batch, step=1 << log_ext, scale=scale)
        return self.scalars_fft(out, log_n + log_ext, inverse=True, shift=shift)

    # -- lookup arguments over the scalar field (libmsm_frlook.so): the multiplicity column of a logUp / plookup-style lookup and the table index
    # of every looked-up value, between the quotient and the commitments
    FRLOOK_MONT256, FRLOOK_MISSING = 2, 0xFFFFFFFF  # MSM_FRLOOK_MONT256, MSM_FRLOOK_MISSING
    FRLOOK_MAX_TABLE, FRLOOK_MAX_ELEMENTS = 1 << 24, 1 << 26  # MSM_FRLOOK_MAX_TABLE, MSM_FRLOOK_MAX_ELEMENTS

    def lookup_table(self, t, n=None):
        """A lookup table over this context's scalar field -> FrLookup (msm_frlook_create_device, include/msm_frlook.h).  t: a CUDA uint8 tensor of
        32-byte scalars in this context's scalar format (canonical, or mont256) -- e.g. the columns of a table folded with a challenge by
        scalars_combine --, of which the first n (default: all, at most 2^24) are the table; host bytes are taken too and go to the device with the
        first count.  The handle keeps a copy of its own: t is free afterwards.  A value may repeat: every match is credited to its lowest
        index.  A value that is not below r raises MsmHipError (code -4).  Every curve's scalar field, Grumpkin's included."""
        self._frmle_field("lookup_table")
        tt, bt, total = self._frvec_vector(t, "t")
        n = total if n is None else int(n)
        if not 1 <= n <= min(total, self.FRLOOK_MAX_TABLE):
            raise ValueError("a table holds 1 .. 2^24 scalars, at most the %d given, not %d" % (total, n))
        mont = bool(getattr(self, "scalar_mont256", False))
        flags = self.FRLOOK_MONT256 if mont else 0
        h = C.c_void_p()
        if tt is not None:
            self._order_after_torch(tt)
            _check(frlook_lib().msm_frlook_create_device(self.curve_id, self.device, lib().msm_hip_stream(self._h), tt.data_ptr(), n, flags, C.byref(h)),
                   "msm_frlook_create_device")
        else:
            _check(frlook_lib().msm_frlook_create(self.curve_id, self.device, C.cast(C.c_char_p(bt), C.c_void_p), n, flags, C.byref(h)), "msm_frlook_create")
        distinct = C.c_size_t()
        _check(frlook_lib().msm_frlook_info(h, None, C.byref(distinct), None), "msm_frlook_info")
        return FrLookup(h, self.curve, self.device, n, distinct.value, mont)

    def scalars_multiplicities(self, table, f, batch=1, n=None, out=None, indices=False, counts=False, strict=True):
        """m[j] = the number of elements of f equal to the table's value j (msm_frlook_count_device): the multiplicity column of a logUp, as
        table.n scalars in this context's scalar format (under mont256 the count k is k * 2^256 mod r).  table: an FrLookup of this context's
        curve, device and scalar format.  f: a CUDA uint8 tensor of batch rows, of which the first n scalars (default: the whole row; any n >= 1)
        are looked up, or host bytes of the same layout.  A table value that repeats gets all its matches at its lowest index and 0 at the others.
        -> m (a CUDA uint8 tensor of table.n x 32 bytes, or `out`; bytes for host bytes), or a tuple of m and what was asked for, in this
        order: indices=True, the table index of every element as a CUDA int32 tensor of batch x n, -1 where the value is not in the table (numpy
        uint32 with 0xFFFFFFFF for host bytes); counts=True, the counts as a CUDA tensor of table.n 32-bit words (torch.uint32; numpy uint32 for
        host bytes); strict=False, the pair (missing, first_missing): how many elements are not in the table and the lowest flat index
        row * n + i among them (None: none).  strict=True raises ValueError naming both instead.  m counts the elements that were found.  An
        element that is not below r raises MsmHipError (code -4)."""
        self._frmle_field("scalars_multiplicities")
        if not isinstance(table, FrLookup) or not table._h:
            raise TypeError("table must be an open FrLookup (lookup_table)")
        mont = bool(getattr(self, "scalar_mont256", False))
        if table.curve != self.curve or table.device != self.device or table.mont256 != mont:
            raise ValueError("the table belongs to %s on device %d with mont256=%s" % (table.curve, table.device, table.mont256))
        batch = int(batch)
        tf, bf, total = self._frvec_vector(f, "f")
        if batch < 1 or total < 1 or total % batch or total > self.FRLOOK_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        stride = total // batch
        n = stride if n is None else int(n)
        if not 1 <= n <= stride:
            raise ValueError("n must lie in [1, %d], the length of a row, not %d" % (stride, n))
        flags = self.FRLOOK_MONT256 if mont else 0
        miss, first = C.c_uint64(), C.c_uint64()
        if tf is None:
            if out is not None:
                raise TypeError("out is for device vectors; host bytes return bytes")
            buf = C.create_string_buffer(32 * table.n)
            idx = np.empty(batch * n, dtype=np.uint32) if indices else None
            cnt = np.empty(table.n, dtype=np.uint32) if counts else None
            _check(frlook_lib().msm_frlook_count(table._h, C.cast(buf, C.c_void_p), cnt.ctypes.data if counts else None, idx.ctypes.data if indices else None,
                                                 C.cast(C.c_char_p(bf), C.c_void_p), n, batch, stride, flags, C.byref(miss), C.byref(first)), "msm_frlook_count")
            m = buf.raw
            if indices:
                idx = idx.reshape(batch, n)
        else:
            if out is None:
                m = torch.empty((table.n, 32), dtype=torch.uint8, device=tf.device)
            elif not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * table.n or not out.is_contiguous() or out.device != tf.device:
                raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes on %s" % (table.n, tf.device))
            else:
                m = out
            idx = torch.empty((batch, n), dtype=torch.int32, device=tf.device) if indices else None
            cnt = torch.empty(table.n, dtype=torch.uint32, device=tf.device) if counts else None
            self._order_after_torch(tf)
            _check(frlook_lib().msm_frlook_count_device(table._h, lib().msm_hip_stream(self._h), m.data_ptr(), cnt.data_ptr() if counts else None,
                                                        idx.data_ptr() if indices else None, tf.data_ptr(), n, batch, stride, flags, C.byref(miss), C.byref(first)),
                   "msm_frlook_count_device")
        if strict and miss.value:
            raise ValueError("%d looked-up values are not in the table; the first is element %d (row %d, position %d)" % (miss.value, first.value, first.value // n,
                                                                                                                        first.value % n))
        res = (m,) + ((idx,) if indices else ()) + ((cnt,) if counts else ())
        if not strict:
            res += ((miss.value, first.value if miss.value else None),)
        return res[0] if len(res) == 1 else res

    def logup(self, table_values, f, beta, batch=1, n=None, lookup=None):
        """The columns of a logUp argument, prepared on the device: with m = scalars_multiplicities(lookup_table(table_values), f),
        h_f[i] = sum_rows 1 / (beta + f[row][i]), i < n, and h_t[j] = m[j] / (beta + t[j]) -> (m, h_f, h_t, sum h_f, sum h_t).  The lookup holds
        exactly when every value is in the table -- ValueError otherwise, as scalars_multiplicities(strict=True) -- and the two sums agree.
        table_values: a CUDA uint8 tensor of 32-byte scalars in this context's scalar format; f, batch, n: as scalars_multiplicities, on the
        device; beta: an integer in [0, r) or its 32 bytes, always a plain integer; lookup: an FrLookup already made of table_values (else one is
        made and closed here).  m, h_f, h_t: new CUDA uint8 tensors of table.n, n and table.n scalars; the sums: 32 host bytes each, in the
        data's form.  Chains scalars_add (beta broadcast), scalars_inverse, scalars_mul and scalars_scan(op="sum", totals=True) behind the
        lookup; the inputs are left untouched.  beta = -value is NOT detected: the vector library's 1 / 0 = 0 applies, and the term of that
        value is then missing from its sum -- draw beta after the columns are committed.  On Grumpkin, whose scalar field the vector library
        has no unit for, the same columns come from the libraries that have one (_logup_without_frvec): scalars_gate for beta + x, the
        products and the row sums, 1 / x as x^(r - 2) in 127 scalars_gate passes (again 1 / 0 = 0), scalars_mle_eval for the two sums --
        the same bytes, some hundred launches more; there batch * n and the table are at most 2^25 scalars."""
        r = self._frmle_field("logup")
        if not (isinstance(table_values, torch.Tensor) and table_values.is_cuda and isinstance(f, torch.Tensor) and f.is_cuda):
            raise TypeError("logup takes CUDA(HIP) uint8 tensors")
        tt, n_t = _as_device_u8(table_values, 32, "table_values")
        tf, total = _as_device_u8(f, 32, "f")
        batch = int(batch)
        if batch < 1 or total < 1 or total % batch:
            raise ValueError("%d scalars are not %d rows" % (total, batch))
        stride = total // batch
        n = stride if n is None else int(n)
        if not 1 <= n <= stride:
            raise ValueError("n must lie in [1, %d], the length of a row, not %d" % (stride, n))
        beta = int.from_bytes(self._frpoly_const(beta, r, "beta"), "little")
        own = lookup is None
        if own:
            lookup = self.lookup_table(tt)
        elif not isinstance(lookup, FrLookup) or lookup.n != n_t:
            raise ValueError("lookup must be the FrLookup of the %d table values" % n_t)
        try:
            m = self.scalars_multiplicities(lookup, tf, batch=batch, n=n)
        finally:
            if own:
                lookup.close()
        den = torch.empty((batch * n, 32), dtype=torch.uint8, device=tf.device)  # a copy: 1 / (beta + f), row after row
        den.view(batch, n, 32).copy_(tf.view(batch, stride, 32)[:, :n])
        if self.curve == "grumpkin":
            return (m,) + self._logup_without_frvec(r, den, tt.view(-1, 32)[:n_t], m, beta, batch, n)
        self.scalars_inverse(self.scalars_add(den, beta))
        h_f = den if batch == 1 else den[:n].clone()
        for row in range(1, batch):
            self.scalars_add(h_f, den[row * n:(row + 1) * n])
        h_t = tt.view(-1, 32)[:n_t].clone()
        self.scalars_mul(self.scalars_inverse(self.scalars_add(h_t, beta)), m)
        _, sum_f = self.scalars_scan(h_f, op="sum", out=torch.empty_like(h_f), totals=True)
        _, sum_t = self.scalars_scan(h_t, op="sum", out=torch.empty_like(h_t), totals=True)
        return m, h_f, h_t, sum_f, sum_t

    def _gate_inverse(self, x, r):
        """1 / x element by element, 1 / 0 = 0, for a CUDA tensor of N = 2^k scalars, where the vector library has no unit: x^(r - 2), two bits
        of the exponent per scalars_gate pass (acc^4 x^d, d <= 3: degree <= 7), between two buffers of two rows (acc, x) because a gate is
        never in place -> a contiguous N x 32 tensor"""
        big = x.shape[0]
        bufs = [torch.empty((2, big, 32), dtype=torch.uint8, device=x.device) for _ in range(2)]
        for b in bufs:
            b[1].copy_(x)
        digits, e = [], r - 2
        while e:
            digits.append(e & 3)
            e >>= 2
        digits.reverse()
        self.scalars_gate(bufs[1], [(1, (1,) * digits[0])], batch=2, out=bufs[0][0])  # (the top digit is not 0)
        cur = 0
        for d in digits[1:]:
            self.scalars_gate(bufs[cur], [(1, (0,) * 4 + (1,) * d)], batch=2, out=bufs[1 - cur][0])
            cur = 1 - cur
        return bufs[cur][0]

    def _logup_without_frvec(self, r, den, table, m, beta, batch, n):
        """logup's columns behind the lookup from scalars_gate and scalars_mle_eval alone.  den: the batch * n looked-up scalars, row after row
        (overwritten); table, m: the table's values and multiplicities -> (h_f, h_t, sum h_f, sum h_t)"""
        def pow2(k):
            return max(2, 1 << (k - 1).bit_length())

        if max(pow2(batch * n), pow2(table.shape[0])) > 1 << 25:
            raise ValueError("on %s logup takes at most 2^25 looked-up scalars and table values" % self.curve)
        one = (pow(2, 256, r) if getattr(self, "scalar_mont256", False) else 1).to_bytes(32, "little")
        dev = den.device

        def inverse_of_beta_plus(v):  # v: count x 32 -> 2^k x 32, the tail 1 / beta
            count, big = v.shape[0], pow2(v.shape[0])
            rows = torch.zeros((2, big, 32), dtype=torch.uint8, device=dev)
            rows[0, :count].copy_(v)
            rows[1].copy_(torch.frombuffer(bytearray(one), dtype=torch.uint8).to(dev))
            return self._gate_inverse(self.scalars_gate(rows, [(1, (0,)), (beta, (1,))], batch=2), r)

        def total(v):  # sum of 2^k scalars = 2^k times their multilinear extension at (1/2, .., 1/2)
            k = v.shape[0].bit_length() - 1
            at_half = int.from_bytes(self.scalars_mle_eval(v, [(r + 1) // 2] * k), "little")
            return (at_half << k) % r

        inv_f = inverse_of_beta_plus(den)
        wide = pow2(n)
        sum_rows = torch.zeros((wide, 32), dtype=torch.uint8, device=dev)
        for first in range(0, batch, self.FRGATE_MAX_ROWS):  # at most 32 rows to a gate, each padded with zeros to 2^k
            count = min(self.FRGATE_MAX_ROWS, batch - first)
            rows = torch.zeros((count, wide, 32), dtype=torch.uint8, device=dev)
            rows[:, :n].copy_(inv_f[first * n:(first + count) * n].view(count, n, 32))
            self.scalars_gate(rows, [(1, (c,)) for c in range(count)], batch=count, out=sum_rows, accumulate=True)
        n_t, big_t = table.shape[0], pow2(table.shape[0])
        pair = torch.zeros((2, big_t, 32), dtype=torch.uint8, device=dev)
        pair[0, :n_t].copy_(m)
        pair[1].copy_(inverse_of_beta_plus(table))
        prod = self.scalars_gate(pair, [(1, (0, 1))], batch=2)  # (zero behind the table: m is padded with zeros)
        sums = [total(v).to_bytes(32, "little") for v in (sum_rows, prod)]
        return sum_rows[:n].clone(), prod[:n_t].clone(), sums[0], sums[1]

    # -- algebraic hashing over the scalar field (libmsm_frhash.so): Poseidon permutations, sponges and Merkle trees on the stream of the
    # commitments
    FRHASH_MONT256, FRHASH_MAX_WIDTH, FRHASH_MAX_FULL_ROUNDS, FRHASH_MAX_PARTIAL_ROUNDS = 2, 12, 16, 128  # MSM_FRHASH_MONT256, MSM_FRHASH_MAX_WIDTH, ..
    FRHASH_MAX_ELEMENTS, FRHASH_MAX_LEVELS = 1 << 26, 64  # MSM_FRHASH_MAX_ELEMENTS, MSM_FRHASH_MAX_LEVELS

    def poseidon(self, t=3, full_rounds=8, partial_rounds=None, round_constants=None, mds=None, capacity=0, capacity_at=0, out_at=0):
        """A Poseidon permutation of width t over this context's scalar field (a G2 context takes its G1's) -> FrHash (msm_frhash_create,
        include/msm_frhash.h).  round_constants ((full_rounds + partial_rounds) * t integers) and mds (t rows of t integers) default to
        poseidon_parameters(curve, t, full_rounds, partial_rounds); give both or neither.  capacity, capacity_at, out_at: the sponge's
        convention, which the handle remembers for scalars_hash and merkle_tree -- (0, 0, 0) is circomlib's poseidon(inputs), (L * 2^64,
        t - 1, 0) halo2's ConstantLength<L>, (2^arity - 1, 0, 1) neptune's.  No device is touched: the tables go there with the first call."""
        r = self._frmle_field("poseidon")
        t, full_rounds = int(t), int(full_rounds)
        if (round_constants is None) != (mds is None):
            raise ValueError("give round_constants and mds, or neither")
        if not 2 <= t <= self.FRHASH_MAX_WIDTH or full_rounds % 2 or not 2 <= full_rounds <= self.FRHASH_MAX_FULL_ROUNDS:
            raise ValueError("a permutation has 2 <= t <= 12 and an even 2 <= full_rounds <= 16")
        if round_constants is None:
            partial_rounds = POSEIDON_PARTIAL_ROUNDS[t] if partial_rounds is None else int(partial_rounds)
            round_constants, mds = poseidon_parameters(self.curve, t, full_rounds, partial_rounds)
        elif partial_rounds is None:
            raise ValueError("parameters of the caller's come with their partial_rounds")
        partial_rounds = int(partial_rounds)
        if not 0 <= partial_rounds <= self.FRHASH_MAX_PARTIAL_ROUNDS:
            raise ValueError("a permutation has 0 .. 128 partial rounds")
        round_constants = [int(c) for c in round_constants]
        mds = [[int(c) for c in row] for row in mds]
        if len(round_constants) != (full_rounds + partial_rounds) * t or len(mds) != t or any(len(row) != t for row in mds):
            raise ValueError("round_constants holds (full_rounds + partial_rounds) * t integers and mds t rows of t")
        if any(not 0 <= c < r for c in round_constants) or any(not 0 <= c < r for row in mds for c in row):
            raise ValueError("round constants and matrix entries must lie in [0, r)")
        capacity_at, out_at = int(capacity_at), int(out_at)
        if not 0 <= capacity_at < t or not 0 <= out_at < t:
            raise ValueError("capacity_at and out_at must lie in [0, t)")
        capacity = int.from_bytes(self._frpoly_const(capacity, r, "capacity"), "little")
        rc_b = b"".join(c.to_bytes(32, "little") for c in round_constants)
        m_b = b"".join(c.to_bytes(32, "little") for row in mds for c in row)
        h = C.c_void_p()
        _check(frhash_lib().msm_frhash_create(self.curve_id, self.device, t, full_rounds, partial_rounds, 5, C.cast(C.c_char_p(rc_b), C.c_void_p),
                                              C.cast(C.c_char_p(m_b), C.c_void_p), 0, C.byref(h)), "msm_frhash_create")
        return FrHash(h, self.curve, self.device, t, full_rounds, partial_rounds, capacity, capacity_at, out_at)

    FRHASH_POSEIDON2 = 16  # MSM_FRHASH_POSEIDON2
    POSEIDON2_WIDTHS = (2, 3, 4, 8, 12)

    def poseidon2(self, t, full_rounds, partial_rounds, round_constants, diagonal, capacity=0, capacity_at=0, out_at=0):
        """A Poseidon2 permutation of width t in {2, 3, 4, 8, 12} over this context's scalar field -> FrHash with kind == "poseidon2"
        (msm_frhash_create under MSM_FRHASH_POSEIDON2; include/msm_frhash.h has the definition), which scalars_permute, scalars_hash,
        merkle_tree and merkle_path take like any other.  round_constants: full_rounds * t + partial_rounds integers in the order of their
        use (t per external round, one per internal round, t per external round).  diagonal: the t integers mu of the internal layer
        s[i] = mu[i] * s[i] + sum(s) -- the internal matrix's diagonal MINUS ONE, what the published parameter files call
        mat_internal_diag_m_1 or internal_matrix_diagonal.  The constants are the caller's: there is no default and no generator.
        capacity, capacity_at, out_at: as for poseidon; Barretenberg's sponge is (L * 2^64, t - 1, 0).  No device is touched."""
        r = self._frmle_field("poseidon2")
        t, full_rounds, partial_rounds = int(t), int(full_rounds), int(partial_rounds)
        if t not in self.POSEIDON2_WIDTHS or full_rounds % 2 or not 2 <= full_rounds <= self.FRHASH_MAX_FULL_ROUNDS:
            raise ValueError("a Poseidon2 permutation has t in {2, 3, 4, 8, 12} and an even 2 <= full_rounds <= 16")
        if not 0 <= partial_rounds <= self.FRHASH_MAX_PARTIAL_ROUNDS:
            raise ValueError("a permutation has 0 .. 128 partial rounds")
        round_constants, diagonal = [int(c) for c in round_constants], [int(c) for c in diagonal]
        if len(round_constants) != full_rounds * t + partial_rounds or len(diagonal) != t:
            raise ValueError("round_constants holds full_rounds * t + partial_rounds integers and diagonal t")
        if any(not 0 <= c < r for c in round_constants) or any(not 0 <= c < r for c in diagonal):
            raise ValueError("round constants and the diagonal must lie in [0, r)")
        capacity_at, out_at = int(capacity_at), int(out_at)
        if not 0 <= capacity_at < t or not 0 <= out_at < t:
            raise ValueError("capacity_at and out_at must lie in [0, t)")
        capacity = int.from_bytes(self._frpoly_const(capacity, r, "capacity"), "little")
        rc_b = b"".join(c.to_bytes(32, "little") for c in round_constants)
        mu_b = b"".join(c.to_bytes(32, "little") for c in diagonal)
        h = C.c_void_p()
        _check(frhash_lib().msm_frhash_create(self.curve_id, self.device, t, full_rounds, partial_rounds, 5, C.cast(C.c_char_p(rc_b), C.c_void_p),
                                              C.cast(C.c_char_p(mu_b), C.c_void_p), self.FRHASH_POSEIDON2, C.byref(h)), "msm_frhash_create")
        return FrHash(h, self.curve, self.device, t, full_rounds, partial_rounds, capacity, capacity_at, out_at, kind="poseidon2")

    def _frhash_handle(self, h):
        if not isinstance(h, FrHash) or not h._h:
            raise TypeError("h must be an open FrHash (poseidon, poseidon2)")
        if SCALAR_FIELDS[h.curve] != SCALAR_FIELDS.get(self.curve) or h.device != self.device:
            raise ValueError("the permutation belongs to the scalar field of %s on device %d" % (h.curve, h.device))
        self._frmle_field("hashing")
        return self.FRHASH_MONT256 if getattr(self, "scalar_mont256", False) else 0

    def scalars_permute(self, h, state, out=None):
        """out = the permutation of every state (msm_frhash_permute_device): state is a CUDA uint8 tensor of n x t x 32 bytes in this
        context's scalar format -- state i is scalars [i t, (i + 1) t) --, or host bytes of the same layout, which return bytes.  out: a
        contiguous CUDA uint8 tensor of the same size, `state` itself (in place) or one that does not overlap it (a new one by default).  An
        element that is not below r raises MsmHipError (code -4)."""
        flags = self._frhash_handle(h)
        ts, bs, total = self._frvec_vector(state, "state")
        if total < h.t or total % h.t or total > self.FRHASH_MAX_ELEMENTS:
            raise ValueError("%d scalars are not 1 .. 2^26 / t states of t = %d" % (total, h.t))
        n = total // h.t
        if ts is None:
            if out is not None:
                raise TypeError("out is for device vectors; host bytes return bytes")
            buf = C.create_string_buffer(32 * total)
            _check(frhash_lib().msm_frhash_permute(h._h, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(bs), C.c_void_p), n, flags), "msm_frhash_permute")
            return buf.raw
        if out is None:
            out = torch.empty((n, h.t, 32), dtype=torch.uint8, device=ts.device)
        else:
            self._frvec_out(out, ts, total, True)
            if out.data_ptr() != ts.data_ptr() and out.data_ptr() < ts.data_ptr() + 32 * total and ts.data_ptr() < out.data_ptr() + 32 * total:
                raise ValueError("out is state itself or does not overlap it")
        self._order_after_torch(ts)
        _check(frhash_lib().msm_frhash_permute_device(h._h, lib().msm_hip_stream(self._h), out.data_ptr(), ts.data_ptr(), n, flags), "msm_frhash_permute_device")
        return out

    def scalars_hash(self, h, a, length, batch=1, stride=None, out=None):
        """out[row] = the sponge of the first `length` scalars of row `row` of a (msm_frhash_hash_device), rate t - 1, under the handle's
        capacity convention; nothing is padded.  a: a CUDA uint8 tensor of 32-byte scalars in this context's scalar format holding `batch`
        rows `stride` scalars apart (default: scalars / batch), of which the scalars behind `length` are not read; or host bytes of the same
        layout, which return bytes.  out: a contiguous CUDA uint8 tensor of batch x 32 bytes that does not overlap a."""
        flags = self._frhash_handle(h)
        ta, ba, total = self._frvec_vector(a, "a")
        batch, length = int(batch), int(length)
        if batch < 1 or total < 1 or total > self.FRHASH_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        if stride is None:
            if total % batch:
                raise ValueError("%d scalars are not %d rows" % (total, batch))
            stride = total // batch
        stride = int(stride)
        if not 1 <= length <= stride or (batch - 1) * stride + length > total:
            raise ValueError("%d rows of %d scalars, %d apart, do not fit the %d scalars given" % (batch, length, stride, total))
        cap = h.capacity.to_bytes(32, "little")
        cap_p = C.cast(C.c_char_p(cap), C.c_void_p)
        if ta is None:
            if out is not None:
                raise TypeError("out is for device vectors; host bytes return bytes")
            buf = C.create_string_buffer(32 * batch)
            _check(frhash_lib().msm_frhash_hash(h._h, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(ba), C.c_void_p), batch, length, stride, cap_p, h.capacity_at, h.out_at,
                                                flags), "msm_frhash_hash")
            return buf.raw
        if out is None:
            out = torch.empty((batch, 32), dtype=torch.uint8, device=ta.device)
        else:
            self._frvec_out(out, ta, batch, True)
            if out.data_ptr() < ta.data_ptr() + 32 * total and ta.data_ptr() < out.data_ptr() + 32 * batch:
                raise ValueError("out overlaps a")
        self._order_after_torch(ta)
        _check(frhash_lib().msm_frhash_hash_device(h._h, lib().msm_hip_stream(self._h), out.data_ptr(), ta.data_ptr(), batch, length, stride, cap_p, h.capacity_at,
                                                   h.out_at, flags), "msm_frhash_hash_device")
        return out

    def _merkle_levels(self, h, n_leaves):
        """the number of nodes of every level above the leaves, the lowest first"""
        a = h.arity
        if a == 1:
            if not 1 <= n_leaves <= self.FRHASH_MAX_LEVELS:
                raise ValueError("a tree of arity 1 is a chain of 1 .. %d levels over one leaf" % self.FRHASH_MAX_LEVELS)
            return [1] * n_leaves
        levels, n = [], n_leaves
        if n < a or n > self.FRHASH_MAX_ELEMENTS:
            raise ValueError("a tree of arity %d has %d^k leaves, k >= 1, at most 2^26, not %d" % (a, a, n_leaves))
        while n > 1:
            if n % a:
                raise ValueError("a tree of arity %d has %d^k leaves, k >= 1, not %d" % (a, a, n_leaves))
            n //= a
            levels.append(n)
        return levels

    def merkle_tree(self, h, leaves, out=None, levels=None):
        """The nodes above the leaves of the tree of arity t - 1 (msm_frhash_merkle_device): the level above the leaves first, the root
        last -- (n - 1) / (arity - 1) scalars for n = arity^k leaves, every node the sponge of the `arity` scalars below it under the handle's
        capacity convention.  leaves: a CUDA uint8 tensor of n x 32 bytes in this context's scalar format, or host bytes (which return
        bytes).  At arity 1 (t = 2) the tree is a chain over ONE leaf and `levels` (1 .. 64) says how long.  out: a contiguous CUDA uint8
        tensor of that many x 32 bytes that does not overlap the leaves.  One launch per level, on this context's stream."""
        flags = self._frhash_handle(h)
        tl, bl, n = self._frvec_vector(leaves, "leaves")
        if h.arity == 1:
            if n != 1 or levels is None:
                raise ValueError("at arity 1 the tree is a chain over one leaf: give levels")
            n = int(levels)
        elif levels is not None:
            raise ValueError("levels is for arity 1; the leaves say how deep a wider tree is")
        count = sum(self._merkle_levels(h, n))
        cap = h.capacity.to_bytes(32, "little")
        cap_p = C.cast(C.c_char_p(cap), C.c_void_p)
        if tl is None:
            if out is not None:
                raise TypeError("out is for device vectors; host bytes return bytes")
            buf = C.create_string_buffer(32 * count)
            _check(frhash_lib().msm_frhash_merkle(h._h, C.cast(buf, C.c_void_p), C.cast(C.c_char_p(bl), C.c_void_p), n, cap_p, h.capacity_at, h.out_at, flags),
                   "msm_frhash_merkle")
            return buf.raw
        if out is None:
            out = torch.empty((count, 32), dtype=torch.uint8, device=tl.device)
        else:
            self._frvec_out(out, tl, count, True)
            if out.data_ptr() < tl.data_ptr() + tl.numel() and tl.data_ptr() < out.data_ptr() + 32 * count:
                raise ValueError("out overlaps the leaves")
        self._order_after_torch(tl)
        _check(frhash_lib().msm_frhash_merkle_device(h._h, lib().msm_hip_stream(self._h), out.data_ptr(), tl.data_ptr(), n, cap_p, h.capacity_at, h.out_at, flags),
               "msm_frhash_merkle_device")
        return out

    def merkle_path(self, h, leaves, nodes, index):
        """The siblings of leaf `index` on its way to the root: a tensor of k x (arity - 1) x 32 bytes, level by level from the leaves up,
        each level's siblings in index order -- with plain torch indexing, nothing is hashed.  leaves and nodes: as merkle_tree took and
        returned them (CUDA tensors, or bytes, which return a list of k lists of 32-byte strings)."""
        if not isinstance(h, FrHash):
            raise TypeError("h must be an FrHash (poseidon)")
        a, index = h.arity, int(index)
        on_device = isinstance(leaves, torch.Tensor)
        lv = leaves.reshape(-1, 32) if on_device else [bytes(leaves)[i:i + 32] for i in range(0, len(bytes(leaves)), 32)]
        nd = nodes.reshape(-1, 32) if on_device else [bytes(nodes)[i:i + 32] for i in range(0, len(bytes(nodes)), 32)]
        n = len(lv)
        counts = self._merkle_levels(h, len(nd) if a == 1 else n)
        if sum(counts) != len(nd) or not 0 <= index < n:
            raise ValueError("nodes is not the tree over these leaves, or index is not a leaf")
        rows, below, first_node = [], lv, 0
        for count in counts:
            first = index - index % a
            rows.append([below[first + p] for p in range(a) if first + p != index])
            index //= a
            below, first_node = nd[first_node:first_node + count], first_node + count
        if on_device:
            return torch.stack([torch.stack(row) if row else lv.new_empty((0, 32)) for row in rows]) if rows else lv.new_empty((0, a - 1, 32))
        return rows

    def msm_batch(self, scalars_dev, n):
        """`batch` MSMs over the resident bases: scalars_dev is a CUDA uint8 tensor of batch x n x 32 bytes -- batch x n x width bytes under
        a narrow format, where the integer dtype of that width is accepted too -- or host bytes of the same layout -> [G1, ...]."""
        w = self.scalar_width
        if isinstance(scalars_dev, (bytes, bytearray)):
            b = bytes(scalars_dev)
            if n <= 0 or len(b) % (w * n):
                raise ValueError("scalars must hold a whole number of n-element vectors")
            batch = len(b) // (w * n)
            out = C.create_string_buffer(self.jb * batch)
            _check(lib().msm_hip_run_batch(self._h, b, n, batch, out), "msm_hip_run_batch")
            return [G1(out.raw[self.jb * k:self.jb * (k + 1)], self.modulus) for k in range(batch)]
        t, rows = _as_device_scalars(scalars_dev, w, signed=self.scalar_signed)
        if n <= 0 or rows % n:
            raise ValueError("scalars must hold a whole number of n-element vectors")
        batch = rows // n
        out = C.create_string_buffer(self.jb * batch)
        self._order_after_torch(t)
        _check(lib().msm_hip_run_batch_device(self._h, t.data_ptr(), n, batch, out), "msm_hip_run_batch_device")
        return [G1(out.raw[self.jb * k:self.jb * (k + 1)], self.modulus) for k in range(batch)]

    def msm_sparse(self, indices, scalars):
        """sum_j scalars[j] * bases[indices[j]] -> G1 (msm_hip_run_sparse): nnz entries, indices in any order, repeats adding up.  Both on the
        device (CUDA tensors: indices int64 / int32 / uint32, scalars as for msm) or both on the host (numpy arrays or bytes).  Host indices are
        checked here: a negative or out-of-range one raises ValueError before anything reaches the device; device indices are checked by the
        kernels (MsmHipError, the context stays usable)."""
        out = C.create_string_buffer(self.jb)
        if isinstance(scalars, torch.Tensor) and scalars.is_cuda:
            ix = _device_indices(indices)
            t, nnz = _as_device_scalars(scalars, self.scalar_width, signed=self.scalar_signed)
            if ix.numel() != nnz:
                raise ValueError("%d indices for %d scalars" % (ix.numel(), nnz))
            self._order_after_torch(t)
            _check(lib().msm_hip_run_sparse_device(self._h, ix.data_ptr(), t.data_ptr(), nnz, out), "msm_hip_run_sparse_device")
        else:
            ix = _host_indices(indices, self.n_bases)
            b, nnz = self._host_scalars(scalars)
            if ix.size != nnz:
                raise ValueError("%d indices for %d scalars" % (ix.size, nnz))
            _check(lib().msm_hip_run_sparse(self._h, ix.ctypes.data, b, nnz, out), "msm_hip_run_sparse")
        return G1(out.raw, self.modulus)

    def launch_sparse(self, indices, scalars, slot=0):
        """msm_sparse's device work into a result slot (0..3), returning at once (msm_hip_launch_sparse_device); finish(slot) collects it.
        Device tensors only."""
        ix = _device_indices(indices)
        t, nnz = _as_device_scalars(scalars, self.scalar_width, signed=self.scalar_signed)
        if ix.numel() != nnz:
            raise ValueError("%d indices for %d scalars" % (ix.numel(), nnz))
        self._order_after_torch(t)
        _check(lib().msm_hip_launch_sparse_device(self._h, ix.data_ptr(), t.data_ptr(), nnz, slot), "msm_hip_launch_sparse_device")
        self._keepalive[slot] = (ix, t)

    def launch(self, scalars_dev, slot=0):
        """Enqueue the device work of one MSM into a result slot (0..3) and return at once."""
        t, n = _as_device_scalars(scalars_dev, self.scalar_width, signed=self.scalar_signed)
        self._order_after_torch(t)
        _check(lib().msm_hip_launch_device(self._h, t.data_ptr(), n, slot), "msm_hip_launch_device")
        self._keepalive[slot] = t

    def launch_host(self, scalars_host, slot=0):
        """`launch` with the scalars in host memory (bytes, n x 32 B): copied on the engine's copy stream into the slot's own
        staging buffer, so the copy of the next MSM overlaps the device work of the current one when slots alternate."""
        b, n = self._host_scalars(scalars_host)
        _check(lib().msm_hip_launch(self._h, b, n, slot), "msm_hip_launch")

    def finish(self, slot=0):
        """Wait for the slot's device work, run the host window combine, return G1."""
        out = C.create_string_buffer(self.jb)
        try:
            _check(lib().msm_hip_finish(self._h, slot, out), "msm_hip_finish")
        finally:
            self._keepalive.pop(slot, None)
        return G1(out.raw, self.modulus)

    # -- window shard (multi-GPU)
    def msm_windows(self, scalars_dev, w_begin, w_end, out_dev=None):
        """Window sums S_w, w in [w_begin, w_end), as a CUDA uint8 tensor [(w_end - w_begin), 96]."""
        t, n = _as_device_u8(scalars_dev, 32, "scalars")
        if out_dev is None:
            out_dev = torch.empty((w_end - w_begin, self.jb), dtype=torch.uint8, device=t.device)
        self._order_after_torch(t)
        _check(lib().msm_hip_run_windows_device(self._h, t.data_ptr(), n, w_begin, w_end, out_dev.data_ptr()),
               "msm_hip_run_windows_device")
        return out_dev

    def launch_windows(self, scalars_dev, w_begin, w_end, slot, out_dev):
        """Asynchronous msm_windows into a result slot (0..3); `out_dev` (CUDA uint8 [w_end - w_begin, 96]) receives the sums."""
        t, n = _as_device_u8(scalars_dev, 32, "scalars")
        self._order_after_torch(t)
        _check(lib().msm_hip_launch_windows_device(self._h, t.data_ptr(), n, w_begin, w_end, slot, out_dev.data_ptr()),
               "msm_hip_launch_windows_device")
        self._keepalive[slot] = (t, out_dev)

    def launch_windows_batch(self, scalars_dev, n, w_begin, w_end, slot, out_dev, inputs_complete=False):
        """Several MSMs per launch: scalars_dev holds nvec contiguous vectors of n scalars (CUDA uint8 [nvec * n, 32]);
        `out_dev` (CUDA uint8 [nvec * (w_end - w_begin), 96], vector-major) receives the window sums.  nvec * windows <= 64; out_dev None keeps the sums in the slot (whole MSMs: finish_batch)."""
        t, rows = _as_device_u8(scalars_dev, 32, "scalars")
        if n <= 0 or rows % n:
            raise ValueError("scalars must hold a whole number of n-element vectors")
        if not inputs_complete:  # True: the caller vouches that the scalars were complete before this call (no stream ordering needed)
            self._order_after_torch(t)
        _check(lib().msm_hip_launch_windows_batch_device(self._h, t.data_ptr(), n, rows // n, w_begin, w_end, slot,
                                                               out_dev.data_ptr() if out_dev is not None else None),
               "msm_hip_launch_windows_batch_device")
        self._keepalive[slot] = (t, out_dev)

    def launch_half_windows_batch(self, scalars_dev, n, hw_begin, hw_end, slot, out_dev, inputs_complete=False):
        """launch_windows_batch over the 8 HALF-length windows of a context whose bases carry their endomorphism images
        (msm_hip_launch_half_windows_batch_device): `out_dev` receives nvec * (hw_end - hw_begin) sums, vector-major."""
        t, rows = _as_device_u8(scalars_dev, 32, "scalars")
        if n <= 0 or rows % n:
            raise ValueError("scalars must hold a whole number of n-element vectors")
        if not inputs_complete:
            self._order_after_torch(t)
        _check(lib().msm_hip_launch_half_windows_batch_device(self._h, t.data_ptr(), n, rows // n, hw_begin, hw_end, slot,
                                                                    out_dev.data_ptr() if out_dev is not None else None),
               "msm_hip_launch_half_windows_batch_device")
        self._keepalive[slot] = (t, out_dev)

    def launch_vwindows_batch(self, scalars_dev, n, v_begin, v_end, slot, out_dev, inputs_complete=False):
        """launch_windows_batch over the VIRTUAL windows of a context whose bases are wide fixed-base tables (set_bases(precompute="wide");
        msm_hip_launch_vwindows_batch_device): `out_dev` (CUDA uint8 [nvec * (v_end - v_begin) * 2, jb], vector-major) receives, for every
        virtual window, its weighted sum and its plain total."""
        t, rows = _as_device_u8(scalars_dev, 32, "scalars")
        if n <= 0 or rows % n:
            raise ValueError("scalars must hold a whole number of n-element vectors")
        if not inputs_complete:
            self._order_after_torch(t)
        _check(lib().msm_hip_launch_vwindows_batch_device(self._h, t.data_ptr(), n, rows // n, v_begin, v_end, slot,
                                                          out_dev.data_ptr() if out_dev is not None else None),
               "msm_hip_launch_vwindows_batch_device")
        self._keepalive[slot] = (t, out_dev)

    def launch_batch(self, scalars_dev, n, slot=0):
        """Enqueue up to 4 WHOLE MSMs (contiguous scalar vectors, CUDA uint8 [nvec * n, 32]) as one launch; finish_batch collects."""
        self.launch_windows_batch(scalars_dev, n, 0, NUM_WINDOWS, slot, None)
        return scalars_dev.numel() // (32 * n)

    def finish_batch(self, slot, nvec):
        """Wait for a launch_batch slot, run the host window combines, return the list of G1 results."""
        out = C.create_string_buffer(self.jb * nvec)
        try:
            _check(lib().msm_hip_finish_batch(self._h, slot, out), "msm_hip_finish_batch")
        finally:
            self._keepalive.pop(slot, None)
        return [G1(out.raw[self.jb * k:self.jb * (k + 1)], self.modulus) for k in range(nvec)]

    def slot_wait_stream(self, slot, stream=None):
        """Make a torch CUDA stream (default: the current one) wait, on the device, for the slot's results."""
        if stream is None:
            stream = torch.cuda.current_stream()
        _check(lib().msm_hip_slot_wait_stream(self._h, slot, stream.cuda_stream), "msm_hip_slot_wait_stream")

    def slot_sync(self, slot):
        """Block until the slot is complete; raises on a device-side input error."""
        try:
            _check(lib().msm_hip_slot_sync(self._h, slot), "msm_hip_slot_sync")
        finally:
            self._keepalive.pop(slot, None)

    @staticmethod
    def combine_windows(window_sums, curve="bn254"):
        """Host Horner over all window sums (bytes or uint8 tensor, num_windows x 96 B) -> G1."""
        if isinstance(window_sums, torch.Tensor):
            window_sums = window_sums.cpu().contiguous().numpy().tobytes()
        b = bytes(window_sums)
        jb = 3 * coord_bytes(curve)
        out = C.create_string_buffer(jb)
        cid, p = CURVES[curve]
        _check(lib().msm_hip_combine_windows_curve(cid, b, len(b) // jb, out), "msm_hip_combine_windows_curve")
        return G1(out.raw, p)

    @staticmethod
    def combine_windows_batch(window_sums, num_windows, curve="bn254"):
        """Host Horner for several MSMs at once: window_sums holds nvec x num_windows x 96 B (bytes, numpy uint8 array or CPU tensor);
        the chains run side by side on the library's host pool.  -> [G1, ...]"""
        if isinstance(window_sums, torch.Tensor):
            window_sums = window_sums.contiguous().numpy()
        a = np.ascontiguousarray(np.frombuffer(window_sums, dtype=np.uint8) if isinstance(window_sums, (bytes, bytearray)) else window_sums, dtype=np.uint8)
        jb = 3 * coord_bytes(curve)
        nvec = a.size // (jb * num_windows)
        if nvec * jb * num_windows != a.size:
            raise ValueError("window sums must be nvec x num_windows x %d bytes" % jb)
        out = C.create_string_buffer(max(jb * nvec, 1))
        cid, p = CURVES[curve]
        _check(lib().msm_hip_combine_windows_batch_curve(cid, a.ctypes.data, num_windows, nvec, out), "msm_hip_combine_windows_batch_curve")
        return [G1(out.raw[jb * k:jb * (k + 1)], p) for k in range(nvec)]

    @staticmethod
    def combine_vwindows_batch(pairs, num_vwindows, curve="bn254"):
        """The finish of window-sharded launches over wide tables: pairs holds nvec x num_vwindows x 2 records (bytes, numpy uint8 array or
        CPU tensor) -- every virtual window's weighted sum and plain total, in virtual-window order -> [G1, ...]"""
        if isinstance(pairs, torch.Tensor):
            pairs = pairs.contiguous().numpy()
        a = np.ascontiguousarray(np.frombuffer(pairs, dtype=np.uint8) if isinstance(pairs, (bytes, bytearray)) else pairs, dtype=np.uint8)
        jb = 3 * coord_bytes(curve)
        nvec = a.size // (2 * jb * num_vwindows)
        if nvec * 2 * jb * num_vwindows != a.size:
            raise ValueError("pairs must be nvec x num_vwindows x 2 x %d bytes" % jb)
        out = C.create_string_buffer(max(jb * nvec, 1))
        cid, p = CURVES[curve]
        _check(lib().msm_hip_combine_vwindows_batch_curve(cid, a.ctypes.data, num_vwindows, nvec, out), "msm_hip_combine_vwindows_batch_curve")
        return [G1(out.raw[jb * k:jb * (k + 1)], p) for k in range(nvec)]

    def virtual_windows(self):
        """virtual windows (of 2^15 bucket slots) of the resident wide tables: 2^(digit bits - 16); 0 without such tables"""
        wb = self.wide_bits()
        return (1 << (wb - 16)) if wb else 0

    # -- synthetic inputs in HBM
    def sample_scalars(self, n, seed):
        t = torch.empty((n, 32), dtype=torch.uint8, device="cuda:%d" % self.device)
        _check(lib().msm_hip_sample_scalars_device(self._h, seed, n, t.data_ptr()), "msm_hip_sample_scalars_device")
        return t

    def sample_points(self, n, seed):
        t = torch.empty((n, self.pb), dtype=torch.uint8, device="cuda:%d" % self.device)
        _check(lib().msm_hip_sample_points_device(self._h, seed, n, t.data_ptr()), "msm_hip_sample_points_device")
        return t

    # -- measurement
    def set_stage_timing(self, level):
        """0: no stage events; 1: only around the SMVP accumulate kernel; 2: every stage boundary (default)."""
        _check(lib().msm_hip_set_stage_timing(self._h, int(level)), "msm_hip_set_stage_timing")

    def stage_ms(self):
        buf = (C.c_float * 10)()
        k = lib().msm_hip_last_stage_ms(self._h, buf, 10)
        names = ["recode_count", "coarse_scan", "coarse_scatter", "fine_sort", "smvp", "smvp_stitch", "bucket_reduce",
                 "device_total", "host_finalise"]
        return {names[j]: float(buf[j]) for j in range(k)}

    # -- window size
    def set_wide_bits(self, bits):
        """digit width (17 .. 20; 0: by the number of bases) of the wide fixed-base tables the next set_bases(precompute="wide") builds"""
        _check(lib().msm_hip_set_wide_bits(self._h, int(bits)), "msm_hip_set_wide_bits")
        self.wide_bits_choice = int(bits)

    def wide_bits(self):
        """digit width of the resident wide tables (0: the bases are not held that way)"""
        return lib().msm_hip_wide_bits(self._h)

    def set_window_bits(self, bits):
        """0: whole-MSM launches pick the signed-digit window from n (12 / 14 / 16 bits); 12, 14 or 16 fixes it."""
        _check(lib().msm_hip_set_window_bits(self._h, int(bits)), "msm_hip_set_window_bits")

    def batch_group_size(self, n):
        """Whole MSMs of n points per launch (launch_batch) for best throughput."""
        return lib().msm_hip_batch_group_size(self._h, n)

    def last_window_bits(self):
        return lib().msm_hip_last_window_bits(self._h)

    @staticmethod
    def window_config(bits):
        """(number of windows, buckets per window) of a window size."""
        nw, nb = C.c_int(), C.c_int()
        _check(lib().msm_hip_window_config(int(bits), C.byref(nw), C.byref(nb)), "msm_hip_window_config")
        return nw.value, nb.value

    @staticmethod
    def endomorphism_window_count(bits):
        """Windows of one 127-bit half at a window size (8 at 16 bits)."""
        v = lib().msm_hip_endomorphism_window_count(int(bits))
        if v < 0:
            raise MsmHipError(v, "msm_hip_endomorphism_window_count")
        return v

    def uses_endomorphism(self):
        return lib().msm_hip_uses_endomorphism(self._h) == 1

    # -- stage read-back (parity tests)
    def set_scalar_format(self, mont256=False, width=32, signed=False):
        """mont256 False: canonical little-endian scalars (default); True: s * 2^256 mod r words (R = 2^256 Montgomery limbs).
        width: bytes per scalar -- 32, or 1 / 2 / 4 / 8 / 16 for narrow scalars (MSM_HIP_SCALARS_U8 .. U64, MSM_HIP_SCALAR_U128: witness columns
        of small values, 128-bit challenges; whole-MSM calls only).  signed: the narrow values are two's-complement integers
        (MSM_HIP_SCALAR_SIGNED: I8 .. I128), a negative one contributing -(|v| * P).  A narrow width cannot be combined with mont256, and only
        a narrow width can be signed."""
        if width not in (1, 2, 4, 8, 16, 32):
            raise ValueError("scalar width must be 1, 2, 4, 8, 16 or 32 bytes, not %r" % (width,))
        if mont256 and width != 32:
            raise ValueError("mont256 scalars are 32 bytes wide")
        if signed and width == 32:
            raise ValueError("signed scalars are 1, 2, 4, 8 or 16 bytes wide")
        fmt = SCALAR_FORMATS[(width, bool(signed))] if width != 32 else (1 if mont256 else 0)
        _check(lib().msm_hip_set_scalar_format(self._h, fmt), "msm_hip_set_scalar_format")
        self.scalar_width, self.scalar_signed = width, bool(signed)
        self.scalar_mont256 = bool(mont256)

    def skew_credit(self):
        """launches left that run k_fine_hist because an earlier 32-byte launch met a huge coarse bin (test hook)"""
        return lib().msm_hip_test_skew_credit(self._h)

    def env_report(self):
        """test hook: env_report() plus the shape of this context's last launch (last_wbits, last_chunk_len, last_planes, last_logr, ...)"""
        return env_report(self._h)

    def set_fine_hist_min_n(self, n):
        _check(lib().msm_hip_set_fine_hist_min_n(self._h, n), "msm_hip_set_fine_hist_min_n")

    def set_debug(self, keep_digit_planes=True):
        _check(lib().msm_hip_set_debug(self._h, 1 if keep_digit_planes else 0), "msm_hip_set_debug")

    def read_digits(self, n, w_count=NUM_WINDOWS):
        a = np.empty((w_count, n), dtype=np.uint16)
        _check(lib().msm_hip_read_digits(self._h, a.ctypes.data, a.size), "msm_hip_read_digits")
        return a

    def read_col_ptr(self, w_count=NUM_WINDOWS, buckets=BUCKETS_PER_WINDOW):
        a = np.empty((w_count, buckets + 1), dtype=np.uint32)
        _check(lib().msm_hip_read_col_ptr(self._h, a.ctypes.data, a.size), "msm_hip_read_col_ptr")
        return a

    def read_val_idxs(self, n, w_count=NUM_WINDOWS):
        a = np.empty((w_count, n), dtype=np.uint32)
        _check(lib().msm_hip_read_val_idxs(self._h, a.ctypes.data, a.size), "msm_hip_read_val_idxs")
        return a

    def read_buckets(self, w_count=NUM_WINDOWS, buckets=BUCKETS_PER_WINDOW):
        a = np.empty((w_count, buckets, self.jb), dtype=np.uint8)
        _check(lib().msm_hip_read_buckets(self._h, a.ctypes.data, a.size), "msm_hip_read_buckets")
        return a

    def read_window_sums(self, w_count=NUM_WINDOWS):
        a = np.empty((w_count, self.jb), dtype=np.uint8)
        _check(lib().msm_hip_read_window_sums(self._h, a.ctypes.data, a.size), "msm_hip_read_window_sums")
        return a

    # -- single-op hooks (≙ tests/field.rs, tests/point.rs)
    def fq_op(self, op, a, b=None):
        code = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "mul_asm": 5, "sqr_asm": 6, "mul2_asm": 7, "mul_asm_lazy": 8,
                "sqr_asm_lazy": 9}[op]
        n = len(a) // self.cb
        out = C.create_string_buffer(max(self.cb * n, 1))
        _check(lib().msm_hip_test_fq_op(self._h, code, a, b, out, n), "msm_hip_test_fq_op")
        return out.raw[:self.cb * n]

    def g1_op(self, op, a, b=None):
        code = {"add": 0, "double": 1, "add_affine": 2, "madd_w_pmp": 3, "madd_w_mm": 4}[op]
        n = len(a) // self.jb
        out = C.create_string_buffer(max(self.jb * n, 1))
        _check(lib().msm_hip_test_g1_op(self._h, code, a, b, out, n), "msm_hip_test_g1_op")
        return out.raw[:self.jb * n]

    def g1_mul_u32(self, a, ks):
        n = len(a) // self.jb
        k = np.ascontiguousarray(ks, dtype=np.uint32)
        out = C.create_string_buffer(max(self.jb * n, 1))
        _check(lib().msm_hip_test_g1_mul_u32(self._h, a, k.ctypes.data, out, n), "msm_hip_test_g1_mul_u32")
        return out.raw[:self.jb * n]


class MultiGpuMsm:
    """Several GPUs driven by ONE process through the C ABI (msm_hip_mgpu_*, include/msm_hip.h): windows of one MSM sharded
    over the devices + gather (RCCL or pinned buffers) + one host window combine; batches dealt out as whole MSMs.
    (bench.py's multi-GPU path is the other shape: one process per GPU over torch.distributed, msm-webgpu_amd/sharding.py.)"""

    GATHER = {"auto": 0, "host": 1, "rccl": 2}

    def __init__(self, device_ids, gather="auto", curve="bn254"):
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        self._h = C.c_void_p()
        self.curve = curve
        self.modulus = CURVES[curve][1]
        self.cb = coord_bytes(curve)
        self.pb, self.jb = 2 * self.cb, 3 * self.cb
        _check(lib().msm_hip_mgpu_create_curve(C.byref(self._h), ids, len(device_ids), self.GATHER[gather], CURVES[curve][0]), "msm_hip_mgpu_create_curve")

    def close(self):
        if self._h:
            lib().msm_hip_mgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_count(self):
        return lib().msm_hip_mgpu_device_count(self._h)

    @property
    def uses_rccl(self):
        return lib().msm_hip_mgpu_uses_rccl(self._h) == 1

    def set_bases(self, points, check_on_curve=False, endomorphism=False, precompute=False, zero_is_identity=False):
        """Replicated on every device.  endomorphism: True: MSM_HIP_BASES_ENDOMORPHISM -- msm_batch runs whole MSMs over the 2n points, and
        the window-sharded calls shard the 8 half-length windows; False: MSM_HIP_BASES_PLAIN; None: the C ABI's default (flags = 0: whole
        object resolves it to the plain set).  precompute: True -- the 16-bit fixed-base tables for the whole MSMs of msm_batch (the
        window-sharded calls ignore them); "wide" -- the wide tables: msm_batch runs whole MSMs on them and the window-sharded calls share
        their virtual windows (set_wide_bits; default 19-bit digits: 8 virtual windows).  zero_is_identity: as MsmContext.set_bases, on every device."""
        b = bytes(points)
        flags = (1 if check_on_curve else 0) | (8 if endomorphism else 0) | (32 if precompute == "wide" else 4 if precompute else 0)
        flags |= BASES_ZERO_IS_IDENTITY if zero_is_identity else 0
        if endomorphism is False and not precompute:
            flags |= 16
        _check(lib().msm_hip_mgpu_set_bases(self._h, b, len(b) // self.pb, flags), "msm_hip_mgpu_set_bases")
        return len(b) // self.pb

    def msm(self, scalars):
        b = bytes(scalars)
        out = C.create_string_buffer(self.jb)
        _check(lib().msm_hip_mgpu_run(self._h, b, len(b) // 32, out), "msm_hip_mgpu_run")
        return G1(out.raw, self.modulus)

    def msm_batch(self, scalars, n):
        b = bytes(scalars)
        batch = len(b) // (32 * n)
        out = C.create_string_buffer(max(self.jb * batch, 1))
        _check(lib().msm_hip_mgpu_run_batch(self._h, b, n, batch, out), "msm_hip_mgpu_run_batch")
        return [G1(out.raw[self.jb * k:self.jb * (k + 1)], self.modulus) for k in range(batch)]

    def set_wide_bits(self, bits):
        """digit width (16 .. 20; 0: 19) of the wide tables the next set_bases(precompute="wide") builds on every device"""
        _check(lib().msm_hip_mgpu_set_wide_bits(self._h, int(bits)), "msm_hip_mgpu_set_wide_bits")

    # -- window-sharded launches of several MSMs, asynchronous (the throughput form)
    @property
    def group_size(self):
        """MSMs per launch that fill a device (msm_hip_mgpu_group_size): 16 / windows per device (8 with endomorphism bases)."""
        return lib().msm_hip_mgpu_group_size(self._h)

    def launch_batch(self, scalars, n, slot=0, inputs_complete=False):
        """`scalars`: nvec x n x 32 B of host bytes (every device uploads them), or a list with one CUDA uint8 tensor per device
        holding the same bytes (inputs_complete: they were synchronised before this call; otherwise every tensor's current torch stream is
        waited for here).  Returns nvec; finish_batch(slot, nvec) collects."""
        if isinstance(scalars, (list, tuple)):
            ts = [_as_device_u8(t, 32, "scalars")[0] for t in scalars]
            rows = ts[0].numel() // 32
            if n <= 0 or rows % n or any(t.numel() != ts[0].numel() for t in ts):
                raise ValueError("every device needs the same whole number of n-element vectors")
            ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            if not inputs_complete:  # the header wants the device scalars complete before the call: wait for whatever torch still has queued on
                for t in ts:          # each tensor's device (the engine's streams are not ordered with torch's)
                    torch.cuda.current_stream(t.device).synchronize()
            _check(lib().msm_hip_mgpu_launch_batch_device(self._h, ptrs, n, rows // n, slot), "msm_hip_mgpu_launch_batch_device")
            self._keep = getattr(self, "_keep", {})
            self._keep[slot] = ts
            return rows // n
        b = bytes(scalars)
        if n <= 0 or len(b) % (32 * n):
            raise ValueError("scalars must hold a whole number of n-element vectors")
        self._keep = getattr(self, "_keep", {})
        self._keep[slot] = b  # the library reads the buffer until finish
        _check(lib().msm_hip_mgpu_launch_batch(self._h, b, n, len(b) // (32 * n), slot), "msm_hip_mgpu_launch_batch")
        return len(b) // (32 * n)

    def inject_fault(self, device_index, launches=1):
        """test hook (msm_hip_mgpu_inject_fault): the next `launches` window-sharded launches fail on that device"""
        _check(lib().msm_hip_mgpu_inject_fault(self._h, device_index, launches), "msm_hip_mgpu_inject_fault")

    def finish_batch(self, slot, nvec):
        out = C.create_string_buffer(self.jb * nvec)
        try:
            _check(lib().msm_hip_mgpu_finish_batch(self._h, slot, out), "msm_hip_mgpu_finish_batch")
        finally:
            getattr(self, "_keep", {}).pop(slot, None)
        return [G1(out.raw[self.jb * k:self.jb * (k + 1)], self.modulus) for k in range(nvec)]


def env_report(handle=None):
    """test hook: the MSM_HIP_* settings as the library resolved them and the part / upload-chunk counts of the last upload-bound call
    (msm_hip_test_env_report), as a dict of ints; `handle` (an MsmContext's) adds the shape of that context's last launch"""
    buf = C.create_string_buffer(4096)
    n = lib().msm_hip_test_env_report(handle, buf, len(buf))
    _check(min(n, 0), "msm_hip_test_env_report")
    return {k: int(v) for k, v in (line.split("=") for line in buf.raw[:n].decode().splitlines())}


def window_range_abi(rank, world, num=NUM_WINDOWS):
    """msm_hip_window_range: the C ABI's partition (must equal sharding.window_range)."""
    b, e = C.c_int(), C.c_int()
    _check(lib().msm_hip_window_range(rank, world, num, C.byref(b), C.byref(e)), "msm_hip_window_range")
    return b.value, e.value


# ------------------------------------------------------------------------------------------------ reference-shaped functions
_default_ctx = {}


def _ctx(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = MsmContext(device)
    return _default_ctx[device]


def compute_msm(points, scalars, device=0):
    """≙ compute_msm (src/cuzk/msm.rs:75): one-shot MSM including base upload; returns G1."""
    ctx = _ctx(device)
    n = ctx.set_bases(points, endomorphism=None)  # the ABI's default: the curve's fastest mode (same group element as the reference's shape)
    ns = (scalars.numel() if isinstance(scalars, torch.Tensor) else len(scalars)) // 32
    if ns != n:
        raise ValueError("points and scalars differ in length (%d vs %d)" % (n, ns))
    return ctx.msm(scalars)


def run_webgpu_msm(g, v, device=0):
    """≙ run_webgpu_msm (src/lib.rs:76-82); the name is the reference's, the device is an MI355X."""
    return compute_msm(g, v, device)


def sample_scalars(n, seed=0, device=0):
    """≙ sample_scalars (src/lib.rs:20-23), seeded; CUDA uint8 tensor [n, 32] in the wire format."""
    return _ctx(device).sample_scalars(n, seed)


def sample_points(n, seed=0, device=0):
    """≙ sample_points (src/lib.rs:36-42), seeded; CUDA uint8 tensor [n, 64] in the wire format."""
    return _ctx(device).sample_points(n, seed)
