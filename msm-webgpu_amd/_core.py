"""What the MSM surface (api.py) and the scalar-field surface (scalars.py) both stand on: the curves and their fields, the loader of
libmsm_hip.so with its error type, and the tensor and byte helpers of the wire format.  It imports neither of the two."""
import ctypes as C
import functools
import os

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


def _check(code, where):
    if code != 0:
        raise MsmHipError(code, where)


# ------------------------------------------------------------------------------------------------ wire format
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


# ------------------------------------------------------------------------------------------------ device tensors
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
