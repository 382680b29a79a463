"""libmsm_frmat.so in the C ABI (include/msm_frmat.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version 1
beside the unchanged other five libraries, a matrix is checked and planned on the host alone -- so a handle exists without a device --, every bad
argument of create and mul is answered before a device is asked for, a product without a device fails with the no-device code and leaves its
buffers alone, and the Python methods raise before any library is reached."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG, ERR_NONCANONICAL = -1, -2, -4
MONT256, WITH_TRANSPOSE, TRANSPOSE = 2, 4, 8


def _header():
    with open(os.path.join(ROOT, "include", "msm_frmat.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    for name, value in (("MONT256", "2u"), ("WITH_TRANSPOSE", "4u"), ("TRANSPOSE", "8u")):
        assert re.search(r"#define MSM_FRMAT_%s %s\s" % (name, value), text), name
    assert re.search(r"typedef struct msm_frmat msm_frmat;", text)
    assert re.search(r"\bint msm_frmat_abi_version\s*\(void\)", text)
    assert re.search(r"\bint msm_frmat_create\s*\(int curve, int device, size_t rows, size_t cols, size_t nnz, const uint32_t\* row_ptr, const uint32_t\* col_idx, "
                     r"const uint8_t\* values, uint32_t flags,\s*msm_frmat\*\* out\)", text)
    assert re.search(r"\bint msm_frmat_info\s*\(const msm_frmat\* m, size_t\* rows, size_t\* cols, size_t\* nnz, uint32_t\* flags\)", text)
    assert re.search(r"\bvoid msm_frmat_destroy\s*\(msm_frmat\* m\)", text)
    assert re.search(r"\bint msm_frmat_mul_device\s*\(const msm_frmat\* m, void\* stream, void\* y, size_t y_len, const void\* x, size_t x_len, uint32_t flags\)", text)
    assert re.search(r"\bint msm_frmat_mul\s*\(const msm_frmat\* m, uint8_t\* y, size_t y_len, const uint8_t\* x, size_t x_len, uint32_t flags\)", text)
    assert re.search(r"\bvoid msm_frmat_release\s*\(void\)", text)
    assert re.search(r"#ifdef MSM_FRMAT_TEST_HOOKS\s+int msm_frmat_test_tile\s*\(int entries\);\s+int msm_frmat_test_last\s*\(int\* launches, int\* levels\);", text)
    full = open(os.path.join(ROOT, "include", "msm_frmat.h")).read()
    for said in ("MSM_HIP_ERR_INVALID_ARG", "MSM_HIP_ERR_NONCANONICAL", "is not read", "ZERO", "Grumpkin", "2^26", "2^28"):  # (the conventions are stated)
        assert said in full, said
    L = api.frmat_lib()
    names = ["abi_version", "create", "info", "destroy", "mul_device", "mul", "release", "test_tile", "test_last"]
    for name in names:
        assert hasattr(L, "msm_frmat_" + name), name
    declared = set(re.findall(r"\b(msm_frmat_\w+)\s*\(", text))
    assert declared == {"msm_frmat_" + n for n in names}  # the header and the library agree, name by name
    out = os.popen("nm -D --defined-only %s" % api._build.FR_LIBRARIES["frmat"].so).read()
    assert set(re.findall(r" T (msm_frmat_(?!ops_)\w+)", out)) == declared
    assert L.msm_frmat_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7 and api.fr_lib().msm_fr_abi_version() == 1 and api.frvec_lib().msm_frvec_abi_version() == 1
    assert api.frpoly_lib().msm_frpoly_abi_version() == 1 and api.frmle_lib().msm_frmle_abi_version() == 1
    Mc = api.MsmContext
    assert (Mc.FRMAT_MONT256, Mc.FRMAT_WITH_TRANSPOSE, Mc.FRMAT_TRANSPOSE) == (2, 4, 8)
    for name in ("scalars_matrix", "scalars_matvec", "r1cs_tables"):
        assert callable(getattr(Mc, name)), name
    for name in ("frmat_lib", "frmat_test_tile", "frmat_last", "frmat_release", "FrMatrix"):
        assert callable(getattr(api, name)), name


def _u32(v):
    return np.array(v, dtype=np.uint32)


def _create(L, rows, cols, ptr, idx, val, curve=0, device=0, flags=0, nnz=None, r_ok=True):
    """-> (code, handle)"""
    h = C.c_void_p()
    p, i = (None if ptr is None else _u32(ptr)), (None if idx is None else _u32(idx))
    vb = None if val is None else b"".join(int(v).to_bytes(32, "little") for v in val)
    n = (len(idx) if idx is not None else 0) if nnz is None else nnz
    code = L.msm_frmat_create(curve, device, rows, cols, n, None if p is None else p.ctypes.data, None if i is None or not i.size else i.ctypes.data,
                              None if not vb else C.cast(C.c_char_p(vb), C.c_void_p), flags, C.byref(h))
    return code, h


def test_create_checks_the_matrix_on_the_host_and_needs_no_device(built):
    from msm_webgpu_amd import api

    L = api.frmat_lib()
    r = api.SCALAR_FIELDS["bn254"]
    inval = ERR_INVALID_ARG
    ptr, idx, val = [0, 2, 3], [1, 0, 1], [5, r - 1, 0]
    for curve in range(7):  # every curve has its field here, Grumpkin included
        code, h = _create(L, 2, 2, ptr, idx, [5, 1, 0], curve=curve, flags=WITH_TRANSPOSE)
        assert code == 0 and h.value, curve
        rows, cols, nnz, flags = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint32()
        assert L.msm_frmat_info(h, C.byref(rows), C.byref(cols), C.byref(nnz), C.byref(flags)) == 0
        assert (rows.value, cols.value, nnz.value, flags.value) == (2, 2, 3, WITH_TRANSPOSE)
        assert L.msm_frmat_info(h, None, None, None, None) == 0
        L.msm_frmat_destroy(h)
    assert L.msm_frmat_info(None, None, None, None, None) == inval
    L.msm_frmat_destroy(None)  # (nothing)

    def bad(*a, **k):
        code, h = _create(L, *a, **k)
        assert not h.value
        return code

    assert bad(2, 2, ptr, idx, val, curve=7) == inval and bad(2, 2, ptr, idx, val, curve=-1) == inval  # no such curve
    assert bad(2, 2, ptr, idx, val, device=-1) == inval
    for flags in (1, 2, 8, 16, WITH_TRANSPOSE | 1):  # an unknown flag (MONT256 and TRANSPOSE belong to mul)
        assert bad(2, 2, ptr, idx, val, flags=flags) == inval, flags
    assert L.msm_frmat_create(0, 0, 2, 2, 3, _u32(ptr).ctypes.data, _u32(idx).ctypes.data, None, 0, None) == inval  # nowhere to put the handle
    # the limits: they come before any array is read
    assert bad(0, 2, [0], [], []) == inval and bad(2, 0, ptr, idx, val) == inval
    assert bad((1 << 26) + 1, 2, None, None, None) == inval and bad(2, (1 << 26) + 1, ptr, idx, val) == inval
    assert bad(2, 2, None, None, None, nnz=(1 << 28) + 1) == inval
    code, h = _create(L, 1, 1 << 26, [0, 1], [(1 << 26) - 1], [1])  # 2^26 columns, the last one in use
    assert code == 0
    L.msm_frmat_destroy(h)
    code, h = _create(L, 1, 1, [0, 0], [], [])  # no entry at all
    assert code == 0
    L.msm_frmat_destroy(h)
    # a missing array
    assert bad(2, 2, None, idx, val) == inval and bad(2, 2, ptr, None, val, nnz=3) == inval and bad(2, 2, ptr, idx, None) == inval
    # the structure
    assert bad(2, 2, [1, 2, 3], idx, val) == inval  # row_ptr[0] != 0
    assert bad(2, 2, [0, 2, 2], idx, val) == inval and bad(2, 2, [0, 2, 4], idx, val) == inval  # row_ptr[rows] != nnz
    assert bad(2, 2, [0, 4, 3], idx, val) == inval and bad(3, 2, [0, 2, 1, 3], idx, val) == inval  # a step down
    assert bad(2, 2, ptr, [1, 2, 1], val) == inval and bad(2, 2, ptr, [1, 0, 0xffffffff], val) == inval  # a column >= cols
    # a value >= r
    for v in (r, r + 1, (1 << 256) - 1):
        assert bad(2, 2, ptr, idx, [5, v, 0]) == ERR_NONCANONICAL and bad(2, 2, ptr, idx, [5, 1, v], flags=WITH_TRANSPOSE) == ERR_NONCANONICAL
    assert bad(2, 2, ptr, [1, 2, 1], [r, 1, 1]) == inval  # both faults: the structure's is reported
    assert _create(L, 2, 2, ptr, idx, [5, api.SCALAR_FIELDS["bls12_381"] - 1, 0], curve=4)[0] == 0  # (each field its own r) ...
    assert bad(2, 2, ptr, idx, [5, api.SCALAR_FIELDS["bls12_381"] - 1, 0], curve=0) == ERR_NONCANONICAL  # ... which BN254's is below


def test_mul_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.frmat_lib()
    inval = ERR_INVALID_ARG
    rows, cols = 3, 5
    ptr, idx, val = [0, 2, 2, 4], [4, 0, 1, 1], [1, 2, 3, 4]
    code, plain = _create(L, rows, cols, ptr, idx, val)
    code2, both = _create(L, rows, cols, ptr, idx, val, flags=WITH_TRANSPOSE)
    assert code == 0 and code2 == 0
    D = lambda off=0: C.c_void_p(1 << 20 | off)  # noqa: E731  (a device address that is never touched: every check below comes first)
    X, Y = D(), D(4096)
    bufs = [C.create_string_buffer(bytes([7 + k]) * (32 * 8), 32 * 8) for k in range(2)]
    hy, hx = [C.cast(b, C.c_void_p) for b in bufs]
    assert L.msm_frmat_mul_device(None, None, Y, rows, X, cols, 0) == inval and L.msm_frmat_mul(None, hy, rows, hx, cols, 0) == inval  # no handle
    assert L.msm_frmat_mul_device(plain, None, None, rows, X, cols, 0) == inval and L.msm_frmat_mul_device(plain, None, Y, rows, None, cols, 0) == inval
    assert L.msm_frmat_mul(plain, None, rows, hx, cols, 0) == inval and L.msm_frmat_mul(plain, hy, rows, None, cols, 0) == inval
    for flags in (1, 4, 16, MONT256 | 1):  # an unknown flag (WITH_TRANSPOSE belongs to create)
        assert L.msm_frmat_mul_device(both, None, Y, rows, X, cols, flags) == inval and L.msm_frmat_mul(both, hy, rows, hx, cols, flags) == inval, flags
    # TRANSPOSE on a handle made without WITH_TRANSPOSE
    assert L.msm_frmat_mul_device(plain, None, Y, cols, X, rows, TRANSPOSE) == inval and L.msm_frmat_mul(plain, hy, cols, hx, rows, TRANSPOSE | MONT256) == inval
    # x_len: cols, or rows with TRANSPOSE
    for x_len in (cols - 1, cols + 1, rows, 0):
        assert L.msm_frmat_mul_device(both, None, Y, rows, X, x_len, 0) == inval and L.msm_frmat_mul(both, hy, rows, hx, x_len, 0) == inval, x_len
    assert L.msm_frmat_mul_device(both, None, Y, cols, X, cols, TRANSPOSE) == inval and L.msm_frmat_mul(both, hy, cols, hx, rows + 1, TRANSPOSE) == inval
    # y_len: at least rows (cols with TRANSPOSE), at most 2^26
    assert L.msm_frmat_mul_device(both, None, Y, rows - 1, X, cols, 0) == inval and L.msm_frmat_mul(both, hy, 0, hx, cols, 0) == inval
    assert L.msm_frmat_mul_device(both, None, Y, cols - 1, X, rows, TRANSPOSE) == inval and L.msm_frmat_mul(both, hy, rows, hx, rows, TRANSPOSE) == inval
    assert L.msm_frmat_mul_device(both, None, C.c_void_p(1 << 40), (1 << 26) + 1, X, cols, 0) == inval
    # an unaligned device pointer
    assert L.msm_frmat_mul_device(both, None, D(4096 + 8), rows, X, cols, 0) == inval and L.msm_frmat_mul_device(both, None, Y, rows, D(4), cols, 0) == inval
    # x and y overlap: the same vector, y inside x, x inside a padded y
    assert L.msm_frmat_mul_device(both, None, X, rows, X, cols, 0) == inval
    assert L.msm_frmat_mul_device(both, None, D(32 * (cols - 1)), rows, X, cols, 0) == inval
    assert L.msm_frmat_mul_device(both, None, X, 8, D(32 * 7), cols, 0) == inval
    assert L.msm_frmat_mul(both, hx, rows, hx, cols, 0) == inval
    # the hooks
    for bad in (1, 3, 6, 1025, 2048, -4):
        assert L.msm_frmat_test_tile(bad) == inval, bad
    assert L.msm_frmat_test_tile(2) == 0 and L.msm_frmat_test_tile(1024) == 0 and L.msm_frmat_test_tile(0) == 0
    assert L.msm_frmat_test_last(None, None) == inval
    if not torch.cuda.is_available():
        before = [b.raw for b in bufs]
        assert L.msm_frmat_mul_device(both, None, Y, rows, X, cols, 0) == ERR_NO_DEVICE and L.msm_frmat_mul(both, hy, rows, hx, cols, MONT256) == ERR_NO_DEVICE
        assert L.msm_frmat_mul_device(both, None, Y, cols, X, rows, TRANSPOSE) == ERR_NO_DEVICE and L.msm_frmat_mul(plain, hy, 8, hx, cols, 0) == ERR_NO_DEVICE
        assert L.msm_frmat_mul_device(both, None, D(32 * cols), rows, X, cols, 0) == ERR_NO_DEVICE  # (y right behind x: apart)
        assert L.msm_frmat_mul_device(both, None, C.c_void_p(1 << 40), 1 << 26, X, cols, 0) == ERR_NO_DEVICE  # y_len = 2^26 exactly
        assert [b.raw for b in bufs] == before
    L.msm_frmat_destroy(plain)
    L.msm_frmat_destroy(both)
    L.msm_frmat_release()  # (nothing held: a no-op)


def _bare_context(curve="bn254", width=32):
    """An MsmContext that never touched the library (no device needed)"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.scalar_width, ctx.scalar_signed, ctx.scalar_mont256, ctx.n_bases, ctx._keepalive = curve, width, False, False, 0, {}
    ctx.curve_id, ctx.modulus = api.CURVES[curve]
    ctx.device = 0
    return ctx


def test_the_python_mirror(built, monkeypatch):
    from msm_webgpu_amd import api

    r = api.SCALAR_FIELDS["bn254"]
    ptr, idx, val = [0, 2, 2, 4], [4, 0, 1, 1], [1, 2, 3, r - 1]
    for curve in ("bn254", "grumpkin", "bn254_g2", "bls12_381"):  # a matrix needs no device: every field, a G2 context its G1's
        ctx = _bare_context(curve)
        for indices in ((ptr, idx), (np.array(ptr, dtype=np.int64), torch.tensor(idx, dtype=torch.int32)), (tuple(ptr), np.array(idx, dtype=np.uint16))):
            mat = ctx.scalars_matrix(3, 5, indices[0], indices[1], val, transpose=True)
            assert (mat.rows, mat.cols, mat.nnz, mat.has_transpose, mat.curve) == (3, 5, 4, True, curve)
            mat.close()
            mat.close()  # (twice is once)
        mat = ctx.scalars_matrix(3, 5, ptr, idx, b"".join(v.to_bytes(32, "little") for v in val))
        assert not mat.has_transpose
        del mat
    ctx = _bare_context()
    mat = ctx.scalars_matrix(3, 5, ptr, idx, val)
    x = bytes(32 * 5)

    def no_call():
        raise AssertionError("the library was called")

    from msm_webgpu_amd import scalars  # (where the wrappers look the loaders up)

    monkeypatch.setattr(scalars, "frmat_lib", no_call)  # (the good call at the end shows that the trap sits in the path)
    for bad in (lambda: ctx.scalars_matrix(0, 5, [0], [], []),
                lambda: ctx.scalars_matrix(3, (1 << 26) + 1, ptr, idx, val),
                lambda: ctx.scalars_matrix(3, 5, ptr[:-1], idx, val),  # row_ptr: its length, its ends, a step down
                lambda: ctx.scalars_matrix(3, 5, [1, 2, 2, 4], idx, val),
                lambda: ctx.scalars_matrix(3, 5, [0, 2, 2, 3], idx, val),
                lambda: ctx.scalars_matrix(3, 5, [0, 3, 2, 4], idx, val),
                lambda: ctx.scalars_matrix(3, 5, ptr, [4, 0, 5, 1], val),  # a column
                lambda: ctx.scalars_matrix(3, 5, ptr, [4, 0, -1, 1], val),
                lambda: ctx.scalars_matrix(3, 5, ptr, [[4, 0], [1, 1]], val),
                lambda: ctx.scalars_matrix(3, 5, ptr, [4.0, 0.0, 1.0, 1.0], val),
                lambda: ctx.scalars_matrix(3, 5, ptr, idx, [1, 2, 3, r]),  # a value
                lambda: ctx.scalars_matrix(3, 5, ptr, idx, [1, 2, 3, -1]),
                lambda: ctx.scalars_matrix(3, 5, ptr, idx, val[:3]),
                lambda: ctx.scalars_matrix(3, 5, ptr, idx, bytes(32 * 4 + 1)),
                lambda: ctx.scalars_matvec(mat, bytes(32 * 4)),  # x: its length
                lambda: ctx.scalars_matvec(mat, bytes(33)),
                lambda: ctx.scalars_matvec(mat, x, transpose=True),  # made without the transposed structure
                lambda: ctx.scalars_matvec(mat, x, pad_to=2),
                lambda: ctx.scalars_matvec(mat, x, pad_to=(1 << 26) + 1),
                lambda: _bare_context("grumpkin").scalars_matvec(mat, x),  # another field's matrix
                lambda: _bare_context(width=8).scalars_matvec(mat, x),  # a narrow scalar format
                lambda: _bare_context(width=16).scalars_matrix(3, 5, ptr, idx, val),
                lambda: ctx.r1cs_tables(mat, mat, object(), x),
                lambda: ctx.r1cs_tables(mat, mat, mat, x, n=3)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ctx.scalars_matvec(object(), x), lambda: ctx.scalars_matvec(mat, x, out=bytearray(32 * 3)), lambda: ctx.r1cs_tables(mat, mat, mat, x)):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(AssertionError, match="the library was called"):  # a good call gets as far as the library
        ctx.scalars_matvec(mat, x, pad_to=4)
    monkeypatch.undo()
    mat.close()
    with pytest.raises(TypeError):  # closed
        ctx.scalars_matvec(mat, x)
