"""libmsm_frvec.so in the C ABI (include/msm_frvec.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version 1
beside an unchanged libmsm_hip.so (version 7) and libmsm_fr.so (version 1), every bad argument is answered before a device is asked for, a call
without a device fails with the no-device code and leaves its buffers alone, and the Python methods raise before any library is reached."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_NO_DEVICE, ERR_INVALID_ARG = -1, -2
ADD, SUB, MUL, MUL_ADD, MUL_SUB = range(5)
SUM, PRODUCT = 0, 1
EXCLUSIVE, MONT256 = 1, 2


def _header():
    with open(os.path.join(ROOT, "include", "msm_frvec.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    for name, value in (("EXCLUSIVE", "1u"), ("MONT256", "2u"), ("ADD", "0"), ("SUB", "1"), ("MUL", "2"), ("MUL_ADD", "3"), ("MUL_SUB", "4"), ("SUM", "0"), ("PRODUCT", "1")):
        assert re.search(r"#define MSM_FRVEC_%s %s\s" % (name, value), text), name
    assert re.search(r"\bint msm_frvec_map_device\s*\(int curve, int device, void\* stream, void\* out, const void\* a, const void\* b, const void\* c, size_t n, int op, "
                     r"const uint8_t\* b_const,\s*const uint8_t\* c_const, uint32_t flags\)", text)
    assert re.search(r"\bint msm_frvec_inverse_device\s*\(int curve, int device, void\* stream, void\* out, const void\* a, size_t n, uint32_t flags\)", text)
    assert re.search(r"\bint msm_frvec_scan_device\s*\(int curve, int device, void\* stream, void\* out, const void\* a, size_t n, size_t batch, int op, uint32_t flags, "
                     r"uint8_t\* totals_host\)", text)
    for name in ("map", "inverse", "scan"):
        assert re.search(r"\bint msm_frvec_%s\s*\(int curve, int device, uint8_t\* out, const uint8_t\* a," % name, text), name
    assert re.search(r"\bvoid msm_frvec_release\s*\(void\)", text) and re.search(r"\bint msm_frvec_abi_version\s*\(void\)", text)
    assert re.search(r"#ifdef MSM_FRVEC_TEST_HOOKS\s+int msm_frvec_test_tile\s*\(int elements\);\s+int msm_frvec_test_last\s*\(int\* launches, int\* levels\);", text)
    full = open(os.path.join(ROOT, "include", "msm_frvec.h")).read()
    assert "Grumpkin" in full and "MSM_HIP_ERR_INVALID_ARG" in full and "MSM_HIP_ERR_NONCANONICAL" in full  # (the header says what is not offered)
    L = api.frvec_lib()
    for name in ("msm_frvec_map_device", "msm_frvec_inverse_device", "msm_frvec_scan_device", "msm_frvec_map", "msm_frvec_inverse", "msm_frvec_scan", "msm_frvec_release",
                 "msm_frvec_abi_version", "msm_frvec_test_tile", "msm_frvec_test_last"):
        assert hasattr(L, name), name
    assert L.msm_frvec_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7 and api.fr_lib().msm_fr_abi_version() == 1  # (the other two libraries are what they were)
    assert api.MsmContext.FRVEC_EXCLUSIVE == 1 and api.MsmContext.FRVEC_MONT256 == 2
    for name in ("scalars_add", "scalars_sub", "scalars_mul", "scalars_mul_add", "scalars_mul_sub", "scalars_inverse", "scalars_scan"):
        assert callable(getattr(api.MsmContext, name)), name
    with open(os.path.join(ROOT, "include", "msm_hip.hpp")) as f:
        src = f.read()
    for name in ("scalars_add(", "scalars_sub(", "scalars_mul(", "scalars_mul_add(", "scalars_mul_sub(", "scalars_inverse(", "scalars_scan(", "msm_frvec_map_device(",
                 "msm_frvec_inverse_device(", "msm_frvec_scan_device("):
        assert name in src, name


def test_the_three_libraries_keep_their_units(built):
    import importlib

    import check_long_branch_hazard as chk

    b = importlib.import_module("msm_webgpu_amd.build")
    assert len(b.TRANSLATION_UNITS) == 8 and len(b.FR_LIBRARIES["fr"].units) == 4
    assert sorted(b.FR_LIBRARIES["frvec"].units) == ["frvec_bls12_381.hip", "frvec_bn254.hip", "frvec_pallas.hip", "frvec_vesta.hip"]
    assert not any(f.startswith("frvec_") for f in b.SOURCES + b.FR_LIBRARIES["fr"].sources)
    assert not any(f.startswith(("ntt_", "msm_", "curve_")) for f in b.FR_LIBRARIES["frvec"].sources)  # (no kernel of the other two)
    for u in b.FR_LIBRARIES["frvec"].units:
        assert os.path.exists(os.path.join(b.CSRC, u)) and u in b.FR_LIBRARIES["frvec"].sources
    assert os.path.basename(b.FR_LIBRARIES["frvec"].so) == "libmsm_frvec.so" and os.path.exists(b.FR_LIBRARIES["frvec"].so) and not b.needs_build(b.FR_LIBRARIES["frvec"])
    for path in chk.compile_to_asm([], units=b.FR_LIBRARIES["fr"].units):  # libmsm_fr.so still holds its one kernel per unit
        with open(path) as f:
            names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), flags=re.M)
        assert len(names) == 1 and "k_ntt_pass" in names[0], (path, names)


def test_the_c_abi_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.frvec_lib()
    r = api.SCALAR_FIELDS["bn254"]
    one, big = (1).to_bytes(32, "little"), r.to_bytes(32, "little")
    n = 4
    bufs = [C.create_string_buffer(bytes([7 + k]) * (32 * n), 32 * n) for k in range(4)]
    out, a, b, c = [C.cast(x, C.c_void_p) for x in bufs]
    D = lambda off=0: C.c_void_p(4096 + off)  # noqa: E731  (a device address that is never touched: every check below comes first)
    inval = ERR_INVALID_ARG
    # the field
    assert L.msm_frvec_map(1, 0, out, a, b, None, n, ADD, None, None, 0) == inval  # Grumpkin
    assert L.msm_frvec_inverse(1, 0, out, a, n, 0) == inval and L.msm_frvec_scan(1, 0, out, a, n, 1, SUM, 0, None) == inval
    assert L.msm_frvec_map(7, 0, out, a, b, None, n, ADD, None, None, 0) == inval  # no such curve
    # the length
    assert L.msm_frvec_map(0, 0, out, a, b, None, 0, ADD, None, None, 0) == inval
    assert L.msm_frvec_inverse(0, 0, out, a, 0, 0) == inval and L.msm_frvec_scan(0, 0, out, a, 0, 1, SUM, 0, None) == inval
    assert L.msm_frvec_scan(0, 0, out, a, n, 0, SUM, 0, None) == inval
    assert L.msm_frvec_map_device(0, 0, None, D(), D(), None, None, (1 << 26) + 1, ADD, one, None, 0) == inval
    assert L.msm_frvec_inverse_device(0, 0, None, D(), D(), (1 << 26) + 1, 0) == inval
    assert L.msm_frvec_scan_device(0, 0, None, D(), D(), 1 << 13, (1 << 13) + 1, SUM, 0, None) == inval  # batch * n > 2^26
    assert L.msm_frvec_scan_device(0, 0, None, D(), D(), 3, 1 << 63, SUM, 0, None) == inval  # (... with a product that wraps)
    # the pointers
    assert L.msm_frvec_map(0, 0, None, a, b, None, n, ADD, None, None, 0) == inval and L.msm_frvec_map(0, 0, out, None, b, None, n, ADD, None, None, 0) == inval
    assert L.msm_frvec_inverse(0, 0, out, None, n, 0) == inval and L.msm_frvec_scan(0, 0, None, a, n, 1, SUM, 0, None) == inval
    assert L.msm_frvec_map_device(0, 0, None, D(8), D(), None, None, n, ADD, one, None, 0) == inval  # misaligned: out, a, b, c
    assert L.msm_frvec_map_device(0, 0, None, D(), D(8), None, None, n, ADD, one, None, 0) == inval
    assert L.msm_frvec_map_device(0, 0, None, D(), D(), D(8 + 1024), None, n, ADD, None, None, 0) == inval
    assert L.msm_frvec_map_device(0, 0, None, D(), D(), None, D(8 + 1024), n, MUL_ADD, one, None, 0) == inval
    assert L.msm_frvec_inverse_device(0, 0, None, D(4), D(), n, 0) == inval and L.msm_frvec_scan_device(0, 0, None, D(), D(4), n, 1, SUM, 0, None) == inval
    # flags and ops
    assert L.msm_frvec_map(0, 0, out, a, b, None, n, ADD, None, None, 4) == inval and L.msm_frvec_map(0, 0, out, a, b, None, n, ADD, None, None, EXCLUSIVE) == inval
    assert L.msm_frvec_inverse(0, 0, out, a, n, EXCLUSIVE) == inval and L.msm_frvec_scan(0, 0, out, a, n, 1, SUM, 4, None) == inval
    assert L.msm_frvec_map(0, 0, out, a, b, None, n, 5, None, None, 0) == inval and L.msm_frvec_map(0, 0, out, a, b, None, n, -1, None, None, 0) == inval
    assert L.msm_frvec_scan(0, 0, out, a, n, 1, 2, 0, None) == inval and L.msm_frvec_scan(0, 0, out, a, n, 1, -1, 0, None) == inval
    # an operand given twice, or missing
    assert L.msm_frvec_map(0, 0, out, a, b, None, n, MUL, one, None, 0) == inval and L.msm_frvec_map(0, 0, out, a, None, None, n, MUL, None, None, 0) == inval
    assert L.msm_frvec_map(0, 0, out, a, b, c, n, MUL_ADD, None, one, 0) == inval and L.msm_frvec_map(0, 0, out, a, b, None, n, MUL_SUB, None, None, 0) == inval
    assert L.msm_frvec_map(0, 0, out, a, b, c, n, SUB, None, None, 0) == inval and L.msm_frvec_map(0, 0, out, a, b, None, n, ADD, None, one, 0) == inval  # (c is not read)
    # a constant >= r
    assert L.msm_frvec_map(0, 0, out, a, None, None, n, ADD, big, None, 0) == inval and L.msm_frvec_map(0, 0, out, a, b, None, n, MUL_ADD, None, big, 0) == inval
    assert L.msm_frvec_map(0, 0, out, a, None, None, n, MUL, b"\xff" * 32, None, MONT256) == inval
    # a partial overlap of the output with an input (the same pointer is the in-place call, and passes on to the device check)
    assert L.msm_frvec_map_device(0, 0, None, D(32), D(), None, None, n, ADD, one, None, 0) == inval
    assert L.msm_frvec_map_device(0, 0, None, D(), D(1024), D(96), None, n, ADD, None, None, 0) == inval
    assert L.msm_frvec_map_device(0, 0, None, D(64), D(1024), D(2048), D(), n, MUL_ADD, None, None, 0) == inval
    assert L.msm_frvec_inverse_device(0, 0, None, D(), D(32 * n - 32), n, 0) == inval
    assert L.msm_frvec_scan_device(0, 0, None, D(32), D(), n, 2, PRODUCT, 0, None) == inval
    assert L.msm_frvec_scan_device(0, 0, None, D(32 * n), D(), n, 2, PRODUCT, 0, None) == inval  # (the second row of the input)
    # the hooks
    assert L.msm_frvec_test_tile(1) == inval and L.msm_frvec_test_tile(1025) == inval and L.msm_frvec_test_tile(-3) == inval
    assert L.msm_frvec_test_tile(2) == 0 and L.msm_frvec_test_tile(0) == 0
    assert L.msm_frvec_test_last(None, None) == inval
    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        tot = C.create_string_buffer(32)
        assert L.msm_frvec_map(0, 0, out, a, b, None, n, ADD, None, None, 0) == ERR_NO_DEVICE
        assert L.msm_frvec_map(0, 0, a, a, None, c, n, MUL_SUB, one, None, MONT256) == ERR_NO_DEVICE  # in place
        assert L.msm_frvec_inverse(4, 0, out, a, n, 0) == ERR_NO_DEVICE and L.msm_frvec_scan(2, 0, out, a, 2, 2, PRODUCT, EXCLUSIVE, C.cast(tot, C.c_void_p)) == ERR_NO_DEVICE
        assert L.msm_frvec_map_device(0, 0, None, D(), D(), None, None, n, ADD, one, None, 0) == ERR_NO_DEVICE
        assert L.msm_frvec_map_device(0, 0, None, D(32 * n), D(), D(64 * n), None, n, ADD, None, None, 0) == ERR_NO_DEVICE  # (apart: no overlap)
        assert L.msm_frvec_inverse_device(0, 0, None, D(), D(), n, 0) == ERR_NO_DEVICE
        assert L.msm_frvec_scan_device(0, 0, None, D(), D(), 1 << 13, 1 << 13, SUM, 0, None) == ERR_NO_DEVICE  # batch * n = 2^26 exactly
        assert [x.raw for x in bufs] == before and tot.raw == bytes(32)
    L.msm_frvec_release()  # (nothing held: a no-op)


def _bare_context(curve="bn254", width=32):
    """An MsmContext that never touched the library (no device needed)"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.scalar_width, ctx.scalar_signed, ctx.scalar_mont256, ctx.n_bases, ctx._keepalive = curve, width, False, False, 0, {}
    ctx.curve_id, ctx.modulus = api.CURVES[curve]
    ctx.device = 0
    return ctx


def test_bad_arguments_raise_before_any_library_call(built, monkeypatch):
    from msm_webgpu_amd import api

    def no_call():
        raise AssertionError("the library was called")

    from msm_webgpu_amd import scalars  # (where the wrappers look the loaders up)

    monkeypatch.setattr(api, "lib", no_call)
    monkeypatch.setattr(scalars, "lib", no_call)
    monkeypatch.setattr(scalars, "fr_lib", no_call)
    monkeypatch.setattr(scalars, "frvec_lib", no_call)
    r = api.SCALAR_FIELDS["bn254"]
    v = bytes(32 * 4)
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        _bare_context().scalars_add(v, v)

    def every_method(ctx):
        return [lambda: ctx.scalars_add(v, v), lambda: ctx.scalars_sub(v, 1), lambda: ctx.scalars_mul(v, v), lambda: ctx.scalars_mul_add(v, v, 1),
                lambda: ctx.scalars_mul_sub(v, 2, v), lambda: ctx.scalars_inverse(v), lambda: ctx.scalars_scan(v)]

    for call in every_method(_bare_context("grumpkin")):  # Grumpkin
        with pytest.raises(ValueError):
            call()
    for width in (1, 2, 4, 8, 16):  # a narrow scalar format
        for call in every_method(_bare_context(width=width)):
            with pytest.raises(ValueError):
                call()
    ctx = _bare_context()
    for bad in (lambda: ctx.scalars_add(v, bytes(32 * 3)),  # a length mismatch
                lambda: ctx.scalars_mul(v, bytes(32 * 5)),
                lambda: ctx.scalars_mul_add(v, v, bytes(32 * 3)),
                lambda: ctx.scalars_mul_sub(v, bytes(64), 1),
                lambda: ctx.scalars_add(bytes(33), 1),  # not whole scalars
                lambda: ctx.scalars_inverse(bytes(31)),
                lambda: ctx.scalars_scan(bytes(65)),
                lambda: ctx.scalars_add(b"", 1),  # nothing at all
                lambda: ctx.scalars_inverse(b""),
                lambda: ctx.scalars_scan(b""),
                lambda: ctx.scalars_add(v, r),  # a constant >= r, or negative
                lambda: ctx.scalars_sub(v, r.to_bytes(32, "little")),
                lambda: ctx.scalars_mul(v, -1),
                lambda: ctx.scalars_mul_add(v, 1, r + 5),
                lambda: ctx.scalars_mul_sub(v, b"\xff" * 32, 1),
                lambda: ctx.scalars_mul_add(v, v, None),  # a missing operand
                lambda: ctx.scalars_scan(v, op="max"),  # a bad op
                lambda: ctx.scalars_scan(v, op=1),
                lambda: ctx._frvec_map("div", v, v, None, None),
                lambda: ctx.scalars_scan(v, batch=3),  # rows that do not divide the vector
                lambda: ctx.scalars_scan(v, batch=0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):  # out belongs to device vectors
        ctx.scalars_inverse(v, out=bytearray(32 * 4))
