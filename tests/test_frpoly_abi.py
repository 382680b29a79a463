"""libmsm_frpoly.so in the C ABI (include/msm_frpoly.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version
1 beside the unchanged other three libraries, every bad argument is answered before a device is asked for, a call without a device fails with the
no-device code and leaves its buffers alone, and the Python methods raise before any library is reached."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG = -1, -2
SHARED_B, MONT256 = 1, 2
NAMES = ("eval", "divide", "dot", "combine", "powers")


def _header():
    with open(os.path.join(ROOT, "include", "msm_frpoly.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    for name, value in (("SHARED_B", "1u"), ("MONT256", "2u"), ("MAX_ROWS", "256")):
        assert re.search(r"#define MSM_FRPOLY_%s %s\s" % (name, value), text), name
    head = r"int curve, int device, void\* stream, "
    assert re.search(r"\bint msm_frpoly_eval_device\s*\(" + head + r"const void\* a, size_t n, size_t batch, const uint8_t\* z, uint32_t flags, uint8_t\* values_host\)", text)
    assert re.search(r"\bint msm_frpoly_divide_device\s*\(" + head + r"void\* out, const void\* a, size_t n, size_t batch, const uint8_t\* z, uint32_t flags,\s*"
                     r"uint8_t\* values_host\)", text)
    assert re.search(r"\bint msm_frpoly_dot_device\s*\(" + head + r"const void\* a, const void\* b, size_t n, size_t batch, uint32_t flags, uint8_t\* values_host\)", text)
    assert re.search(r"\bint msm_frpoly_combine_device\s*\(" + head + r"void\* out, const void\* a, size_t n, size_t batch, const uint8_t\* coeffs_host, uint32_t flags\)", text)
    assert re.search(r"\bint msm_frpoly_powers_device\s*\(" + head + r"void\* out, size_t n, const uint8_t\* g, const uint8_t\* c, uint32_t flags\)", text)
    for name in NAMES:
        assert re.search(r"\bint msm_frpoly_%s\s*\(int curve, int device, (const )?uint8_t\* " % name, text), name
    assert re.search(r"\bvoid msm_frpoly_release\s*\(void\)", text) and re.search(r"\bint msm_frpoly_abi_version\s*\(void\)", text)
    assert re.search(r"#ifdef MSM_FRPOLY_TEST_HOOKS\s+int msm_frpoly_test_tile\s*\(int elements\);\s+int msm_frpoly_test_last\s*\(int\* launches, int\* levels\);", text)
    full = open(os.path.join(ROOT, "include", "msm_frpoly.h")).read()
    assert "Grumpkin" in full and "MSM_HIP_ERR_INVALID_ARG" in full and "MSM_HIP_ERR_NONCANONICAL" in full  # (the header says what is not offered)
    L = api.frpoly_lib()
    for name in ["msm_frpoly_" + n + s for n in NAMES for s in ("", "_device")] + ["msm_frpoly_release", "msm_frpoly_abi_version", "msm_frpoly_test_tile",
                                                                                  "msm_frpoly_test_last"]:
        assert hasattr(L, name), name
    assert L.msm_frpoly_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7 and api.fr_lib().msm_fr_abi_version() == 1 and api.frvec_lib().msm_frvec_abi_version() == 1
    assert api.MsmContext.FRPOLY_SHARED_B == 1 and api.MsmContext.FRPOLY_MONT256 == 2 and api.MsmContext.FRPOLY_MAX_ROWS == 256
    for name in ("scalars_eval", "scalars_divide", "scalars_dot", "scalars_combine", "scalars_powers", "kzg_open"):
        assert callable(getattr(api.MsmContext, name)), name
    for name in ("frpoly_lib", "frpoly_test_tile", "frpoly_last", "frpoly_release"):
        assert callable(getattr(api, name)), name


def test_the_c_abi_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.frpoly_lib()
    r = api.SCALAR_FIELDS["bn254"]
    one, big = (1).to_bytes(32, "little"), r.to_bytes(32, "little")
    n = 4
    bufs = [C.create_string_buffer(bytes([7 + k]) * (32 * n), 32 * n) for k in range(3)]
    out, a, b = [C.cast(x, C.c_void_p) for x in bufs]
    val = C.create_string_buffer(32 * 4)
    v = C.cast(val, C.c_void_p)
    D = lambda off=0: C.c_void_p(4096 + off)  # noqa: E731  (a device address that is never touched: every check below comes first)
    inval = ERR_INVALID_ARG

    def every(curve=0, n=n, batch=1, z=one, flags=0, coeffs=one * 4):
        """each host form once, with the one argument under test changed"""
        return [L.msm_frpoly_eval(curve, 0, a, n, batch, z, flags, v), L.msm_frpoly_divide(curve, 0, out, a, n, batch, z, flags, None),
                L.msm_frpoly_dot(curve, 0, a, b, n, batch, flags, v), L.msm_frpoly_combine(curve, 0, out, a, n, batch, coeffs, flags),
                L.msm_frpoly_powers(curve, 0, out, n, z, one, flags)]

    assert every(curve=1) == [inval] * 5  # Grumpkin
    assert every(curve=7) == [inval] * 5  # no such curve
    assert every(n=0) == [inval] * 5  # the length
    assert every(batch=0)[:4] == [inval] * 4
    assert L.msm_frpoly_eval_device(0, 0, None, D(), 1 << 13, (1 << 13) + 1, one, 0, v) == inval  # batch * n > 2^26
    assert L.msm_frpoly_divide_device(0, 0, None, D(), D(), (1 << 26) + 1, 1, one, 0, None) == inval
    assert L.msm_frpoly_dot_device(0, 0, None, D(), D(), 3, 1 << 63, 0, v) == inval  # (... with a product that wraps)
    assert L.msm_frpoly_combine_device(0, 0, None, D(), D(), 1 << 20, 65, one * 65, 0) == inval
    assert L.msm_frpoly_powers_device(0, 0, None, D(), (1 << 26) + 1, one, one, 0) == inval
    assert L.msm_frpoly_combine_device(0, 0, None, D(), D(), 2, 257, one * 257, 0) == inval  # more than 256 rows
    # a constant >= r: z, g, c, a coefficient
    assert every(z=big)[:2] == [inval] * 2 and every(z=big)[4] == inval and every(z=b"\xff" * 32, flags=MONT256)[0] == inval
    assert L.msm_frpoly_powers(0, 0, out, n, one, big, 0) == inval
    assert L.msm_frpoly_combine(0, 0, out, a, 2, 2, one + big, 0) == inval
    # a missing pointer
    assert L.msm_frpoly_eval(0, 0, None, n, 1, one, 0, v) == inval and L.msm_frpoly_eval(0, 0, a, n, 1, None, 0, v) == inval and L.msm_frpoly_eval(0, 0, a, n, 1, one, 0, None) == inval
    assert L.msm_frpoly_divide(0, 0, None, a, n, 1, one, 0, None) == inval and L.msm_frpoly_dot(0, 0, a, None, n, 1, 0, v) == inval
    assert L.msm_frpoly_combine(0, 0, out, a, n, 1, None, 0) == inval and L.msm_frpoly_powers(0, 0, None, n, one, one, 0) == inval
    # an unaligned device pointer
    assert L.msm_frpoly_eval_device(0, 0, None, D(8), n, 1, one, 0, v) == inval
    assert L.msm_frpoly_divide_device(0, 0, None, D(4), D(1024), n, 1, one, 0, None) == inval and L.msm_frpoly_divide_device(0, 0, None, D(1024), D(8), n, 1, one, 0, None) == inval
    assert L.msm_frpoly_dot_device(0, 0, None, D(), D(1024 + 8), n, 1, 0, v) == inval
    assert L.msm_frpoly_combine_device(0, 0, None, D(8), D(1024), n, 1, one, 0) == inval and L.msm_frpoly_powers_device(0, 0, None, D(4), n, one, one, 0) == inval
    # an unknown flag; the shared b belongs to the dot product alone
    assert every(flags=4) == [inval] * 5
    res = every(flags=SHARED_B)
    assert res[:2] + res[3:] == [inval] * 4
    # a partial overlap of the output with the input (the same pointer is the in-place call, and passes on to the device check)
    assert L.msm_frpoly_divide_device(0, 0, None, D(32), D(), n, 1, one, 0, None) == inval
    assert L.msm_frpoly_divide_device(0, 0, None, D(32 * n), D(), n, 2, one, 0, None) == inval  # (the second row of the input)
    assert L.msm_frpoly_combine_device(0, 0, None, D(32 * n), D(), n, 2, one * 2, 0) == inval  # (row 1: only row 0 may be the output)
    assert L.msm_frpoly_combine_device(0, 0, None, D(32), D(), n, 1, one, 0) == inval
    # the hooks
    assert L.msm_frpoly_test_tile(1) == inval and L.msm_frpoly_test_tile(1025) == inval and L.msm_frpoly_test_tile(-3) == inval
    assert L.msm_frpoly_test_tile(2) == 0 and L.msm_frpoly_test_tile(1024) == 0 and L.msm_frpoly_test_tile(0) == 0
    assert L.msm_frpoly_test_last(None, None) == inval
    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        assert every() == [ERR_NO_DEVICE] * 5 and every(flags=MONT256, z=(r - 1).to_bytes(32, "little")) == [ERR_NO_DEVICE] * 5
        assert L.msm_frpoly_dot(4, 0, a, b, 2, 2, SHARED_B, v) == ERR_NO_DEVICE
        assert L.msm_frpoly_divide_device(0, 0, None, D(), D(), n, 1, one, 0, v) == ERR_NO_DEVICE  # in place
        assert L.msm_frpoly_divide_device(2, 0, None, D(32 * n), D(), n, 1, one, 0, None) == ERR_NO_DEVICE  # (apart: no overlap)
        assert L.msm_frpoly_combine_device(3, 0, None, D(), D(), n, 2, one * 2, 0) == ERR_NO_DEVICE  # in place on row 0
        assert L.msm_frpoly_combine_device(0, 0, None, D(64 * n), D(), n, 2, one * 2, 0) == ERR_NO_DEVICE
        assert L.msm_frpoly_eval_device(0, 0, None, D(), 1 << 13, 1 << 13, one, 0, v) == ERR_NO_DEVICE  # batch * n = 2^26 exactly
        assert L.msm_frpoly_combine_device(0, 0, None, D(), D(), 2, 256, one * 256, 0) == ERR_NO_DEVICE
        assert [x.raw for x in bufs] == before and val.raw == bytes(32 * 4)
    L.msm_frpoly_release()  # (nothing held: a no-op)


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
    for name in ("lib", "fr_lib", "frvec_lib", "frpoly_lib"):
        monkeypatch.setattr(scalars, name, no_call)
    r = api.SCALAR_FIELDS["bn254"]
    v = bytes(32 * 4)
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        _bare_context().scalars_eval(v, 1)

    def every_method(ctx):
        return [lambda: ctx.scalars_eval(v, 1), lambda: ctx.scalars_divide(v, 1), lambda: ctx.scalars_dot(v, v), lambda: ctx.scalars_combine(v, [1, 2]),
                lambda: ctx.scalars_powers(2, 4), lambda: ctx.kzg_open(v, 1)]

    for call in every_method(_bare_context("grumpkin")):  # Grumpkin
        with pytest.raises(ValueError):
            call()
    for width in (1, 8, 16):  # a narrow scalar format
        for call in every_method(_bare_context(width=width)):
            with pytest.raises(ValueError):
                call()
    ctx = _bare_context()
    for bad in (lambda: ctx.scalars_eval(bytes(33), 1),  # not whole scalars
                lambda: ctx.scalars_divide(bytes(31), 1),
                lambda: ctx.scalars_eval(b"", 1),  # nothing at all
                lambda: ctx.scalars_dot(b"", b""),
                lambda: ctx.scalars_eval(v, r),  # a constant >= r, or negative
                lambda: ctx.scalars_divide(v, -1),
                lambda: ctx.scalars_divide(v, b"\xff" * 32),
                lambda: ctx.scalars_eval(v, bytes(31)),
                lambda: ctx.scalars_combine(v, [1, r]),
                lambda: ctx.scalars_powers(r, 4),
                lambda: ctx.scalars_powers(2, 4, scale=r + 1),
                lambda: ctx.scalars_eval(v, 1, batch=3),  # rows that do not divide the vector
                lambda: ctx.scalars_divide(v, 1, batch=0),
                lambda: ctx.scalars_combine(v, [1, 2, 3]),
                lambda: ctx.scalars_combine(v, []),  # no row, too many rows
                lambda: ctx.scalars_combine(bytes(32 * 257), [1] * 257),
                lambda: ctx.scalars_dot(v, bytes(32 * 3)),  # a length mismatch
                lambda: ctx.scalars_dot(v, bytes(32 * 2), batch=1),
                lambda: ctx.scalars_powers(2, 0),  # a bad length
                lambda: ctx.scalars_powers(2, (1 << 26) + 1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):  # out belongs to device vectors
        ctx.scalars_divide(v, 1, out=bytearray(32 * 4))
