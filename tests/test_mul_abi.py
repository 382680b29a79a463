"""The batch scalar multiplication calls of the C ABI (include/msm_hip.h: msm_hip_mul_each, msm_hip_mul_base and their _device forms) and
their mirrors, without a GPU: the symbols are declared and exported, fail loudly without a device, the Python binding and the C++ wrapper
have their methods, bad arguments raise before anything reaches the library, and bytes_to_points inverts points_to_bytes."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUL = ("msm_hip_mul_each", "msm_hip_mul_each_device", "msm_hip_mul_base", "msm_hip_mul_base_device")


def _header():
    with open(os.path.join(ROOT, "include", "msm_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_mul_symbols_are_declared_and_exported(built):
    import msm_webgpu_amd as m

    text = _header()
    assert re.search(r"#define MSM_HIP_MUL_BASES_ORDER_R 1u", text)
    for name in MUL:
        assert re.search(r"\bint %s\s*\(msm_hip_ctx\* ctx, " % name, text), name
        assert hasattr(m.lib(), name), name
    assert re.search(r"\bint msm_hip_test_mul_last\s*\(const msm_hip_ctx\* ctx, int\* path, int\* table_bits, int\* chunk\)", text)
    assert hasattr(m.lib(), "msm_hip_test_mul_last")
    assert re.search(r"\bint msm_hip_test_mul_policy\s*\(msm_hip_ctx\* ctx, size_t table_min_n, int table_bits\)", text)
    assert hasattr(m.lib(), "msm_hip_test_mul_policy")
    assert m.lib().msm_hip_abi_version() == 7  # (the calls arrived within version 7)


def test_mul_calls_without_a_device_fail_loudly(built):
    import msm_webgpu_amd as m

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = m.lib()
    out = C.create_string_buffer(64)
    assert L.msm_hip_mul_each(None, bytes(32), 1, out, 0) == -1
    assert L.msm_hip_mul_each_device(None, None, 0, None, 0) == -1
    assert L.msm_hip_mul_base(None, 0, bytes(32), 1, out, 0) == -1
    assert L.msm_hip_mul_base_device(None, 0, None, 0, None, 0) == -1


def test_python_binding_has_the_mul_methods(built):
    import msm_webgpu_amd as m
    from msm_webgpu_amd import api

    assert callable(api.MsmContext.mul_each)
    assert callable(api.MsmContext.mul_base)
    assert callable(api.bytes_to_points) and m.bytes_to_points is api.bytes_to_points


def test_cpp_wrapper_has_the_mul_methods():
    with open(os.path.join(ROOT, "include", "msm_hip.hpp")) as f:
        src = f.read()
    for name in ("mul_each(", "mul_each_device(", "mul_base(", "mul_base_device("):
        assert name in src, name


def _bare_context(n_bases, width=32):
    """An MsmContext that never touched the library (no device needed): n_bases as after set_bases"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.cb, ctx.pb, ctx.jb, ctx.scalar_width, ctx.scalar_signed, ctx.n_bases, ctx._keepalive = "bn254", 32, 64, 96, width, False, n_bases, {}
    ctx.curve_id, ctx.modulus = api.CURVES["bn254"]
    return ctx


def test_bad_arguments_raise_before_any_library_call(built, monkeypatch):
    from msm_webgpu_amd import api

    def no_call():
        raise AssertionError("the library was called")

    monkeypatch.setattr(api, "lib", no_call)
    ctx = _bare_context(8)
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        ctx.mul_each(bytes(32))
    for call in (lambda s, **kw: ctx.mul_each(s, **kw), lambda s, **kw: ctx.mul_base(0, s, **kw)):
        with pytest.raises(ValueError):  # not a whole number of 32-byte scalars
            call(bytes(33))
        with pytest.raises(TypeError):   # `out` belongs to the device form
            call(bytes(32), out=bytearray(64))
    with pytest.raises(ValueError):
        ctx.mul_base(-1, bytes(32))
    for width in (1, 2, 4, 8, 16):       # a narrow format set on the context: 32-byte scalars only
        narrow = _bare_context(8, width)
        with pytest.raises(ValueError):
            narrow.mul_each(bytes(32))
        with pytest.raises(ValueError):
            narrow.mul_base(0, bytes(32))


def test_bytes_to_points_inverts_points_to_bytes(built):
    from msm_webgpu_amd import api
    from oracle import bn254_ref as ref

    pts = ref.sample_points(5, 6)
    seq = [None, pts[0], pts[1], None, None, pts[2], None]
    raw = api.points_to_bytes(seq, zero_is_identity=True)
    assert api.bytes_to_points(raw) == seq
    assert api.points_to_bytes(api.bytes_to_points(raw), zero_is_identity=True) == raw
    assert api.bytes_to_points(b"") == []
    with pytest.raises(ValueError):
        api.bytes_to_points(bytes(65))
    # the other wire formats: 48-byte coordinates, and Fq2 coordinates c0 || c1
    rec = b"".join(int(v).to_bytes(48, "little") for v in (7, 9))
    assert api.bytes_to_points(rec + bytes(96), "bls12_381") == [(7, 9), None]
    rec = b"".join(int(v).to_bytes(32, "little") for v in (1, 2, 3, 4))
    assert api.bytes_to_points(bytes(128) + rec, "bn254_g2") == [None, ((1, 2), (3, 4))]
