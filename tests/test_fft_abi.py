"""The group FFT over the resident bases in the C ABI (include/msm_hip.h: msm_hip_bases_fft and its _device form) and its mirrors, without a
GPU: the symbols are declared and exported within ABI version 7, fail with the no-device code without a device, the Python binding and the C++
wrapper have their methods, root_of_unity gives primitive roots on the five G1 curves, and bad arguments raise before the library is reached."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G1_CURVES = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")


def _header():
    with open(os.path.join(ROOT, "include", "msm_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_fft_symbols_are_declared_and_exported(built):
    import msm_webgpu_amd as m

    text = _header()
    assert re.search(r"#define MSM_HIP_FFT_SCALE_INV_N 2u", text)
    assert re.search(r"\bint msm_hip_bases_fft\s*\(msm_hip_ctx\* ctx, const uint8_t omega\[32\], int log_n, uint8_t\* out_xy_host, uint32_t flags\)", text)
    assert re.search(r"\bint msm_hip_bases_fft_device\s*\(msm_hip_ctx\* ctx, const uint8_t omega\[32\], int log_n, void\* out_xy_dev, uint32_t flags\)", text)
    assert re.search(r"\bint msm_hip_test_fft_last\s*\(const msm_hip_ctx\* ctx, int\* stages, int\* ladder\)", text)
    for name in ("msm_hip_bases_fft", "msm_hip_bases_fft_device", "msm_hip_test_fft_last"):
        assert hasattr(m.lib(), name), name
    assert m.lib().msm_hip_abi_version() == 7  # (the calls arrived within version 7)


def test_fft_calls_without_a_context_fail_loudly(built):
    import msm_webgpu_amd as m

    L = m.lib()
    want = -2 if torch.cuda.is_available() else -1  # no context: MSM_HIP_ERR_NO_DEVICE where the process has no device, else MSM_HIP_ERR_INVALID_ARG
    out = C.create_string_buffer(64)
    one = (1).to_bytes(32, "little")
    assert L.msm_hip_bases_fft(None, one, 0, out, 0) == want
    assert L.msm_hip_bases_fft_device(None, one, 0, None, 0) == want
    assert out.raw == bytes(64)


def test_python_binding_and_cpp_wrapper_have_the_fft_methods(built):
    import msm_webgpu_amd as m
    from msm_webgpu_amd import api

    for name in ("bases_fft", "lagrange_bases", "fft_last"):
        assert callable(getattr(api.MsmContext, name)), name
    assert callable(api.root_of_unity) and m.root_of_unity is api.root_of_unity
    assert api.MsmContext.FFT_SCALE_INV_N == 2
    with open(os.path.join(ROOT, "include", "msm_hip.hpp")) as f:
        src = f.read()
    for name in ("bases_fft(", "bases_fft_device(", "msm_hip_bases_fft(", "msm_hip_bases_fft_device("):
        assert name in src, name


@pytest.mark.parametrize("curve", G1_CURVES)
def test_root_of_unity_is_primitive(curve):
    from msm_webgpu_amd import api

    ref = __import__("oracle.%s_ref" % curve, fromlist=["R"])
    r = api.SCALAR_FIELDS[curve]
    assert r == ref.R
    two_adicity = ((r - 1) & -(r - 1)).bit_length() - 1
    assert two_adicity == {"bn254": 28, "grumpkin": 1, "pallas": 32, "vesta": 32, "bls12_381": 32}[curve]
    assert api.root_of_unity(curve, 0) == 1
    for log_n in (1, 2, 5, 10, 20, 28):
        if log_n > two_adicity:
            with pytest.raises(ValueError):
                api.root_of_unity(curve, log_n)
            continue
        w = api.root_of_unity(curve, log_n)
        assert 0 < w < r and pow(w, 1 << (log_n - 1), r) == r - 1
        assert api.root_of_unity(curve, log_n, inverse=True) * w % r == 1
    with pytest.raises(ValueError):
        api.root_of_unity(curve, two_adicity + 1)
    with pytest.raises(ValueError):
        api.root_of_unity(curve, -1)


def test_grumpkin_has_no_fourth_root_of_unity():
    from msm_webgpu_amd import api

    assert api.root_of_unity("grumpkin", 1) == api.SCALAR_FIELDS["grumpkin"] - 1
    with pytest.raises(ValueError):
        api.root_of_unity("grumpkin", 2)


def _bare_context(n_bases):
    """An MsmContext that never touched the library (no device needed): n_bases as after set_bases"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.cb, ctx.pb, ctx.jb, ctx.scalar_width, ctx.scalar_signed, ctx.n_bases, ctx._keepalive = "bn254", 32, 64, 96, 32, False, n_bases, {}
    ctx.curve_id, ctx.modulus = api.CURVES["bn254"]
    ctx.device = 0
    return ctx


def test_bad_arguments_raise_before_any_library_call(built, monkeypatch):
    from msm_webgpu_amd import api

    def no_call():
        raise AssertionError("the library was called")

    monkeypatch.setattr(api, "lib", no_call)
    w = api.root_of_unity("bn254", 3)
    for n_bases in (0, 6):  # log_n=None: all the bases, which must be a power of two
        with pytest.raises(ValueError):
            _bare_context(n_bases).bases_fft(w)
        with pytest.raises(ValueError):
            _bare_context(n_bases).lagrange_bases()
    ctx = _bare_context(8)
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        ctx.bases_fft(w, 3)
    with pytest.raises(ValueError):  # omega as bytes: 32 of them
        ctx.bases_fft(bytes(31), 3)
    with pytest.raises(OverflowError):  # ... as an integer: below 2^256
        ctx.bases_fft(1 << 256, 3)
    with pytest.raises(TypeError):   # `out` is a device tensor
        ctx.bases_fft(w, 3, out=bytearray(8 * 64))
