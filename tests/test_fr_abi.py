"""libmsm_fr.so in the C ABI (include/msm_fr.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version 1 beside
an unchanged libmsm_hip.so (version 7, the same kernels), a call without a device fails with the no-device code, and bad arguments raise before
the library is reached."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_NO_DEVICE, ERR_INVALID_ARG = -1, -2


def _header():
    with open(os.path.join(ROOT, "include", "msm_fr.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    assert re.search(r"#define MSM_FR_SCALE_INV_N 1u", text) and re.search(r"#define MSM_FR_MONT256 2u", text)
    assert re.search(r"\bint msm_fr_ntt_device\s*\(int curve, int device, void\* stream, void\* data_dev, int log_n, size_t batch, const uint8_t omega\[32\], "
                     r"const uint8_t\* pre_shift,\s*const uint8_t\* post_shift, uint32_t flags\)", text)
    assert re.search(r"\bint msm_fr_ntt\s*\(int curve, int device, uint8_t\* data_host, int log_n, size_t batch, const uint8_t omega\[32\]", text)
    assert re.search(r"\bvoid msm_fr_release\s*\(void\)", text) and re.search(r"\bint msm_fr_abi_version\s*\(void\)", text)
    assert re.search(r"#ifdef MSM_FR_TEST_HOOKS\s+int msm_fr_test_pass_bits\s*\(int b\);\s+int msm_fr_test_last\s*\(int\* passes, int\* pass_bits\);", text)
    L = api.fr_lib()
    for name in ("msm_fr_ntt_device", "msm_fr_ntt", "msm_fr_release", "msm_fr_abi_version", "msm_fr_test_pass_bits", "msm_fr_test_last"):
        assert hasattr(L, name), name
    assert L.msm_fr_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7  # (the MSM library is what it was)
    assert api.MsmContext.FR_SCALE_INV_N == 1 and api.MsmContext.FR_MONT256 == 2 and callable(api.MsmContext.scalars_fft)
    with open(os.path.join(ROOT, "include", "msm_hip.hpp")) as f:
        src = f.read()
    for name in ("scalars_fft(", "msm_fr_ntt_device(", "msm_fr_ntt("):
        assert name in src, name


def test_scalar_fields_of_the_g2_groups():
    from msm_webgpu_amd import api

    assert api.SCALAR_FIELDS["bn254_g2"] == api.SCALAR_FIELDS["bn254"] and api.SCALAR_FIELDS["bls12_381_g2"] == api.SCALAR_FIELDS["bls12_381"]


def test_the_c_abi_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.fr_lib()
    one = (1).to_bytes(32, "little")
    data = C.create_string_buffer(64)
    ptr = C.cast(data, C.c_void_p)
    w1 = (api.SCALAR_FIELDS["bn254"] - 1).to_bytes(32, "little")
    assert L.msm_fr_ntt(1, 0, ptr, 0, 1, one, None, None, 0) == ERR_INVALID_ARG  # Grumpkin
    assert L.msm_fr_ntt(0, 0, ptr, 27, 1, one, None, None, 0) == ERR_INVALID_ARG  # log_n out of range
    assert L.msm_fr_ntt(0, 0, ptr, -1, 1, one, None, None, 0) == ERR_INVALID_ARG
    assert L.msm_fr_ntt(0, 0, ptr, 1, 1, one, None, None, 0) == ERR_INVALID_ARG  # 1 is not a primitive square root of 1
    assert L.msm_fr_ntt(0, 0, ptr, 0, 1, w1, None, None, 0) == ERR_INVALID_ARG  # ... and at n = 1 omega is 1
    assert L.msm_fr_ntt(0, 0, ptr, 1, 1, w1, None, None, 4) == ERR_INVALID_ARG  # unknown flag
    assert L.msm_fr_ntt(0, 0, None, 1, 1, w1, None, None, 0) == ERR_INVALID_ARG
    assert L.msm_fr_ntt(0, 0, ptr, 1, 1, w1, b"\xff" * 32, None, 0) == ERR_INVALID_ARG  # a shift >= r
    assert L.msm_fr_ntt_device(0, 0, None, C.c_void_p(8), 1, 1, w1, None, None, 0) == ERR_INVALID_ARG  # misaligned device pointer
    assert L.msm_fr_test_pass_bits(11) == ERR_INVALID_ARG and L.msm_fr_test_pass_bits(0) == 0
    if not torch.cuda.is_available():
        assert L.msm_fr_ntt(0, 0, ptr, 1, 1, w1, None, None, 0) == ERR_NO_DEVICE
        assert L.msm_fr_ntt_device(0, 0, None, C.c_void_p(4096), 1, 1, w1, None, None, 0) == ERR_NO_DEVICE
        assert data.raw == bytes(64)
    L.msm_fr_release()  # (nothing cached: a no-op)


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
    r = api.SCALAR_FIELDS["bn254"]
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        _bare_context().scalars_fft(bytes(32 * 8))
    with pytest.raises(ValueError):  # Grumpkin: r - 1 = 2 * odd
        _bare_context("grumpkin").scalars_fft(bytes(64))
    ctx = _bare_context()
    with pytest.raises(ValueError):  # log_n out of range: beyond 26, beyond the field's 2-adicity, negative
        ctx.scalars_fft(bytes(32), log_n=27)
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(32), log_n=-1)
    with pytest.raises(ValueError):  # the size does not match
        ctx.scalars_fft(bytes(32 * 3))
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(32 * 8), log_n=2)
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(32 * 8), batch=3)
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(33))
    with pytest.raises(ValueError):  # a non-primitive omega: of too small an order, not a root of unity at all, >= r, of the wrong length
        ctx.scalars_fft(bytes(32 * 8), omega=api.root_of_unity("bn254", 2))
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(32 * 8), omega=5)
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(32 * 8), omega=api.root_of_unity("bn254", 3) + r)
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(32 * 8), omega=bytes(31))
    with pytest.raises(ValueError):
        ctx.scalars_fft(bytes(32), omega=r - 1)
    with pytest.raises(ValueError):  # a shift that has no inverse
        ctx.scalars_fft(bytes(32 * 8), shift=r)
    for width in (1, 2, 4, 8, 16):  # a narrow scalar format
        with pytest.raises(ValueError):
            _bare_context(width=width).scalars_fft(bytes(32 * 8))


def test_libmsm_hip_holds_the_kernels_it_held(built):
    """the scalar-field units are a library of their own: libmsm_hip.so's translation units and the kernels in their device assembly are unchanged"""
    import check_long_branch_hazard as chk
    from msm_webgpu_amd import build as _unused  # noqa: F401
    import importlib

    b = importlib.import_module("msm_webgpu_amd.build")
    assert len(b.TRANSLATION_UNITS) == 8 and not any(u.startswith("fr_") for u in b.TRANSLATION_UNITS)
    assert not any(f.startswith(("fr_", "ntt_")) for f in b.SOURCES)
    assert sorted(b.FR_LIBRARIES["fr"].units) == ["fr_bls12_381.hip", "fr_bn254.hip", "fr_pallas.hip", "fr_vesta.hip"]
    counts = []
    for path in chk.compile_to_asm([]):
        with open(path) as f:
            names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), flags=re.M)
        assert not any("ntt" in n for n in names), path
        counts.append(len(names))
    assert len(counts) == 8 and sum(counts) == 141 + 5 * 42 + 2 * 36
    for path in chk.compile_to_asm([], units=b.FR_LIBRARIES["fr"].units):  # ... and each field's unit holds its one kernel, in its own namespace
        with open(path) as f:
            names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), flags=re.M)
        field = os.path.basename(path).split("-hip-")[0]
        assert len(names) == 1 and ("%d%s" % (len(field), field)) in names[0] and "k_ntt_pass" in names[0], (path, names)
