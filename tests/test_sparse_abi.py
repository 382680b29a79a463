"""The sparse MSM calls of the C ABI (include/msm_hip.h) and their mirrors, without a GPU: the three symbols are declared and exported, fail
loudly without a device, the Python binding has its methods, and host indices are checked before anything reaches the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE = ("msm_hip_run_sparse", "msm_hip_run_sparse_device", "msm_hip_launch_sparse_device")


def _header():
    with open(os.path.join(ROOT, "include", "msm_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_sparse_symbols_are_declared_and_exported(built):
    import msm_webgpu_amd as m

    text = _header()
    for name in SPARSE:
        assert re.search(r"\bint %s\s*\(msm_hip_ctx\* ctx, const uint32_t\* indices_" % name, text), name
        assert hasattr(m.lib(), name), name
    assert m.lib().msm_hip_abi_version() == 7  # (the sparse calls arrived within version 7)


def test_sparse_calls_without_a_device_fail_loudly(built):
    import msm_webgpu_amd as m

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = m.lib()
    out = C.create_string_buffer(96)
    idx = (C.c_uint32 * 1)(0)
    assert L.msm_hip_run_sparse(None, idx, bytes(32), 1, out) == -1
    assert L.msm_hip_run_sparse_device(None, None, None, 0, out) == -1
    assert L.msm_hip_launch_sparse_device(None, None, None, 0, 0) == -1


def test_python_binding_has_the_sparse_methods(built):
    from msm_webgpu_amd import api

    assert callable(api.MsmContext.msm_sparse)
    assert callable(api.MsmContext.launch_sparse)


def test_cpp_wrapper_has_the_sparse_methods():
    with open(os.path.join(ROOT, "include", "msm_hip.hpp")) as f:
        src = f.read()
    for name in ("msm_sparse(", "msm_sparse_bytes(", "msm_sparse_device(", "launch_sparse_device("):
        assert name in src, name


def _bare_context(n_bases):
    """An MsmContext that never touched the library (no device needed): n_bases as after set_bases"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.jb, ctx.scalar_width, ctx.n_bases, ctx._keepalive = "bn254", 96, 32, n_bases, {}
    ctx.curve_id, ctx.modulus = api.CURVES["bn254"]
    return ctx


@pytest.mark.parametrize("bad", [[0, 1000], [-1, 3], [5, 2**40]])
def test_host_index_check_raises_before_any_library_call(built, monkeypatch, bad):
    from msm_webgpu_amd import api

    def no_call():
        raise AssertionError("the library was called")

    ctx = _bare_context(1000)
    monkeypatch.setattr(api, "lib", no_call)
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        ctx.msm_sparse(np.array([0, 999], dtype=np.int64), bytes(64))
    with pytest.raises(ValueError):
        ctx.msm_sparse(np.array(bad, dtype=np.int64), bytes(32 * len(bad)))
    with pytest.raises(ValueError):  # (int32 too)
        ctx.msm_sparse(np.array([999, 1000], dtype=np.int32), bytes(64))
    with pytest.raises(ValueError):  # one index per scalar
        ctx.msm_sparse(np.array([1, 2, 3], dtype=np.uint32), bytes(64))


def test_host_indices_become_contiguous_uint32():
    from msm_webgpu_amd import api

    a = api._host_indices(np.arange(10, dtype=np.int64)[::2], 10)
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"] and a.tolist() == [0, 2, 4, 6, 8]
    assert api._host_indices(np.array([], dtype=np.int32), 0).size == 0
    with pytest.raises(TypeError):
        api._host_indices(np.array([1.0]), 10)
