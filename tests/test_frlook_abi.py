"""libmsm_frlook.so in the C ABI (include/msm_frlook.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version 1
beside the unchanged other seven libraries, the host form of create checks its keys and counts the distinct ones on the host, every bad
argument of create and of a count is answered before a device is asked for, a call without a device fails with the no-device code and leaves
its buffers alone, and the Python methods raise before any library is reached."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import frlook_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG, ERR_NONCANONICAL = -1, -2, -4
MONT256 = 2


def _header():
    with open(os.path.join(ROOT, "include", "msm_frlook.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    for name, value in (("MONT256", "2u"), ("MISSING", "0xFFFFFFFFu"), ("MAX_TABLE", r"\(1u << 24\)"), ("MAX_ELEMENTS", r"\(1u << 26\)")):
        assert re.search(r"#define MSM_FRLOOK_%s %s\s" % (name, value), text), name
    assert re.search(r"\bint msm_frlook_create_device\s*\(int curve, int device, void\* stream, const void\* table, size_t n_t, uint32_t flags, msm_frlook\*\* out\)", text)
    assert re.search(r"\bint msm_frlook_create\s*\(int curve, int device, const uint8_t\* table, size_t n_t, uint32_t flags, msm_frlook\*\* out\)", text)
    assert re.search(r"\bint msm_frlook_info\s*\(const msm_frlook\* t, size_t\* n_t, size_t\* distinct, uint32_t\* flags\)", text)
    tail = r"size_t n, size_t batch, size_t stride,\s*uint32_t flags,\s*uint64_t\* missing, uint64_t\* first_missing\)"
    assert re.search(r"\bint msm_frlook_count_device\s*\(const msm_frlook\* t, void\* stream, void\* m_out, uint32_t\* counts_out, uint32_t\* idx_out, const void\* f, " + tail, text)
    assert re.search(r"\bint msm_frlook_count\s*\(const msm_frlook\* t, uint8_t\* m_out, uint32_t\* counts_out, uint32_t\* idx_out, const uint8_t\* f, " + tail, text)
    assert re.search(r"\bvoid msm_frlook_destroy\s*\(msm_frlook\* t\)", text) and re.search(r"\bvoid msm_frlook_release\s*\(void\)", text)
    assert re.search(r"\bint msm_frlook_abi_version\s*\(void\)", text) and re.search(r"\bint msm_frlook_test_hash_bits\s*\(int bits\)", text)
    full = open(os.path.join(ROOT, "include", "msm_frlook.h")).read()
    for word in ("Grumpkin", "MSM_HIP_ERR_INVALID_ARG", "MSM_HIP_ERR_NONCANONICAL", "LOWEST index", "UINT64_MAX", "ONE device-to-host copy"):  # (the conventions are stated)
        assert word in full, word
    L = api.frlook_lib()
    for name in ("msm_frlook_create", "msm_frlook_create_device", "msm_frlook_info", "msm_frlook_destroy", "msm_frlook_count", "msm_frlook_count_device",
                 "msm_frlook_release", "msm_frlook_abi_version", "msm_frlook_test_hash_bits"):
        assert hasattr(L, name), name
    assert L.msm_frlook_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7 and api.fr_lib().msm_fr_abi_version() == 1 and api.frvec_lib().msm_frvec_abi_version() == 1
    assert api.frpoly_lib().msm_frpoly_abi_version() == 1 and api.frmle_lib().msm_frmle_abi_version() == 1 and api.frmat_lib().msm_frmat_abi_version() == 1
    assert api.frgate_lib().msm_frgate_abi_version() == 1
    X = api.MsmContext
    assert (X.FRLOOK_MONT256, X.FRLOOK_MISSING, X.FRLOOK_MAX_TABLE, X.FRLOOK_MAX_ELEMENTS) == (2, 0xFFFFFFFF, 1 << 24, 1 << 26)
    for name in ("lookup_table", "scalars_multiplicities", "logup"):
        assert callable(getattr(X, name)), name
    for name in ("frlook_lib", "lib_frlook", "frlook_release", "frlook_test_hash_bits"):
        assert callable(getattr(api, name)), name
    assert api.lib_frlook is api.frlook_lib
    for name in ("close", "__enter__", "__exit__"):
        assert callable(getattr(api.FrLookup, name)), name


def _create(L, table, curve=0, flags=0, n_t=None, device=0):
    h = C.c_void_p()
    rc = L.msm_frlook_create(curve, device, M.to_bytes(table) if table is not None else None, len(table) if n_t is None else n_t, flags, C.byref(h))
    return rc, h


def _info(L, h):
    n_t, distinct, flags = C.c_size_t(), C.c_size_t(), C.c_uint32()
    assert L.msm_frlook_info(h, C.byref(n_t), C.byref(distinct), C.byref(flags)) == 0
    return n_t.value, distinct.value, flags.value


def test_the_host_form_of_create_checks_and_counts_on_the_host(built):
    """no device is touched: the keys are compared with r and the distinct ones counted by the kernels' own insertion, run serially"""
    from msm_webgpu_amd import api

    L = api.frlook_lib()
    rnd = rng(81)
    for curve, field in ((0, "bn254"), (1, "grumpkin"), (2, "pallas"), (3, "vesta"), (4, "bls12_381"), (5, "bn254"), (6, "bls12_381")):
        r = api.SCALAR_FIELDS[field]
        for name in ("random 1", "random 65", "range 1025", "tripled", "identical", "zero and r - 1", "wrapping chain"):
            table = M.table(name, r, rnd)
            for bits in (0, 1):
                assert L.msm_frlook_test_hash_bits(bits) == 0
                for flags in (0, MONT256):
                    stored = M.mont(table, r) if flags else table
                    rc, h = _create(L, stored, curve, flags)
                    assert rc == 0 and _info(L, h) == (len(table), len(set(table)), flags), (field, name, bits, flags)
                    L.msm_frlook_destroy(h)
        assert L.msm_frlook_test_hash_bits(0) == 0
        for bad in (r, r + 1, (1 << 256) - 1):  # a key that is not below r, first, in the middle, last
            for at in (0, 2, 4):
                rc, h = _create(L, [1, 2, 3, 4, 5][:at] + [bad] + [1, 2, 3, 4, 5][at + 1:], curve)
                assert rc == ERR_NONCANONICAL and not h.value, (field, hex(bad), at)
        rc, h = _create(L, [r - 1, 0], curve)
        assert rc == 0
        L.msm_frlook_destroy(h)
    assert L.msm_frlook_test_hash_bits(33) == ERR_INVALID_ARG and L.msm_frlook_test_hash_bits(-1) == ERR_INVALID_ARG
    assert L.msm_frlook_info(None, None, None, None) == ERR_INVALID_ARG
    L.msm_frlook_destroy(None)  # (nothing)


def test_the_c_abi_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.frlook_lib()
    inval = ERR_INVALID_ARG
    h = C.c_void_p()
    one = M.to_bytes([1])
    T = 1 << 20  # a device address that is never touched: every check below comes first
    # ---- create, both forms
    assert L.msm_frlook_create(7, 0, one, 1, 0, C.byref(h)) == inval and L.msm_frlook_create(-1, 0, one, 1, 0, C.byref(h)) == inval  # no such curve
    assert L.msm_frlook_create_device(7, 0, None, C.c_void_p(T), 1, 0, C.byref(h)) == inval
    assert L.msm_frlook_create(0, -1, one, 1, 0, C.byref(h)) == inval and L.msm_frlook_create_device(0, -1, None, C.c_void_p(T), 1, 0, C.byref(h)) == inval
    assert L.msm_frlook_create(0, 0, one, 0, 0, C.byref(h)) == inval and L.msm_frlook_create_device(0, 0, None, C.c_void_p(T), 0, 0, C.byref(h)) == inval  # n_t
    assert L.msm_frlook_create_device(0, 0, None, C.c_void_p(T), (1 << 24) + 1, 0, C.byref(h)) == inval
    for flags in (1, 4, 8, 1 << 31):
        assert L.msm_frlook_create(0, 0, one, 1, flags, C.byref(h)) == inval and L.msm_frlook_create_device(0, 0, None, C.c_void_p(T), 1, flags, C.byref(h)) == inval
    assert L.msm_frlook_create(0, 0, None, 1, 0, C.byref(h)) == inval and L.msm_frlook_create_device(0, 0, None, None, 1, 0, C.byref(h)) == inval  # no table
    assert L.msm_frlook_create(0, 0, one, 1, 0, None) == inval and L.msm_frlook_create_device(0, 0, None, C.c_void_p(T), 1, 0, None) == inval  # nowhere to put it
    assert L.msm_frlook_create_device(0, 0, None, C.c_void_p(T + 8), 1, 0, C.byref(h)) == inval  # an unaligned device pointer
    assert not h.value
    # ---- count: a handle made on the host, of 8 entries
    n_t, n = 8, 6
    rc, h = _create(L, list(range(n_t)))
    assert rc == 0
    rc, hm = _create(L, list(range(n_t)), flags=MONT256)
    assert rc == 0
    bufs = [C.create_string_buffer(bytes(32 * 2 * n), 32 * 2 * n), C.create_string_buffer(b"\x07" * (32 * n_t), 32 * n_t), C.create_string_buffer(b"\x08" * (4 * n_t), 4 * n_t),
            C.create_string_buffer(b"\x09" * (4 * 2 * n), 4 * 2 * n)]
    f, m, cnt, idx = [C.cast(x, C.c_void_p) for x in bufs]
    miss, first = C.c_uint64(77), C.c_uint64(78)
    F, MO, CN, IX = 1 << 20, 1 << 16, 1 << 12, 1 << 8

    def dev(t=h, m=MO, cnt=CN, idx=IX, f=F, n=n, batch=2, stride=None, flags=0):
        return L.msm_frlook_count_device(t, None, C.c_void_p(m) if m else None, C.c_void_p(cnt) if cnt else None, C.c_void_p(idx) if idx else None,
                                         C.c_void_p(f) if f else None, n, batch, n if stride is None else stride, flags, C.byref(miss), C.byref(first))

    def host(t=h, m=m, cnt=cnt, idx=idx, f=f, n=n, batch=2, stride=None, flags=0):
        return L.msm_frlook_count(t, m, cnt, idx, f, n, batch, n if stride is None else stride, flags, C.byref(miss), C.byref(first))

    def both(**kw):
        return [dev(**kw), host(**kw)]

    assert both(t=None) == [inval] * 2  # the handle
    assert both(n=0) == [inval] * 2 and both(batch=0) == [inval] * 2 and both(stride=n - 1) == [inval] * 2
    assert dev(n=1, batch=2, stride=(1 << 25) + 1) == inval and dev(n=1, batch=1, stride=(1 << 26) + 1) == inval  # batch * stride > 2^26
    assert dev(n=2, batch=2, stride=1 << 63) == inval and dev(n=2, batch=1 << 63, stride=2) == inval  # (... with a product that wraps)
    assert both(flags=1) == [inval] * 2 and both(flags=4) == [inval] * 2 and both(flags=1 << 31) == [inval] * 2
    assert both(flags=MONT256) == [inval] * 2 and both(t=hm, flags=0) == [inval] * 2  # the form is the handle's
    assert dev(f=0) == inval and host(f=None) == inval  # nothing to look up
    # unaligned pointers: 16 bytes for scalars (the device form), 4 for words (both)
    assert dev(f=F + 8) == inval and dev(m=MO + 4) == inval and dev(cnt=CN + 2) == inval and dev(idx=IX + 1) == inval
    assert host(cnt=C.c_void_p(cnt.value + 2)) == inval and host(idx=C.c_void_p(idx.value + 1)) == inval
    # every output apart from f and from each other, in whole or in part
    assert dev(m=F) == inval and dev(m=F + 32 * (2 * n - 1)) == inval and dev(m=F - 32 * (n_t - 1)) == inval
    assert dev(m=F + 32 * 15, stride=8) == inval  # (all of f[0 .. batch stride), the gaps included)
    assert dev(cnt=F + 4) == inval and dev(idx=F + 32 * 2 * n - 4) == inval
    assert dev(cnt=MO) == inval and dev(cnt=MO + 32 * n_t - 4) == inval and dev(idx=MO + 16) == inval and dev(idx=CN + 4 * (n_t - 1)) == inval
    assert host(m=f) == inval and host(cnt=f) == inval and host(idx=C.c_void_p(m.value + 32)) == inval and host(idx=cnt) == inval
    # the host form compares f with r on the host
    r = api.SCALAR_FIELDS["bn254"]
    for at in (0, n - 1, n, 2 * n - 1):
        bad = C.create_string_buffer(M.to_bytes([1] * at + [r] + [2] * (2 * n - 1 - at)), 32 * 2 * n)
        assert host(f=C.cast(bad, C.c_void_p)) == ERR_NONCANONICAL, at
    gap = C.create_string_buffer(M.to_bytes([1, 2, r, 3, 4, (1 << 256) - 1]), 32 * 6)  # n = 2 of a stride of 3: the third of a row is not read
    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        assert both() == [ERR_NO_DEVICE] * 2 and both(t=hm, flags=MONT256) == [ERR_NO_DEVICE] * 2
        assert both(m=None, cnt=None, idx=None) == [ERR_NO_DEVICE] * 2  # a pure membership check
        assert both(m=None) == [ERR_NO_DEVICE] * 2 and both(cnt=None, idx=None) == [ERR_NO_DEVICE] * 2
        assert host(f=C.cast(gap, C.c_void_p), n=2, stride=3) == ERR_NO_DEVICE
        assert dev(n=1, batch=1, stride=1 << 26) == ERR_NO_DEVICE and dev(n=1 << 13, batch=1 << 13, stride=1 << 13, m=None, cnt=None, idx=None) == ERR_NO_DEVICE  # 2^26 exactly
        assert dev(m=F + 32 * 2 * n) == ERR_NO_DEVICE and dev(m=F - 32 * n_t) == ERR_NO_DEVICE  # (apart: right behind, right before)
        assert dev(m=F + 32 * 16, stride=8) == ERR_NO_DEVICE and dev(cnt=MO + 32 * n_t) == ERR_NO_DEVICE
        assert L.msm_frlook_create_device(0, 0, None, C.c_void_p(T), 1 << 24, MONT256, C.byref(C.c_void_p())) == ERR_NO_DEVICE
        assert [x.raw for x in bufs] == before and (miss.value, first.value) == (77, 78)
    L.msm_frlook_destroy(h)
    L.msm_frlook_destroy(hm)
    L.msm_frlook_release()  # (nothing held: a no-op)


def _bare_context(curve="bn254", width=32, mont=False):
    """An MsmContext that never touched the library (no device needed)"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.scalar_width, ctx.scalar_signed, ctx.scalar_mont256, ctx.n_bases, ctx._keepalive = curve, width, False, mont, 0, {}
    ctx.curve_id, ctx.modulus = api.CURVES[curve]
    ctx.device = 0
    return ctx


def test_python_tables_from_host_bytes_and_bad_arguments(built):
    from msm_webgpu_amd import api

    r = api.SCALAR_FIELDS["bn254"]
    ctx = _bare_context()
    with ctx.lookup_table(M.to_bytes([5, 7, 5, 9, 7, 5])) as t:  # host bytes: no device is touched
        assert (t.n, t.distinct, t.mont256, t.curve) == (6, 3, False, "bn254") and t._h
        for bad in (lambda: ctx.scalars_multiplicities(t, bytes(33)),  # not whole scalars
                    lambda: ctx.scalars_multiplicities(t, b""),
                    lambda: ctx.scalars_multiplicities(t, bytes(32 * 6), batch=4),  # rows that do not divide the buffer
                    lambda: ctx.scalars_multiplicities(t, bytes(32 * 6), batch=0),
                    lambda: ctx.scalars_multiplicities(t, bytes(32 * 6), batch=2, n=4),  # longer than a row
                    lambda: ctx.scalars_multiplicities(t, bytes(32 * 6), n=0),
                    lambda: _bare_context(mont=True).scalars_multiplicities(t, bytes(32 * 6)),  # another scalar format
                    lambda: _bare_context("pallas").scalars_multiplicities(t, bytes(32 * 6))):  # another field
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(TypeError):  # out belongs to device vectors
            ctx.scalars_multiplicities(t, bytes(32 * 6), out=bytearray(32 * 6))
        if not torch.cuda.is_available():
            with pytest.raises(api.MsmHipError):
                ctx.scalars_multiplicities(t, bytes(32 * 6))
    assert not t._h
    with pytest.raises(TypeError):
        ctx.scalars_multiplicities(t, bytes(32))  # a closed table
    with pytest.raises(TypeError):
        ctx.scalars_multiplicities(None, bytes(32))
    g = _bare_context("grumpkin", mont=True).lookup_table(M.to_bytes(M.mont([1, 2, 2], api.SCALAR_FIELDS["grumpkin"])), n=2)  # every curve's field, the first n
    assert (g.n, g.distinct, g.mont256) == (2, 2, True)
    g.close()
    with pytest.raises(api.MsmHipError):
        ctx.lookup_table(M.to_bytes([r]))
    for bad in (lambda: ctx.lookup_table(b""), lambda: ctx.lookup_table(bytes(31)), lambda: ctx.lookup_table(bytes(64), n=3), lambda: ctx.lookup_table(bytes(64), n=0),
                lambda: _bare_context(width=8).lookup_table(bytes(64)), lambda: _bare_context(width=8).logup(bytes(64), bytes(64), 1)):
        with pytest.raises(ValueError):
            bad()
    for c in (ctx, _bare_context("grumpkin")):  # logup stays on the device, on every curve's field
        with pytest.raises(TypeError):
            c.logup(bytes(64), bytes(64), 1)
