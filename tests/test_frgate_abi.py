"""libmsm_frgate.so in the C ABI (include/msm_frgate.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version 1
beside the unchanged other six libraries, every bad argument is answered before a device is asked for, a call without a device fails with the
no-device code and leaves its buffers alone, and the Python methods raise before any library is reached."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG = -1, -2
MONT256, ACCUMULATE = 2, 4


def _header():
    with open(os.path.join(ROOT, "include", "msm_frgate.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    for name, value in (("MONT256", "2u"), ("ACCUMULATE", "4u"), ("MAX_DEGREE", "8"), ("MAX_TERMS", "64"), ("MAX_ROWS", "32")):
        assert re.search(r"#define MSM_FRGATE_%s %s\s" % (name, value), text), name
    assert re.search(r"typedef struct msm_frgate_term \{\s*uint8_t coeff\[32\];\s*uint32_t degree;\s*uint32_t rows\[8\];\s*int32_t rots\[8\];\s*\} msm_frgate_term;", text)
    tail = r"size_t n, size_t batch, size_t stride, const msm_frgate_term\* terms,\s*size_t num_terms,\s*size_t step, const %s\* scale, size_t scale_len, uint32_t flags\)"
    assert re.search(r"\bint msm_frgate_apply_device\s*\(int curve, int device, void\* stream, void\* out, const void\* a, " + tail % "void", text)
    assert re.search(r"\bint msm_frgate_apply\s*\(int curve, int device, uint8_t\* out, const uint8_t\* a, " + tail % "uint8_t", text)
    assert re.search(r"\bvoid msm_frgate_release\s*\(void\)", text) and re.search(r"\bint msm_frgate_abi_version\s*\(void\)", text)
    full = open(os.path.join(ROOT, "include", "msm_frgate.h")).read()
    assert "Grumpkin" in full and "MSM_HIP_ERR_INVALID_ARG" in full and "MSM_HIP_ERR_NONCANONICAL" in full and "never in place" in full  # (the conventions are stated)
    L = api.frgate_lib()
    for name in ("msm_frgate_apply", "msm_frgate_apply_device", "msm_frgate_release", "msm_frgate_abi_version"):
        assert hasattr(L, name), name
    assert L.msm_frgate_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7 and api.fr_lib().msm_fr_abi_version() == 1 and api.frvec_lib().msm_frvec_abi_version() == 1
    assert api.frpoly_lib().msm_frpoly_abi_version() == 1 and api.frmle_lib().msm_frmle_abi_version() == 1 and api.frmat_lib().msm_frmat_abi_version() == 1
    assert C.sizeof(api.FrgateTerm) == 100 and C.sizeof(api.FrmleTerm) == 52
    M = api.MsmContext
    assert (M.FRGATE_MONT256, M.FRGATE_ACCUMULATE, M.FRGATE_MAX_DEGREE, M.FRGATE_MAX_TERMS, M.FRGATE_MAX_ROWS) == (2, 4, 8, 64, 32)
    for name in ("scalars_gate", "vanishing_inverse", "quotient"):
        assert callable(getattr(M, name)), name
    for name in ("frgate_lib", "frgate_release"):
        assert callable(getattr(api, name)), name


def _terms(api, items):
    """[(coeff bytes, ((row, rotation), ..)), ..]"""
    arr = (api.FrgateTerm * len(items))()
    for t, (coeff, factors) in zip(arr, items):
        t.coeff[:] = coeff
        t.degree = len(factors)
        t.rows[:len(factors)] = [f[0] for f in factors]
        t.rots[:len(factors)] = [f[1] for f in factors]
    return arr


def test_the_c_abi_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.frgate_lib()
    r = api.SCALAR_FIELDS["bn254"]
    one, big = (1).to_bytes(32, "little"), r.to_bytes(32, "little")
    n = 8
    bufs = [C.create_string_buffer(bytes([7 + k]) * (32 * 2 * n), 32 * 2 * n) for k in range(3)]
    out, a, sc = [C.cast(x, C.c_void_p) for x in bufs]
    inval = ERR_INVALID_ARG
    good = _terms(api, [(one, ((0, 0), (1, 1)))])
    A, OUT, SC = 1 << 20, 1 << 16, 1 << 12  # device addresses that are never touched: every check below comes first

    def dev(curve=0, out=OUT, a=A, n=n, batch=2, stride=None, terms=good, num_terms=1, step=1, scale=None, scale_len=0, flags=0):
        return L.msm_frgate_apply_device(curve, 0, None, C.c_void_p(out), C.c_void_p(a), n, batch, n if stride is None else stride, terms, num_terms, step,
                                         C.c_void_p(scale) if scale else None, scale_len, flags)

    def host(curve=0, out=out, a=a, n=n, batch=2, stride=None, terms=good, num_terms=1, step=1, scale=None, scale_len=0, flags=0):
        return L.msm_frgate_apply(curve, 0, out, a, n, batch, n if stride is None else stride, terms, num_terms, step, scale, scale_len, flags)

    def both(**kw):
        return [dev(**kw), host(**kw)]

    assert both(curve=7) == [inval] * 2 and both(curve=-1) == [inval] * 2  # no such curve
    for bad_n in (0, 3, 6, 12, 1 << 27):  # not a power of two, or beyond 2^26
        assert dev(n=bad_n, stride=1 << 27 if bad_n > 16 else 16, batch=1) == inval, bad_n
    assert both(batch=0) == [inval] * 2 and both(stride=n - 1) == [inval] * 2
    assert dev(batch=33, terms=_terms(api, [(one, ((0, 0),))])) == inval  # more than 32 rows
    assert dev(n=1 << 13, batch=32, stride=(1 << 21) + 1) == inval  # batch * stride > 2^26
    assert dev(n=2, batch=2, stride=1 << 63) == inval  # (... with a product that wraps)
    assert both(step=0) == [inval] * 2 and both(step=n + 1) == [inval] * 2
    # the scale's length
    for bad_len in (0, 3, 6, 2 * n):
        assert dev(scale=SC, scale_len=bad_len) == inval and host(scale=sc, scale_len=bad_len) == inval, bad_len
    # the flags
    assert both(flags=1) == [inval] * 2 and both(flags=8) == [inval] * 2 and both(flags=1 << 31) == [inval] * 2
    # the terms: their number, a degree, a row, a coefficient -- in both data forms
    assert both(num_terms=0) == [inval] * 2 and both(terms=None) == [inval] * 2
    assert both(terms=_terms(api, [(one, ((0, 0),))] * 65), num_terms=65) == [inval] * 2
    zero_degree, nine = _terms(api, [(one, ((0, 0),))]), _terms(api, [(one, ((0, 0),) * 8)])
    zero_degree[0].degree, nine[0].degree = 0, 9
    assert both(terms=zero_degree) == [inval] * 2 and both(terms=nine) == [inval] * 2
    assert both(terms=_terms(api, [(one, ((0, 0), (2, 0)))])) == [inval] * 2  # row 2 of two rows
    assert both(terms=_terms(api, [(big, ((0, 0),))])) == [inval] * 2 and both(terms=_terms(api, [(b"\xff" * 32, ((0, 0),))]), flags=MONT256) == [inval] * 2
    # a missing pointer
    assert host(out=None) == inval and host(a=None) == inval and dev(out=0) == inval and dev(a=0) == inval
    # an unaligned device pointer
    assert dev(out=OUT + 8) == inval and dev(a=A + 4) == inval and dev(scale=SC + 8, scale_len=4) == inval
    # out overlapping the rows or the scale, in whole or in part: never in place
    assert dev(out=A) == inval and dev(out=A + 32) == inval and dev(out=A - 32) == inval
    assert dev(out=A + 32 * n) == inval  # (the second row)
    assert dev(out=A + 32 * 20, stride=16) == inval and dev(out=A + 32 * 24, stride=16) == inval  # (all of a[0 .. batch stride), the gaps included)
    assert dev(out=SC, scale=SC, scale_len=4) == inval and dev(out=SC + 32 * 3, scale=SC, scale_len=4) == inval and dev(out=SC - 32 * (n - 1), scale=SC, scale_len=4) == inval
    assert host(out=a) == inval and host(out=C.c_void_p(a.value + 32)) == inval and host(out=sc, scale=sc, scale_len=4) == inval
    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        assert both() == [ERR_NO_DEVICE] * 2 and both(flags=MONT256 | ACCUMULATE) == [ERR_NO_DEVICE] * 2
        for curve in range(7):  # every curve has its field here, Grumpkin included
            assert both(curve=curve) == [ERR_NO_DEVICE] * 2, curve
        assert dev(scale=SC, scale_len=1) == ERR_NO_DEVICE and dev(scale=SC, scale_len=n) == ERR_NO_DEVICE and host(scale=sc, scale_len=4) == ERR_NO_DEVICE
        assert both(n=1, batch=1, terms=_terms(api, [(one, ((0, -5),))])) == [ERR_NO_DEVICE] * 2  # a single element
        assert both(step=n) == [ERR_NO_DEVICE] * 2
        far = _terms(api, [((r - 1).to_bytes(32, "little"), ((1, 2 ** 31 - 1), (1, -2 ** 31), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (1, 1)))] * 64)
        assert both(terms=far, num_terms=64) == [ERR_NO_DEVICE] * 2  # (a row may repeat; any rotation)
        assert dev(out=A + 32 * 32, stride=16) == ERR_NO_DEVICE and dev(out=A - 32 * n) == ERR_NO_DEVICE  # (apart: right behind, right before)
        assert dev(n=1 << 13, batch=32, stride=1 << 21, terms=_terms(api, [(one, ((31, 0),))]), out=1 << 40) == ERR_NO_DEVICE  # batch * stride = 2^26 exactly
        assert [x.raw for x in bufs] == before
    L.msm_frgate_release()  # (nothing held: a no-op)


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
    for name in ("lib", "fr_lib", "frvec_lib", "frpoly_lib", "frmle_lib", "frmat_lib", "frgate_lib"):
        monkeypatch.setattr(scalars, name, no_call)
    r = api.SCALAR_FIELDS["bn254"]
    v = bytes(32 * 8)
    T = [(1, (0, (1, -1)))]
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        _bare_context().scalars_gate(v, T, batch=2)

    for width in (1, 8, 16):  # a narrow scalar format
        ctx = _bare_context(width=width)
        for call in (lambda: ctx.scalars_gate(v, T, batch=2), lambda: ctx.vanishing_inverse(2, 1, 7), lambda: ctx.quotient(v, T, 2, 2, 1, 7)):
            with pytest.raises(ValueError):
                call()
    for curve in ("grumpkin", "bn254_g2", "pallas"):  # every curve is offered: these get as far as the library
        with pytest.raises(AssertionError, match="the library was called"):
            _bare_context(curve).scalars_gate(v, T, batch=2)
    for name in ("vanishing_inverse", "quotient"):  # the transforms' fields only
        with pytest.raises(ValueError):
            getattr(_bare_context("grumpkin"), name)(*((2, 1, 7) if name == "vanishing_inverse" else (v, T, 2, 2, 1, 7)))
    ctx = _bare_context()
    for bad in (lambda: ctx.scalars_gate(bytes(33), T),  # not whole scalars
                lambda: ctx.scalars_gate(b"", T),  # nothing at all
                lambda: ctx.scalars_gate(bytes(32 * 6), [(1, (0,))]),  # not a power of two
                lambda: ctx.scalars_gate(v, T, batch=2, n=3),
                lambda: ctx.scalars_gate(v, T, batch=2, n=8),  # longer than a row
                lambda: ctx.scalars_gate(v, T, batch=3),  # rows that do not divide the buffer
                lambda: ctx.scalars_gate(v, T, batch=0),
                lambda: ctx.scalars_gate(bytes(32 * 66), [(1, (0,))], batch=33),  # more than 32 rows
                lambda: ctx.scalars_gate(v, T, batch=2, step=0),
                lambda: ctx.scalars_gate(v, T, batch=2, step=5),
                lambda: ctx.scalars_gate(v, [], batch=2),  # no term, too many terms
                lambda: ctx.scalars_gate(v, T * 65, batch=2),
                lambda: ctx.scalars_gate(v, [(1, ())], batch=2),  # a degree
                lambda: ctx.scalars_gate(v, [(1, (0,) * 9)], batch=2),
                lambda: ctx.scalars_gate(v, [(1, (0, 2))], batch=2),  # a row
                lambda: ctx.scalars_gate(v, [(1, ((-1, 0),))], batch=2),
                lambda: ctx.scalars_gate(v, [(1, ((0, 2 ** 31),))], batch=2),  # a rotation beyond 32 bits
                lambda: ctx.scalars_gate(v, [(r, (0,))], batch=2),  # a coefficient
                lambda: ctx.scalars_gate(v, [(-1, (0,))], batch=2),
                lambda: ctx.scalars_gate(v, T, batch=2, scale=bytes(32 * 3)),  # a scale that is no power of two, or longer than n
                lambda: ctx.scalars_gate(v, T, batch=2, scale=bytes(32 * 8)),
                lambda: ctx.scalars_gate(v, T, batch=2, scale=bytes(31)),
                lambda: ctx.scalars_gate(v, T, batch=2, accumulate=True),  # nothing to add onto
                lambda: ctx.scalars_gate(v, T, batch=2, accumulate=True, out=bytes(32 * 3)),
                lambda: ctx.vanishing_inverse(-1, 1, 7),
                lambda: ctx.vanishing_inverse(2, 1, 1),  # shift^n = 1: the coset is H
                lambda: ctx.vanishing_inverse(27, 2, 7)):  # no such root of unity
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):  # out belongs to device vectors
        ctx.scalars_gate(v, T, batch=2, out=bytearray(32 * 4))
    with pytest.raises(TypeError):  # the quotient stays on the device
        ctx.quotient(v, T, 2, 2, 1, 7)
