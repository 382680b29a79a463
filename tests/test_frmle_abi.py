"""libmsm_frmle.so in the C ABI (include/msm_frmle.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version 1
beside the unchanged other four libraries, every bad argument is answered before a device is asked for, a call without a device fails with the
no-device code and leaves its buffers alone, and the Python methods raise before any library is reached."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG = -1, -2
MONT256 = 2
NAMES = ("fold", "eval", "eq", "round")


def _header():
    with open(os.path.join(ROOT, "include", "msm_frmle.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    for name, value in (("MONT256", "2u"), ("MAX_DEGREE", "4"), ("MAX_TERMS", "8"), ("MAX_ROWS", "16")):
        assert re.search(r"#define MSM_FRMLE_%s %s\s" % (name, value), text), name
    assert re.search(r"typedef struct msm_frmle_term \{\s*uint8_t coeff\[32\];\s*uint32_t degree;\s*uint32_t rows\[4\];\s*\} msm_frmle_term;", text)
    head = r"int curve, int device, void\* stream, "
    assert re.search(r"\bint msm_frmle_fold_device\s*\(" + head + r"void\* out, const void\* a, size_t n, size_t batch, size_t stride, const uint8_t\* c, uint32_t flags\)", text)
    assert re.search(r"\bint msm_frmle_eval_device\s*\(" + head + r"const void\* a, size_t n, size_t batch, size_t stride, const uint8_t\* point, uint32_t flags,\s*"
                     r"uint8_t\* values_host\)", text)
    assert re.search(r"\bint msm_frmle_eq_device\s*\(" + head + r"void\* out, size_t n, const uint8_t\* point, const uint8_t\* c, uint32_t flags\)", text)
    assert re.search(r"\bint msm_frmle_round_device\s*\(" + head + r"void\* a, size_t n, size_t batch, size_t stride, const msm_frmle_term\* terms, size_t num_terms,\s*"
                     r"const uint8_t\* fold_by, uint32_t flags, uint8_t\* values_host\)", text)
    for name in NAMES:
        assert re.search(r"\bint msm_frmle_%s\s*\(int curve, int device, (const )?uint8_t\* " % name, text), name
    assert re.search(r"\bvoid msm_frmle_release\s*\(void\)", text) and re.search(r"\bint msm_frmle_abi_version\s*\(void\)", text)
    assert re.search(r"#ifdef MSM_FRMLE_TEST_HOOKS\s+int msm_frmle_test_tile\s*\(int elements\);\s+int msm_frmle_test_last\s*\(int\* launches, int\* levels\);", text)
    full = open(os.path.join(ROOT, "include", "msm_frmle.h")).read()
    assert "TOP bit" in full and "Grumpkin" in full and "MSM_HIP_ERR_INVALID_ARG" in full and "MSM_HIP_ERR_NONCANONICAL" in full  # (the conventions are stated)
    L = api.frmle_lib()
    for name in ["msm_frmle_" + n + s for n in NAMES for s in ("", "_device")] + ["msm_frmle_release", "msm_frmle_abi_version", "msm_frmle_test_tile", "msm_frmle_test_last"]:
        assert hasattr(L, name), name
    assert L.msm_frmle_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7 and api.fr_lib().msm_fr_abi_version() == 1 and api.frvec_lib().msm_frvec_abi_version() == 1
    assert api.frpoly_lib().msm_frpoly_abi_version() == 1
    assert C.sizeof(api.FrmleTerm) == 52
    M = api.MsmContext
    assert (M.FRMLE_MONT256, M.FRMLE_MAX_DEGREE, M.FRMLE_MAX_TERMS, M.FRMLE_MAX_ROWS) == (2, 4, 8, 16)
    for name in ("scalars_mle_fold", "scalars_mle_eval", "scalars_eq", "scalars_sumcheck_round", "sumcheck_prove"):
        assert callable(getattr(M, name)), name
    for name in ("frmle_lib", "frmle_test_tile", "frmle_last", "frmle_release"):
        assert callable(getattr(api, name)), name


def _terms(api, items):
    arr = (api.FrmleTerm * len(items))()
    for t, (coeff, rows) in zip(arr, items):
        t.coeff[:] = coeff
        t.degree = len(rows)
        t.rows[:len(rows)] = rows
    return arr


def test_the_c_abi_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.frmle_lib()
    r = api.SCALAR_FIELDS["bn254"]
    one, big = (1).to_bytes(32, "little"), r.to_bytes(32, "little")
    n = 8
    bufs = [C.create_string_buffer(bytes([7 + k]) * (32 * 2 * n), 32 * 2 * n) for k in range(2)]
    out, a = [C.cast(x, C.c_void_p) for x in bufs]
    val = C.create_string_buffer(32 * 5)
    v = C.cast(val, C.c_void_p)
    D = lambda off=0: C.c_void_p(4096 + off)  # noqa: E731  (a device address that is never touched: every check below comes first)
    inval = ERR_INVALID_ARG
    good = _terms(api, [(one, (0, 1))])

    def every(curve=0, n=n, batch=2, stride=None, c=one, point=one * 3, flags=0, terms=good, num_terms=1, fold_by=None):
        """each host form once, with the one argument under test changed"""
        stride = n if stride is None else stride
        return [L.msm_frmle_fold(curve, 0, out, a, n, batch, stride, c, flags), L.msm_frmle_eval(curve, 0, a, n, batch, stride, point, flags, v),
                L.msm_frmle_eq(curve, 0, out, n, point, c, flags), L.msm_frmle_round(curve, 0, a, n, batch, stride, terms, num_terms, fold_by, flags, v)]

    assert every(curve=7) == [inval] * 4 and every(curve=-1) == [inval] * 4  # no such curve
    for bad_n in (0, 3, 6, 12):  # not a power of two
        assert every(n=bad_n, stride=16) == [inval] * 4, bad_n
    assert every(n=1)[0] == inval and every(n=1)[3] == inval  # nothing to bind (eval and eq take n = 1)
    assert every(n=2, fold_by=one)[3] == inval  # the fused round needs two variables
    res = every(batch=0)
    assert res[:2] + res[3:] == [inval] * 3
    res = every(stride=n - 1)  # rows that overlap
    assert res[:2] + res[3:] == [inval] * 3
    assert L.msm_frmle_fold_device(0, 0, None, D(), D(), 1 << 13, (1 << 13) + 1, 1 << 13, one, 0) == inval  # batch * stride > 2^26
    assert L.msm_frmle_eval_device(0, 0, None, D(), 2, 1 << 63, 2, one, 0, v) == inval  # (... with a product that wraps)
    assert L.msm_frmle_eq_device(0, 0, None, D(), 1 << 27, one * 27, one, 0) == inval
    assert L.msm_frmle_round_device(0, 0, None, D(), 1 << 27, 1, 1 << 27, good, 1, None, 0, v) == inval
    assert L.msm_frmle_round_device(0, 0, None, D(), 4, 17, 4, good, 1, None, 0, v) == inval  # more than 16 rows
    # a constant >= r: the challenge, a coordinate of the point, the scale, a coefficient, fold_by -- in both data forms
    assert every(c=big)[0] == inval and every(c=big)[2] == inval and every(c=b"\xff" * 32, flags=MONT256)[0] == inval
    res = every(point=one * 2 + big)
    assert res[1:3] == [inval] * 2
    assert every(terms=_terms(api, [(big, (0,))]))[3] == inval and every(fold_by=big)[3] == inval
    # the terms: their number, a degree, a row
    assert every(num_terms=0)[3] == inval and every(terms=_terms(api, [(one, (0,))] * 9), num_terms=9)[3] == inval
    zero_degree = _terms(api, [(one, (0,))])
    zero_degree[0].degree = 0
    five = _terms(api, [(one, (0, 0, 0, 0))])
    five[0].degree = 5
    assert every(terms=zero_degree)[3] == inval and every(terms=five)[3] == inval
    assert every(terms=_terms(api, [(one, (0, 2))]))[3] == inval  # row 2 of two rows
    # a missing pointer
    assert L.msm_frmle_fold(0, 0, None, a, n, 1, n, one, 0) == inval and L.msm_frmle_fold(0, 0, out, None, n, 1, n, one, 0) == inval
    assert L.msm_frmle_fold(0, 0, out, a, n, 1, n, None, 0) == inval
    assert L.msm_frmle_eval(0, 0, None, n, 1, n, one * 3, 0, v) == inval and L.msm_frmle_eval(0, 0, a, n, 1, n, None, 0, v) == inval
    assert L.msm_frmle_eval(0, 0, a, n, 1, n, one * 3, 0, None) == inval
    assert L.msm_frmle_eq(0, 0, None, n, one * 3, one, 0) == inval and L.msm_frmle_eq(0, 0, out, n, None, one, 0) == inval and L.msm_frmle_eq(0, 0, out, n, one * 3, None, 0) == inval
    assert L.msm_frmle_round(0, 0, None, n, 2, n, good, 1, None, 0, v) == inval and L.msm_frmle_round(0, 0, a, n, 2, n, None, 1, None, 0, v) == inval
    assert L.msm_frmle_round(0, 0, a, n, 2, n, good, 1, None, 0, None) == inval
    # an unaligned device pointer
    assert L.msm_frmle_fold_device(0, 0, None, D(8), D(1024), n, 1, n, one, 0) == inval and L.msm_frmle_fold_device(0, 0, None, D(1024), D(4), n, 1, n, one, 0) == inval
    assert L.msm_frmle_eval_device(0, 0, None, D(8), n, 1, n, one * 3, 0, v) == inval and L.msm_frmle_eq_device(0, 0, None, D(4), n, one * 3, one, 0) == inval
    assert L.msm_frmle_round_device(0, 0, None, D(8), n, 2, n, good, 1, None, 0, v) == inval
    # an unknown flag
    assert every(flags=4) == [inval] * 4 and every(flags=1) == [inval] * 4
    # a partial overlap of fold's output with its input (the same pointer is the in-place call, and passes on to the device check)
    assert L.msm_frmle_fold_device(0, 0, None, D(32), D(), n, 1, n, one, 0) == inval
    assert L.msm_frmle_fold_device(0, 0, None, D(32 * n), D(), n, 2, n, one, 0) == inval  # (the second row of the input)
    assert L.msm_frmle_fold_device(0, 0, None, D(32 * 20), D(), n, 2, 16, one, 0) == inval  # (inside the rows' span: (batch - 1) stride + n)
    # the hooks
    for bad in (1, 3, 6, 1025, 2048, -4):
        assert L.msm_frmle_test_tile(bad) == inval, bad
    assert L.msm_frmle_test_tile(2) == 0 and L.msm_frmle_test_tile(1024) == 0 and L.msm_frmle_test_tile(0) == 0
    assert L.msm_frmle_test_last(None, None) == inval
    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        assert every() == [ERR_NO_DEVICE] * 4 and every(flags=MONT256, c=(r - 1).to_bytes(32, "little"), fold_by=(r - 1).to_bytes(32, "little")) == [ERR_NO_DEVICE] * 4
        for curve in range(7):  # every curve has its field here, Grumpkin included
            assert every(curve=curve) == [ERR_NO_DEVICE] * 4, curve
        assert every(n=1, batch=1)[1:3] == [ERR_NO_DEVICE] * 2 and L.msm_frmle_eval(0, 0, a, 1, 3, 2, None, 0, v) == ERR_NO_DEVICE  # (no point for n = 1)
        assert every(stride=n + 8, batch=1, terms=_terms(api, [(one, (0,))])) == [ERR_NO_DEVICE] * 4  # (a stride beyond n)
        assert every(terms=_terms(api, [(one, (1, 1, 1, 1))]))[3] == ERR_NO_DEVICE  # (a row may repeat)
        assert L.msm_frmle_fold_device(0, 0, None, D(), D(), n, 1, n, one, 0) == ERR_NO_DEVICE  # in place
        assert L.msm_frmle_fold_device(2, 0, None, D(32 * 24), D(), n, 2, 16, one, 0) == ERR_NO_DEVICE  # (apart: behind the span)
        assert L.msm_frmle_eval_device(0, 0, None, D(), 1 << 13, 1 << 13, 1 << 13, one * 13, 0, v) == ERR_NO_DEVICE  # batch * stride = 2^26 exactly
        assert L.msm_frmle_round_device(4, 0, None, D(), 4, 16, 4, _terms(api, [(one, (15, 0, 15, 0))] * 8), 8, one, 0, v) == ERR_NO_DEVICE
        assert [x.raw for x in bufs] == before and val.raw == bytes(32 * 5)
    L.msm_frmle_release()  # (nothing held: a no-op)


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
    for name in ("lib", "fr_lib", "frvec_lib", "frpoly_lib", "frmle_lib"):
        monkeypatch.setattr(scalars, name, no_call)
    r = api.SCALAR_FIELDS["bn254"]
    v = bytes(32 * 8)
    T = [(1, (0, 1))]
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        _bare_context().scalars_mle_fold(v, 1)

    def every_method(ctx):
        return [lambda: ctx.scalars_mle_fold(v, 1), lambda: ctx.scalars_mle_eval(v, [1, 2, 3]), lambda: ctx.scalars_eq([1, 2]), lambda: ctx.scalars_sumcheck_round(v, T, batch=2)]

    for width in (1, 8, 16):  # a narrow scalar format
        for call in every_method(_bare_context(width=width)):
            with pytest.raises(ValueError):
                call()
    for curve in ("grumpkin", "bn254_g2", "pallas"):  # every curve is offered: these get as far as the library
        calls = every_method(_bare_context(curve))
        for call in calls[:2] + calls[3:]:  # (scalars_eq allocates its device tensor first)
            with pytest.raises(AssertionError, match="the library was called"):
                call()
    ctx = _bare_context()
    for bad in (lambda: ctx.scalars_mle_fold(bytes(33), 1),  # not whole scalars
                lambda: ctx.scalars_mle_eval(b"", []),  # nothing at all
                lambda: ctx.scalars_mle_fold(bytes(32 * 6), 1),  # not a power of two
                lambda: ctx.scalars_mle_fold(v, 1, n=3),
                lambda: ctx.scalars_mle_fold(v, 1, n=16),  # longer than a row
                lambda: ctx.scalars_mle_fold(bytes(32), 1),  # nothing to bind
                lambda: ctx.scalars_mle_fold(v, 1, batch=3),  # rows that do not divide the buffer
                lambda: ctx.scalars_mle_fold(v, 1, batch=0),
                lambda: ctx.scalars_mle_fold(v, r),  # a constant >= r, or negative
                lambda: ctx.scalars_mle_fold(v, -1),
                lambda: ctx.scalars_mle_fold(v, bytes(31)),
                lambda: ctx.scalars_mle_eval(v, [1, 2]),  # a point of the wrong length
                lambda: ctx.scalars_mle_eval(v, [1, 2, r]),
                lambda: ctx.scalars_mle_eval(v, [1], n=4),
                lambda: ctx.scalars_eq([1, r]),
                lambda: ctx.scalars_eq([1, 2], scale=r),
                lambda: ctx.scalars_eq([1] * 27),
                lambda: ctx.scalars_sumcheck_round(v, [], batch=2),  # no term, too many terms
                lambda: ctx.scalars_sumcheck_round(v, T * 9, batch=2),
                lambda: ctx.scalars_sumcheck_round(v, [(1, ())], batch=2),  # a degree
                lambda: ctx.scalars_sumcheck_round(v, [(1, (0, 0, 0, 0, 0))], batch=2),
                lambda: ctx.scalars_sumcheck_round(v, [(1, (0, 2))], batch=2),  # a row
                lambda: ctx.scalars_sumcheck_round(v, [(1, (-1,))], batch=2),
                lambda: ctx.scalars_sumcheck_round(v, [(r, (0,))], batch=2),  # a coefficient
                lambda: ctx.scalars_sumcheck_round(v, T, batch=2, fold=r),
                lambda: ctx.scalars_sumcheck_round(v, T, batch=4, fold=1),  # two scalars to a row: the fused round needs four
                lambda: ctx.scalars_sumcheck_round(bytes(32 * 64), [(1, (0,))], batch=32)):  # more than 16 rows
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):  # out belongs to device tables
        ctx.scalars_mle_fold(v, 1, out=bytearray(32 * 8))
    with pytest.raises(TypeError):  # the prover runs in place on the device
        ctx.sumcheck_prove(v, T, 2, lambda j, values: 1)
