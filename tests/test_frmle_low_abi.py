"""MSM_FRMLE_LOW_FIRST (include/msm_frmle.h) without a GPU: the flag and its in-place rule are in the header, the four host forms accept it alone
and with MSM_FRMLE_MONT256 and with nothing else, the low-first model (tests/frmle_low_model.py) is the top-first one (tests/frmle_model.py) on
the bit-reversed table, and msm-webgpu_amd/multilinear.py stands beside the pinned modules and refuses an unknown order before any call."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import frmle_low_model as L
from tests import frmle_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG = -1, -2
MONT256, LOW_FIRST = 2, 8
R_MODEL = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def test_the_header_defines_the_flag_and_states_the_in_place_rule():
    full = open(os.path.join(ROOT, "include", "msm_frmle.h")).read()
    code = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define MSM_FRMLE_LOW_FIRST 8u\s", code)
    flat = " ".join(full.replace("*", " ").split())
    assert "TOP bit" in full and "is not offered" not in full
    assert "the elements [n / 2, n) of the row are UNSPECIFIED afterwards and the elements [n, stride) are untouched" in flat
    assert "leaves everything behind the result as it was" in flat  # (the difference from the top-first contract is stated)
    assert "2 launches" in flat and "launches = levels + 1" in flat  # (what msm_frmle_test_last reports)
    from msm_webgpu_amd import multilinear

    assert multilinear.LOW_FIRST == LOW_FIRST


def test_the_host_forms_take_the_flag_alone_and_with_mont256_only(built):
    from msm_webgpu_amd import api

    lib = api.frmle_lib()
    r = api.SCALAR_FIELDS["bn254"]
    one = (1).to_bytes(32, "little")
    n = 8
    bufs = [C.create_string_buffer(bytes([7 + k]) * (32 * 2 * n), 32 * 2 * n) for k in range(2)]
    out, a = [C.cast(x, C.c_void_p) for x in bufs]
    val = C.create_string_buffer(32 * 5)
    v = C.cast(val, C.c_void_p)
    term = (api.FrmleTerm * 1)()
    term[0].coeff[:] = one
    term[0].degree = 2
    term[0].rows[:2] = (0, 1)

    def every(flags, fold_by=None, curve=0, c=one):
        return [lib.msm_frmle_fold(curve, 0, out, a, n, 2, n, c, flags), lib.msm_frmle_eval(curve, 0, a, n, 2, n, one * 3, flags, v),
                lib.msm_frmle_eq(curve, 0, out, n, one * 3, c, flags), lib.msm_frmle_round(curve, 0, a, n, 2, n, term, 1, fold_by, flags, v)]

    for bad in (LOW_FIRST | 4, LOW_FIRST | 1, LOW_FIRST | 16, 12, 9):
        assert every(bad) == [ERR_INVALID_ARG] * 4, bad
    # the other checks hold under the flag: a constant >= r, n too small for the fused round
    assert every(LOW_FIRST, c=r.to_bytes(32, "little"))[0] == ERR_INVALID_ARG
    assert lib.msm_frmle_round(0, 0, a, 2, 2, n, term, 1, one, LOW_FIRST, v) == ERR_INVALID_ARG
    assert lib.msm_frmle_abi_version() == 1
    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        for flags in (LOW_FIRST, LOW_FIRST | MONT256):
            assert every(flags) == [ERR_NO_DEVICE] * 4, flags  # (past the host's checks: on the parent these are ERR_INVALID_ARG)
            assert every(flags, fold_by=one)[3] == ERR_NO_DEVICE
            for curve in range(7):
                assert every(flags, curve=curve) == [ERR_NO_DEVICE] * 4, curve
        assert [x.raw for x in bufs] == before and val.raw == bytes(32 * 5)


def test_low_first_is_top_first_on_the_bit_reversed_table():
    r, rnd = R_MODEL, rng(71)
    terms = [(5, (0, 1, 2)), (r - 1, (0, 2)), (3, (1, 1, 1, 1)), (9, (2,))]
    for k in (1, 2, 3, 5):
        n = 1 << k
        rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(3)]
        rev = [L.bit_reversed(row) for row in rows]
        assert L.bit_reversed(rev[0]) == rows[0]
        c = rnd.randrange(r)
        point = [rnd.randrange(r) for _ in range(k)]
        # fold: the low-first result, bit-reversed over its k - 1 bits, is the top-first fold of the bit-reversed table
        assert [L.bit_reversed(L.fold(row, c, r)) for row in rows] == [M.fold(row, c, r) for row in rev]
        assert L.round_values(rows, terms, r) == M.round_values(rev, terms, r)
        challenge = lambda j, values: (values[0] * 7 + values[-1] + j) % r  # noqa: E731  (depends on the transcript)
        assert L.prove(rows, terms, challenge, r) == M.prove(rev, terms, challenge, r)
        # eval: the same point on the reversed table, or the reversed point on the same table
        assert L.evaluate(rows[0], point, r) == M.evaluate(rev[0], point, r) == M.evaluate(rows[0], point[::-1], r)
        assert L.bit_reversed(L.eq(point, r, 7)) == M.eq(point, r, 7) and L.eq(point, r, 7) == M.eq(point[::-1], r, 7)
        folds = L.gemini_folds(rows[0], point, r)
        assert [len(f) for f in folds] == [n >> (j + 1) for j in range(k)] and folds[-1] == [L.evaluate(rows[0], point, r)]
    assert L.evaluate([3], [], r) == 3 and L.eq([], r, 4) == [4] and L.bit_reversed([9]) == [9]
    # x_0 is bit 0: a point of bits picks the element they spell
    a = list(range(100, 108))
    assert [L.evaluate(a, [i & 1, (i >> 1) & 1, (i >> 2) & 1], r) for i in range(8)] == a
    assert L.eq([1, 0, 1], r) == [0, 0, 0, 0, 0, 1, 0, 0] and L.eq([1, 1, 0], r) == [0, 0, 0, 1, 0, 0, 0, 0]
    assert L.fold([1, 2, 10, 20], 0, r) == [1, 10] and L.fold([1, 2, 10, 20], 1, r) == [2, 20]


def test_the_gemini_identity_holds_in_the_model():
    """f_(j+1)(x^2) = (1 - u) (f_j(x) + f_j(-x)) / 2 + u (f_j(x) - f_j(-x)) / (2 x): the even and odd coefficients of f_j"""
    r, rnd = R_MODEL, rng(72)
    a = [rnd.randrange(r) for _ in range(16)]
    point = [rnd.randrange(r) for _ in range(4)]
    x = rnd.randrange(1, r)
    fs = [a] + L.gemini_folds(a, point, r)
    for j, u in enumerate(point):
        plus, minus = L.horner(fs[j], x, r), L.horner(fs[j], r - x, r)
        want = ((1 - u) * (plus + minus) * pow(2, -1, r) + u * (plus - minus) * pow(2 * x, -1, r)) % r
        assert L.horner(fs[j + 1], x * x % r, r) == want


def test_multilinear_stands_beside_the_pinned_modules():
    pkg = os.path.join(ROOT, "msm-webgpu_amd")
    assert os.path.exists(os.path.join(pkg, "multilinear.py"))
    for name in ("api.py", "scalars.py", "__init__.py", "_core.py"):
        with open(os.path.join(pkg, name)) as f:
            assert not re.search(r"^\s*(from|import)\b.*\bmultilinear\b|import_module\(.*multilinear", f.read(), flags=re.M), name
    import inspect

    from msm_webgpu_amd import multilinear as ml

    want = {"fold": "(ctx, a, c, batch=1, n=None, out=None, order='low')", "evaluate": "(ctx, a, point, batch=1, n=None, order='low')",
            "eq": "(ctx, point, scale=1, out=None, order='low')", "sumcheck_round": "(ctx, a, terms, batch=1, n=None, fold=None, order='low')",
            "sumcheck_prove": "(ctx, a, terms, batch, challenge, order='low')", "gemini_folds": "(ctx, a, point)",
            "gemini_open": "(ctx, coeffs, point, challenge)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(ml, name))) == sig, name


def _bare_context(curve="bn254"):
    """An MsmContext that never touched the library (no device needed)"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.scalar_width, ctx.scalar_signed, ctx.scalar_mont256, ctx.n_bases, ctx._keepalive = curve, 32, False, False, 0, {}
    ctx.curve_id, ctx.modulus = api.CURVES[curve]
    ctx.device = 0
    return ctx


def test_an_unknown_order_raises_before_any_library_call(built, monkeypatch):
    from msm_webgpu_amd import api, scalars
    from msm_webgpu_amd import multilinear as ml

    def no_call():
        raise AssertionError("the library was called")

    monkeypatch.setattr(api, "lib", no_call)
    for name in ("lib", "frmle_lib", "frpoly_lib"):
        monkeypatch.setattr(scalars, name, no_call)
    ctx = _bare_context()
    v = bytes(32 * 8)
    T = [(1, (0, 1))]
    with pytest.raises(AssertionError, match="the library was called"):  # (the trap sits in the path: a well-formed call reaches it)
        ml.fold(ctx, v, 1)
    with pytest.raises(AssertionError, match="the library was called"):
        ml.sumcheck_round(_bare_context("grumpkin"), v, T, batch=2, order="top")
    for order in ("bad", "LOW", None, 8):
        for call in (lambda: ml.fold(ctx, v, 1, order=order), lambda: ml.evaluate(ctx, v, [1, 2, 3], order=order), lambda: ml.eq(ctx, [1, 2], order=order),
                     lambda: ml.sumcheck_round(ctx, v, T, batch=2, order=order), lambda: ml.sumcheck_prove(ctx, v, T, 2, lambda j, values: 1, order=order)):
            with pytest.raises(ValueError, match="order"):
                call()
    for bad in (lambda: ml.fold(ctx, bytes(32), 1), lambda: ml.fold(ctx, v, api.SCALAR_FIELDS["bn254"]), lambda: ml.evaluate(ctx, v, [1, 2]),
                lambda: ml.eq(ctx, [1] * 27), lambda: ml.sumcheck_round(ctx, v, T, batch=4, fold=1), lambda: ml.sumcheck_round(ctx, v, [(1, (0, 2))], batch=2)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ml.sumcheck_prove(ctx, v, T, 2, lambda j, values: 1)
    with pytest.raises(TypeError):
        ml.gemini_folds(ctx, v, [1, 2, 3])
    with pytest.raises(TypeError):
        ml.gemini_open(ctx, v, [1, 2, 3], lambda commitments: 1)
