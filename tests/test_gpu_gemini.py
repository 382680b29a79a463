"""Gemini's multilinear-to-univariate folds and the prover's first two moves of a HyperKZG-style opening on the device (msm-webgpu_amd/
multilinear.py: gemini_folds, gemini_open) over a small monomial SRS built with mul_base, on BN254 and BLS12-381: the folds against the model by
index bits (tests/frmle_low_model.py), the value against evaluate() and the model, every commitment against msm of the model's fold, and the
verifier's identity between consecutive folds in host integers."""
import importlib

import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from msm_webgpu_amd import multilinear as ml
from tests import frmle_low_model as L
from tests.util import rng

pytestmark = pytest.mark.gpu
SIZES = (2, 8, 64, 1024)


def dev(vals):
    return torch.frombuffer(bytearray(L.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return L.from_bytes(t.cpu().numpy().tobytes())


@pytest.fixture(scope="module", params=["bn254", "bls12_381"])
def srs(request, built):
    """a context whose resident bases are tau^j G, j < 1024"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    curve = request.param
    ref = importlib.import_module("oracle.%s_ref" % curve)
    r = api.SCALAR_FIELDS[curve]
    ctx = m.MsmContext(0, curve)
    ctx.set_bases(ref.points_to_bytes([ref.G]))
    tau = rng(900).randrange(2, r)
    ctx.set_bases(ctx.mul_base(0, ctx.scalars_powers(tau, max(SIZES))))
    yield curve, r, ctx
    ctx.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
def test_folds_commitments_and_the_verifiers_identity(srs, n, mont):
    curve, r, ctx = srs
    ctx.set_scalar_format(mont256=mont)
    try:
        k = n.bit_length() - 1
        rnd = rng(910 + n)
        a = [rnd.randrange(r) for _ in range(n)]
        a[0], a[-1] = r - 1, 0
        point = [rnd.randrange(r) for _ in range(k)]
        form = (lambda v: L.mont(v, r)) if mont else list
        back = (lambda v: L.mont(v, r, back=True)) if mont else list
        t = dev(form(a))
        model = L.gemini_folds(a, point, r)
        value = L.evaluate(a, point, r)
        assert model[-1] == [value]
        # the folds: one tensor f_1 | .. | f_k of n - 1 scalars; a untouched; one launch each
        folds = ml.gemini_folds(ctx, t, point)
        assert tuple(folds.shape) == (n - 1, 32) and back(host(folds)) == [x for f in model for x in f], (curve, n)
        assert host(t) == form(a) and api.frmle_last() == (1, 1)
        assert ml.gemini_slices(n) == [(n - (n >> j), n >> (j + 1)) for j in range(k)]
        # the opening
        seen = []

        def challenge(commitments):
            seen.append(commitments)
            return 0x1234567 + n

        got_value, commitments, x, evals = ml.gemini_open(ctx, t, point, challenge)
        assert host(t) == form(a) and seen == [commitments] and x == 0x1234567 + n and len(commitments) == k - 1 and len(evals) == 32 * 3 * k
        assert got_value == ml.evaluate(ctx, t, point) and back(L.from_bytes(got_value)) == [value]
        for c, f in zip(commitments, model):
            assert c.to_affine_bytes() == ctx.msm(dev(form(f))).to_affine_bytes(), (curve, n)
        e = back(L.from_bytes(evals))
        e = [e[3 * j:3 * j + 3] for j in range(k)]
        fs = [a] + model
        for j in range(k):
            assert e[j] == [L.horner(fs[j], z, r) for z in (x, r - x, x * x % r)], (curve, n, j)
            plus, minus, u = e[j][0], e[j][1], point[j]
            want = ((1 - u) * (plus + minus) * pow(2, -1, r) + u * (plus - minus) * pow(2 * x, -1, r)) % r
            assert want == (e[j + 1][2] if j + 1 < k else value), (curve, n, j)
    finally:
        ctx.set_scalar_format(mont256=False)


def test_a_challenge_outside_the_field_and_a_table_beyond_the_bases_raise(srs):
    curve, r, ctx = srs
    t = dev([5, 6, 7, 8])
    for bad in (0, r, -1):
        with pytest.raises(ValueError):
            ml.gemini_open(ctx, t, [1, 2], lambda commitments: bad)
    with pytest.raises(ValueError):
        ml.gemini_open(ctx, dev([1] * 2048), [1] * 11, lambda commitments: 3)
    with pytest.raises(ValueError):
        ml.gemini_folds(ctx, t, [1, 2, 3])
    with pytest.raises(ValueError):
        ml.gemini_folds(ctx, dev([1, 2, 3]), [1])
    assert host(t) == [5, 6, 7, 8]
