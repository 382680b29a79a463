"""What a prover computes between a transform and the next commitment, on BN254 through the engine's own pieces end to end (MsmContext.scalars_*,
scalars_fft, mul_base, lagrange_bases, msm):
(a) a permutation argument's grand product z[i + 1] = z[i] (f[i] + beta id[i] + gamma) / (f[i] + beta sigma[i] + gamma), which closes at 1 exactly
    when f is constant along the cycles of sigma, committed over a Lagrange SRS;
(b) a QAP quotient h = (a b - c) / Z computed on a coset, checked as the polynomial identity A B - C = H (X^n - 1) at a random point."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from oracle import bn254_ref
from tests import frvec_model as M
from tests import ntt_model as N
from tests.util import rng

pytestmark = pytest.mark.gpu
R = bn254_ref.R


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


def _cycles(sigma):
    seen, out = set(), []
    for s in range(len(sigma)):
        if s not in seen:
            cyc, k = [], s
            while k not in seen:
                seen.add(k)
                cyc.append(k)
                k = sigma[k]
            out.append(cyc)
    return out


def _grand_product(ctx, f, ident, sigma, beta, gamma):
    """-> (z on the device, the row's total): z = exclusive product scan of num / den"""
    fg = ctx.scalars_add(dev(f), gamma)
    num = ctx.scalars_mul_add(dev(ident), beta, fg, out=torch.empty_like(fg))
    den = ctx.scalars_mul_add(dev(sigma), beta, fg)
    ratio = ctx.scalars_mul(num, ctx.scalars_inverse(den))
    z, total = ctx.scalars_scan(ratio, op="product", exclusive=True, totals=True)
    return z, M.from_bytes(total)[0]


@pytest.mark.parametrize("log_n", [6, 10])
def test_permutation_grand_product(built, log_n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1 << log_n
    rnd = rng(7000 + log_n)
    sigma = list(range(n))
    rnd.shuffle(sigma)
    cycles = _cycles(sigma)
    f = [0] * n
    for cyc in cycles:
        v = rnd.randrange(R)
        for k in cyc:
            f[k] = v
    beta, gamma, tau = rnd.randrange(1, R), rnd.randrange(R), rnd.randrange(2, R)
    ident = list(range(n))
    ctx = m.MsmContext(0)
    try:
        z, total = _grand_product(ctx, f, ident, sigma, beta, gamma)
        num = M.map_op("mul_add", ident, beta, M.map_op("add", f, gamma, None, R), R)
        den = M.map_op("mul_add", sigma, beta, M.map_op("add", f, gamma, None, R), R)
        want, want_total = M.scan(M.map_op("mul", num, M.inverse(den, R), None, R), "product", True, R)
        assert host(z) == want and total == want_total[0] == 1 and want[0] == 1
        # one cell altered on a cycle of length >= 2 (a fixed point of sigma cancels itself): the product no longer closes
        cell = next(c for c in cycles if len(c) >= 2)[0]
        g = list(f)
        g[cell] = (g[cell] + 1) % R
        assert _grand_product(ctx, g, ident, sigma, beta, gamma)[1] != 1
        # the commitment to z from its evaluations over the Lagrange SRS is the commitment from its coefficients over the monomial SRS
        ctx.set_bases(bn254_ref.points_to_bytes([bn254_ref.G]))
        srs = ctx.mul_base(0, M.to_bytes([pow(tau, j, R) for j in range(n)]))
        ctx.set_bases(srs)
        coeffs = ctx.scalars_fft(z.clone(), inverse=True)
        from_coefficients = ctx.msm(coeffs)
        ctx.set_bases(ctx.lagrange_bases())
        from_evaluations = ctx.msm(z)
        assert from_evaluations.to_affine_bytes() == from_coefficients.to_affine_bytes()
        z_tau = sum(c * pow(tau, j, R) for j, c in enumerate(host(coeffs))) % R
        ctx.set_bases(bn254_ref.points_to_bytes([bn254_ref.G]))
        assert ctx.msm(M.to_bytes([z_tau])).to_affine_bytes() == from_evaluations.to_affine_bytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("log_n", [6, 10])
def test_qap_quotient_on_a_coset(built, log_n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1 << log_n
    rnd = rng(7100 + log_n)
    a, b = [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]
    g = rnd.randrange(2, R)
    while pow(g, n, R) == 1:
        g = rnd.randrange(2, R)
    ctx = m.MsmContext(0)
    try:
        da, db = dev(a), dev(b)
        dc = ctx.scalars_mul(da, db, out=torch.empty_like(da))  # c = a b on the domain
        assert host(dc) == M.map_op("mul", a, b, None, R)
        for t in (da, db, dc):
            ctx.scalars_fft(t, inverse=True)  # the coefficients of A, B, C ...
        A, B, Cc = host(da), host(db), host(dc)
        assert A == N.intt(a, api.root_of_unity("bn254", log_n), R)
        for t in (da, db, dc):
            ctx.scalars_fft(t, shift=g)  # ... and their values on the coset g H, where Z = X^n - 1 is the constant g^n - 1
        h = ctx.scalars_mul_sub(da, db, dc)
        ctx.scalars_mul(h, pow(pow(g, n, R) - 1, R - 2, R))
        ctx.scalars_fft(h, inverse=True, shift=g)
        H = host(h)
        assert H[n - 1] == 0 and any(H)  # deg H <= n - 2
        x = rnd.randrange(R)
        ev = lambda p: sum(c * pow(x, j, R) for j, c in enumerate(p)) % R  # noqa: E731
        assert (ev(A) * ev(B) - ev(Cc)) % R == ev(H) * (pow(x, n, R) - 1) % R
    finally:
        ctx.close()
