"""What a prover does after its last commitment, on BN254 through the engine's own pieces end to end (MsmContext.scalars_powers, mul_base,
scalars_combine, kzg_open, scalars_fft, scalars_dot, lagrange_bases, msm):
(a) a batched KZG opening: four polynomials folded with powers of gamma, opened at z over a monomial SRS; the witness satisfies
    q(tau) (tau - z) = f(tau) - y, its commitment is q(tau) G, and the commitment to the fold is the fold of the commitments;
(b) the same opening in evaluation form, as EIP-4844 computes it: y = (z^n - 1) / n sum p_i w^i / (z - w^i) and q_i = (p_i - y) / (w^i - z) over the
    domain of the n-th roots of unity, committed over the Lagrange SRS to the same point."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from oracle import bn254_ref
from tests import frpoly_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
R = bn254_ref.R


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


def point(g1):
    return bn254_ref.bytes_to_points(g1.to_affine_bytes())[0]


@pytest.mark.parametrize("log_n", [6, 10])
def test_batched_kzg_opening_in_both_forms(built, log_n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1 << log_n
    rnd = rng(8000 + log_n)
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(4)]
    tau, gamma, z = rnd.randrange(2, R), rnd.randrange(2, R), rnd.randrange(2, R)
    omega = api.root_of_unity("bn254", log_n)
    assert pow(z, n, R) != 1  # (z is not in the domain)
    ctx = m.MsmContext(0)
    try:
        # (a) the SRS tau^j G from the power vector, the fold, the opening
        generator = bn254_ref.points_to_bytes([bn254_ref.G])
        ctx.set_bases(generator)
        taus = ctx.scalars_powers(tau, n)
        assert host(taus) == M.powers(tau, n, R)
        srs = ctx.mul_base(0, taus)
        ctx.set_bases(srs)
        rows = dev([x for p in polys for x in p])
        gammas = M.powers(gamma, 4, R)
        commitments = [ctx.msm(rows[k * n:(k + 1) * n].clone()) for k in range(4)]
        f = ctx.scalars_combine(rows, gammas)
        F = host(f)
        assert F == M.combine(polys, gammas, R)
        y_bytes, witness = ctx.kzg_open(f, z)
        assert host(f) == F  # (the opening leaves the polynomial alone)
        y = M.from_bytes(y_bytes)[0]
        assert y == M.evaluate(F, z, R) and y_bytes == ctx.scalars_eval(f, z)
        q = host(ctx.scalars_divide(f, z, out=torch.empty_like(f)))
        assert q[n - 1] == 0 and M.evaluate(q, tau, R) * (tau - z) % R == (M.evaluate(F, tau, R) - y) % R
        fold = ctx.msm(f)
        want = bn254_ref.INF
        for c, k in zip(commitments, gammas):
            want = bn254_ref.add(want, bn254_ref.mul(k, point(c)))
        assert point(fold) == want  # C_f = sum gamma^k C_k by the oracle's group law
        # (b) evaluation form over the Lagrange SRS
        p = ctx.scalars_fft(f.clone())  # p_i = f(w^i)
        domain = ctx.scalars_powers(omega, n)
        shifted = ctx.scalars_sub(domain, z, out=torch.empty_like(domain))  # w^i - z
        inv = ctx.scalars_inverse(shifted)
        weights = ctx.scalars_mul(domain, inv)  # w^i / (w^i - z)
        s = M.from_bytes(ctx.scalars_dot(p, weights))[0]
        y_eval = (1 - pow(z, n, R)) * pow(n, R - 2, R) * s % R
        assert y_eval == y
        q_eval = ctx.scalars_mul(ctx.scalars_sub(p, y_eval), inv)
        assert host(q_eval) == [M.evaluate(q, pow(omega, i, R), R) for i in range(n)]
        ctx.set_bases(ctx.lagrange_bases())
        assert ctx.msm(q_eval).to_affine_bytes() == witness.to_affine_bytes()
        # the witness is q(tau) G
        ctx.set_bases(generator)
        assert ctx.msm(M.to_bytes([M.evaluate(q, tau, R)])).to_affine_bytes() == witness.to_affine_bytes()
        assert bytes(ctx.mul_base(0, M.to_bytes([M.evaluate(q, tau, R)])))[:64] == witness.to_affine_bytes()
    finally:
        ctx.close()
