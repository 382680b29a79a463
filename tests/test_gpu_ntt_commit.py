"""NTT -> MSM end to end on BN254 through the engine's own pieces: a monomial SRS [tau^j G] from mul_base, its Lagrange form from lagrange_bases,
and the scalar-field NTT between the two.  A polynomial's commitment from its coefficients over the monomial SRS equals the commitment from its
evaluations (scalars_fft of the coefficients, on the device) over the Lagrange SRS; the inverse transform of the evaluations gives the
coefficients back."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from oracle import bn254_ref
from tests import ntt_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
R = bn254_ref.R


@pytest.mark.parametrize("log_n", [6, 10])
def test_commitment_from_coefficients_equals_commitment_from_evaluations(built, log_n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1 << log_n
    rnd = rng(5000 + log_n)
    tau = rnd.randrange(2, R)
    a = [rnd.randrange(R) for _ in range(n)]
    ctx = m.MsmContext(0)
    try:
        ctx.set_bases(bn254_ref.points_to_bytes([bn254_ref.G]))
        srs = ctx.mul_base(0, M.to_bytes([pow(tau, j, R) for j in range(n)]))  # [tau^j G]
        ctx.set_bases(srs)
        coeffs = torch.frombuffer(bytearray(M.to_bytes(a)), dtype=torch.uint8).reshape(n, 32).cuda()
        from_coefficients = ctx.msm(coeffs)
        lagrange = ctx.lagrange_bases()  # [L_i(tau) G] for the same omega that scalars_fft takes by default
        evals = ctx.scalars_fft(coeffs.clone())
        assert M.from_bytes(evals.cpu().numpy().tobytes()) == M.ntt(a, api.root_of_unity("bn254", log_n), R)
        ctx.set_bases(lagrange)
        from_evaluations = ctx.msm(evals)  # the transform's output straight into the MSM
        assert from_evaluations == from_coefficients
        assert from_coefficients.to_affine_bytes() == from_evaluations.to_affine_bytes()
        # ... which is p(tau) G
        p_tau = sum(c * pow(tau, j, R) for j, c in enumerate(a)) % R
        ctx.set_bases(bn254_ref.points_to_bytes([bn254_ref.G]))
        assert ctx.msm(M.to_bytes([p_tau])).to_affine_bytes() == from_coefficients.to_affine_bytes()
        back = ctx.scalars_fft(evals, inverse=True)
        assert torch.equal(back, coeffs)
    finally:
        ctx.close()
