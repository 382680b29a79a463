"""A whole sumcheck on the device, on the curves of the provers that run one (Pallas, Grumpkin), through MsmContext.sumcheck_prove: the claim
sum_x eq(tau, x) (A(x) B(x) - C(x)) over 2^11 points, rows eq, A, B, C in one buffer, a deterministic challenge function.  The transcript
verifies with the model's verifier (tests/frmle_model.py), the final values are the rows' multilinear extensions at the challenge point
(scalars_mle_eval of untouched copies), and a commitment to a row made before the proof is what it is after it."""
import hashlib

import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frmle_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
K = 11


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


@pytest.mark.parametrize("curve", ["pallas", "grumpkin"])
def test_sumcheck_prove_end_to_end(built, curve):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = api.SCALAR_FIELDS[curve]
    n = 1 << K
    rnd = rng(9000 + len(curve))
    tau = [rnd.randrange(r) for _ in range(K)]
    A, B, C = ([rnd.randrange(r) for _ in range(n)] for _ in range(3))
    terms = [(1, (0, 1, 2)), (r - 1, (0, 3))]  # eq A B - eq C
    ctx = m.MsmContext(0, curve)
    try:
        ctx.set_bases(ctx.sample_points(n, 77))
        table = torch.empty(4, n, 32, dtype=torch.uint8, device="cuda")
        ctx.scalars_eq(tau, out=table[0])
        table[1:] = dev(A + B + C).reshape(3, n, 32)
        rows = [M.eq(tau, r), A, B, C]
        assert host(table[0]) == rows[0]
        kept = table.clone()
        commitment = ctx.msm(kept[1]).to_affine_bytes()
        seen = []

        def challenge(j, values):
            seen.append((j, values))
            return int.from_bytes(hashlib.sha256(b"round %d" % j + values).digest(), "little") % r

        transcript, point, finals = ctx.sumcheck_prove(table, terms, 4, challenge)
        assert len(transcript) == K and len(point) == K and [j for j, _ in seen] == list(range(K)) and [v for _, v in seen] == transcript
        assert all(len(v) == 32 * 4 for v in transcript)  # degree 3
        claim = M.claimed_sum(rows, terms, r)
        assert M.verify(claim, [M.from_bytes(v) for v in transcript], point, M.from_bytes(finals), terms, r)
        assert not M.verify((claim + 1) % r, [M.from_bytes(v) for v in transcript], point, M.from_bytes(finals), terms, r)
        # the final values: the untouched rows at the challenge point, by the device and by the model
        assert finals == ctx.scalars_mle_eval(kept, point, batch=4)
        assert M.from_bytes(finals)[0] == M.eq_value(tau, point, r) and M.from_bytes(finals)[1] == M.evaluate(A, point, r)
        # the first round against the model, and the commitment made before the proof
        assert M.from_bytes(transcript[0]) == M.round_values(rows, terms, r)
        assert host(kept[1]) == A and ctx.msm(kept[1]).to_affine_bytes() == commitment
    finally:
        ctx.close()
