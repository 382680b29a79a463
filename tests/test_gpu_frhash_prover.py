"""Hashing beside the rest of a prover, on the device: the evaluations of a polynomial of 2^10 coefficients (scalars_fft) committed to by a Merkle
tree (merkle_tree), whose paths (merkle_path) the model's verifier accepts for the first, a middle and the last leaf and refuses once a sibling
is changed; and the permutation put together from scalars_gate calls -- u = s + c over a row of ones, then sum_j M[i][j] u_j^5 --, which shares
no code with the hashing kernels, against scalars_permute on 64 states."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frhash_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
LOG_N = 10
CASES = [("bn254", False), ("bn254", True), ("bls12_381", False)]


@pytest.fixture(scope="module")
def contexts(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(curve="bn254", mont=False):
        if curve not in made:
            made[curve] = m.MsmContext(0, curve)
        made[curve].set_scalar_format(mont256=mont)
        return made[curve]

    yield get
    for c in made.values():
        c.close()
    api.frhash_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def plain(vals, r, mont):
    return M.unmont(vals, r) if mont else list(vals)


@pytest.mark.parametrize("curve,mont", CASES, ids=["%s-%s" % (c, "mont256" if f else "canonical") for c, f in CASES])
def test_a_merkle_commitment_to_evaluations_and_its_paths(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r, rnd = api.SCALAR_FIELDS[curve], rng(1500)
    n = 1 << LOG_N
    coeffs = [rnd.randrange(r) for _ in range(n)]
    evals = ctx.scalars_fft(dev(form(coeffs, r, mont)), LOG_N)
    p = M.standard(r, 3)
    with ctx.poseidon() as h:
        nodes = ctx.merkle_tree(h, evals)
        assert nodes.is_cuda and tuple(nodes.shape) == (n - 1, 32)
        leaves, tree = plain(host(evals), r, mont), plain(host(nodes), r, mont)
        root = tree[-1]
        for index in (0, 345, n - 1):
            path = ctx.merkle_path(h, evals, nodes, index)
            assert path.is_cuda and tuple(path.shape) == (LOG_N, 1, 32)
            siblings = [plain(host(level), r, mont) for level in path]
            assert p.verify(leaves[index], index, siblings, root), (curve, mont, index)
            siblings[LOG_N // 2][0] ^= 1  # a flipped sibling
            assert not p.verify(leaves[index], index, siblings, root)
            assert not p.verify(leaves[index], index ^ 1, [plain(host(level), r, mont) for level in path], root)
    # a tree of arity 4 over the same leaves: three siblings a level
    p5 = M.standard(r, 5)
    with ctx.poseidon(t=5) as h:
        nodes = ctx.merkle_tree(h, evals)
        path = ctx.merkle_path(h, evals, nodes, 777)
        assert tuple(path.shape) == (LOG_N // 2, 3, 32)
        assert p5.verify(leaves[777], 777, [plain(host(level), r, mont) for level in path], plain(host(nodes), r, mont)[-1])


@pytest.mark.parametrize("curve,mont", CASES, ids=["%s-%s" % (c, "mont256" if f else "canonical") for c, f in CASES])
def test_the_permutation_chained_from_gates_agrees(contexts, curve, mont):
    """what a user did before: per round one gate for u = s + c (the constants as coefficients of a row of ones) and one per output element
    for sum_j M[i][j] u_j^5, or M[i][0] u_0^5 + sum_{j > 0} M[i][j] u_j in a partial round -- 2 t launches a round"""
    ctx = contexts(curve, mont)
    r, rnd = api.SCALAR_FIELDS[curve], rng(1600)
    t, rf, rp, n = 3, 8, 5, 64  # (fewer partial rounds than the standard 57: the chain is 2 t launches a round)
    rc, mds = api.poseidon_parameters(curve, t, rf, rp)
    states = [[rnd.randrange(r) for _ in range(t)] for _ in range(n)]
    # the chain works on columns: row i holds element i of every state; row t holds ones
    cols = torch.empty((t + 1, n, 32), dtype=torch.uint8, device="cuda")
    for i in range(t):
        cols[i] = dev(form([s[i] for s in states], r, mont))
    cols[t] = dev(form([1] * n, r, mont))
    u = torch.empty_like(cols)
    u[t] = cols[t]
    for k in range(rf + rp):
        full = k < rf // 2 or k >= rf // 2 + rp
        for i in range(t):
            ctx.scalars_gate(cols, [(1, (i,)), (rc[k * t + i], (t,))], batch=t + 1, out=u[i])
        for i in range(t):
            terms = [(mds[i][j], (j,) * 5 if full or j == 0 else (j,)) for j in range(t)]
            ctx.scalars_gate(u, terms, batch=t + 1, out=cols[i])
    chained = [host(cols[i]) for i in range(t)]
    with ctx.poseidon(t, rf, rp) as h:
        fused = host(ctx.scalars_permute(h, dev(form([x for s in states for x in s], r, mont))))
    assert fused == [chained[i][k] for k in range(n) for i in range(t)]
    p = M.standard(r, t, rf, rp)
    assert plain(fused[:t], r, mont) == p.permute(states[0])
