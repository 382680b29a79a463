"""Poseidon2 on the device (include/msm_frhash.h under MSM_FRHASH_POSEIDON2; MsmContext.poseidon2, scalars_permute, scalars_hash, merkle_tree,
merkle_path) against the pure-Python model (tests/frhash2_model.py), byte for byte: 1, 64 and 65 permutations at the full tile and 65 with four
lanes to a workgroup, in place and out of place, both data forms, all five widths on BN254 and BLS12-381 and t = 3 and t = 12 on the other three
fields, with R_F = 8 and R_P = 56, without internal rounds and with two external rounds alone; the rejection of a value >= r with a correct call
behind it; sponges under the three capacity conventions with a stride whose padding must not be read; trees of arity 2, 3 and 1 with their
paths; a check that does not rest on the new model -- without internal rounds the permutation is the EXISTING Poseidon kernel's with M_E as its
dense matrix, run on M_E x, device against device; and a Poseidon and a Poseidon2 handle of one width alive and called in turn."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frhash2_model as M2
from tests import frhash_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
ERR_NONCANONICAL = -4
ROUNDS = ((8, 56), (8, 0), (2, 0))
CASES = [(c, t) for c in ("bn254", "bls12_381") for t in M2.WIDTHS] + [(c, t) for c in ("grumpkin", "pallas", "vesta") for t in (3, 12)]


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
    api.frhash_test_tile(0)
    for c in made.values():
        c.close()
    api.frhash_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def host(t):
    return M.from_bytes(raw(t))


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def flat(rows):
    return [x for row in rows for x in row]


def handle(ctx, p):
    return ctx.poseidon2(p.t, p.full_rounds, p.partial_rounds, p.rc, p.mu, capacity=p.capacity, capacity_at=p.capacity_at, out_at=p.out_at)


# ---- permutations ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,t", CASES, ids=["%s-t%d" % c for c in CASES])
def test_permutations_of_every_count_and_form(contexts, curve, t):
    r, rnd = api.SCALAR_FIELDS[curve], rng(2000 + t)
    states = [[r - 1] * t, [0] * t] + [[rnd.randrange(r) for _ in range(t)] for _ in range(63)]
    for rf, rp in ROUNDS:
        p = M2.sample(r, t, rf, rp)
        images = [p.permute(s) for s in states]  # (once for both forms)
        for mont in (False, True):
            ctx = contexts(curve, mont)
            with handle(ctx, p) as h:
                assert h.kind == "poseidon2"
                for tile, n in ((0, 1), (0, 64), (0, 65), (4, 65)):  # 64 lanes to a workgroup; four, so that 65 states span 17 workgroups
                    api.frhash_test_tile(tile)
                    src = dev(form(flat(states[:n]), r, mont))
                    before = raw(src)
                    want = M.to_bytes(form(flat(images[:n]), r, mont))
                    big = torch.full((3, n * t, 32), 0xFF, dtype=torch.uint8, device="cuda")  # out of place, into the middle of a buffer of 0xFF
                    got = ctx.scalars_permute(h, src, out=big[1])
                    assert got.data_ptr() == big[1].data_ptr() and raw(big[1]) == want, (curve, t, rf, rp, mont, tile, n)
                    assert raw(big[0]) == b"\xff" * (32 * n * t) and raw(big[2]) == b"\xff" * (32 * n * t) and raw(src) == before
                    assert raw(ctx.scalars_permute(h, src, out=src)) == want, (curve, t, rf, rp, mont, tile, n, "in place")
                api.frhash_test_tile(0)
                assert ctx.scalars_permute(h, M.to_bytes(form(flat(states[:3]), r, mont))) == M.to_bytes(form(flat(images[:3]), r, mont))  # the host form


def test_the_pattern_that_reaches_the_bounds(contexts):
    """state, constants, mu and capacity all r - 1 at t = 12, through the device's multipliers: permutations, and a sponge of three blocks"""
    for curve in ("bn254", "bls12_381", "pallas"):
        r, t = api.SCALAR_FIELDS[curve], 12
        p = M2.Poseidon2(r, t, 8, 56, [r - 1] * (8 * t + 56), [r - 1] * t, capacity=r - 1, capacity_at=t - 1, out_at=t - 1)
        ctx = contexts(curve)
        with handle(ctx, p) as h:
            assert host(ctx.scalars_permute(h, dev([r - 1] * t + [0] * t))) == p.permute([r - 1] * t) + p.permute([0] * t), curve
            row = [r - 1] * (2 * (t - 1) + 1)
            assert host(ctx.scalars_hash(h, dev(row), len(row))) == [p.hash(row)], curve


def test_a_value_not_below_r_is_reported_and_the_next_call_is_correct(contexts):
    r, rnd = api.SCALAR_FIELDS["bn254"], rng(2100)
    p = M2.sample(r, 4)
    states = [[rnd.randrange(r) for _ in range(4)] for _ in range(65)]
    want = flat(p.permute(s) for s in states)
    ctx = contexts("bn254")
    with handle(ctx, p) as h:
        for bad in (r, (1 << 256) - 1):
            vals = flat(states)
            vals[-1] = bad  # an element of the last state
            with pytest.raises(api.MsmHipError) as e:
                ctx.scalars_permute(h, dev(vals))
            assert e.value.code == ERR_NONCANONICAL
            assert host(ctx.scalars_permute(h, dev(flat(states)))) == want
        with pytest.raises(api.MsmHipError) as e:
            ctx.scalars_hash(h, dev([1, 2, r]), 3)
        assert e.value.code == ERR_NONCANONICAL
        assert host(ctx.scalars_hash(h, dev([1, 2, 3]), 3)) == [p.hash([1, 2, 3])]


# ---- sponges ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", (3, 4))
def test_sponges_under_the_three_conventions(contexts, t):
    for curve in ("bn254", "bls12_381"):
        r, rnd = api.SCALAR_FIELDS[curve], rng(2200 + t)
        for k, length in enumerate((1, t - 1, t, 2 * (t - 1) + 1)):
            stride = length + 2
            rows = [[rnd.randrange(r) for _ in range(length)] for _ in range(5)]
            for c, convention in enumerate(((0, 0, 0), ((length << 64) % r, t - 1, 0), ((1 << (t - 1)) - 1, 0, 1))):
                mont = bool((k + c) & 1)
                p = M2.sample(r, t, capacity=convention[0], capacity_at=convention[1], out_at=convention[2])
                ctx = contexts(curve, mont)
                padded = flat(form(row, r, mont) + [r, (1 << 256) - 1] for row in rows)  # (the padding is not below r and must not be read)
                with handle(ctx, p) as h:
                    got = ctx.scalars_hash(h, dev(padded), length, batch=len(rows), stride=stride)
                    assert host(got) == form([p.hash(row) for row in rows], r, mont), (curve, t, length, convention)


# ---- trees ------------------------------------------------------------------------------------------------------------------------------------------
def test_trees_and_their_paths(contexts):
    r, rnd = api.SCALAR_FIELDS["bn254"], rng(2300)
    ctx = contexts("bn254")
    for t, n in ((3, 64), (4, 27)):
        p = M2.sample(r, t, capacity=(1 << (t - 1)) - 1, capacity_at=0, out_at=1)
        leaves = [rnd.randrange(r) for _ in range(n)]
        levels = p.merkle(leaves)
        with handle(ctx, p) as h:
            d_leaves = dev(leaves)
            nodes = ctx.merkle_tree(h, d_leaves)
            assert host(nodes) == flat(levels), (t, n)
            for index in (0, n // 2 + 1, n - 1):
                path = ctx.merkle_path(h, d_leaves, nodes, index)
                assert tuple(path.shape) == (len(levels), t - 2, 32)
                siblings = [host(row) for row in path]
                assert siblings == p.path(leaves, levels, index) and p.verify(leaves[index], index, siblings, levels[-1][0]), (t, index)  # rehashed in the model
            assert ctx.merkle_tree(h, M.to_bytes(leaves)) == M.to_bytes(flat(levels))  # the host form
    p = M2.sample(r, 2)
    with handle(ctx, p) as h:
        assert host(ctx.merkle_tree(h, dev([5]), levels=3)) == p.merkle_chain(5, 3)


# ---- against the existing Poseidon kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", (4, 12))
def test_without_internal_rounds_it_is_poseidon_with_the_dense_external_matrix(contexts, t):
    """With R_P = 0, Poseidon2 is the initial M_E and then R_F rounds of (constants, S-box, M_E): on x it gives what a Poseidon handle with
    mds = M_E as a dense matrix, R_P = 0 and the same constants gives on M_E x.  M_E x is formed on the host, from the matrix; the two
    permutations are compared device against device, and no model of either takes part."""
    for curve in ("bn254", "bls12_381"):
        r, rnd = api.SCALAR_FIELDS[curve], rng(2400 + t)
        rf = 8
        rc = [rnd.randrange(r) for _ in range(rf * t)]
        m_e = M2.external_matrix(t)
        states = [[r - 1] * t] + [[rnd.randrange(r) for _ in range(t)] for _ in range(64)]
        moved = [[sum(c * x for c, x in zip(row, s)) % r for row in m_e] for s in states]
        ctx = contexts(curve)
        with ctx.poseidon2(t, rf, 0, rc, [rnd.randrange(r) for _ in range(t)]) as new, ctx.poseidon(t, rf, 0, round_constants=rc, mds=m_e) as old:
            assert (new.kind, old.kind) == ("poseidon2", "poseidon")
            a, b = ctx.scalars_permute(new, dev(flat(states))), ctx.scalars_permute(old, dev(flat(moved)))
            assert torch.equal(a, b) and raw(a) != raw(dev(flat(states))), (curve, t)


# ---- two kinds of handle at once --------------------------------------------------------------------------------------------------------------------
def test_a_poseidon_and_a_poseidon2_handle_alive_together(contexts):
    """the two tables are of different lengths behind the same head; each handle keeps its own and is first used while the other is alive"""
    r, rnd = api.SCALAR_FIELDS["bn254"], rng(2500)
    ctx = contexts("bn254")
    for t in (3, 8):
        old_model, new_model = M.standard(r, t, 8, 56), M2.sample(r, t, 8, 56)
        states = [[rnd.randrange(r) for _ in range(t)] for _ in range(9)]
        want_old, want_new = flat(old_model.permute(s) for s in states), flat(new_model.permute(s) for s in states)
        row = states[0] + states[1]
        with ctx.poseidon(t, 8, 56) as old, handle(ctx, new_model) as new:
            for _ in range(2):
                assert host(ctx.scalars_permute(new, dev(flat(states)))) == want_new, t
                assert host(ctx.scalars_permute(old, dev(flat(states)))) == want_old, t
                assert host(ctx.scalars_hash(old, dev(row), len(row))) == [old_model.hash(row)]
                assert host(ctx.scalars_hash(new, dev(row), len(row))) == [new_model.hash(row)]
