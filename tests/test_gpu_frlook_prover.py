"""MsmContext.logup on the device: the columns of a logUp argument over a 256-entry table and 2 rows of 1024 looked-up values, with a fixed beta
that meets no pole -- the two sums agree with each other and with the model (tests/frlook_model.py), h_f and h_t are the model's, m is what
scalars_multiplicities gives; a column with one foreign value raises with its index; and on BN254 the commitment to m is the MSM of the counts
as 4-byte scalars.

logup runs on BN254, BLS12-381 and Grumpkin.  On Grumpkin, whose scalar field the vector library has no unit for, MsmContext.logup takes the
same columns from scalars_gate and scalars_mle_eval (scalars.py: _logup_without_frvec); the test asks the same bytes of it."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frlook_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
N_T, ROWS, N = 256, 2, 1024
BETA = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211122334455667788
CASES = [("bn254", False), ("bn254", True), ("bls12_381", False), ("grumpkin", False), ("grumpkin", True)]
IDS = ["%s-%s" % (c, "mont256" if f else "canonical") for c, f in CASES]


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
    api.frlook_release()
    api.frvec_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def witness(r, seed):
    """a table of 256 different values and 2 rows of 1024 of them, a fifth of the table never looked up, a tenth of the elements one value
    (padding); beta meets no pole"""
    rnd = rng(seed)
    table = [rnd.randrange(r) for _ in range(N_T)]
    used = table[:N_T - N_T // 5]
    rows = [[used[0] if rnd.randrange(10) == 0 else used[rnd.randrange(len(used))] for _ in range(N)] for _ in range(ROWS)]
    beta = BETA % r
    assert len(set(table)) == N_T and all((beta + v) % r for v in table)
    return table, rows, beta


@pytest.mark.parametrize("curve,mont", CASES, ids=IDS)
def test_logup_columns_and_totals(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    table, rows, beta = witness(r, 990)
    want_m, want_hf, want_ht, want_sf, want_st = M.logup(table, rows, beta, r)
    assert want_sf == want_st and sum(want_m) == ROWS * N
    t_dev, f_dev = dev(form(table, r, mont)), dev(form(rows[0] + rows[1], r, mont))
    kept_t, kept_f = t_dev.clone(), f_dev.clone()
    got_m, h_f, h_t, sum_f, sum_t = ctx.logup(t_dev, f_dev, beta, batch=ROWS)
    assert torch.equal(t_dev, kept_t) and torch.equal(f_dev, kept_f)  # the inputs are left untouched
    assert sum_f == sum_t and M.from_bytes(sum_f) == form([want_sf], r, mont)
    assert tuple(got_m.shape) == (N_T, 32) and host(got_m) == form(want_m, r, mont)
    assert tuple(h_f.shape) == (N, 32) and host(h_f) == form(want_hf, r, mont)
    assert tuple(h_t.shape) == (N_T, 32) and host(h_t) == form(want_ht, r, mont)
    with ctx.lookup_table(t_dev) as look:  # m is what scalars_multiplicities gives; a table made once serves again
        assert torch.equal(ctx.scalars_multiplicities(look, f_dev, batch=ROWS), got_m)
        again = ctx.logup(t_dev, f_dev, beta, batch=ROWS, lookup=look)
        assert torch.equal(again[0], got_m) and torch.equal(again[1], h_f) and torch.equal(again[2], h_t) and again[3:] == (sum_f, sum_t)
        assert look._h  # (not closed by logup)


@pytest.mark.parametrize("curve,mont", CASES, ids=IDS)
def test_multiplicities_and_a_foreign_value(contexts, curve, mont):
    """the lookup itself on every case's field: m against the model, and a strict call on a column with one foreign value"""
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    table, rows, beta = witness(r, 991)
    counts = M.lookup(table, rows)[0]
    with ctx.lookup_table(dev(form(table, r, mont))) as look:
        assert (look.n, look.distinct) == (N_T, N_T)
        assert host(ctx.scalars_multiplicities(look, dev(form(rows[0] + rows[1], r, mont)), batch=ROWS)) == form(counts, r, mont)
        at = N + 517
        foreign = next(v for v in range(2, r) if v not in set(table))
        rows[1][517] = foreign
        with pytest.raises(ValueError, match=r"1 looked-up values are not in the table; the first is element %d \(row 1, position 517\)" % at):
            ctx.scalars_multiplicities(look, dev(form(rows[0] + rows[1], r, mont)), batch=ROWS)
        with pytest.raises(ValueError, match=r"the first is element %d " % at):
            ctx.logup(dev(form(table, r, mont)), dev(form(rows[0] + rows[1], r, mont)), beta, batch=ROWS, lookup=look)


def test_the_commitment_to_m_is_the_msm_of_the_counts(contexts):
    ctx = contexts("bn254", False)
    r = api.SCALAR_FIELDS["bn254"]
    table, rows, _ = witness(r, 992)
    ctx.set_bases(ctx.sample_points(N_T, 43))
    with ctx.lookup_table(dev(table)) as look:
        got_m, counts = ctx.scalars_multiplicities(look, dev(rows[0] + rows[1]), batch=ROWS, counts=True)
    wide = ctx.msm(got_m)
    ctx.set_scalar_format(width=4)
    try:
        narrow = ctx.msm(counts)
    finally:
        ctx.set_scalar_format()
    assert wide == narrow and not wide.is_identity()
