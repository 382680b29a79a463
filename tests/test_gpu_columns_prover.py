"""msm_webgpu_amd.columns on the device, as a prover uses it: halo2's permuted columns of a lookup into a table with repeated values on every
curve's scalar field and in both scalar forms -- the argument's four properties, checked on integers --, plookup's sorted vector, and halo2's
grand product, whose closing value is one exactly when the permutations hold."""
import pytest
import torch

from tests import frcol_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
N = 1025
CURVES = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")


def _dev(values):
    return torch.frombuffer(bytearray(M.to_bytes(values)), dtype=torch.uint8).cuda().view(-1, 32)


def _ints(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


@pytest.fixture(scope="module", params=[(c, m) for c in CURVES for m in (False, True)], ids=lambda p: "%s-%s" % (p[0], "mont256" if p[1] else "canonical"))
def field(request, built):
    """(context, columns, r, stored(v): the integers as the context's form stores them)"""
    import msm_webgpu_amd as m
    from msm_webgpu_amd import api, columns

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    curve, mont = request.param
    r = api.SCALAR_FIELDS[curve]
    c = m.MsmContext(0, curve)
    c.set_scalar_format(mont256=mont)
    yield c, columns, r, (lambda v: [x * (1 << 256) % r for x in v]) if mont else (lambda v: list(v))
    c.close()


def _table_and_column(r, rnd, n=N):
    """a table of n values of which a third repeat an earlier one, and a column of n of its values, skewed towards a few"""
    t = []
    for _ in range(n):
        t.append(t[rnd.randrange(len(t))] if t and rnd.random() < 0.33 else rnd.randrange(r))
    a = [t[rnd.randrange(n) if rnd.random() < 0.5 else rnd.randrange(12)] for _ in range(n)]
    return t, a


def test_lookup_columns_have_halo2s_properties(field):
    ctx, col, r, stored = field
    rnd = rng(121)
    t, a = _table_and_column(r, rnd)
    assert len(set(t)) < N
    dt, da = _dev(stored(t)), _dev(stored(a))
    a_perm, s_perm = col.lookup_columns(ctx, dt, da)
    got_a, got_s = _ints(a_perm), _ints(s_perm)
    assert M.halo2_holds(stored(a), stored(t), got_a, got_s)
    want_a, want_s, _ = M.pair(stored(t), M.lookup_counts(t, a))  # and the bytes are the definition's
    assert got_a == want_a and got_s == want_s
    assert _ints(dt) == stored(t) and _ints(da) == stored(a)  # the inputs are untouched
    with ctx.lookup_table(dt) as look:  # a lookup that is already there
        again = col.lookup_columns(ctx, dt, da, lookup=look)
    assert _ints(again[0]) == got_a and _ints(again[1]) == got_s
    have = set(stored(t))
    foreign = next(v for v in range(1, 1 << 20) if v not in have)
    spoiled = stored(a)
    spoiled[N // 2] = foreign
    with pytest.raises(ValueError):
        col.lookup_columns(ctx, dt, _dev(spoiled))
    with pytest.raises(ValueError):
        col.lookup_columns(ctx, dt, da[:-1])  # one length


def test_sorted_by_table_is_plookups_vector(field):
    ctx, col, r, stored = field
    rnd = rng(122)
    t = [rnd.randrange(r) for _ in range(300)]  # plookup's table holds distinct values
    f = [t[rnd.randrange(300) if rnd.random() < 0.5 else 7] for _ in range(2 * 513)]
    s = col.sorted_by_table(ctx, _dev(stored(t)), _dev(stored(f)), batch=2)
    assert s.shape == (2 * 513 + 300, 32) and M.plookup_holds(stored(f), stored(t), _ints(s))
    s = col.sorted_by_table(ctx, _dev(stored(t)), _dev(stored(f)), batch=2, n=100)
    assert M.plookup_holds(stored(f[:100] + f[513:613]), stored(t), _ints(s))
    with pytest.raises(ValueError):
        col.sorted_by_table(ctx, _dev(stored(t)), _dev(stored(f[:-1] + [(t[0] + 1) % r if (t[0] + 1) % r not in t else 0])))


# ---- an output that shares bytes with an input or with the other output: refused by name, before the C call, with nothing written --------------------
# (call, the operand that is the output, the operand it cuts, how: the output starts `shift` scalars behind the other's start)
CUTS = [(call, out, other, shift) for call, out, other in (("expand", "out", "t"), ("pair", "out[0]", "t"), ("pair", "out[1]", "t"), ("pair", "out[0]", "out[1]"),
                                                            ("gather", "out", "a")) for shift in (0, 1, -3)]


@pytest.fixture(scope="module")
def plain_context(built):
    import msm_webgpu_amd as m
    from msm_webgpu_amd import columns

    c = m.MsmContext(0, "bn254")
    yield c, columns
    c.close()


@pytest.mark.parametrize("call,out,other,shift", CUTS, ids=lambda v: str(v).replace(" ", ""))
def test_an_output_that_cuts_an_operand_is_refused_by_name(plain_context, call, out, other, shift):
    """n_t = 4.  The library refuses an overlap before it forms the sum of the counts: the message names the two operands and speaks neither
    of a sum nor of an index, every byte stays as it was, and a correct call right afterwards is right."""
    ctx, col = plain_context
    rnd = rng(124)
    values = [rnd.randrange(1 << 250) for _ in range(24)]
    buf = _dev(values)
    before = _ints(buf)
    t, apart_a, apart_s = buf[8:12], buf[16:20], buf[20:24]  # the input, and outputs that lie apart from it and from one another
    cut = buf[8 + shift:12 + shift]  # shares bytes with t: the same start, one scalar on, three scalars before
    counts = torch.tensor([2, 0, 1, 1], dtype=torch.int32, device="cuda")
    idx = torch.tensor([3, -1, 0, 3], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError) as e:
        if call == "expand":
            col.expand(ctx, t, counts, 4, out=cut)
        elif call == "gather":
            col.gather(ctx, t, idx, out=cut)
        elif other == "t":
            col.permuted_pair(ctx, t, counts, out=(cut, apart_s) if out == "out[0]" else (apart_a, cut))
        else:  # the two outputs cut one another, both apart from t
            col.permuted_pair(ctx, t, counts, out=(apart_a, buf[16 + shift:20 + shift]))
    said = str(e.value)
    assert "%s overlaps %s" % (out, other) in said and "add up to" not in said and "index" not in said, said
    assert _ints(buf) == before and counts.tolist() == [2, 0, 1, 1] and idx.tolist() == [3, -1, 0, 3]
    tv = values[8:12]
    if call == "expand":
        assert _ints(col.expand(ctx, t, counts, 4, out=apart_a)) == M.expand(tv, [2, 0, 1, 1])
    elif call == "gather":
        assert _ints(col.gather(ctx, t, idx, out=apart_a)) == M.gather(tv, [3, M.MISSING, 0, 3])[0]
    else:
        got = col.permuted_pair(ctx, t, counts, out=(apart_a, apart_s))
        assert (_ints(got[0]), _ints(got[1])) == M.pair(tv, [2, 0, 1, 1])[:2]
    assert _ints(buf[:16]) == before[:16]  # the correct call wrote its outputs and nothing else


def test_a_wrong_sum_and_a_bad_index_keep_their_messages(plain_context):
    """operands that lie apart: the sum the library reported is named, and so is the index"""
    ctx, col = plain_context
    t = _dev([5, 6, 7, 8])
    counts = torch.tensor([2, 0, 1, 2], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="add up to 5, not to the 4 outputs"):
        col.expand(ctx, t, counts, 4)
    with pytest.raises(ValueError, match="add up to 5, not to the 4 rows"):
        col.permuted_pair(ctx, t, counts)
    wrapped = torch.tensor([-0x80000000] * 4, dtype=torch.int32, device="cuda")  # four counts of 2^31: zero in 32 bits
    with pytest.raises(ValueError, match="add up to %d" % (1 << 33)):
        col.expand(ctx, t, wrapped, 4)
    with pytest.raises(ValueError, match="neither below the 4 scalars"):
        col.gather(ctx, t, torch.tensor([0, 4], dtype=torch.int32, device="cuda"))


def _one(ctx, r):
    return ((1 << 256) % r if ctx.scalar_mont256 else 1).to_bytes(32, "little")


def test_halo2_lookup_closes_at_one(field):
    ctx, col, r, stored = field
    rnd = rng(123)
    t, a = _table_and_column(r, rnd)
    beta, gamma = rnd.randrange(r), rnd.randrange(r)
    dt, da = _dev(stored(t)), _dev(stored(a))
    if ctx.curve == "grumpkin":  # the vector library has no unit for its scalar field: its own refusal
        with pytest.raises(ValueError, match="grumpkin"):
            col.halo2_lookup(ctx, dt, da, beta, gamma)
        return
    a_perm, s_perm, z, total = col.halo2_lookup(ctx, dt, da, beta, gamma)
    pa, ps, _ = M.pair(t, M.lookup_counts(t, a))
    assert _ints(a_perm) == stored(pa) and _ints(s_perm) == stored(ps)
    want_z, want_total = M.grand_product(a, t, pa, ps, beta, gamma, r)
    assert want_total == 1 and _ints(z) == stored(want_z) and total == _one(ctx, r)
    # one element of a_perm altered before the product (the chain of halo2_lookup, copied): the product does not close
    spoiled = a_perm.clone()
    spoiled[N // 3] = _dev(stored([(pa[N // 3] + 1) % r]))[0]
    num = ctx.scalars_mul(ctx.scalars_add(da.clone(), beta), ctx.scalars_add(dt.clone(), gamma))
    den = ctx.scalars_mul(ctx.scalars_add(spoiled, beta), ctx.scalars_add(s_perm.clone(), gamma))
    _, bad = ctx.scalars_scan(ctx.scalars_mul(num, ctx.scalars_inverse(den)), op="product", exclusive=True, totals=True)
    assert bad != _one(ctx, r)
