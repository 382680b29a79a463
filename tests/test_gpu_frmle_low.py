"""MSM_FRMLE_LOW_FIRST on the device (include/msm_frmle.h; msm-webgpu_amd/multilinear.py) against the pure-Python model by index bits
(tests/frmle_low_model.py), byte for byte: every call at n = 2, 4, 8, 64 on the five fields in both data forms with one and three rows a stride
beyond n apart; the fold apart and in place; the fused round from n = 4; two and three levels under the tile hook; n = 2^12 with two rows in
place, where the outputs of a launch span several workgroups and the scratch rows and their copy home are exercised; order="top" against the
context's own methods; the device against itself on the bit-reversed table; whole proofs; the rejection of a value >= r; ordering behind
torch's stream; the host forms; the launch counts the header documents."""
import ctypes as C

import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from msm_webgpu_amd import multilinear as ml
from tests import frmle_low_model as L
from tests.util import rng

pytestmark = pytest.mark.gpu
T = 1024  # csrc/frmle_kernels.h: FRMLE_TILE
ERR_NONCANONICAL = -4
R = api.SCALAR_FIELDS["bn254"]
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")


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
    api.frmle_test_tile(0)
    for c in made.values():
        c.close()
    api.frmle_release()


def dev(vals):
    return torch.frombuffer(bytearray(L.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def host(t):
    return L.from_bytes(raw(t))


def form(vals, r, mont):
    return L.mont(vals, r) if mont else list(vals)


def values_of(b, r, mont):
    return L.mont(L.from_bytes(b), r, back=True) if mont else L.from_bytes(b)


def planted(r, n, seed):
    """random values with 0, 1 and r - 1 planted where the length allows; the last one is r - 1"""
    rnd = rng(seed)
    v = [rnd.randrange(r) for _ in range(n)]
    for k, e in enumerate((r - 1, 0, 1)):
        if 2 * k + 1 < n:
            v[(7 * k + 1) % n] = e
    v[n - 1] = r - 1
    return v


def strided(rows, stride, filler):
    return [x for row in rows for x in list(row) + [filler] * (stride - len(row))]


def heads(t, batch, stride, width):
    """the first `width` scalars of every row"""
    return [host(t.reshape(batch, stride, 32)[v, :width]) for v in range(batch)]


def tails(t, batch, stride, n):
    """the scalars [n, stride) of every row"""
    return [host(t.reshape(batch, stride, 32)[v, n:]) for v in range(batch)] if stride > n else []


def levels(count, tile=T):
    k = 1
    while -(-count // tile) > 1:
        count, k = -(-count // tile), k + 1
    return k


def fused_shape(n, tile=T):
    """(launches, levels) of a low-first round with fold_by, as include/msm_frmle.h states them"""
    if n == 4:
        return 1, 1
    lv = 1 + levels(2 * -(-n // (4 * tile)), tile)
    return lv + 1, lv


# ---- every call at the small sizes, on every field, in both forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_every_call_at_the_small_sizes(contexts, curve, mont):
    ctx = contexts(curve, mont)
    api.frmle_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for n in (2, 4, 8, 64):
        for batch in (1, 3):
            k, stride = n.bit_length() - 1, n + 5
            rnd = rng(600 + n + batch)
            rows = [planted(r, n, 601 + n + j) for j in range(batch)]
            stored = form(strided(rows, stride, 9), r, mont)
            src = dev(stored)
            what = (curve, mont, n, batch)
            point = [rnd.randrange(r) for _ in range(k)]
            c = rnd.randrange(r)
            folded = [L.fold(row, c, r) for row in rows]
            assert values_of(ml.evaluate(ctx, src, point, batch=batch, n=n), r, mont) == [L.evaluate(row, point, r) for row in rows], what + ("eval",)
            assert api.frmle_last() == (levels(n), levels(n)) and host(src) == stored
            # the fold apart: n / 2 scalars of every row of out written, a only read
            out = torch.full_like(src, 0xEE)
            assert ml.fold(ctx, src, c, batch=batch, n=n, out=out) is out and host(src) == stored and api.frmle_last() == (1, 1)
            assert heads(out, batch, stride, n // 2) == [form(f, r, mont) for f in folded], what + ("fold apart",)
            assert raw(out.reshape(batch, stride, 32)[:, n // 2:]) == b"\xee" * (32 * batch * (stride - n // 2)), what + ("fold apart",)
            # the fold in place: the first n / 2 scalars; [n, stride) untouched; 1 launch at n = 2, 2 above
            t = src.clone()
            assert ml.fold(ctx, t, c, batch=batch, n=n) is t and api.frmle_last() == ((1, 1) if n == 2 else (2, 1))
            assert heads(t, batch, stride, n // 2) == [form(f, r, mont) for f in folded], what + ("fold in place",)
            assert tails(t, batch, stride, n) == tails(src, batch, stride, n)
            terms = [(rnd.randrange(r), (0, batch - 1, 0)), (r - 1, (batch - 1,))]
            assert values_of(ml.sumcheck_round(ctx, src, terms, batch=batch, n=n), r, mont) == L.round_values(rows, terms, r), what + ("round",)
            assert api.frmle_last() == (levels(n // 2), levels(n // 2)) and host(src) == stored
            if n >= 4:
                t = src.clone()
                got = ml.sumcheck_round(ctx, t, terms, batch=batch, n=n, fold=c)
                assert values_of(got, r, mont) == L.round_values(folded, terms, r), what + ("fused round",)
                assert api.frmle_last() == fused_shape(n)
                assert heads(t, batch, stride, n // 2) == [form(f, r, mont) for f in folded], what + ("fused fold",)
                assert tails(t, batch, stride, n) == tails(src, batch, stride, n)


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
def test_eq_and_evaluate_at_zero_one_and_five_variables(contexts, mont):
    for curve in FIELDS:
        ctx = contexts(curve, mont)
        r = api.SCALAR_FIELDS[curve]
        rnd = rng(620)
        for k in (0, 1, 5):
            n = 1 << k
            a = planted(r, n, 621 + k)
            point = [rnd.randrange(r) for _ in range(k)]
            scale = rnd.randrange(r)
            table = ml.eq(ctx, point, scale=scale)
            assert tuple(table.shape) == (n, 32) and host(table) == form(L.eq(point, r, scale), r, mont), (curve, k)
            assert values_of(ml.evaluate(ctx, dev(form(a, r, mont)), point), r, mont) == [L.evaluate(a, point, r)], (curve, k)
            assert values_of(ml.evaluate(ctx, table, point), r, mont) == [scale * sum(x * x for x in L.eq(point, r)) % r]
    ctx = contexts("bn254", False)
    bits = [1, 0, 1, 1, 0]  # the point of bits spells the index, bit 0 first
    hot = host(ml.eq(ctx, bits, scale=R - 1, out=torch.zeros(32, 32, dtype=torch.uint8, device="cuda")))
    assert hot[0b01101] == R - 1 and sum(1 for x in hot if x) == 1


# ---- levels, workgroups, the schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,n", [(2, 8), (4, 64), (8, 128)])
def test_two_and_three_levels_under_the_tile_hook(contexts, tile, n):
    api.frmle_test_tile(tile)
    try:
        for mont in (False, True):
            ctx = contexts("bn254", mont)
            rnd = rng(630 + n)
            rows = [planted(R, n, 631 + n + j) for j in range(3)]
            stride = n + 5
            src = dev(form(strided(rows, stride, 9), R, mont))
            before = host(src)
            point = [rnd.randrange(R) for _ in range(n.bit_length() - 1)]
            assert values_of(ml.evaluate(ctx, src, point, batch=3, n=n), R, mont) == [L.evaluate(row, point, R) for row in rows]
            assert api.frmle_last() == (levels(n, tile), levels(n, tile))
            terms = [(3, (0, 1, 2, 0)), (R - 1, (2, 2))]
            assert values_of(ml.sumcheck_round(ctx, src, terms, batch=3, n=n), R, mont) == L.round_values(rows, terms, R)
            assert api.frmle_last() == (levels(n // 2, tile), levels(n // 2, tile)) and levels(n // 2, tile) in (2, 3) and host(src) == before
            c = rnd.randrange(R)
            folded = [L.fold(row, c, R) for row in rows]
            assert values_of(ml.sumcheck_round(ctx, src, terms, batch=3, n=n, fold=c), R, mont) == L.round_values(folded, terms, R)
            assert api.frmle_last() == fused_shape(n, tile) and fused_shape(n, tile)[1] in (2, 3)
            assert heads(src, 3, stride, n // 2) == [form(f, R, mont) for f in folded]
            assert [x[n:] for x in (before[v * stride:(v + 1) * stride] for v in range(3))] == tails(src, 3, stride, n)
    finally:
        api.frmle_test_tile(0)
        contexts("bn254", False)


def test_in_place_where_the_outputs_span_several_workgroups(contexts):
    """n = 2^12, two rows: 2 x 1024 outputs to each launch of the fold (8 workgroups), the scratch rows of 1024 scalars and their copy home; the
    fused round's two launches of 512 pairs, a tile each"""
    ctx = contexts()
    api.frmle_test_tile(0)
    n = 1 << 12
    rows = [planted(R, n, 640), planted(R, n, 641)[::-1]]
    src = dev(rows[0] + rows[1])
    c = rng(642).randrange(R)
    folded = [L.fold(row, c, R) for row in rows]
    t = src.clone()
    ml.fold(ctx, t, c, batch=2)
    assert api.frmle_last() == (2, 1) and heads(t, 2, n, n // 2) == folded
    again = src.clone()
    ml.fold(ctx, again, c, batch=2)
    assert raw(again) == raw(t)  # (the unspecified halves too: the same bytes on every run)
    terms = [(5, (0, 1, 1)), (R - 3, (0,))]
    t = src.clone()
    assert L.from_bytes(ml.sumcheck_round(ctx, t, terms, batch=2, fold=c)) == L.round_values(folded, terms, R)
    assert api.frmle_last() == (3, 2) == fused_shape(n) and heads(t, 2, n, n // 2) == folded
    # the next round in the same buffer, n halved: what the first one left behind n / 2 is not read
    c2 = c + 1
    assert L.from_bytes(ml.sumcheck_round(ctx, t, terms, batch=2, n=n // 2, fold=c2)) == L.round_values([L.fold(f, c2, R) for f in folded], terms, R)


def test_order_top_is_the_contexts_own_method(contexts):
    for mont in (False, True):
        ctx = contexts("bn254", mont)
        n, stride = 64, 70
        rnd = rng(650)
        rows = [planted(R, n, 651 + j) for j in range(3)]
        src = dev(form(strided(rows, stride, 9), R, mont))
        point = [rnd.randrange(R) for _ in range(6)]
        c = rnd.randrange(R)
        terms = [(7, (0, 1, 2)), (R - 1, (1,))]
        assert ml.evaluate(ctx, src, point, batch=3, n=n, order="top") == ctx.scalars_mle_eval(src, point, batch=3, n=n)
        assert raw(ml.eq(ctx, point, scale=c, order="top")) == raw(ctx.scalars_eq(point, scale=c))
        assert raw(ml.fold(ctx, src.clone(), c, batch=3, n=n, order="top")) == raw(ctx.scalars_mle_fold(src.clone(), c, batch=3, n=n))
        assert api.frmle_last() == (1, 1)
        assert ml.sumcheck_round(ctx, src, terms, batch=3, n=n, order="top") == ctx.scalars_sumcheck_round(src, terms, batch=3, n=n)
        a, b = src.clone(), src.clone()
        assert ml.sumcheck_round(ctx, a, terms, batch=3, n=n, fold=c, order="top") == ctx.scalars_sumcheck_round(b, terms, batch=3, n=n, fold=c) and raw(a) == raw(b)
        a, b = dev(form(rows[0] + rows[1], R, mont)), dev(form(rows[0] + rows[1], R, mont))
        challenge = lambda j, values: (int.from_bytes(values[:32], "little") + j) % R  # noqa: E731
        assert ml.sumcheck_prove(ctx, a, terms[1:], 2, challenge, order="top") == ctx.sumcheck_prove(b, terms[1:], 2, challenge)
    contexts("bn254", False)


def test_low_first_is_top_first_on_the_bit_reversed_table_device_against_device(contexts):
    ctx = contexts()
    n = 256
    rows = [planted(R, n, 660 + j) for j in range(2)]
    low, top = dev(rows[0] + rows[1]), dev(L.bit_reversed(rows[0]) + L.bit_reversed(rows[1]))
    rnd = rng(662)
    point = [rnd.randrange(R) for _ in range(8)]
    c = rnd.randrange(R)
    terms = [(3, (0, 1, 0)), (R - 2, (1, 1))]
    assert ml.evaluate(ctx, low, point, batch=2) == ctx.scalars_mle_eval(top, point, batch=2)
    assert ml.sumcheck_round(ctx, low, terms, batch=2) == ctx.scalars_sumcheck_round(top, terms, batch=2)
    assert host(ml.eq(ctx, point)) == L.bit_reversed(host(ctx.scalars_eq(point)))
    a, b = low.clone(), top.clone()
    assert ml.sumcheck_round(ctx, a, terms, batch=2, fold=c) == ctx.scalars_sumcheck_round(b, terms, batch=2, fold=c)
    assert [L.bit_reversed(x) for x in heads(a, 2, n, n // 2)] == heads(b, 2, n, n // 2)
    a, b = low.clone(), top.clone()
    ml.fold(ctx, a, c, batch=2), ctx.scalars_mle_fold(b, c, batch=2)
    assert [L.bit_reversed(x) for x in heads(a, 2, n, n // 2)] == heads(b, 2, n, n // 2)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 11])
def test_a_whole_proof_against_the_models_transcript(contexts, k):
    mont = k % 2 == 0
    ctx = contexts("bn254", mont)
    n = 1 << k
    rnd = rng(670 + k)
    rows = [[rnd.randrange(R) for _ in range(n)] for _ in range(4)]
    terms = [(rnd.randrange(R), (0, 1, 2)), (R - 1, (3,))]  # degree 3 over four rows
    want = L.prove(rows, terms, lambda j, v: (v[0] + 3 * v[1] + 5 * v[3] + j) % R, R)
    t = dev(form([x for row in rows for x in row], R, mont))
    rounds, point, finals = ml.sumcheck_prove(ctx, t, terms, 4, lambda j, b: (lambda v: (v[0] + 3 * v[1] + 5 * v[3] + j) % R)(values_of(b, R, mont)))
    assert ([values_of(b, R, mont) for b in rounds], point, values_of(finals, R, mont)) == want
    contexts("bn254", False)


# ---- errors, ordering, host forms -------------------------------------------------------------------------------------------------------------------
def test_a_value_not_below_r_is_refused_and_the_next_call_succeeds(contexts):
    ctx = contexts()
    n = 2 * T
    a = planted(R, 2 * n, 680)
    good = dev(a)
    terms = [(1, (0, 1))]
    want = L.to_bytes(L.round_values([a[:n], a[n:]], terms, R))
    for bad, at in ((R, n + n - 3), ((1 << 256) - 1, n + 2)):  # (read by the in-place launch, and by the launch into scratch)
        b = list(a)
        b[at] = bad
        calls = [lambda: ml.fold(ctx, dev(b), 3, batch=2), lambda: ml.fold(ctx, dev(b), 3, batch=2, out=torch.zeros(2 * n, 32, dtype=torch.uint8, device="cuda")),
                 lambda: ml.evaluate(ctx, dev(b), [3] * 11, batch=2), lambda: ml.sumcheck_round(ctx, dev(b), terms, batch=2),
                 lambda: ml.sumcheck_round(ctx, dev(b), [(1, (0,))], batch=2, fold=5), lambda: ml.fold(ctx, L.to_bytes(b), 3, batch=2)]
        for j, call in enumerate(calls):
            with pytest.raises(m.MsmHipError) as e:
                call()
            assert e.value.code == ERR_NONCANONICAL, j
            assert ml.sumcheck_round(ctx, good, terms, batch=2) == want, j
        assert len(ml.sumcheck_round(ctx, dev(b), [(1, (0,))], batch=2)) == 64  # (row 1 is not read)


def test_a_tensor_with_pending_work_on_a_torch_stream(contexts):
    ctx = contexts()
    n = 1 << 12
    a = planted(R, n, 690)
    src = dev(a)
    big = torch.ones(1 << 24, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        u = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
        for _ in range(8):  # work that is still running on the stream when the call is made, and behind it the data the call reads
            big = big * 1.0001 + 1.0
        u.copy_(src, non_blocking=True)
        got = ml.fold(ctx, u, 7)
    assert host(got)[:n // 2] == L.fold(a, 7, R)
    t = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
    for _ in range(8):
        big = big * 1.0001 + 1.0
    t.copy_(src, non_blocking=True)
    assert L.from_bytes(ml.sumcheck_round(ctx, t, [(1, (0, 0))], fold=9)) == L.round_values([L.fold(a, 9, R)], [(1, (0, 0))], R)


def test_host_forms(contexts):
    for mont in (False, True):
        ctx = contexts("bn254", mont)
        n, stride = 2 * T, 2 * T + 3
        rows = [planted(R, n, 700), planted(R, n, 701)]
        fa = L.to_bytes(form(strided(rows, stride, 4), R, mont))
        point = [rng(702 + j).randrange(R) for j in range(11)]
        assert values_of(ml.evaluate(ctx, fa, point, batch=2, n=n), R, mont) == [L.evaluate(x, point, R) for x in rows]
        folded = [L.fold(x, point[0], R) for x in rows]

        def check(left):
            got = values_of(left, R, mont)
            assert [got[v * stride:v * stride + n // 2] for v in range(2)] == folded and [got[v * stride + n:(v + 1) * stride] for v in range(2)] == [[4] * 3] * 2

        check(ml.fold(ctx, fa, point[0], batch=2, n=n))
        terms = [(9, (0, 1, 1)), (R - 1, (0,))]
        assert values_of(ml.sumcheck_round(ctx, fa, terms, batch=2, n=n), R, mont) == L.round_values(rows, terms, R)
        values, left = ml.sumcheck_round(ctx, fa, terms, batch=2, n=n, fold=point[0])
        assert values_of(values, R, mont) == L.round_values(folded, terms, R)
        check(left)
        lib, out = api.frmle_lib(), bytearray(32 * 8)
        raw_out = (C.c_char * len(out)).from_buffer(out)
        assert lib.msm_frmle_eq(0, 0, C.cast(raw_out, C.c_void_p), 8, L.to_bytes(point[:3]), (2).to_bytes(32, "little"), 8 | (2 if mont else 0)) == 0
        assert L.from_bytes(bytes(out)) == form(L.eq(point[:3], R, 2), R, mont)
    contexts("bn254", False)
