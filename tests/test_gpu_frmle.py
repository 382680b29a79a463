"""The sumcheck over multilinear tables on the device (include/msm_frmle.h; MsmContext.scalars_mle_fold .. scalars_sumcheck_round) against the
pure-Python model (tests/frmle_model.py), byte for byte: fold, eval, eq and round around a lane's four elements, at one tile (T = 1024), at two
tiles and past them, over two and three levels under the tile hook with full and partial top tiles, rows with a stride beyond n, every degree,
repeated rows, eight terms over sixteen rows, the fused fold with the challenges 0, 1, r - 1 and a random one; both data forms, the five fields
and a G2 context; the rejection of a value >= r; ordering behind torch's stream; the host forms; and one three-level case at 2^21 checked
against closed forms, without a big-integer loop on the host."""
import ctypes as C

import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frmle_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
T = 1024  # csrc/frmle_kernels.h: FRMLE_TILE
ERR_NONCANONICAL, ERR_INVALID_ARG = -4, -2
R = api.SCALAR_FIELDS["bn254"]
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
SIZES = (1, 2, 4, 8, 512, 1024, 2048, 4096)


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
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def host(t):
    return M.from_bytes(raw(t))


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def planted(r, n, seed):
    """random values with the edge values 0, 1 and r - 1 planted where the length allows; the last one is r - 1"""
    rnd = rng(seed)
    v = [rnd.randrange(r) for _ in range(n)]
    for k, e in enumerate((r - 1, 0, 1)):
        if 2 * k + 1 < n:
            v[(7 * k + 1) % n] = e
    v[n - 1] = r - 1
    return v


def levels(n, tile=T):
    k = 1
    while -(-n // tile) > 1:
        n, k = -(-n // tile), k + 1
    return k


def strided(rows, stride, filler):
    return [x for row in rows for x in list(row) + [filler] * (stride - len(row))]


def values_of(b, r, mont):
    return M.mont(M.from_bytes(b), r, back=True) if mont else M.from_bytes(b)


# ---- every call at every size, field and form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_every_call_at_every_size(contexts, curve, mont):
    ctx = contexts(curve, mont)
    api.frmle_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for n in SIZES:
        k = n.bit_length() - 1
        rnd = rng(400 + n)
        rows = [planted(r, n, 401 + n), planted(r, n, 402 + n)[::-1]]
        stored = form(rows[0] + rows[1], r, mont)
        src = dev(stored)
        point = [rnd.randrange(r) for _ in range(k)]
        what = (curve, mont, n)
        assert ctx.scalars_mle_eval(src, point, batch=2) == M.to_bytes(form([M.evaluate(row, point, r) for row in rows], r, mont)), what + ("eval",)
        assert api.frmle_last() == (levels(n), levels(n)) and host(src) == stored
        scale = rnd.randrange(r)
        table = ctx.scalars_eq([z.to_bytes(32, "little") for z in point], scale=scale)
        assert tuple(table.shape) == (n, 32) and raw(table) == M.to_bytes(form(M.eq(point, r, scale), r, mont)), what + ("eq",)
        assert api.frmle_last() == (1, 1)
        if n < 2:
            continue
        c = rnd.randrange(r)
        folded = [M.fold(row, c, r) for row in rows]
        out = torch.full_like(src, 0xEE)
        assert ctx.scalars_mle_fold(src, c, batch=2, out=out) is out and host(src) == stored, what + ("fold into out",)
        got = host(out.reshape(2, n, 32)[:, :n // 2])
        assert got == form(folded[0] + folded[1], r, mont) and raw(out.reshape(2, n, 32)[:, n // 2:]) == b"\xee" * (32 * n), what + ("fold into out",)
        t = src.clone()
        assert ctx.scalars_mle_fold(t, c, batch=2) is t and api.frmle_last() == (1, 1)
        assert host(t) == form(folded[0] + rows[0][n // 2:] + folded[1] + rows[1][n // 2:], r, mont), what + ("fold in place",)
        terms = [(rnd.randrange(r), (0, 1, 0)), (r - 1, (1,))]
        want = M.round_values(rows, terms, r)
        assert ctx.scalars_sumcheck_round(src, terms, batch=2) == M.to_bytes(form(want, r, mont)), what + ("round",)
        assert api.frmle_last() == (levels(n // 2), levels(n // 2)) and host(src) == stored
        if n >= 4:
            t = src.clone()
            assert ctx.scalars_sumcheck_round(t, terms, batch=2, fold=c) == M.to_bytes(form(M.round_values(folded, terms, r), r, mont)), what + ("fused round",)
            assert api.frmle_last() == (levels(n // 4), levels(n // 4))
            assert host(t) == form(folded[0] + rows[0][n // 2:] + folded[1] + rows[1][n // 2:], r, mont), what + ("fused fold",)


@pytest.mark.parametrize("tile,n", [(2, 8), (4, 16), (4, 64), (8, 128)])
def test_two_and_three_levels_under_the_tile_hook(contexts, tile, n):
    """eval: levels of n, with a full (4, 16), (4, 64) and a partial (2, 8: always full; 8, 128: one variable) top tile; round: levels of n / 2"""
    api.frmle_test_tile(tile)
    try:
        for mont in (False, True):
            ctx = contexts("bn254", mont)
            k = n.bit_length() - 1
            rnd = rng(410 + n)
            rows = [planted(R, n, 411 + n + j) for j in range(3)]
            stride = n + 5
            src = dev(form(strided(rows, stride, 9), R, mont))
            before = host(src)
            point = [rnd.randrange(R) for _ in range(k)]
            assert values_of(ctx.scalars_mle_eval(src, point, batch=3, n=n), R, mont) == [M.evaluate(row, point, R) for row in rows]
            assert api.frmle_last() == (levels(n, tile), levels(n, tile)) and levels(n, tile) in (2, 3)
            terms = [(3, (0, 1, 2, 0)), (R - 1, (2, 2))]
            assert values_of(ctx.scalars_sumcheck_round(src, terms, batch=3, n=n), R, mont) == M.round_values(rows, terms, R)
            assert api.frmle_last() == (levels(n // 2, tile), levels(n // 2, tile)) and host(src) == before
            c = rnd.randrange(R)
            folded = [M.fold(row, c, R) for row in rows]
            assert values_of(ctx.scalars_sumcheck_round(src, terms, batch=3, n=n, fold=c), R, mont) == M.round_values(folded, terms, R)
            assert api.frmle_last() == (levels(n // 4, tile), levels(n // 4, tile))
            assert host(src) == form(strided([f + row[n // 2:] for f, row in zip(folded, rows)], stride, 9), R, mont)
            ctx.scalars_mle_fold(src, 1, batch=3, n=n)
            assert api.frmle_last() == (1, 1)
            ctx.scalars_eq(point)
            assert api.frmle_last() == (1, 1)
    finally:
        api.frmle_test_tile(0)
        contexts("bn254", False)


# ---- round ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
def test_round_terms_rows_and_challenges(contexts, mont):
    ctx = contexts("bn254", mont)
    api.frmle_test_tile(0)
    rnd = rng(420)
    n, batch, stride = 64, 16, 70
    rows = [planted(R, n, 421 + j) for j in range(batch)]
    stored = form(strided(rows, stride, 5), R, mont)
    src = dev(stored)
    row = lambda: rnd.randrange(batch)  # noqa: E731
    kinds = {"degree 1": [(rnd.randrange(R), (row(),))], "degree 2": [(1, (row(), row()))], "degree 3": [(R - 1, (row(), row(), row()))],
             "degree 4": [(rnd.randrange(R), (row(), row(), row(), row()))], "a row four times": [(7, (3, 3, 3, 3))], "a row twice": [(1, (15, 15))],
             "a zero coefficient": [(0, (1, 2, 3)), (1, (4,))], "eight terms over sixteen rows": [((1, R - 1, rnd.randrange(R), 0)[j % 4], (2 * j, 2 * j + 1, j)[:1 + j % 3]) for j in range(8)]}
    for name, terms in kinds.items():
        got = ctx.scalars_sumcheck_round(src, terms, batch=batch, n=n)
        assert len(got) == 32 * (M.degree(terms) + 1) and values_of(got, R, mont) == M.round_values(rows, terms, R), name
        assert host(src) == stored, name
        for c in (0, 1, R - 1, rnd.randrange(2, R - 1)):
            t = src.clone()
            folded = [M.fold(x, c, R) for x in rows]
            assert values_of(ctx.scalars_sumcheck_round(t, terms, batch=batch, n=n, fold=c), R, mont) == M.round_values(folded, terms, R), (name, c)
            # the folded halves; behind them, and between the rows, everything as it was
            assert host(t) == form(strided([f + x[n // 2:] for f, x in zip(folded, rows)], stride, 5), R, mont), (name, c)
    # the smallest tables: n = 2 without the fold, n = 4 with it
    two = [planted(R, 2, 430), planted(R, 2, 431)]
    terms = [(5, (0, 1)), (R - 2, (1,))]
    assert values_of(ctx.scalars_sumcheck_round(dev(form(two[0] + two[1], R, mont)), terms, batch=2), R, mont) == M.round_values(two, terms, R)
    four = [planted(R, 4, 432), planted(R, 4, 433)]
    t = dev(form(four[0] + four[1], R, mont))
    folded = [M.fold(x, 11, R) for x in four]
    assert values_of(ctx.scalars_sumcheck_round(t, terms, batch=2, fold=11), R, mont) == M.round_values(folded, terms, R)
    assert host(t) == form(folded[0] + four[0][2:] + folded[1] + four[1][2:], R, mont)
    with pytest.raises(ValueError):
        ctx.scalars_sumcheck_round(dev(two[0] + two[1]), terms, batch=2, fold=11)


def test_eq_scales_and_a_one_hot_table(contexts):
    for mont in (False, True):
        ctx = contexts("bn254", mont)
        rnd = rng(440)
        point = [rnd.randrange(R) for _ in range(7)]
        assert host(ctx.scalars_eq(point, scale=0)) == [0] * 128
        ones = ctx.scalars_eq(point, scale=1, out=torch.zeros(128, 32, dtype=torch.uint8, device="cuda"))
        assert host(ones) == form(M.eq(point, R), R, mont) and sum(M.eq(point, R)) % R == 1
        bits = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1]  # the point of bits spells the index, top bit first
        at = int("".join(str(b) for b in bits), 2)
        hot = host(ctx.scalars_eq(bits, scale=R - 1))
        assert hot[at] == form([R - 1], R, mont)[0] and sum(1 for x in hot if x) == 1
        assert host(ctx.scalars_eq([], scale=6)) == form([6], R, mont)
    contexts("bn254", False)


# ---- errors, ordering, host forms, another group ---------------------------------------------------------------------------------------------------
def test_a_value_not_below_r_is_refused_and_the_next_call_succeeds(contexts):
    ctx = contexts()
    n = 2 * T
    a = planted(R, 2 * n, 450)
    good = dev(a)
    terms = [(1, (0, 1))]
    want = M.to_bytes(M.round_values(M.rows_of(a, 2), terms, R))
    for bad in (R, (1 << 256) - 1):
        b = list(a)
        b[n + n - 3] = bad
        calls = [lambda: ctx.scalars_mle_fold(dev(b), 3, batch=2), lambda: ctx.scalars_mle_eval(dev(b), [3] * 11, batch=2), lambda: ctx.scalars_sumcheck_round(dev(b), terms, batch=2),
                 lambda: ctx.scalars_sumcheck_round(dev(b), [(1, (0,))], batch=2, fold=5), lambda: ctx.scalars_mle_eval(M.to_bytes(b), [3] * 11, batch=2)]
        for k, call in enumerate(calls):
            with pytest.raises(m.MsmHipError) as e:
                call()
            assert e.value.code == ERR_NONCANONICAL, k
            assert ctx.scalars_sumcheck_round(good, terms, batch=2) == want, k
        assert len(ctx.scalars_sumcheck_round(dev(b), [(1, (0,))], batch=2)) == 64  # (row 1 is not read)


def test_a_tensor_with_pending_work_on_a_torch_stream(contexts):
    ctx = contexts()
    n = 1 << 12
    a = planted(R, n, 460)
    point = [rng(461).randrange(R) for _ in range(12)]
    src = dev(a)
    big = torch.ones(1 << 24, device="cuda")
    t = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
    for _ in range(8):  # work that is still running on torch's stream when the call is made ...
        big = big * 1.0001 + 1.0
    t.copy_(src, non_blocking=True)  # ... and behind it the data the call reads
    assert ctx.scalars_mle_eval(t, point) == M.to_bytes([M.evaluate(a, point, R)])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        u = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
        for _ in range(8):
            big = big * 1.0001 + 1.0
        u.copy_(src, non_blocking=True)
        got = ctx.scalars_mle_fold(u, 7)
    assert host(got)[:n // 2] == M.fold(a, 7, R)


def test_host_forms(contexts):
    for mont in (False, True):
        ctx = contexts("bn254", mont)
        n, stride = 2 * T, 2 * T + 3
        rows = [planted(R, n, 470), planted(R, n, 471)]
        fa = M.to_bytes(form(strided(rows, stride, 4), R, mont))
        point = [rng(472 + j).randrange(R) for j in range(11)]
        assert ctx.scalars_mle_eval(fa, point, batch=2, n=n) == M.to_bytes(form([M.evaluate(x, point, R) for x in rows], R, mont))
        folded = [M.fold(x, point[0], R) for x in rows]
        after = M.to_bytes(form(strided([f + x[n // 2:] for f, x in zip(folded, rows)], stride, 4), R, mont))
        assert ctx.scalars_mle_fold(fa, point[0], batch=2, n=n) == after
        terms = [(9, (0, 1, 1)), (R - 1, (0,))]
        assert ctx.scalars_sumcheck_round(fa, terms, batch=2, n=n) == M.to_bytes(form(M.round_values(rows, terms, R), R, mont))
        values, left = ctx.scalars_sumcheck_round(fa, terms, batch=2, n=n, fold=point[0])
        assert values == M.to_bytes(form(M.round_values(folded, terms, R), R, mont)) and left == after
        L, out = api.frmle_lib(), bytearray(32 * 8)
        raw_out = (C.c_char * len(out)).from_buffer(out)
        assert L.msm_frmle_eq(0, 0, C.cast(raw_out, C.c_void_p), 8, M.to_bytes(point[:3]), (2).to_bytes(32, "little"), 2 if mont else 0) == 0
        assert M.from_bytes(bytes(out)) == form(M.eq(point[:3], R, 2), R, mont)
    ctx = contexts("bn254", False)
    api.frmle_release()  # scratch, constants and staging gone, and back with the next call
    assert ctx.scalars_mle_eval(M.to_bytes([2, 3]), [5]) == M.to_bytes([7])


def test_a_g2_context_takes_the_field_of_its_g1(contexts):
    ctx = contexts("bn254_g2")
    a = planted(R, 64, 480)
    point = [0x1234567890ABCDEF + j for j in range(6)]
    assert ctx.scalars_mle_eval(dev(a), point) == M.to_bytes([M.evaluate(a, point, R)])
    assert host(ctx.scalars_eq(point[:3])) == M.eq(point[:3], R)
    assert values_of(ctx.scalars_sumcheck_round(dev(a), [(1, (0, 0))]), R, False) == M.round_values([a], [(1, (0, 0))], R)


def test_bad_shapes_are_refused_and_the_device_is_left_alone(contexts):
    ctx = contexts()
    t = dev([1, 2, 3, 4, 5, 6, 7, 8])
    one = (1).to_bytes(32, "little")
    L = api.frmle_lib()
    assert L.msm_frmle_fold_device(0, 0, None, t.data_ptr() + 32, t.data_ptr(), 4, 1, 4, one, 0) == ERR_INVALID_ARG  # a partial overlap
    assert L.msm_frmle_fold_device(0, 0, None, t.data_ptr(), t.data_ptr(), 6, 1, 8, one, 0) == ERR_INVALID_ARG  # not a power of two
    assert L.msm_frmle_fold_device(7, 0, None, t.data_ptr(), t.data_ptr(), 8, 1, 8, one, 0) == ERR_INVALID_ARG
    assert host(t) == [1, 2, 3, 4, 5, 6, 7, 8]
    with pytest.raises(ValueError):
        ctx.scalars_mle_fold(t, 1, out=torch.zeros(4, 32, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ctx.scalars_mle_eval(t, [1, 2])
    before = torch.cuda.current_device()
    assert ctx.scalars_mle_eval(t, [1, 0, 1]) == M.to_bytes([6])  # (the point of bits 101 picks element 5)
    assert torch.cuda.current_device() == before and host(t) == [1, 2, 3, 4, 5, 6, 7, 8]


# ---- the design tile over three levels, against closed forms ---------------------------------------------------------------------------------------
def test_three_levels_at_the_design_tile_against_closed_forms(contexts):
    """eq(w) and eq(u) at n = 2^21, built on the device: eval(eq(w), u) = prod_j (w_j u_j + (1 - w_j)(1 - u_j)); the round values of eq(w) eq(u) are
    eq1(w_0, t) eq1(u_0, t) prod_{j >= 1} (..); after the fold by c the tails move on by one variable.  No loop over the table on the host."""
    ctx = contexts()
    api.frmle_test_tile(0)
    k = 21
    n = 1 << k
    rnd = rng(490)
    w, u = [rnd.randrange(R) for _ in range(k)], [rnd.randrange(R) for _ in range(k)]
    buf = torch.empty(2, n, 32, dtype=torch.uint8, device="cuda")
    ctx.scalars_eq(w, out=buf[0])
    ctx.scalars_eq(u, out=buf[1])
    assert api.frmle_last() == (1, 1)
    assert ctx.scalars_mle_eval(buf, u, batch=2) == M.to_bytes([M.eq_value(w, u, R), M.eq_value(u, u, R)]) and api.frmle_last() == (3, 3)
    at = torch.tensor(sorted({0, 1, 2, 3, 4, 63, 64, n // 2, n - 1} | {rnd.randrange(n) for _ in range(40)}), device="cuda")
    bit = lambda i, j: (i >> (k - 1 - j)) & 1  # noqa: E731
    for row, p in ((0, w), (1, u)):
        assert host(buf[row][at]) == [M.eq_value(p, [bit(int(i), j) for j in range(k)], R) for i in at.tolist()]
    terms = [(1, (0, 1))]
    tail = M.eq_value(w[1:], u[1:], R)
    assert M.from_bytes(ctx.scalars_sumcheck_round(buf, terms, batch=2)) == [M.eq1(w[0], t, R) * M.eq1(u[0], t, R) * tail % R for t in range(3)]
    assert api.frmle_last() == (2, 2)  # (2^20 pairs)
    c = rnd.randrange(R)
    head, tail = M.eq1(w[0], c, R) * M.eq1(u[0], c, R) % R, M.eq_value(w[2:], u[2:], R)
    assert M.from_bytes(ctx.scalars_sumcheck_round(buf, terms, batch=2, fold=c)) == [head * M.eq1(w[1], t, R) * M.eq1(u[1], t, R) * tail % R for t in range(3)]
    # the folded tables are eq1(w_0, c) eq(w_1 .., .) and the like: their value at the rest of u, over n / 2 elements
    assert ctx.scalars_mle_eval(buf, u[1:], batch=2, n=n // 2) == M.to_bytes([M.eq1(w[0], c, R) * tail * M.eq1(w[1], u[1], R) % R,
                                                                              M.eq1(u[0], c, R) * M.eq_value(u[1:], u[1:], R) % R])
