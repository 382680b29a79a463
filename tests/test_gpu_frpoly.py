"""Polynomial opening over the scalar field on the device (include/msm_frpoly.h; MsmContext.scalars_eval .. scalars_powers) against the
pure-Python model (tests/frpoly_model.py: plain Horner), byte for byte: evaluation and division by X - z around a lane's four elements, one tile
(T = 1024) and two tiles, over two and three levels under the tile hook and at 2^20 + 1 at the design's tile, in place and out of place, over
rows; the dot product with its own and a shared second operand; the combination of 1 .. 256 rows; the powers of 0, 1, r - 1, a root of unity and a
random base; both data forms, the four fields and a G2 context; the rejection of a value >= r; ordering behind torch's stream; the host forms."""
import ctypes as C

import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frpoly_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
T = 1024  # csrc/frpoly_kernels.h: FRPOLY_TILE
ERR_NONCANONICAL, ERR_INVALID_ARG = -4, -2
R = api.SCALAR_FIELDS["bn254"]
FIELDS = ("bn254", "pallas", "vesta", "bls12_381")
SIZES = (1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 1)


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
    api.frpoly_test_tile(0)
    for c in made.values():
        c.close()
    api.frpoly_release()


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


def points(r, seed):
    return (0, 1, r - 1, rng(seed).randrange(2, r - 1))


def _check_eval_and_divide(ctx, r, a, batch, mont, what, zs=None):
    """eval, divide into `out` (the input stays), divide in place; the last coefficient of every quotient is 0 and the values are eval's"""
    n = len(a) // batch
    stored = form(a, r, mont)
    src = dev(stored)
    for z in zs or points(r, 200 + n):
        want = [M.divide(row, z, r) for row in M.rows_of(a, batch)]
        want_q = M.to_bytes(form([x for q, _ in want for x in q], r, mont))
        want_v = M.to_bytes(form([v for _, v in want], r, mont))
        assert ctx.scalars_eval(src, z, batch=batch) == want_v, what + (z, "eval")
        out = torch.full_like(src, 0xEE)
        got, values = ctx.scalars_divide(src, z, batch=batch, out=out, values=True)
        assert got is out and raw(out) == want_q and values == want_v and host(src) == stored, what + (z, "divide into out")
        assert all(v == 0 for v in host(out)[n - 1::n])
        t = src.clone()
        assert ctx.scalars_divide(t, z, batch=batch) is t and raw(t) == want_q, what + (z, "divide in place")


# ---- eval and divide ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_eval_and_divide(contexts, curve, mont):
    ctx = contexts(curve, mont)
    api.frpoly_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for n in SIZES:
        _check_eval_and_divide(ctx, r, planted(r, n, 210 + n), 1, mont, (curve, mont, n))
        ctx.scalars_eval(dev(form([1] * n, r, mont)), 1)
        assert api.frpoly_last() == ((1, 1) if n <= T else (2, 2)), n
        ctx.scalars_divide(dev(form([1] * n, r, mont)), 1)
        assert api.frpoly_last() == ((1, 1) if n <= T else (3, 2)), n  # the tiles' folds, the top level's scan, the tiles' scans


def test_the_edges_of_a_division(contexts):
    """z = 0 is a shift; one coefficient gives [0] and the coefficient; all 0, all r - 1, a single nonzero in the last place"""
    ctx = contexts()
    a = planted(R, 2 * T + 1, 220)
    got, values = ctx.scalars_divide(dev(a), 0, values=True)
    assert host(got) == a[1:] + [0] and M.from_bytes(values) == [a[0]]
    got, values = ctx.scalars_divide(dev([R - 5]), R - 1, values=True)
    assert host(got) == [0] and M.from_bytes(values) == [R - 5]
    n = T + 3
    last = [0] * n
    last[n - 1] = R - 2
    for a in ([0] * n, [R - 1] * n, last):
        _check_eval_and_divide(ctx, R, a, 1, False, ("edges",))


@pytest.mark.parametrize("tile,n,levels", [(2, 7, 3), (4, 16, 2), (4, 17, 3), (6, 41, 3), (8, 73, 3)])
def test_two_and_three_levels_under_the_tile_hook(contexts, tile, n, levels):
    ctx = contexts()
    api.frpoly_test_tile(tile)
    try:
        a = planted(R, 2 * n, 230 + n)
        _check_eval_and_divide(ctx, R, a, 2, False, (tile, n))
        assert api.frpoly_last() == (2 * levels - 1, levels)
        ctx.scalars_eval(dev(a), 3, batch=2)
        assert api.frpoly_last() == (levels, levels)
        _check_eval_and_divide(contexts("bn254", True), R, a, 2, True, (tile, n, "mont256"))
        contexts("bn254", False)
        b = planted(R, 2 * n, 231 + n)
        assert M.from_bytes(ctx.scalars_dot(dev(a), dev(b), batch=2)) == [M.dot(x, y, R) for x, y in zip(M.rows_of(a, 2), M.rows_of(b, 2))]
        assert api.frpoly_last() == (levels, levels)
        assert M.from_bytes(ctx.scalars_dot(dev(a), dev(b[:n]), batch=2)) == [M.dot(x, b[:n], R) for x in M.rows_of(a, 2)]
    finally:
        api.frpoly_test_tile(0)


@pytest.mark.parametrize("batch,n", [(3, T + 1), (1000, 1), (7, 3)])
def test_rows(contexts, batch, n):
    ctx = contexts()
    api.frpoly_test_tile(0)
    a = planted(R, batch * n, 240 + n)
    _check_eval_and_divide(ctx, R, a, batch, False, (batch, n), zs=(R - 1, rng(241).randrange(R)))
    with pytest.raises(ValueError):
        ctx.scalars_eval(dev(a), 1, batch=batch + 1 if (batch * n) % (batch + 1) else batch * n + 1)


def test_a_long_vector(contexts):
    """three levels at the design's tile: 2^20 + 1 coefficients, the whole quotient against Python's Horner"""
    ctx = contexts()
    api.frpoly_test_tile(0)
    n = (1 << 20) + 1
    rnd = rng(250)
    blob = bytearray(rnd.randbytes(32 * n))
    blob[31::32] = bytes(n)  # (248-bit values: below r)
    blob[-32:] = (R - 1).to_bytes(32, "little")
    a = M.from_bytes(bytes(blob))
    z = rnd.randrange(2, R)
    src = torch.frombuffer(blob, dtype=torch.uint8).reshape(-1, 32).cuda()
    want, value = M.divide(a, z, R)
    assert ctx.scalars_eval(src, z) == M.to_bytes([value]) and api.frpoly_last() == (3, 3)
    got, values = ctx.scalars_divide(src, z, values=True)
    assert api.frpoly_last() == (5, 3) and values == M.to_bytes([value])
    assert raw(got) == M.to_bytes(want)


# ---- dot ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_dot(contexts, curve, mont):
    ctx = contexts(curve, mont)
    api.frpoly_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for n in (1, T + 1, 2 * T + 1):
        for batch in (1, 3):
            a, b = planted(r, batch * n, 260 + n), planted(r, batch * n, 261 + n)[::-1]
            da, db = dev(form(a, r, mont)), dev(form(b, r, mont))
            want = [M.dot(x, y, r) for x, y in zip(M.rows_of(a, batch), M.rows_of(b, batch))]
            assert ctx.scalars_dot(da, db, batch=batch) == M.to_bytes(form(want, r, mont)), (curve, mont, n, batch, "per row")
            assert api.frpoly_last() == ((1, 1) if n <= T else (2, 2))
            shared = [M.dot(x, b[:n], r) for x in M.rows_of(a, batch)]
            assert ctx.scalars_dot(da, dev(form(b[:n], r, mont)), batch=batch) == M.to_bytes(form(shared, r, mont)), (curve, mont, n, batch, "shared")
            assert host(da) == form(a, r, mont) and host(db) == form(b, r, mont)
        top = dev(form([r - 1] * n, r, mont))  # all r - 1: the largest products
        assert ctx.scalars_dot(top, top) == M.to_bytes(form([n % r], r, mont)), (curve, mont, n)


# ---- combine -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_combine(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    n = T + 1
    rnd = rng(270)
    for batch in (1, 2, 17, 256) if curve == "bn254" else (2, 17):
        a = planted(r, batch * n, 271 + batch)
        rows = M.rows_of(a, batch)
        coeffs = [rnd.randrange(r) for _ in range(batch)]
        coeffs[0] = r - 1
        if batch > 2:
            coeffs[1], coeffs[2] = 0, 1
        want = M.to_bytes(form(M.combine(rows, coeffs, r), r, mont))
        src = dev(form(a, r, mont))
        out = ctx.scalars_combine(src, coeffs)
        assert tuple(out.shape) == (n, 32) and raw(out) == want and host(src) == form(a, r, mont), (curve, mont, batch)
        given = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
        assert ctx.scalars_combine(src, [c.to_bytes(32, "little") for c in coeffs], out=given) is given and raw(given) == want
        first = src[:n]  # in place on row 0: the other rows stay
        assert ctx.scalars_combine(src, coeffs, out=first) is first and raw(src[:n]) == want and host(src[n:]) == form(a[n:], r, mont), (curve, mont, batch, "in place")
        assert api.frpoly_last() == (1, 1)
    assert raw(ctx.scalars_combine(dev(form([r - 1] * (2 * n), r, mont)), [r - 1, r - 1])) == M.to_bytes(form([2] * n, r, mont))


# ---- powers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_powers(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    rnd = rng(280)
    root = api.root_of_unity(curve, 10)
    assert pow(root, 512, r) == r - 1
    for g in (0, 1, r - 1, root, rnd.randrange(2, r)):
        for n in (1, 5, T + 1):
            for scale in (1, rnd.randrange(2, r)) + ((0, r - 1) if n == 5 else ()):
                got = ctx.scalars_powers(g, n, scale=scale)
                assert tuple(got.shape) == (n, 32) and raw(got) == M.to_bytes(form(M.powers(g, n, r, scale), r, mont)), (curve, mont, g, n, scale)
        n = (1 << 20) + 3  # five windows of the lane's number: sampled, with the ends
        scale = rnd.randrange(2, r)
        got = ctx.scalars_powers(g.to_bytes(32, "little"), n, scale=scale, out=torch.zeros(n, 32, dtype=torch.uint8, device="cuda"))
        at = sorted({0, 1, 2, 3, 4, 63, 64, 4 * 4096 - 1, 4 * 4096, 4 * 65536 + 1, n - 4, n - 3, n - 2, n - 1} | {rnd.randrange(n) for _ in range(50)})
        picked = got[torch.tensor(at, device="cuda")]
        assert host(picked) == form([scale * pow(g, i, r) % r for i in at], r, mont), (curve, mont, g)
    assert api.frpoly_last() == (1, 1)
    assert host(ctx.scalars_powers(0, 6, scale=9)) == form([9, 0, 0, 0, 0, 0], r, mont)


# ---- errors, ordering, host forms, another group -----------------------------------------------------------------------------------------------
def test_a_value_not_below_r_is_refused_and_the_next_call_succeeds(contexts):
    ctx = contexts()
    n = T + 5
    a = planted(R, n, 290)
    good = dev(a)
    for bad in (R, (1 << 256) - 1):
        b = list(a)
        b[n - 3] = bad
        calls = [lambda: ctx.scalars_eval(dev(b), 3), lambda: ctx.scalars_divide(dev(b), 3), lambda: ctx.scalars_divide(dev(b[n - 8:]), 3), lambda: ctx.scalars_dot(dev(b), good),
                 lambda: ctx.scalars_dot(good, dev(b)), lambda: ctx.scalars_combine(dev(a + b), [1, 2]), lambda: ctx.scalars_eval(M.to_bytes(b), 3)]
        for k, call in enumerate(calls):
            with pytest.raises(m.MsmHipError) as e:
                call()
            assert e.value.code == ERR_NONCANONICAL, k
            assert ctx.scalars_eval(good, 3) == M.to_bytes([M.evaluate(a, 3, R)]), k


def test_a_tensor_with_pending_work_on_a_torch_stream(contexts):
    ctx = contexts()
    n = 1 << 12
    a = planted(R, n, 300)
    src = dev(a)
    big = torch.ones(1 << 24, device="cuda")
    t = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
    for _ in range(8):  # work that is still running on torch's stream when the call is made ...
        big = big * 1.0001 + 1.0
    t.copy_(src, non_blocking=True)  # ... and behind it the data the call reads
    assert ctx.scalars_eval(t, 5) == M.to_bytes([M.evaluate(a, 5, R)])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        u = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
        for _ in range(8):
            big = big * 1.0001 + 1.0
        u.copy_(src, non_blocking=True)
        got = ctx.scalars_divide(u, 7)
    assert host(got) == M.divide(a, 7, R)[0]


def test_host_forms(contexts):
    for mont in (False, True):
        ctx = contexts("bn254", mont)
        n = T + 2
        a, b = planted(R, 2 * n, 310), planted(R, 2 * n, 311)
        fa, fb = M.to_bytes(form(a, R, mont)), M.to_bytes(form(b, R, mont))
        want = [M.divide(row, 11, R) for row in M.rows_of(a, 2)]
        assert ctx.scalars_eval(fa, 11, batch=2) == M.to_bytes(form([v for _, v in want], R, mont))
        got, values = ctx.scalars_divide(fa, 11, batch=2, values=True)
        assert got == M.to_bytes(form([x for q, _ in want for x in q], R, mont)) and values == M.to_bytes(form([v for _, v in want], R, mont))
        assert ctx.scalars_dot(fa, fb, batch=2) == M.to_bytes(form([M.dot(x, y, R) for x, y in zip(M.rows_of(a, 2), M.rows_of(b, 2))], R, mont))
        assert ctx.scalars_dot(fa, fb[:32 * n], batch=2) == M.to_bytes(form([M.dot(x, b[:n], R) for x in M.rows_of(a, 2)], R, mont))
        assert ctx.scalars_combine(fa, [5, R - 6]) == M.to_bytes(form(M.combine(M.rows_of(a, 2), [5, R - 6], R), R, mont))
        L, out = api.frpoly_lib(), bytearray(32 * 7)
        raw_out = (C.c_char * len(out)).from_buffer(out)
        assert L.msm_frpoly_powers(0, 0, C.cast(raw_out, C.c_void_p), 7, (3).to_bytes(32, "little"), (2).to_bytes(32, "little"), 2 if mont else 0) == 0
        assert M.from_bytes(bytes(out)) == form(M.powers(3, 7, R, 2), R, mont)
    contexts("bn254", False)
    api.frpoly_release()  # scratch, constants and staging gone, and back with the next call
    assert ctx.scalars_eval(M.to_bytes([2, 3]), 5) == M.to_bytes([17])


def test_a_g2_context_takes_the_field_of_its_g1(contexts):
    ctx = contexts("bn254_g2")
    a = planted(R, 65, 320)
    z = 0x1234567890ABCDEF
    got, values = ctx.scalars_divide(dev(a), z.to_bytes(32, "little"), values=True)
    assert (host(got), M.from_bytes(values)[0]) == M.divide(a, z, R)
    assert host(ctx.scalars_powers(z, 9)) == M.powers(z, 9, R)


def test_grumpkin_and_bad_shapes_are_refused(contexts):
    with pytest.raises(ValueError):
        contexts("grumpkin").scalars_eval(dev([1, 2]), 1)
    ctx = contexts()
    t = dev([1, 2, 3, 4])
    one = (1).to_bytes(32, "little")
    L = api.frpoly_lib()
    assert L.msm_frpoly_divide_device(1, 0, None, t.data_ptr(), t.data_ptr(), 4, 1, one, 0, None) == ERR_INVALID_ARG
    assert L.msm_frpoly_divide_device(0, 0, None, t.data_ptr() + 32, t.data_ptr(), 3, 1, one, 0, None) == ERR_INVALID_ARG  # a partial overlap
    assert L.msm_frpoly_combine_device(0, 0, None, t.data_ptr() + 64, t.data_ptr(), 2, 2, one * 2, 0) == ERR_INVALID_ARG  # (row 1 as the output)
    assert host(t) == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        ctx.scalars_dot(t, dev([1, 2, 3]))
    with pytest.raises(ValueError):
        ctx.scalars_divide(t, 1, out=torch.zeros(3, 32, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        ctx.scalars_dot(t, bytes(32 * 4))  # a host vector beside a device vector
    before = torch.cuda.current_device()
    assert ctx.scalars_eval(t, 2) == M.to_bytes([1 + 4 + 12 + 32])
    assert torch.cuda.current_device() == before and host(t) == [1, 2, 3, 4]
