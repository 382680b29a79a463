"""Vector arithmetic over the scalar field on the device (include/msm_frvec.h; MsmContext.scalars_add .. scalars_scan) against the pure-Python
model (tests/frvec_model.py), byte for byte: the five maps with vector and constant operands, in place on every operand and out of place; the batch
inverse and the four scans below and around one wave and one tile (T = 1024), over two and three levels of totals under the tile hook, over rows
that end inside a tile; zeros, r - 1, both data forms, the four fields and a G2 context; the rejection of a value >= r; ordering behind torch's
stream; the host forms."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frvec_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
T = 1024  # csrc/frvec_kernels.h: FRVEC_TILE
ERR_NONCANONICAL, ERR_INVALID_ARG = -4, -2
R = api.SCALAR_FIELDS["bn254"]
FIELDS = ("bn254", "pallas", "vesta", "bls12_381")
SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)


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
    api.frvec_test_tile(0)
    for c in made.values():
        c.close()
    api.frvec_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def host(t):
    return M.from_bytes(raw(t))


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def nonzero(vals, fill=2):
    """the same values with every zero replaced (a zero would hide every product behind it)"""
    return [v if v else fill for v in vals]


def planted(r, n, seed):
    """random values with the edge values 0, 1 and r - 1 planted where the length allows"""
    rnd = rng(seed)
    v = [rnd.randrange(r) for _ in range(n)]
    for k, e in enumerate((r - 1, 0, 1)):
        if 2 * k + 1 < n:
            v[(7 * k + 1) % n] = e
    v[n - 1] = r - 1
    return v


# ---- map ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_every_map(contexts, curve, mont):
    """every op at every size, b and c as vectors and as constants, out of place and in place on a, on b and on c"""
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    rnd = rng(40)
    for n in (1, 2, 63, 64, 65, 257, 4099):
        a, b, c = planted(r, n, 41 + n), planted(r, n, 42 + n)[::-1], planted(r, n, 43 + n)
        if n > 2:
            b[1], c[1] = r - 1, r - 1  # (r - 1) (r - 1) + (r - 1): the largest operands together
        da, db, dc = (dev(form(v, r, mont)) for v in (a, b, c))
        for op in M.MAPS:
            three = op in ("mul_add", "mul_sub")
            method = getattr(ctx, "scalars_" + op)
            edges = (0, 1) if n == 65 else ()  # (the constants 0 and 1 are met at one size)
            for bk in (b, r - 1, rnd.randrange(r)) + edges:
                for ck in ((c, rnd.randrange(r)) + edges[:1] if three else (None,)):
                    want = M.to_bytes(form(M.map_op(op, a, bk, ck, r), r, mont))
                    operands = [db if bk is b else bk] + ([dc if ck is c else ck] if three else [])
                    what = (curve, mont, n, op, bk is b, ck is c)
                    out = torch.zeros_like(da)
                    assert method(da, *operands, out=out) is out and raw(out) == want and raw(da) == M.to_bytes(form(a, r, mont)), what  # out of place
                    t = da.clone()
                    assert method(t, *operands) is t and raw(t) == want, what + ("in place on a",)
                    for k, operand in enumerate(operands):
                        if isinstance(operand, torch.Tensor):
                            args = list(operands)
                            args[k] = operand.clone()
                            assert raw(method(da, *args, out=args[k])) == want, what + ("in place on operand", k)
            same = M.to_bytes(form(M.map_op(op, a, a, a if three else None, r), r, mont))  # one tensor in every place
            t = da.clone()
            assert raw(method(t, t, t) if three else method(t, t)) == same, (curve, mont, n, op, "a op a")


def test_map_constants_as_bytes_and_a_g2_context(contexts):
    ctx = contexts("bn254_g2")
    a = planted(R, 65, 50)
    k = 0x1234567890ABCDEF
    assert host(ctx.scalars_mul(dev(a), k.to_bytes(32, "little"))) == M.map_op("mul", a, k, None, R)
    assert host(ctx.scalars_mul_sub(dev(a), bytearray(k.to_bytes(32, "little")), 5)) == M.map_op("mul_sub", a, k, 5, R)


# ---- inverse -----------------------------------------------------------------------------------------------------------------------------------
def _sizes(curve):
    return SIZES if curve == "bn254" else (65, T + 1)


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_inverse(contexts, curve, mont):
    ctx = contexts(curve, mont)
    api.frvec_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for n in _sizes(curve):
        a = planted(r, n, 60 + n)
        want = M.to_bytes(form(M.inverse(a, r), r, mont))
        t = dev(form(a, r, mont))
        assert ctx.scalars_inverse(t) is t and raw(t) == want, (curve, n)
        assert api.frvec_last() == ((1, 1) if n <= T else (3, 2)), n  # one tile: one launch; more: the tiles' products, their inverses, the elements
        src, out = dev(form(a, r, mont)), torch.zeros_like(t)
        assert ctx.scalars_inverse(src, out=out) is out and raw(out) == want and host(src) == form(a, r, mont), (curve, n, "out of place")


def test_inverse_of_zeros(contexts):
    ctx = contexts()
    for n in (1, 65, T + 1):
        assert host(ctx.scalars_inverse(dev([0] * n))) == [0] * n
    n = 2 * T + 3  # a zero on each side of every tile boundary: the neighbours are inverted all the same
    a = planted(R, n, 70)
    for k in (0, T - 1, T, 2 * T - 1, 2 * T, n - 1):
        a[k] = 0
    assert host(ctx.scalars_inverse(dev(a))) == M.inverse(a, R)


# ---- scan --------------------------------------------------------------------------------------------------------------------------------------
def _check_scans(ctx, r, a, batch, mont, what):
    src = dev(form(a, r, mont))
    for op in ("sum", "product"):
        for exclusive in (False, True):
            want, want_totals = M.scan(a, op, exclusive, r, batch)
            t = src.clone()
            got, totals = ctx.scalars_scan(t, op=op, exclusive=exclusive, batch=batch, totals=True)
            assert got is t and raw(t) == M.to_bytes(form(want, r, mont)), what + (op, exclusive)
            assert totals == M.to_bytes(form(want_totals, r, mont)), what + (op, exclusive, "totals")


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_scans(contexts, curve, mont):
    ctx = contexts(curve, mont)
    api.frvec_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for n in _sizes(curve):
        a = nonzero(planted(r, n, 80 + n))  # (test_a_zero_in_a_product_scan has the zero)
        _check_scans(ctx, r, a, 1, mont, (curve, n))
        assert api.frvec_last() == ((1, 1) if n <= T else (3, 2)), n
    a = planted(r, 65, 81)
    out = torch.zeros(65, 32, dtype=torch.uint8, device="cuda")
    src = dev(form(a, r, mont))
    assert ctx.scalars_scan(src, op="sum", out=out) is out and host(out) == form(M.scan(a, "sum", False, r)[0], r, mont) and host(src) == form(a, r, mont)


@pytest.mark.parametrize("tile,n,levels", [(2, 2 * 2 + 2 + 1, 3), (4, 4 * 4 + 4 + 1, 3), (8, 8 * 8 + 8 + 1, 3), (6, 41, 3), (4, 16, 2), (4, 17, 3)])
def test_a_second_level_of_totals_under_the_tile_hook(contexts, tile, n, levels):
    ctx = contexts()
    api.frvec_test_tile(tile)
    try:
        a = nonzero(planted(R, 2 * n, 90 + n), 3)
        _check_scans(ctx, R, a, 2, False, (tile, n))
        assert api.frvec_last() == (2 * levels - 1, levels)
        _check_scans(contexts("bn254", True), R, a, 2, True, (tile, n, "mont256"))
        contexts("bn254", False)
        b = planted(R, n, 91 + n)  # the inverse on the same small tiles: zeros stay where they are
        assert host(ctx.scalars_inverse(dev(b))) == M.inverse(b, R) and api.frvec_last() == (2 * levels - 1, levels)
        assert host(ctx.scalars_inverse(dev([0] * n))) == [0] * n  # (every product is 1)
    finally:
        api.frvec_test_tile(0)


@pytest.mark.parametrize("batch,n", [(3, T + 1), (1000, 1), (7, 3)])
def test_rows(contexts, batch, n):
    ctx = contexts()
    api.frvec_test_tile(0)
    a = nonzero(planted(R, batch * n, 100 + n), 7)
    _check_scans(ctx, R, a, batch, False, (batch, n))
    with pytest.raises(ValueError):
        ctx.scalars_scan(dev(a), batch=batch + 1 if (batch * n) % (batch + 1) else batch * n + 1)


def test_a_zero_in_a_product_scan(contexts):
    """everything behind the zero is zero, and the next row is not touched by it"""
    ctx = contexts()
    n = T + 40
    a = nonzero(planted(R, 2 * n, 110), 9)
    a[n // 2] = 0
    got, totals = ctx.scalars_scan(dev(a), op="product", batch=2, totals=True)
    got = host(got)
    want, want_totals = M.scan(a, "product", False, R, 2)
    assert got == want and M.from_bytes(totals) == want_totals
    assert all(v != 0 for v in got[:n // 2]) and got[n // 2:n] == [0] * (n - n // 2) and all(v != 0 for v in got[n:]) and want_totals[0] == 0 != want_totals[1]


def test_sums_of_rows_of_r_minus_one(contexts):
    ctx = contexts()
    n = T + 3
    a = [R - 1] * (2 * n)
    got, totals = ctx.scalars_scan(dev(a), op="sum", batch=2, totals=True)
    assert host(got) == [(R - 1) * (i + 1) % R for i in range(n)] * 2 and M.from_bytes(totals) == [(R - 1) * n % R] * 2


def test_a_long_vector(contexts):
    ctx = contexts()
    api.frvec_test_tile(0)
    n = (1 << 16) + 1
    a = nonzero(planted(R, n, 120), 11)
    a[40000] = 0
    assert raw(ctx.scalars_inverse(dev(a))) == M.to_bytes(M.inverse(a, R))
    a[40000] = 13
    src = dev(a)
    got, totals = ctx.scalars_scan(src.clone(), op="product", exclusive=True, totals=True)
    want, want_totals = M.scan(a, "product", True, R)
    assert raw(got) == M.to_bytes(want) and totals == M.to_bytes(want_totals) and api.frvec_last() == (3, 2)
    assert raw(ctx.scalars_scan(src, op="sum")) == M.to_bytes(M.scan(a, "sum", False, R)[0])


# ---- errors, ordering, host forms --------------------------------------------------------------------------------------------------------------
def test_a_value_not_below_r_is_refused_and_the_next_call_succeeds(contexts):
    ctx = contexts()
    n = T + 5
    a = planted(R, n, 130)
    good = dev(a)
    for bad in (R, (1 << 256) - 1):
        b = list(a)
        b[n - 3] = bad
        calls = [lambda: ctx.scalars_add(dev(b), 1), lambda: ctx.scalars_mul(good.clone(), dev(b)), lambda: ctx.scalars_mul_add(good.clone(), 3, dev(b)),
                 lambda: ctx.scalars_inverse(dev(b)), lambda: ctx.scalars_scan(dev(b), op="sum"), lambda: ctx.scalars_scan(dev(b), op="product", exclusive=True),
                 lambda: ctx.scalars_inverse(M.to_bytes(b))]
        for k, call in enumerate(calls):
            with pytest.raises(m.MsmHipError) as e:
                call()
            assert e.value.code == ERR_NONCANONICAL, k
            assert host(ctx.scalars_inverse(good.clone())) == M.inverse(a, R), k


def test_a_tensor_with_pending_work_on_a_torch_stream(contexts):
    ctx = contexts()
    n = 1 << 12
    a = planted(R, n, 140)
    src = dev(a)
    big = torch.ones(1 << 24, device="cuda")
    t = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
    for _ in range(8):  # work that is still running on torch's stream when the call is made ...
        big = big * 1.0001 + 1.0
    t.copy_(src, non_blocking=True)  # ... and behind it the data the call reads
    got = ctx.scalars_mul_add(t, 3, 5)
    assert host(got) == M.map_op("mul_add", a, 3, 5, R)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        u = torch.zeros(n, 32, dtype=torch.uint8, device="cuda")
        for _ in range(8):
            big = big * 1.0001 + 1.0
        u.copy_(src, non_blocking=True)
        got = ctx.scalars_inverse(u)
    assert host(got) == M.inverse(a, R)


def test_host_forms(contexts):
    for mont in (False, True):
        ctx = contexts("bn254", mont)
        n = T + 2
        a, b = planted(R, n, 150), planted(R, n, 151)
        fa, fb = M.to_bytes(form(a, R, mont)), M.to_bytes(form(b, R, mont))
        assert ctx.scalars_mul_sub(fa, fb, 9) == M.to_bytes(form(M.map_op("mul_sub", a, b, 9, R), R, mont))
        assert ctx.scalars_add(fa, fb) == M.to_bytes(form(M.map_op("add", a, b, None, R), R, mont))
        assert ctx.scalars_inverse(fa) == M.to_bytes(form(M.inverse(a, R), R, mont))
        got, totals = ctx.scalars_scan(fa + fb, op="sum", exclusive=True, batch=2, totals=True)
        want, want_totals = M.scan(a + b, "sum", True, R, 2)
        assert got == M.to_bytes(form(want, R, mont)) and totals == M.to_bytes(form(want_totals, R, mont))
    contexts("bn254", False)
    api.frvec_release()  # scratch and staging gone, and back with the next call
    assert ctx.scalars_inverse(M.to_bytes([2])) == M.to_bytes([(R + 1) // 2])


def test_grumpkin_and_bad_shapes_are_refused(contexts):
    with pytest.raises(ValueError):
        contexts("grumpkin").scalars_inverse(dev([1, 2]))
    ctx = contexts()
    t = dev([1, 2, 3, 4])
    one = (1).to_bytes(32, "little")
    L = api.frvec_lib()
    assert L.msm_frvec_inverse_device(1, 0, None, t.data_ptr(), t.data_ptr(), 4, 0) == ERR_INVALID_ARG
    assert L.msm_frvec_map_device(0, 0, None, t.data_ptr() + 32, t.data_ptr(), None, None, 3, 0, one, None, 0) == ERR_INVALID_ARG  # a partial overlap
    assert host(t) == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        ctx.scalars_add(t, dev([1, 2, 3]))
    with pytest.raises(ValueError):
        ctx.scalars_add(t, t, out=torch.zeros(3, 32, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        ctx.scalars_add(t, bytes(32 * 4))  # a host vector beside a device vector
    before = torch.cuda.current_device()
    ctx.scalars_add(t, 1)
    assert torch.cuda.current_device() == before and host(t) == [2, 3, 4, 5]
