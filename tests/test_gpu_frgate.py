"""Constraint evaluation on the device (include/msm_frgate.h; MsmContext.scalars_gate) against the pure-Python model (tests/frgate_model.py), byte
for byte: below a workgroup, at one and past several (n = 1 .. 4096), rotations 0, +-1, +-3 and beyond n that wrap from the first elements to the
last and back, steps 1, 4 and n, rows with a stride beyond n, rows 0 and 31 of 32, degrees 1 and 8, a row repeated with different rotations, 1, 32,
33 and 64 terms (the lane's sum is tidied every 32), coefficients and planted data 0, 1 and r - 1, no scale and scales of 1, 4 and n elements,
ACCUMULATE onto planted values; an output pre-filled with 0xFF whose neighbours stay untouched; the same bytes on a second run; both data forms,
the five fields and a G2 context; ordering behind torch's stream; the host form; and the rejection of a value >= r where, and only where, an
element is read."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frgate_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
ERR_NONCANONICAL = -4
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
SIZES = (1, 2, 4, 64, 512, 1024, 2048, 4096)


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
    api.frgate_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def host(t):
    return M.from_bytes(raw(t))


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def planted(r, n, seed):
    """random values with the edge values 0, 1 and r - 1 planted where the length allows; the first is 1 and the last r - 1 (what a wrap reads)"""
    rnd = rng(seed)
    v = [rnd.randrange(r) for _ in range(n)]
    for k, e in enumerate((r - 1, 0, 1)):
        if 2 * k + 1 < n:
            v[(7 * k + 1) % n] = e
    if n > 1:
        v[0] = 1
    v[n - 1] = r - 1
    return v


def strided(rows, stride, filler):
    return [x for row in rows for x in list(row) + [filler] * (stride - len(row))]


# ---- every size, field and form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_every_size_field_and_form(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    for n in SIZES:
        rnd = rng(700 + n)
        batch, stride = 3, n + 5
        rows = [planted(r, n, 701 + n + v) for v in range(batch)]
        src = dev(strided([form(row, r, mont) for row in rows], stride, r))  # (the gaps hold r: they are not read)
        before = raw(src)
        what = (curve, mont, n)
        # rotations 0, +-1, +-3 and one that wraps more than once; a row twice in a term with different rotations
        terms = [(rnd.randrange(r), (0, (1, 1), (0, -1))), (r - 1, ((2, 3), (1, -3))), (1, ((2, 2 * n + 1),)), (0, (1, 1))]
        # step 1, no scale, into the middle row of a buffer of 0xFF
        big = torch.full((3, n, 32), 0xFF, dtype=torch.uint8, device="cuda")
        middle = big[1]
        assert ctx.scalars_gate(src, terms, batch=batch, n=n, out=middle) is middle
        want = M.apply(rows, terms, n, 1, None, None, r)
        assert host(big[1]) == form(want, r, mont), what + ("step 1",)
        assert raw(big[0]) == b"\xff" * (32 * n) and raw(big[2]) == b"\xff" * (32 * n) and raw(src) == before, what
        again = ctx.scalars_gate(src, terms, batch=batch, n=n)
        assert tuple(again.shape) == (n, 32) and raw(again) == raw(big[1]), what + ("a second run",)
        # step 4 (n below 4: step n), a scale of as many elements, added onto planted values
        step = min(4, n)
        scale = [(r - 1, rnd.randrange(r), 0, 1)[j % 4] for j in range(step)]
        acc = planted(r, n, 750 + n)
        out = dev(form(acc, r, mont))
        assert ctx.scalars_gate(src, terms, batch=batch, n=n, step=step, scale=dev(form(scale, r, mont)), out=out, accumulate=True) is out
        assert host(out) == form(M.apply(rows, terms, n, step, scale, acc, r), r, mont), what + ("step 4, accumulate",)
        # step n (every rotation is the identity), scales of one and of n elements
        for scale in ([rnd.randrange(r)], planted(r, n, 760 + n)):
            got = ctx.scalars_gate(src, terms, batch=batch, n=n, step=n, scale=dev(form(scale, r, mont)))
            assert host(got) == form(M.apply(rows, terms, n, n, scale, None, r), r, mont), what + ("step n", len(scale))
        assert raw(src) == before


def test_a_g2_context_takes_its_g1s_field(contexts):
    for curve, g1 in (("bn254_g2", "bn254"), ("bls12_381_g2", "bls12_381")):
        r = api.SCALAR_FIELDS[g1]
        rows = [planted(r, 64, 770), planted(r, 64, 771)]
        terms = [(5, (0, (1, -1))), (r - 1, ((1, 3),))]
        want = M.apply(rows, terms, 64, 1, None, None, r)
        assert host(contexts(curve).scalars_gate(dev(rows[0] + rows[1]), terms, batch=2)) == want
        assert host(contexts(g1).scalars_gate(dev(rows[0] + rows[1]), terms, batch=2)) == want


# ---- degrees, terms, rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_degrees_terms_and_rows(contexts, curve):
    ctx = contexts(curve)
    r, rnd = api.SCALAR_FIELDS[curve], rng(780)
    n, batch, stride = 64, 32, 80
    rows = [planted(r, n, 781 + v) for v in range(batch)]
    src = dev(strided(rows, stride, r))
    row = lambda: rnd.randrange(batch)  # noqa: E731
    rot = lambda: rnd.choice((0, 1, -1, 3, -3, 17, -40))  # noqa: E731
    kinds = {
        "degree 1": [(rnd.randrange(r), (row(),))],
        "degree 8": [(rnd.randrange(r), tuple((row(), rot()) for _ in range(8)))],
        "rows 0 and 31": [(1, (0, (31, 1))), (r - 1, ((31, -1), 0, 31))],
        "a row eight times with different rotations": [(1, tuple((5, j - 4) for j in range(8)))],
        "coefficients 0, 1, r - 1": [(0, (row(), row())), (1, ((row(), rot()),)), (r - 1, ((row(), rot()), (row(), rot())))],
    }
    for count in (1, 32, 33, 64):  # (the lane's sum is tidied after every 32 terms)
        kinds["%d terms" % count] = [((1, r - 1, rnd.randrange(r), 0)[j % 4], tuple((row(), rot()) for _ in range(1 + j % 8))) for j in range(count)]
    scale = [rnd.randrange(r) for _ in range(4)]
    ds = dev(scale)
    for name, terms in kinds.items():
        for step in (1, 4):
            got = ctx.scalars_gate(src, terms, batch=batch, n=n, step=step)
            assert host(got) == M.apply(rows, terms, n, step, None, None, r), (curve, name, step)
        got = ctx.scalars_gate(src, terms, batch=batch, n=n, step=4, scale=ds)
        assert host(got) == M.apply(rows, terms, n, 4, scale, None, r), (curve, name, "scale")
    # several workgroups: 33 terms, the rotations wrapping from the first workgroup to the last and back
    n = 2048
    rows = [planted(r, n, 790 + v) for v in range(4)]
    terms = [((1, r - 1, rnd.randrange(r))[j % 3], ((j % 4, (1, -1, 3, -3, 0)[j % 5]), ((j + 1) % 4, -(j % 7)))[:1 + j % 2]) for j in range(33)]
    got = ctx.scalars_gate(dev(strided(rows, n, 0)), terms, batch=4, step=4)
    assert host(got) == M.apply(rows, terms, n, 4, None, None, r), (curve, "2048 x 33 terms")


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS)
def test_the_values_that_reach_the_bounds(contexts, curve, mont):
    """64 terms of degree 8 with every STORED element, coefficient and scale r - 1, accumulated onto r - 1: the lane's sum at its largest before each
    tidy (every element sees the same values: the model computes one)"""
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    n = 512
    top = (M.mont([r - 1], r, back=True) if mont else [r - 1])[0]  # the plain value whose stored form is r - 1
    src = dev([r - 1] * (2 * n))
    for count in (32, 33, 64):
        terms = [(r - 1, tuple((j % 2, j - 3) for j in range(8)))] * count
        out = dev([r - 1] * n)
        ctx.scalars_gate(src, terms, batch=2, scale=dev([r - 1]), out=out, accumulate=True)
        want = M.apply([[top], [top]], terms, 1, 1, [top], [top], r)
        assert host(out) == form(want, r, mont) * n, (curve, mont, count)
        got = ctx.scalars_gate(src, terms, batch=2)
        assert host(got) == form(M.apply([[top], [top]], terms, 1, 1, None, None, r), r, mont) * n, (curve, mont, count)


# ---- ordering, the host form -----------------------------------------------------------------------------------------------------------------------
def test_input_written_by_a_torch_op_immediately_before_the_call(contexts):
    ctx = contexts()
    r = api.SCALAR_FIELDS["bn254"]
    n = 4096
    rows = [planted(r, n, 800), planted(r, n, 801)]
    staged = dev(rows[0] + rows[1])
    terms = [(3, (0, (1, 1))), (r - 1, ((0, -1),))]
    want = M.apply(rows, terms, n, 1, None, None, r)
    for _ in range(3):
        src = torch.zeros_like(staged)
        filler = torch.ones((1 << 22,), dtype=torch.float32, device="cuda")
        filler.mul_(2.0)  # (work ahead of the copy on torch's stream)
        src.copy_(staged)
        assert host(ctx.scalars_gate(src, terms, batch=2)) == want


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
def test_the_host_form(contexts, mont):
    ctx = contexts("pallas", mont)
    r, rnd = api.SCALAR_FIELDS["pallas"], rng(810)
    n, batch, stride = 512, 2, 515
    rows = [planted(r, n, 811), planted(r, n, 812)]
    flat = M.to_bytes(strided([form(row, r, mont) for row in rows], stride, r))  # (the gaps hold r: they are not read)
    terms = [(rnd.randrange(r), (0, (1, -3), (0, 1))), (1, ((1, 600),))]
    got = ctx.scalars_gate(flat, terms, batch=batch, n=n, step=4)
    assert isinstance(got, bytes) and M.from_bytes(got) == form(M.apply(rows, terms, n, 4, None, None, r), r, mont)
    scale, acc = [rnd.randrange(r) for _ in range(4)], planted(r, n, 813)
    got = ctx.scalars_gate(flat, terms, batch=batch, n=n, scale=M.to_bytes(form(scale, r, mont)), out=M.to_bytes(form(acc, r, mont)), accumulate=True)
    assert M.from_bytes(got) == form(M.apply(rows, terms, n, 1, scale, acc, r), r, mont)
    with pytest.raises(TypeError):  # a device scale with host rows
        ctx.scalars_gate(flat, terms, batch=batch, n=n, scale=dev(scale))


def test_an_output_that_overlaps_an_input_raises(contexts):
    ctx = contexts()
    buf = dev([1] * 256)
    terms = [(1, (0, (1, 1)))]
    for out in (buf[:64], buf[64:128], buf[100:164]):  # the rows themselves, in whole or in part
        with pytest.raises(ValueError):
            ctx.scalars_gate(buf[:128], terms, batch=2, out=out)
    with pytest.raises(ValueError):  # the gap behind n belongs to the rows too
        ctx.scalars_gate(buf, terms, batch=2, n=64, out=buf[64:128])
    scale = dev([1] * 64)
    with pytest.raises(ValueError):
        ctx.scalars_gate(buf[:128], terms, batch=2, scale=scale, out=scale)
    assert host(ctx.scalars_gate(buf[:128], terms, batch=2, out=buf[128:192])) == [1] * 64  # right behind the rows: apart


# ---- a value >= r is reported where, and only where, it is read --------------------------------------------------------------------------------------
def test_noncanonical_where_and_only_where_an_element_is_read(contexts):
    ctx = contexts()
    r = api.SCALAR_FIELDS["bn254"]
    n, stride = 1024, 1030
    rows = [[3] * n, [4] * n, [5] * n]
    terms = [(1, (0, (2, 1)))]  # row 1 is not named
    want = M.apply(rows, terms, n, 1, None, None, r)

    def run(rows=rows, filler=1, scale=None, acc=None):
        src = dev(strided(rows, stride, filler))
        out = dev(acc) if acc is not None else torch.full((n, 32), 0xFF, dtype=torch.uint8, device="cuda")  # (0xFF..FF is not below r)
        return host(ctx.scalars_gate(src, terms, batch=3, n=n, scale=dev(scale) if scale is not None else None, out=out, accumulate=acc is not None))

    def refused(**kw):
        with pytest.raises(m.MsmHipError) as e:
            run(**kw)
        return e.value.code == ERR_NONCANONICAL

    assert run() == want  # (out, full of 0xFF, is not read without ACCUMULATE)
    for bad in (r, (1 << 256) - 1):
        assert run(filler=bad) == want  # behind n: not read
        for at in (0, 700, n - 1):
            poisoned = lambda v: [row if k != v else row[:at] + [bad] + row[at + 1:] for k, row in enumerate(rows)]  # noqa: E731
            assert run(rows=poisoned(1)) == want  # an unnamed row: not read
            assert refused(rows=poisoned(0)) and refused(rows=poisoned(2))
            assert refused(scale=[1] * (at % 4) + [bad] + [1] * (3 - at % 4))
            assert refused(acc=[2] * at + [bad] + [2] * (n - 1 - at))
            assert run() == want  # (the next call is unaffected)
    assert run(acc=[2] * n) == [(v + 2) % r for v in want]
