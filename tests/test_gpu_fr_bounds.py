"""The inputs that reach the lazy bounds of the scalar-field kernels, on the device.  Every kernel header of csrc/ntt_kernels.h, frvec_kernels.h,
frpoly_kernels.h, frmle_kernels.h and frmat_kernels.h states how far a lazy 9 x 29-bit value (csrc/fq29.h) may grow before the next product or
fq_tidy, names the input pattern that reaches that bound, and has the host program run it under g++ -DFQ_CHECK.  That run multiplies with the
portable loop of fq_mul; the device multiplies through the generated csrc/fq29_asm.h, which no FQ_CHECK run executes.  These tests run the same
patterns through the shipped multiplier, on every field each library is built for and in both data forms, byte for byte against the pure-Python
models (tests/ntt_model.py, frvec_model.py, frpoly_model.py, frmle_model.py, frmat_model.py) or a closed form.  docs/launch_matrix.md, "Values
that reach the kernels' bounds", lists the bounds and the test of each; tests/test_gpu_frgate.py and tests/test_gpu_frhash.py hold the gate
kernel's and Poseidon's.

A kernel sees the STORED words.  In the mont256 form a plain r - 1 is stored as (r - 1) 2^256 mod r, which is no extreme of anything, so every
mont256 case runs twice: on the plain pattern (what the host tests build) and on the plain value whose stored form is r - 1 (`top`).

The time of a test is the Python model's, not the device's: each case but the two at 2^19 is well under a second (their own figures are in their
docstring)."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frmat_model as MAT
from tests import frmle_model as MLE
from tests import frpoly_model as POLY
from tests import frvec_model as VEC
from tests import ntt_model as NTT
from tests.test_frmle_host import _tables as mle_tables
from tests.test_ntt_host import _inputs as ntt_inputs
from tests.util import rng

pytestmark = pytest.mark.gpu
T = 1024  # FRVEC_TILE, FRPOLY_TILE, FRMLE_TILE (pairs for the round), FRMAT_TILE, and 2^NTT_PASS_BITS
FOUR = ("bn254", "pallas", "vesta", "bls12_381")  # libmsm_fr, libmsm_frvec, libmsm_frpoly
FIVE = FOUR + ("grumpkin",)  # libmsm_frmle, libmsm_frmat
FORMS = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])


@pytest.fixture(scope="module")
def contexts(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(curve, mont=False):
        if curve not in made:
            made[curve] = m.MsmContext(0, curve)
        made[curve].set_scalar_format(mont256=mont)
        return made[curve]

    yield get
    api.fr_test_pass_bits(0)
    for c in made.values():
        c.close()
    api.fr_release()
    api.frvec_release()
    api.frpoly_release()
    api.frmle_release()
    api.frmat_release()


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def dev(vals):
    return torch.frombuffer(bytearray(to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def form(vals, r, mont):
    """plain values -> the stored ones"""
    return VEC.mont(vals, r) if mont else list(vals)


def tops(r, mont):
    """the plain values to run a pattern of r - 1 with: r - 1, and in the mont256 form also the value that is STORED as r - 1"""
    return (r - 1, VEC.mont([r - 1], r, back=True)[0]) if mont else (r - 1,)


# ---- 1. the NTT: ten levels and a product ------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("curve", FOUR)
def test_ntt_ten_levels_and_a_product(contexts, curve, mont):
    """csrc/ntt_kernels.h:21-25: a tile value gains at most 3r per level, so it is below 32r after ten levels, and the product that follows takes
    32 r * r of the field's FQ_HEADROOM r^2 (BLS12-381: 70).  One tile of 2^10 at the design pass width is the only one-pass shape with ten levels.
    The inputs of tests/test_ntt_host.py::test_a_full_tile_keeps_its_bounds (random, all r - 1, all 0, a delta of 1 at the last index, r - 1 at
    index 0) and r - 1 alternating with 0.  Forward without a factor (the store's fq_mul(x, fq_one())), forward on a coset (the pre table on the
    way in), inverse with 1 / n (the post table's high level alone) and inverse with the shift (both levels).  The transform is linear and the
    kernel does not know the form: the mont256 case is the same code on other words, a 2^256 mod r, as in the host test."""
    ctx = contexts(curve, mont)
    api.fr_test_pass_bits(0)
    r, rnd = api.SCALAR_FIELDS[curve], rng(2000)
    n = T
    w = api.root_of_unity(curve, 10)
    g = rnd.randrange(2, r)
    inputs = ntt_inputs(r, n, rnd)
    inputs["r - 1 and 0"] = [r - 1, 0] * (n // 2)
    assert inputs["all r - 1"] == [r - 1] * n and inputs["delta"] == [0] * (n - 1) + [1]
    for name, a in inputs.items():
        runs = (("forward", dict(), NTT.ntt(a, w, r)), ("coset", dict(shift=g), NTT.ntt(a, w, r, pre=g)),
                ("inverse", dict(inverse=True), NTT.intt(a, w, r)), ("inverse, shift", dict(inverse=True, shift=g), NTT.intt(a, w, r, shift=g)))
        for what, kw, want in runs:
            t = dev(form(a, r, mont))
            assert ctx.scalars_fft(t, **kw) is t and api.fr_last() == (1, 10)
            assert raw(t) == to_bytes(form(want, r, mont)), (curve, mont, name, what)


# ---- 2. the NTT: the first size with a ten-level strided pass ---------------------------------------------------------------------------------------
def _functional(a, out, w, rho, r):
    """-> (sum_i rho^i out[i], (rho^n - 1) sum_j a[j] / (rho w^j - 1)) mod r: equal where out[i] = sum_j a[j] w^(i j), since then sum_i rho^i out[i] =
    sum_j a[j] sum_i (rho w^j)^i.  Horner on the left; on the right one running power, one batch inversion (three products an element) and one
    product by a[j].  Every rho w^j - 1 must be invertible: asserted."""
    n = len(a)
    left = 0
    for x in reversed(out):
        left = (left * rho + x) % r
    d, x = [0] * n, rho
    for j in range(n):
        d[j] = x - 1
        x = x * w % r
    prefix, p = [1] * n, 1
    for j in range(n):  # prefix[j] = d[0] .. d[j - 1]
        prefix[j] = p
        p = p * d[j] % r
    assert p != 0, "rho w^j = 1 for some j"
    inv, total = pow(p, r - 2, r), 0
    for j in range(n - 1, -1, -1):  # inv = 1 / (d[0] .. d[j])
        total += a[j] * (inv * prefix[j] % r)
        inv = inv * d[j] % r
    return left, (pow(rho, n, r) - 1) * total % r


def test_the_functional_finds_one_wrong_element():
    """the identity of _functional on the CPU at 2^8 against the model, and that it does not hold with one output off by one (no GPU is used;
    the mark is the module's)"""
    r, rnd = api.SCALAR_FIELDS["bls12_381"], rng(2090)
    n = 256
    w = api.root_of_unity("bls12_381", 8)
    a = [rnd.randrange(r) for _ in range(n)]
    out = NTT.ntt(a, w, r)
    rho = rnd.randrange(2, r)
    left, right = _functional(a, out, w, rho, r)
    assert left == right
    out[n - 3] = (out[n - 3] + 1) % r
    left, right = _functional(a, out, w, rho, r)
    assert left != right


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_ntt_first_size_with_a_ten_level_strided_pass(contexts, curve):
    """csrc/ntt_kernels.h:21-25 again -- below 32r after ten levels, 32 r * r of 70 r^2 into the next product -- where that product is the twiddle
    between two passes: plan_digits gives 7 + 7 at 2^14, 9 + 9 at 2^18 and 10 + 9 at 2^19, the smallest size whose strided pass has ten levels;
    its store multiplies by omega^e from the two-level table with e up to 511 * 1023, beyond 2^13.  Canonical words below 2^248 with r - 1 and 0
    planted.  The model's NTT is too slow at this size: the whole output is checked with one random linear functional (_functional), which a
    wrong output vector passes with probability at most n / r, and the inverse transform with 1 / n must give the input back.
    The time is the host's.  Measured on a CPU without a GPU at 2^19, per field: the functional 1.2 s (BLS12-381) and 1.3 s (BN254), the two
    conversions from bytes to integers 0.1 s each, the random input 0.1 s."""
    ctx = contexts(curve, False)
    api.fr_test_pass_bits(0)
    r, rnd = api.SCALAR_FIELDS[curve], rng(2100)
    log_n = 19
    n = 1 << log_n
    blob = bytearray(rnd.randbytes(32 * n))
    blob[31::32] = bytes(n)  # (248-bit values: below r)
    for k, at in enumerate((0, 1, 511, 512, n // 2 - 1, n // 2, n - 2, n - 1) + tuple(rnd.randrange(n) for _ in range(24))):
        blob[32 * at:32 * at + 32] = ((r - 1) if k % 2 == 0 else 0).to_bytes(32, "little")
    a = from_bytes(bytes(blob))
    src = torch.frombuffer(blob, dtype=torch.uint8).reshape(-1, 32).cuda()
    t = src.clone()
    ctx.scalars_fft(t)
    assert api.fr_last() == (2, 10)
    w = api.root_of_unity(curve, log_n)
    rho = rnd.randrange(2, r)
    assert pow(rho, n, r) != 1  # rho w^j != 1 for every j: rho is no n-th root of unity (_functional asserts it of every j as well)
    left, right = _functional(a, from_bytes(raw(t)), w, rho, r)
    assert left == right, curve
    ctx.scalars_fft(t, inverse=True)
    assert api.fr_last() == (2, 10) and torch.equal(t, src), curve


# ---- 3. frmle ----------------------------------------------------------------------------------------------------------------------------------------
def _extreme_tables(r, n, top):
    """the tables of tests/test_frmle_host.py::test_round_at_the_lazy_bounds that are not all 0 or random, with `top` for r - 1"""
    tables = mle_tables(r, n, rng(0))
    return {name: [top if v == r - 1 else v for v in tables[name]] for name in ("lo 0, hi r - 1", "lo r - 1, hi 0", "all r - 1")}


@FORMS
@pytest.mark.parametrize("curve", FIVE)
def test_frmle_round_at_the_lazy_bounds(contexts, curve, mont):
    """csrc/frmle_kernels.h:25-34 and the static_asserts of :97-98.  The values at t = 4 are below 5r (lo = 0, hi = r - 1 gives 4 (r - 1)), the first
    product of a chain takes two of them, 25 r^2 of the field's FQ_HEADROOM r^2 (BLS12-381: 70); a lane's sum is 4 pairs x 8 terms x 2r = 64r of the
    70r that fq_tidy takes.  The pattern of tests/test_frmle_host.py::test_round_at_the_lazy_bounds: two equal rows with the lo half 0 and the hi half
    r - 1, the reverse, and all r - 1; eight equal terms of degree 4 with the coefficient r - 1 (eight equal terms are eight times one: the model
    computes one).  n = 16, and n = 2048: one full tile of 1024 pairs, four to every lane.  Without the fold, and fused with the fold by r - 1
    (the bind, :9-10: 3 r * r), where 4096 elements leave 1024 pairs and is run as well."""
    ctx = contexts(curve, mont)
    api.frmle_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    terms = [(r - 1, (0, 1, 0, 1))] * 8
    for top in tops(r, mont):
        for n in (16, 2 * T, 4 * T):
            for name, table in _extreme_tables(r, n, top).items():
                rows = [table, table]
                what = (curve, mont, top == r - 1, n, name)
                stored = form(table + table, r, mont)
                src = dev(stored)
                if n <= 2 * T:
                    want = [8 * v % r for v in MLE.round_values(rows, terms[:1], r)]
                    assert ctx.scalars_sumcheck_round(src, terms, batch=2) == to_bytes(form(want, r, mont)), what
                    assert api.frmle_last() == (1, 1) and raw(src) == to_bytes(stored), what
                folded = [MLE.fold(table, r - 1, r)] * 2
                want = [8 * v % r for v in MLE.round_values(folded, terms[:1], r)]
                assert ctx.scalars_sumcheck_round(src, terms, batch=2, fold=r - 1) == to_bytes(form(want, r, mont)), what + ("fused",)
                assert api.frmle_last() == (1, 1)
                assert raw(src) == to_bytes(form((folded[0] + table[n // 2:]) * 2, r, mont)), what + ("the folded rows",)


@FORMS
@pytest.mark.parametrize("curve", FIVE)
def test_frmle_bind_at_its_bound(contexts, curve, mont):
    """csrc/frmle_kernels.h:9-10: the bind's difference hi - lo + 2r is below 3r, and its product by the challenge takes 3 r * r of the field's
    FQ_HEADROOM r^2 (BLS12-381: 70).  fold and eval at n = 1024 (eval: one full tile, ten binds deep) on the two tables of the round's test -- fold
    pairs the halves, so lo = 0, hi = r - 1 is its largest difference -- and on r - 1 alternating with 0 and the reverse, the largest under eval's
    first bind, which pairs neighbours.  The challenge r - 1 (every variable of eval's point), then a random one."""
    ctx = contexts(curve, mont)
    api.frmle_test_tile(0)
    r, rnd = api.SCALAR_FIELDS[curve], rng(2300)
    n = T
    for top in tops(r, mont):
        tables = _extreme_tables(r, n, top)
        pairs = ([tables["lo 0, hi r - 1"], tables["lo r - 1, hi 0"]], [[0, top] * (n // 2), [top, 0] * (n // 2)])
        for k, rows in enumerate(pairs):
            stored = form(rows[0] + rows[1], r, mont)
            src = dev(stored)
            for c in (r - 1, rnd.randrange(2, r - 1)):
                what = (curve, mont, top == r - 1, k, c == r - 1)
                out = torch.full_like(src, 0xEE)
                assert ctx.scalars_mle_fold(src, c, batch=2, out=out) is out and raw(src) == to_bytes(stored)
                got = out.reshape(2, n, 32)
                assert raw(got[:, :n // 2]) == to_bytes(form(MLE.fold(rows[0], c, r) + MLE.fold(rows[1], c, r), r, mont)), what + ("fold",)
                assert raw(got[:, n // 2:]) == b"\xee" * (32 * n)
                point = [c] * 10 if c == r - 1 else [rnd.randrange(r) for _ in range(10)]
                assert ctx.scalars_mle_eval(src, point, batch=2) == to_bytes(form([MLE.evaluate(row, point, r) for row in rows], r, mont)), what + ("eval",)
                assert api.frmle_last() == (1, 1)


# ---- 4. frmat ----------------------------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("curve", FIVE)
def test_frmat_one_row_over_a_full_tile(contexts, curve, mont):
    """csrc/frmat_kernels.h:27-31 and the static_assert of :68: a product of a value and an element of x is r * r of FQ_HEADROOM r^2, a lane's lazy
    sum of FRMAT_E = 4 products of < 2r each is below 8r of the FQ_HEADROOM r (70) that fq_tidy takes.  The pattern of
    tests/test_frmat_host.py::test_a_full_tile_of_one_row_at_the_lazy_bound: one row of 1024 entries -- every lane adds four products --, and of
    1025, which spills into a second tile and a second level; all columns distinct; (value, x) = (r - 1, r - 1), (r - 1, 0), (1, r - 1).
    (r - 1)(r - 1) = 1, so y = n for the first and -n for the last.  The matrix values are plain in either form and the product is linear in x:
    with x STORED as r - 1 in the mont256 form the stored y is n, and -n."""
    ctx = contexts(curve, mont)
    api.frmat_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for n in (T, T + 1):
        ptr, idx = [0, n], list(range(n))
        lv = MAT.levels(ptr, T)
        assert lv == (1 if n == T else 2)
        for v, xv, closed in ((r - 1, r - 1, n % r), (r - 1, 0, 0), (1, r - 1, -n % r)):
            mat = ctx.scalars_matrix(1, n, ptr, idx, [v] * n)
            what = (curve, mont, n, v == 1, xv == 0)
            y = ctx.scalars_matvec(mat, dev(form([xv] * n, r, mont)))
            assert api.frmat_last() == (lv + 1, lv), what
            assert MAT.matvec(1, n, ptr, idx, [v] * n, [xv] * n, r) == [closed]
            assert tuple(y.shape) == (1, 32) and raw(y) == to_bytes(form([closed], r, mont)), what
            if mont:
                assert raw(ctx.scalars_matvec(mat, dev([xv] * n))) == to_bytes([closed]), what + ("x stored as it is",)
            mat.close()


# ---- 5. frpoly ---------------------------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("curve", FOUR)
def test_frpoly_eval_and_divide_of_r_minus_one(contexts, curve, mont):
    """csrc/frpoly_kernels.h:11-12 and :130, :167, :211: between two products a fold's or a suffix scan's value is a lazy sum below 21r (a tile's
    Horner total below 19r), which the next product takes with a weight below r: 21 r * r of the field's FQ_HEADROOM r^2 (BLS12-381: 70); frp_exact
    (:132) tidies at most 84r.  All coefficients r - 1 at n = 1024 -- one full tile, every lane's three Horner products and all eight steps of the
    tree and of the scan -- and 1025, which adds the second level and the carry-in; z = r - 1, 1 and a random point.  eval, divide into another
    tensor and divide in place."""
    ctx = contexts(curve, mont)
    api.frpoly_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for top in tops(r, mont):
        for n in (T, T + 1):
            a = [top] * n
            stored = to_bytes(form(a, r, mont))
            src = dev(form(a, r, mont))
            for z in (r - 1, 1, rng(2500 + n).randrange(2, r - 1)):
                what = (curve, mont, top == r - 1, n, z)
                q, value = POLY.divide(a, z, r)
                want_q, want_v = to_bytes(form(q, r, mont)), to_bytes(form([value], r, mont))
                assert ctx.scalars_eval(src, z) == want_v, what + ("eval",)
                assert api.frpoly_last() == ((1, 1) if n <= T else (2, 2))
                out = torch.full_like(src, 0xEE)
                got, values = ctx.scalars_divide(src, z, out=out, values=True)
                assert got is out and raw(out) == want_q and values == want_v and raw(src) == stored, what + ("divide into out",)
                assert api.frpoly_last() == ((1, 1) if n <= T else (3, 2))
                t = src.clone()
                assert ctx.scalars_divide(t, z) is t and raw(t) == want_q, what + ("divide in place",)


@FORMS
@pytest.mark.parametrize("curve", FOUR)
def test_frpoly_combine_across_its_tidy_interval(contexts, curve, mont):
    """csrc/frpoly_kernels.h:233: the combination's lazy sum is tidied every eight terms and stays below 18r (eight products of < 2r on a tidied
    value of < 2r) of the FQ_HEADROOM r (70) that the tidy takes.  8, 9, 16 and 17 rows -- one interval, one more, two, one more -- of n = 65
    elements, every element and every coefficient r - 1: (r - 1)(r - 1) = 1, so every output is the number of rows.  The combination is linear in
    the data: with the data STORED as r - 1 in the mont256 form the stored output is the number of rows."""
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    n = 65
    for batch in (8, 9, 16, 17):
        coeffs = [r - 1] * batch
        assert POLY.combine([[r - 1] * n] * batch, coeffs, r) == [batch] * n
        src = dev(form([r - 1] * (batch * n), r, mont))
        out = ctx.scalars_combine(src, coeffs)
        assert tuple(out.shape) == (n, 32) and raw(out) == to_bytes(form([batch] * n, r, mont)), (curve, mont, batch)
        assert api.frpoly_last() == (1, 1)
        if mont:
            assert raw(ctx.scalars_combine(dev([r - 1] * (batch * n)), coeffs)) == to_bytes([batch] * n), (curve, batch, "stored as it is")


# ---- 6. frvec ----------------------------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("curve", FOUR)
def test_frvec_inverse_scans_and_mul_add_of_r_minus_one(contexts, curve, mont):
    """csrc/frvec_kernels.h states no lazy bound: every product there takes two exact values below 2r (:104, :141, :193), 4 r^2 of FQ_HEADROOM r^2.
    What reaches it is the largest operands: all r - 1 at n = 1024 (one full tile) and 1025 (a second level).  The inverse of r - 1 is r - 1; the
    sums are k (r - 1), the products alternate between r - 1 and 1; (r - 1)(r - 1) + (r - 1) = 0.  The vector whose STORED words are r - 1 in the
    mont256 form is compared with the model alone."""
    ctx = contexts(curve, mont)
    api.frvec_test_tile(0)
    r = api.SCALAR_FIELDS[curve]
    for top in tops(r, mont):
        for n in (T, T + 1):
            a = [top] * n
            src = dev(form(a, r, mont))
            what = (curve, mont, top == r - 1, n)
            closed = top == r - 1
            want = VEC.inverse(a, r)
            assert not closed or want == [r - 1] * n
            out = torch.zeros_like(src)
            assert ctx.scalars_inverse(src, out=out) is out and raw(out) == to_bytes(form(want, r, mont)), what + ("inverse",)
            assert api.frvec_last() == ((1, 1) if n <= T else (3, 2))
            for op in ("sum", "product"):
                for exclusive in (False, True):
                    want, want_totals = VEC.scan(a, op, exclusive, r)
                    if closed:
                        first = 1 if exclusive else 0  # (the number of elements behind output i is i + 1 - first)
                        assert want == ([(i + 1 - first) * (r - 1) % r for i in range(n)] if op == "sum" else [(r - 1, 1)[(i + first) % 2] for i in range(n)])
                        assert want_totals == ([n * (r - 1) % r] if op == "sum" else [(1, r - 1)[n % 2]])
                    t = src.clone()
                    got, totals = ctx.scalars_scan(t, op=op, exclusive=exclusive, totals=True)
                    assert got is t and raw(t) == to_bytes(form(want, r, mont)), what + (op, exclusive)
                    assert totals == to_bytes(form(want_totals, r, mont)), what + (op, exclusive, "totals")
                    assert api.frvec_last() == ((1, 1) if n <= T else (3, 2))
            want = VEC.map_op("mul_add", a, a, a, r)
            assert not closed or want == [0] * n
            out = torch.full_like(src, 0xEE)
            assert ctx.scalars_mul_add(src, src.clone(), src.clone(), out=out) is out and raw(out) == to_bytes(form(want, r, mont)), what + ("mul_add",)
            t = src.clone()
            assert raw(ctx.scalars_mul_add(t, t, t)) == to_bytes(form(want, r, mont)), what + ("mul_add, one tensor in every place",)
