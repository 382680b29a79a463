"""libmsm_frmle.so's calls on the CPU: the identities the pure-Python model (tests/frmle_model.py) must satisfy, and a stand-alone program
(tests/host_harness/frmle_harness.cpp) that runs the constants and levels of csrc/frmle_plan.h and, lane by lane, the functions the kernels call
(csrc/frmle_kernels.h) -- fold, eval with its tree, eq with its tables, round with and without the fused fold and the sums above it, with the tile
passed in -- compiled with g++ -DFQ_CHECK so that every limb and value bound of csrc/fq29.h is asserted, against that model.  The five fields,
both data forms.  Host logic only."""
import os
import struct
import subprocess

import pytest

from tests import frmle_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
T = 1024  # the design's tile (csrc/frmle_kernels.h: FRMLE_TILE)


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
R_MODEL = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def test_model_eval_is_the_inner_product_with_eq():
    r, rnd = R_MODEL, rng(1)
    for k in (0, 1, 2, 5):
        a = [rnd.randrange(r) for _ in range(1 << k)]
        z = [rnd.randrange(r) for _ in range(k)]
        e = M.eq(z, r)
        assert len(e) == 1 << k and M.evaluate(a, z, r) == sum(x * y for x, y in zip(a, e)) % r
        w = [rnd.randrange(r) for _ in range(k)]
        assert M.evaluate(M.eq(w, r), z, r) == M.eq_value(w, z, r)
        assert M.eq(z, r, 7) == [7 * x % r for x in e]
    # the first variable is the top bit: a point of bits picks the element they spell
    a = list(range(100, 108))
    assert [M.evaluate(a, [(i >> 2) & 1, (i >> 1) & 1, i & 1], r) for i in range(8)] == a
    assert M.eq([1, 0, 1], r) == [0, 0, 0, 0, 0, 1, 0, 0]


def test_model_round_values():
    r, rnd = R_MODEL, rng(2)
    k = 4
    rows = [[rnd.randrange(r) for _ in range(1 << k)] for _ in range(3)]
    terms = [(5, (0, 1, 2)), (r - 1, (0, 2)), (3, (1, 1, 1, 1)), (9, (2,))]
    g = M.round_values(rows, terms, r)
    assert len(g) == 5 and (g[0] + g[1]) % r == M.claimed_sum(rows, terms, r)
    # eq(w) eq(u): the closed form of its round values
    w, u = [rnd.randrange(r) for _ in range(k)], [rnd.randrange(r) for _ in range(k)]
    tail = M.eq_value(w[1:], u[1:], r)
    assert M.round_values([M.eq(w, r), M.eq(u, r)], [(1, (0, 1))], r) == [M.eq1(w[0], t, r) * M.eq1(u[0], t, r) * tail % r for t in range(3)]
    # the fused round is fold, then round
    c = rnd.randrange(r)
    folded = [M.fold(row, c, r) for row in rows]
    transcript, point, finals = M.prove(rows, terms, lambda j, v: c + j, r)
    assert transcript[0] == g and transcript[1] == M.round_values(folded, terms, r) and point == [c, c + 1, c + 2, c + 3]
    assert finals == [M.evaluate(row, point, r) for row in rows]
    assert M.verify(M.claimed_sum(rows, terms, r), transcript, point, finals, terms, r)
    assert not M.verify(M.claimed_sum(rows, terms, r) + 1, transcript, point, finals, terms, r)
    bad = [list(v) for v in transcript]
    bad[2][1] = (bad[2][1] + 1) % r
    assert not M.verify(M.claimed_sum(rows, terms, r), bad, point, finals, terms, r)


# ---- the program -----------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frmle_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frm_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frmle_harness.cpp"), "-o", exe])
    return exe


def _call(exe, tmp, args, payload):
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(payload)
    p = subprocess.run([exe] + [str(a) for a in args] + [str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3), (p.returncode, p.stderr[-500:])
    return p.returncode, M.from_bytes(fout.read_bytes())


def _form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def _back(vals, r, mont):
    return M.mont(vals, r, back=True) if mont else vals


def _strided(rows, stride, filler):
    """the rows `stride` apart, `filler` between them"""
    out = []
    for v, row in enumerate(rows):
        out += list(row) + ([filler] * (stride - len(row)) if v + 1 < len(rows) else [])
    return out


def _unstrided(flat, n, batch, stride):
    return [flat[v * stride:v * stride + n] for v in range(batch)]


def run_fold(exe, tmp, r, rows, c, stride, mont):
    n = len(rows[0])
    rc, got = _call(exe, tmp, ["fold", n, len(rows), stride], M.to_bytes([c]) + M.to_bytes(_form(_strided(rows, stride, 1), r, mont)))
    return rc, _unstrided(_back(got, r, mont), n, len(rows), stride)


def run_eval(exe, tmp, r, rows, point, stride, tile, mont):
    rc, got = _call(exe, tmp, ["eval", len(rows[0]), len(rows), stride, tile], M.to_bytes(point) + M.to_bytes(_form(_strided(rows, stride, 1), r, mont)))
    return rc, _back(got, r, mont)


def run_eq(exe, tmp, r, point, c, mont):
    rc, got = _call(exe, tmp, ["eq", 1 << len(point), int(mont)], M.to_bytes([c]) + M.to_bytes(point))
    return rc, _back(got, r, mont)


def term_bytes(terms):
    return b"".join(int(c).to_bytes(32, "little") + struct.pack("<5I", len(rows), *(tuple(rows) + (0,) * (4 - len(rows)))) for c, rows in terms)


def run_round(exe, tmp, r, rows, terms, stride, tile, mont, fold_by=None):
    """-> (status, values, the rows as the call leaves them)"""
    n = len(rows[0])
    head = (M.to_bytes([fold_by]) if fold_by is not None else b"") + term_bytes(terms)
    rc, got = _call(exe, tmp, ["round", n, len(rows), stride, tile, int(mont), int(fold_by is not None), len(terms)],
                    head + M.to_bytes(_form(_strided(rows, stride, 1), r, mont)))
    got = _back(got, r, mont)
    points = M.degree(terms) + 1
    return rc, got[:points], _unstrided(got[points:], n, len(rows), stride)


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frmle_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _challenges(r, rnd):
    return (0, 1, r - 1, rnd.randrange(2, r - 1))


def _tables(r, n, rnd):
    h = n // 2
    return {"all 0": [0] * n, "all r - 1": [r - 1] * n, "lo 0, hi r - 1": [0] * h + [r - 1] * (n - h), "lo r - 1, hi 0": [r - 1] * h + [0] * (n - h),
            "random": [rnd.randrange(r) for _ in range(n)]}


@pytest.mark.parametrize("mont", [False, True])
def test_fold_against_the_model(harness, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(41)
    for n, batch, stride in ((2, 1, 2), (8, 3, 8), (16, 2, 21), (1024, 1, 1024)):
        for name, flat in _tables(r, n, rnd).items():
            rows = [flat] + [[rnd.randrange(r) for _ in range(n)] for _ in range(batch - 1)]
            for c in _challenges(r, rnd):
                rc, got = run_fold(exe, tmp, r, rows, c, stride, mont)
                assert rc == 0, (field, name)
                for row, out in zip(rows, got):  # the folded half, and the rest of the row as it was
                    assert out[:n // 2] == M.fold(row, c, r) and out[n // 2:] == row[n // 2:], (field, n, name, c)


# (n, tile): one level with a partial quad, one and two lanes, a full tile; two and three levels with a full and a partial top tile
EVAL_SHAPES = [(1, T), (2, T), (4, T), (8, T), (512, T), (1024, T), (2048, T), (4096, T), (8, 2), (16, 4), (64, 4), (128, 8), (32, 8)]


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n,tile", EVAL_SHAPES)
def test_eval_against_the_model(harness, n, tile, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(42 + n)
    k = n.bit_length() - 1
    batch, stride = (2, n + 3) if n <= 128 else (1, n)
    names = ("all r - 1", "lo 0, hi r - 1", "random") if n > 128 else tuple(_tables(r, n, rnd))
    for name in names:
        rows = [_tables(r, n, rnd)[name]] + [[rnd.randrange(r) for _ in range(n)] for _ in range(batch - 1)]
        points = [[rnd.randrange(r) for _ in range(k)], [(0, 1, r - 1)[j % 3] for j in range(k)]]
        for point in points:
            rc, got = run_eval(exe, tmp, r, rows, point, stride, tile, mont)
            assert rc == 0 and got == [M.evaluate(row, point, r) for row in rows], (field, n, tile, name)


@pytest.mark.parametrize("mont", [False, True])
def test_eq_against_the_model(harness, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(43)
    for k in (0, 1, 2, 3, 5, 6, 7, 10, 11):  # one, two and three windows of the lane's number; a partial quad
        for point in ([rnd.randrange(r) for _ in range(k)], [(1, 0, r - 1)[j % 3] for j in range(k)], [j & 1 for j in range(k)]):
            for c in (1, 0, r - 1, rnd.randrange(r)) if k <= 6 else (rnd.randrange(r),):
                rc, got = run_eq(exe, tmp, r, point, c, mont)
                assert rc == 0 and got == M.eq(point, r, c), (field, k, c)


def _terms_of_every_kind(r, rnd, batch):
    row = lambda: rnd.randrange(batch)  # noqa: E731
    return {"degree 1": [(rnd.randrange(r), (row(),))], "degree 2": [(1, (row(), row()))], "degree 3": [(r - 1, (row(), row(), row()))],
            "degree 4": [(rnd.randrange(r), (row(), row(), row(), row()))], "a row four times": [(3, (0, 0, 0, 0))], "a zero coefficient": [(0, (0, 0)), (5, (batch - 1,))],
            "eight terms": [((1, r - 1, rnd.randrange(r), 0)[j % 4], tuple(row() for _ in range(1 + j % 4))) for j in range(8)]}


# (n, batch, stride, tile): the design tile at one tile and past it; the hook's tiles at two and three levels
ROUND_SHAPES = [(2, 1, 2, T), (4, 2, 4, T), (8, 3, 11, T), (1024, 2, 1024, T), (4096, 2, 4096, T), (8, 3, 8, 2), (16, 16, 16, 4), (64, 2, 70, 4), (128, 2, 128, 8)]


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n,batch,stride,tile", ROUND_SHAPES)
def test_round_against_the_model(harness, n, batch, stride, tile, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(44 + n)
    rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(batch)]
    kinds = _terms_of_every_kind(r, rnd, batch)
    if n > 128:
        kinds = {k: kinds[k] for k in ("degree 2", "eight terms")}
    for name, terms in kinds.items():
        rc, values, after = run_round(exe, tmp, r, rows, terms, stride, tile, mont)
        assert rc == 0 and values == M.round_values(rows, terms, r) and after == rows, (field, n, name)
        if n >= 4:
            for c in _challenges(r, rnd) if n <= 16 else (rnd.randrange(r),):
                folded = [M.fold(row, c, r) for row in rows]
                rc, values, after = run_round(exe, tmp, r, rows, terms, stride, tile, mont, fold_by=c)
                assert rc == 0 and values == M.round_values(folded, terms, r), (field, n, name, c)
                assert after == [f + row[n // 2:] for f, row in zip(folded, rows)], (field, n, name, c)


@pytest.mark.parametrize("mont", [False, True])
def test_round_at_the_lazy_bounds(harness, mont):
    """the data that maximise the values at t (lo = 0, hi = r - 1: 4 (r - 1) at t = 4) and the lane's sums (eight terms, four pairs to a lane), at
    degree 4, with the program's bound checks on"""
    field, exe, tmp = harness
    r, rnd = _r(field), rng(45)
    for n, tile in ((4096, T), (16, 8)):  # (2048 pairs: every lane of the design tile has its four)
        for name, table in _tables(r, n, rnd).items():
            if n > 16 and name in ("all 0", "random"):
                continue
            rows = [table, table]
            for coeff in (r - 1, 1) if n == 16 else (r - 1,):
                terms = [(coeff, (0, 1, 0, 1))] * 8  # (eight equal terms: the model computes one)
                rc, values, _ = run_round(exe, tmp, r, rows, terms, n, tile, mont)
                assert rc == 0 and values == [8 * v % r for v in M.round_values(rows, terms[:1], r)], (field, name)
                rc, values, _ = run_round(exe, tmp, r, rows, terms, n, tile, mont, fold_by=r - 1)
                assert rc == 0 and values == [8 * v % r for v in M.round_values([M.fold(t, r - 1, r) for t in rows], terms[:1], r)], (field, name)


def test_the_number_of_levels():
    """what plan_levels gives at the sizes the GPU tests name: eval counts the elements, round the pairs"""
    def levels(n, t):
        k = 1
        while -(-n // t) > 1:
            n, k = -(-n // t), k + 1
        return k

    assert [levels(n, T) for n in (1, 1024, 2048, 1 << 20, 1 << 21)] == [1, 1, 2, 2, 3]
    assert [levels(n, t) for t, n in ((2, 8), (4, 16), (4, 64), (8, 128))] == [3, 2, 3, 3]
    assert [levels(n // 2, t) for t, n in ((2, 8), (4, 16), (4, 64), (8, 128))] == [2, 2, 3, 2]


def test_a_value_not_below_r_is_reported(harness):
    field, exe, tmp = harness
    r = _r(field)
    n = 32
    rows = [[3] * n, [4] * n]
    terms = [(1, (0, 1))]
    assert run_round(exe, tmp, r, rows, terms, n, 8, False)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        for at in (5, n - 1):
            rows[1][at] = bad
            assert run_fold(exe, tmp, r, rows, 5, n, False)[0] == 3, hex(bad)
            assert run_eval(exe, tmp, r, rows, [2] * 5, n, 8, False)[0] == 3
            assert run_eval(exe, tmp, r, rows, [2] * 5, n, T, False)[0] == 3
            assert run_round(exe, tmp, r, rows, terms, n, 8, False)[0] == 3
            assert run_round(exe, tmp, r, rows, [(1, (0,))], n, 8, False, fold_by=2)[0] == 3  # (the fold reads every row)
            assert run_round(exe, tmp, r, rows, [(1, (0,))], n, 8, False)[0] == 0  # (row 1 is not read)
            rows[1][at] = 4


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the slots, the levels, the tables and the data; shifts)"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r = _r(field)
    rnd = rng(49)
    for n, batch, stride, tile in ((2048, 1, 2048, T), (64, 3, 67, 4), (8, 2, 8, 2)):
        k = n.bit_length() - 1
        rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(batch)]
        rows[0][0], rows[-1][-1] = 0, r - 1
        point = [rnd.randrange(r) for _ in range(k)]
        assert run_eval(exe, tmp_path, r, rows, point, stride, tile, True) == (0, [M.evaluate(row, point, r) for row in rows])
        assert run_fold(exe, tmp_path, r, rows, point[0], stride, True) == (0, [M.fold(row, point[0], r) + row[n // 2:] for row in rows])
        assert run_eq(exe, tmp_path, r, point, 7, True) == (0, M.eq(point, r, 7))
        terms = [(rnd.randrange(r), (0, batch - 1, 0)), (r - 1, (batch - 1,))]
        assert run_round(exe, tmp_path, r, rows, terms, stride, tile, True)[:2] == (0, M.round_values(rows, terms, r))
        folded = [M.fold(row, point[0], r) for row in rows]
        assert run_round(exe, tmp_path, r, rows, terms, stride, tile, True, fold_by=point[0]) == (0, M.round_values(folded, terms, r),
                                                                                                  [f + row[n // 2:] for f, row in zip(folded, rows)])
