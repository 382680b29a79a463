"""The two variable orders of libmsm_frmle.so on the CPU: a stand-alone program (tests/host_harness/frmle_low_harness.cpp) runs fold, round and
the fused round as csrc/frmle_host.h launches them -- the schedules of csrc/frmle_plan.h, the lane functions of csrc/frmle_kernels.h, compiled
with g++ -DFQ_CHECK so that every bound of csrc/fq29.h is asserted -- against the models: tests/frmle_low_model.py under MSM_FRMLE_LOW_FIRST,
tests/frmle_model.py without it.  The five fields, both data forms, the all-(r - 1) table.  The in-place schedules run with the lanes of every
launch ascending, descending and with the workgroups interleaved: equal bytes in all three is what pins that no launch stores where one of its
own lanes reads.  Host logic only."""
import os
import struct
import subprocess

import pytest

from tests import frmle_low_model as L
from tests import frmle_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
T = 1024  # the design's tile (csrc/frmle_kernels.h: FRMLE_TILE)
ORDERS = (0, 1, 2)  # lanes ascending, descending, workgroups interleaved
FILL = 0xEEEEEEEE  # what the program's separate output begins as, in every 32-bit word
WHAT_FILL = int.from_bytes(struct.pack("<8I", *([FILL] * 8)), "little")


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frmle_low_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frm_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frmle_low_harness.cpp"), "-o", exe])
    return exe


def _call(exe, tmp, args, payload):
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(payload)
    p = subprocess.run([exe] + [str(a) for a in args] + [str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3), (p.returncode, p.stderr[-500:])
    return p.returncode, fout.read_bytes()


def _strided(rows, stride, filler):
    out = []
    for v, row in enumerate(rows):
        out += list(row) + ([filler] * (stride - len(row)) if v + 1 < len(rows) else [])
    return out


def _unstrided(flat, n, batch, stride):
    return [flat[v * stride:v * stride + n] for v in range(batch)]


def _form(vals, r, mont):
    return L.mont(vals, r) if mont else list(vals)


def _back(vals, r, mont):
    return L.mont(vals, r, back=True) if mont else vals


def run_fold(exe, tmp, r, rows, c, stride, low, order, apart=False):
    """-> (status, the rows as the call leaves them, the separate output's rows or None, every element the program wrote out).  Plain integers:
    a bind is linear in the data, and k_frmle_fold does not know their form."""
    n, batch = len(rows[0]), len(rows)
    rc, raw = _call(exe, tmp, ["fold", int(low), order, int(apart), n, batch, stride], L.to_bytes([c]) + L.to_bytes(_strided(rows, stride, 1)))
    got = L.from_bytes(raw)
    count = (batch - 1) * stride + n
    return rc, _unstrided(got[:count], n, batch, stride), _unstrided(got[count:], n, batch, stride) if apart else None, got


def term_bytes(terms):
    return b"".join(int(c).to_bytes(32, "little") + struct.pack("<5I", len(rows), *(tuple(rows) + (0,) * (4 - len(rows)))) for c, rows in terms)


def run_round(exe, tmp, r, rows, terms, stride, tile, mont, low, order, fold_by=None):
    """-> (status, values, the rows as the call leaves them, (launches, levels))"""
    n, batch = len(rows[0]), len(rows)
    head = (L.to_bytes([fold_by]) if fold_by is not None else b"") + term_bytes(terms)
    rc, raw = _call(exe, tmp, ["round", int(low), order, n, batch, stride, tile, int(mont), int(fold_by is not None), len(terms)],
                    head + L.to_bytes(_form(_strided(rows, stride, 1), r, mont)))
    got = L.from_bytes(raw)
    shape = tuple(got[-2:])
    got = _back(got[:-2], r, mont)
    points = L.degree(terms) + 1
    return rc, got[:points], _unstrided(got[points:], n, batch, stride), shape


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frmle_low_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _tables(r, n, rnd):
    return {"all r - 1": [r - 1] * n, "even 0, odd r - 1": [0, r - 1] * (n // 2), "even r - 1, odd 0": [r - 1, 0] * (n // 2), "random": [rnd.randrange(r) for _ in range(n)]}


def _challenges(r, rnd):
    return (0, 1, r - 1, rnd.randrange(2, r - 1))


# (n, batch, stride): one pair; the smallest split; rows apart; outputs in several workgroups (2^11: 512 outputs to a launch, 2^12 with two rows: 8 workgroups)
FOLD_SHAPES = [(2, 1, 2), (4, 2, 4), (8, 3, 11), (64, 2, 70), (2048, 1, 2048), (4096, 2, 4099)]


@pytest.mark.parametrize("low", [False, True])
def test_fold_in_both_orders_against_the_models(harness, low):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(81)
    model = L if low else M
    for n, batch, stride in FOLD_SHAPES:
        names = _tables(r, n, rnd) if n <= 64 else ("all r - 1", "random")
        for name in names:
            rows = [_tables(r, n, rnd)[name]] + [[rnd.randrange(r) for _ in range(n)] for _ in range(batch - 1)]
            for c in _challenges(r, rnd) if n <= 64 else (rnd.randrange(2, r),):
                want = [model.fold(row, c, r) for row in rows]
                flats = set()
                for order in ORDERS:
                    rc, after, _, flat = run_fold(exe, tmp, r, rows, c, stride, low, order)
                    assert rc == 0 and [row[:n // 2] for row in after] == want, (field, n, name, c, order)
                    if not low:  # top first: what lies behind the result is as it was
                        assert [row[n // 2:] for row in after] == [row[n // 2:] for row in rows]
                    if stride > n:  # the elements [n, stride) are untouched in both orders
                        assert all(x == 1 for v in range(batch - 1) for x in flat[v * stride + n:(v + 1) * stride])
                    flats.add(tuple(flat))
                assert len(flats) == 1, (field, n, name)  # (the unspecified upper half too: the bytes do not depend on the order of the lanes)
                rc, after, out, _ = run_fold(exe, tmp, r, rows, c, stride, low, 1, apart=True)
                assert rc == 0 and after == rows and [row[:n // 2] for row in out] == want, (field, n, name, "apart")
                assert all(x == WHAT_FILL for row in out for x in row[n // 2:]), (field, n, "apart: only n / 2 elements of a row are written")


def _terms_of_every_kind(r, rnd, batch):
    row = lambda: rnd.randrange(batch)  # noqa: E731
    return {"degree 1": [(rnd.randrange(r), (row(),))], "degree 2": [(1, (row(), row()))], "degree 3": [(r - 1, (row(), row(), row()))],
            "degree 4": [(rnd.randrange(r), (row(), row(), row(), row()))],
            "eight terms": [((1, r - 1, rnd.randrange(r), 0)[j % 4], tuple(row() for _ in range(1 + j % 4))) for j in range(8)]}


# (n, batch, stride, tile): the smallest sizes; the design tile at one tile and past it (2^12: two launches of one tile of 512 pairs each, 2^14: of four); the
# hook's tiles at two and three levels
ROUND_SHAPES = [(2, 1, 2, T), (4, 2, 4, T), (8, 3, 11, T), (64, 2, 70, T), (4096, 2, 4096, T), (16384, 1, 16384, T), (8, 3, 8, 2), (64, 2, 70, 4), (128, 2, 128, 8)]


def levels_and_launches(n, tile, low, fused):
    """what include/msm_frmle.h says msm_frmle_test_last reports for a round"""
    def levels(count):
        k = 1
        while -(-count // tile) > 1:
            count, k = -(-count // tile), k + 1
        return k

    if not fused:
        return levels(n // 2), levels(n // 2)
    if not low:
        return levels(n // 4), levels(n // 4)
    if n == 4:
        return 1, 1
    lv = 1 + levels(2 * -(-n // (4 * tile)))  # (two launches of n / 8 pairs over tiles of tile / 2)
    return lv + 1, lv


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("low", [False, True])
@pytest.mark.parametrize("n,batch,stride,tile", ROUND_SHAPES)
def test_round_in_both_orders_against_the_models(harness, n, batch, stride, tile, low, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(82 + n)
    model = L if low else M
    rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(batch)]
    rows[0] = [r - 1] * n
    kinds = _terms_of_every_kind(r, rnd, batch)
    if n > 128:
        kinds = {k: kinds[k] for k in ("degree 3",)}
    elif mont:
        kinds = {k: kinds[k] for k in ("degree 2", "eight terms")}
    for name, terms in kinds.items():
        rc, values, after, shape = run_round(exe, tmp, r, rows, terms, stride, tile, mont, low, 0)
        assert rc == 0 and values == model.round_values(rows, terms, r) and after == rows, (field, n, name)
        assert shape == levels_and_launches(n, tile, low, False), (n, tile, shape)
        if n >= 4:
            for c in ((r - 1, rnd.randrange(r)) if n <= 16 else (rnd.randrange(r),)):
                folded = [model.fold(row, c, r) for row in rows]
                seen = set()
                for order in ORDERS:
                    rc, values, after, shape = run_round(exe, tmp, r, rows, terms, stride, tile, mont, low, order, fold_by=c)
                    assert rc == 0 and values == model.round_values(folded, terms, r), (field, n, name, c, order)
                    assert [row[:n // 2] for row in after] == folded, (field, n, name, c, order)
                    assert shape == levels_and_launches(n, tile, low, True), (n, tile, shape)
                    if not low:
                        assert [row[n // 2:] for row in after] == [row[n // 2:] for row in rows]
                    seen.add(tuple(x for row in after for x in row))
                assert len(seen) == 1, (field, n, name)


def test_a_whole_proof_in_the_low_order(harness):
    """round, then fused rounds with n halving in one buffer, against the model's transcript (the elements behind n / 2 are never read again)"""
    field, exe, tmp = harness
    r, rnd = _r(field), rng(83)
    terms = [(3, (0, 1, 2)), (r - 2, (3,))]
    for k in (1, 2, 3, 6):
        n = 1 << k
        rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(4)]
        transcript, point, finals = L.prove(rows, terms, lambda j, v: (v[0] + 3 * v[1] + j) % r, r)
        live, got = [list(row) for row in rows], []
        for j in range(k):
            m = n >> max(j - 1, 0)
            rc, values, after, _ = run_round(exe, tmp, r, [row[:m] for row in live], terms, m, 8, False, True, 1, fold_by=point[j - 1] if j else None)
            assert rc == 0
            live = after
            got.append(values)
        assert got == transcript, (field, k)
        assert [L.fold(row[:2], point[-1], r)[0] for row in live] == finals


def test_a_value_not_below_r_is_reported_in_the_low_order(harness):
    field, exe, tmp = harness
    r = _r(field)
    n = 32
    rows = [[3] * n, [4] * n]
    for bad in (r, (1 << 256) - 1):
        for at in (0, 5, n - 1):  # (the scratch launch's inputs and the in-place launch's)
            rows[1][at] = bad
            assert run_fold(exe, tmp, r, rows, 5, n, True, 0)[0] == 3
            assert run_fold(exe, tmp, r, rows, 5, n, True, 0, apart=True)[0] == 3
            assert run_round(exe, tmp, r, rows, [(1, (0, 1))], n, 8, False, True, 0)[0] == 3
            assert run_round(exe, tmp, r, rows, [(1, (0,))], n, 8, False, True, 0, fold_by=2)[0] == 3  # (the fold reads every row)
            assert run_round(exe, tmp, r, rows, [(1, (0,))], n, 8, False, True, 0)[0] == 0  # (row 1 is not read)
            rows[1][at] = 4


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan: the scratch rows, the levels, the words behind the terms, the shifts"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r = _r(field)
    rnd = rng(89)
    for n, batch, stride, tile in ((4096, 2, 4096, T), (64, 3, 67, 4), (8, 2, 8, 2), (4, 1, 4, T), (2, 2, 3, T)):
        rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(batch)]
        rows[0][0], rows[-1][-1] = 0, r - 1
        c = rnd.randrange(r)
        terms = [(rnd.randrange(r), (0, batch - 1, 0)), (r - 1, (batch - 1,))]
        for low, model in ((True, L), (False, M)):
            folded = [model.fold(row, c, r) for row in rows]
            for order in ORDERS:
                rc, after, _, _ = run_fold(exe, tmp_path, r, rows, c, stride, low, order)
                assert rc == 0 and [row[:n // 2] for row in after] == folded
            rc, after, out, _ = run_fold(exe, tmp_path, r, rows, c, stride, low, 2, apart=True)
            assert rc == 0 and after == rows and [row[:n // 2] for row in out] == folded
            rc, values, _, _ = run_round(exe, tmp_path, r, rows, terms, stride, tile, True, low, 1)
            assert rc == 0 and values == model.round_values(rows, terms, r)
            if n >= 4:
                for order in ORDERS:
                    rc, values, after, _ = run_round(exe, tmp_path, r, rows, terms, stride, tile, True, low, order, fold_by=c)
                    assert rc == 0 and values == model.round_values(folded, terms, r) and [row[:n // 2] for row in after] == folded
