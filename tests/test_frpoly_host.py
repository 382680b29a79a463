"""libmsm_frpoly.so's calls on the CPU: a stand-alone program (tests/host_harness/frpoly_harness.cpp) runs the constants and levels of
csrc/frpoly_plan.h and, lane by lane, the functions the kernels call (csrc/frpoly_kernels.h) -- the fold with its tree, the suffix scan with its
carry-in, the dot product, the combination and the powers, with the tile passed in -- compiled with g++ -DFQ_CHECK so that every limb and value
bound of csrc/fq29.h is asserted, against the pure-Python model (tests/frpoly_model.py: plain Horner).  All four fields, both data forms.  Host
logic only."""
import os
import subprocess

import pytest

from tests import frpoly_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "pallas", "vesta", "bls12_381")
T = 1024  # the design's tile (csrc/frpoly_kernels.h: FRPOLY_TILE)


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frpoly_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frp_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frpoly_harness.cpp"), "-o", exe])
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


def run_eval(exe, tmp, r, a, z, batch, tile, mont):
    rc, got = _call(exe, tmp, ["eval", len(a) // batch, batch, tile, int(mont)], M.to_bytes([z]) + M.to_bytes(_form(a, r, mont)))
    return rc, _back(got, r, mont)


def run_divide(exe, tmp, r, a, z, batch, tile, mont):
    rc, got = _call(exe, tmp, ["divide", len(a) // batch, batch, tile, int(mont)], M.to_bytes([z]) + M.to_bytes(_form(a, r, mont)))
    got = _back(got, r, mont)
    return rc, got[:len(a)], got[len(a):]


def run_dot(exe, tmp, r, a, b, batch, tile, mont):
    n = len(a) // batch
    rc, got = _call(exe, tmp, ["dot", n, batch, tile, int(mont), int(len(b) == n and batch > 1)], M.to_bytes(_form(a, r, mont)) + M.to_bytes(_form(b, r, mont)))
    return rc, _back(got, r, mont)


def run_combine(exe, tmp, r, rows, coeffs, mont):
    flat = [x for row in rows for x in row]
    rc, got = _call(exe, tmp, ["combine", len(rows[0]), len(rows), int(mont)], M.to_bytes(coeffs) + M.to_bytes(_form(flat, r, mont)))
    return rc, _back(got, r, mont)


def run_powers(exe, tmp, r, g, c, n, mont):
    rc, got = _call(exe, tmp, ["powers", n, int(mont)], M.to_bytes([g, c]))
    return rc, _back(got, r, mont)


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frpoly_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _inputs(r, n, rnd):
    last = [0] * n
    last[n - 1] = r - 2
    return {"all 0": [0] * n, "all r - 1": [r - 1] * n, "a single nonzero in the last place": last, "random": [rnd.randrange(r) for _ in range(n)]}


def _points(r, rnd):
    return (0, 1, r - 1, rnd.randrange(2, r - 1))


# one, two and three levels; rows that end inside a tile; a tile that is no multiple of a lane's four elements; the carry-in in a slot of its
# own (tile 2, 6), at a lane's first slot (tile 4) and behind the last lane (tile 1024)
SHAPES = [(1, 3, T), (5, 1, T), (T + 1, 2, T), (2 * T + 3, 1, T), (7, 2, 2), (16, 1, 4), (17, 3, 4), (41, 1, 6), (73, 1, 6)]


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n,batch,tile", SHAPES)
def test_eval_and_divide_against_the_model(harness, n, batch, tile, mont):
    field, exe, tmp = harness
    r = _r(field)
    rnd = rng(31 + n)
    for name, a in _inputs(r, n * batch, rnd).items():
        if tile == T and n > T and name == "all 0":
            continue
        for z in _points(r, rnd):
            rows = M.rows_of(a, batch)
            want = [M.divide(row, z, r) for row in rows]
            rc, values = run_eval(exe, tmp, r, a, z, batch, tile, mont)
            assert rc == 0 and values == [v for _, v in want], (field, name, z)
            rc, got, values = run_divide(exe, tmp, r, a, z, batch, tile, mont)
            assert rc == 0 and got == [x for q, _ in want for x in q] and values == [v for _, v in want], (field, name, z)
            assert all(got[(v + 1) * n - 1] == 0 for v in range(batch))


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n,batch,tile", [(1, 2, T), (T + 1, 2, T), (2 * T + 1, 1, T), (7, 3, 2), (41, 2, 6)])
def test_dot_against_the_model(harness, n, batch, tile, mont):
    field, exe, tmp = harness
    r = _r(field)
    rnd = rng(32 + n)
    for name, a in _inputs(r, n * batch, rnd).items():
        for b in ([r - 1] * (n * batch), [rnd.randrange(r) for _ in range(n * batch)], [rnd.randrange(r) for _ in range(n)]):
            rows, brows = M.rows_of(a, batch), M.rows_of(b, len(b) // n)
            want = [M.dot(row, brows[v % len(brows)], r) for v, row in enumerate(rows)]
            rc, got = run_dot(exe, tmp, r, a, b, batch, tile, mont)
            assert rc == 0 and got == want, (field, name, len(b))


@pytest.mark.parametrize("mont", [False, True])
def test_combine_against_the_model(harness, mont):
    field, exe, tmp = harness
    r = _r(field)
    rnd = rng(33)
    n = 19
    for batch in (1, 2, 8, 9, 17, 256):
        for name, flat in _inputs(r, n * batch, rnd).items():
            rows = M.rows_of(flat, batch)
            for coeffs in ([r - 1] * batch, [rnd.randrange(r) for _ in range(batch)], [(0, 1, r - 1)[k % 3] for k in range(batch)]):
                rc, got = run_combine(exe, tmp, r, rows, coeffs, mont)
                assert rc == 0 and got == M.combine(rows, coeffs, r), (field, batch, name)


@pytest.mark.parametrize("mont", [False, True])
def test_powers_against_the_model(harness, mont):
    field, exe, tmp = harness
    r = _r(field)
    rnd = rng(34)
    for n in (1, 4, 5, 63, 64, 65, 4 * 256 + 3, 4 * 4096 + 1):  # one, two, three and four windows of the lane's number
        for g in _points(r, rnd):
            for c in (1, r - 1, rnd.randrange(r)) + ((0,) if n == 5 else ()):
                rc, got = run_powers(exe, tmp, r, g, c, n, mont)
                assert rc == 0 and got == M.powers(g, n, r, c), (field, n, g, c)


def test_the_number_of_levels():
    """what plan_levels gives at the sizes the GPU tests name"""
    def levels(n, t):
        k = 1
        while -(-n // t) > 1:
            n, k = -(-n // t), k + 1
        return k

    assert levels(T, T) == 1 and levels(T + 1, T) == 2 and levels(T * T, T) == 2 and levels(T * T + 1, T) == 3
    assert [levels(n, t) for t, n in ((2, 7), (4, 16), (4, 17), (6, 41), (8, 73))] == [3, 2, 3, 3, 3]


def test_a_value_not_below_r_is_reported(harness):
    field, exe, tmp = harness
    r = _r(field)
    a = [3] * 40
    assert run_divide(exe, tmp, r, a, 5, 1, 8, False)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        a[17] = bad
        assert run_eval(exe, tmp, r, a, 5, 1, 8, False)[0] == 3, hex(bad)
        assert run_divide(exe, tmp, r, a, 5, 2, 8, False)[0] == 3
        assert run_divide(exe, tmp, r, a, 5, 1, T, False)[0] == 3  # (one level: the suffix scan reads the data first)
        assert run_dot(exe, tmp, r, a, [1] * 40, 1, 8, False)[0] == 3 and run_dot(exe, tmp, r, [1] * 40, a, 1, 8, False)[0] == 3
        assert run_combine(exe, tmp, r, [[1] * 40, a], [2, 3], False)[0] == 3


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the slots, the levels, the tables and the data; shifts)"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r = _r(field)
    rnd = rng(39)
    for n, batch, tile in ((T + 5, 1, T), (73, 2, 8), (7, 3, 2)):
        a = [rnd.randrange(r) for _ in range(n * batch)]
        a[0], a[-1] = 0, r - 1
        z = rnd.randrange(r)
        want = [M.divide(row, z, r) for row in M.rows_of(a, batch)]
        rc, got, values = run_divide(exe, tmp_path, r, a, z, batch, tile, True)
        assert rc == 0 and got == [x for q, _ in want for x in q] and values == [v for _, v in want]
        assert run_eval(exe, tmp_path, r, a, z, batch, tile, True) == (0, values)
        assert run_dot(exe, tmp_path, r, a, a[:n], batch, tile, True) == (0, [M.dot(row, a[:n], r) for row in M.rows_of(a, batch)])
        rows = M.rows_of(a, batch)
        assert run_combine(exe, tmp_path, r, rows, list(range(2, 2 + batch)), True) == (0, M.combine(rows, list(range(2, 2 + batch)), r))
        assert run_powers(exe, tmp_path, r, z, 7, n, True) == (0, M.powers(z, n, r, 7))
