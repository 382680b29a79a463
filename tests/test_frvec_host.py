"""libmsm_frvec.so's calls on the CPU: a stand-alone program (tests/host_harness/frvec_harness.cpp) runs the constants and levels of
csrc/frvec_plan.h and, lane by lane, the functions the kernels call (csrc/frvec_kernels.h) -- the map, the forward and backward sweeps of the
inverse with its product tree and Fermat chain, the fold and scan phases with the tile passed in -- compiled with g++ -DFQ_CHECK so that every limb
and value bound of csrc/fq29.h is asserted, against the pure-Python model (tests/frvec_model.py).  All four fields, both data forms.  Host logic only."""
import os
import subprocess

import pytest

from tests import frvec_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "pallas", "vesta", "bls12_381")
T = 1024  # the design's tile (csrc/frvec_kernels.h: FRVEC_TILE)


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frvec_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frv_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frvec_harness.cpp"), "-o", exe])
    return exe


def _call(exe, tmp, args, payload):
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(payload)
    p = subprocess.run([exe] + [str(a) for a in args] + [str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3), (p.returncode, p.stderr[-500:])
    return p.returncode, M.from_bytes(fout.read_bytes())


def _form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def run_map(exe, tmp, r, op, a, b, c, mont):
    """a, b, c: plain values; b / c an integer for a constant.  The constants go in canonical, the vectors in the data's form."""
    n = len(a)
    bc, cc = isinstance(b, int), isinstance(c, int)
    head = M.to_bytes([b if bc else 0, c if cc else 0])
    vecs = [_form(a, r, mont), [0] * n if bc else _form(b, r, mont), [0] * n if cc or c is None else _form(c, r, mont)]
    rc, got = _call(exe, tmp, ["map", n, M.OPS[op], int(bc), int(cc), int(mont)], head + b"".join(M.to_bytes(v) for v in vecs))
    return rc, M.mont(got, r, back=True) if mont else got


def run_inverse(exe, tmp, r, a, tile, mont):
    rc, got = _call(exe, tmp, ["inverse", len(a), tile, int(mont)], M.to_bytes(_form(a, r, mont)))
    return rc, M.mont(got, r, back=True) if mont else got


def run_scan(exe, tmp, r, a, batch, tile, op, exclusive, mont):
    n = len(a) // batch
    rc, got = _call(exe, tmp, ["scan", n, batch, tile, M.SCANS[op], int(exclusive), int(mont)], M.to_bytes(_form(a, r, mont)))
    got = M.mont(got, r, back=True) if mont else got
    return rc, got[:len(a)], got[len(a):]


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frvec_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _inputs(r, n, tile, rnd):
    """the vectors the bounds are asserted on: the extremes, a single nonzero, a zero at each end of every tile, random values"""
    ends = [rnd.randrange(1, r) for _ in range(n)]
    for k in range(0, n, tile):
        ends[k] = 0
        ends[min(k + tile, n) - 1] = 0
    single = [0] * n
    single[n // 2] = r - 2
    return {"all 0": [0] * n, "all r - 1": [r - 1] * n, "all 1": [1] * n, "single nonzero": single, "zeros at the ends of a tile": ends,
            "random": [rnd.randrange(r) for _ in range(n)]}


@pytest.mark.parametrize("mont", [False, True])
def test_map_against_the_model(harness, mont):
    field, exe, tmp = harness
    r = _r(field)
    n = 67
    rnd = rng(21)
    for name, a in _inputs(r, n, 16, rnd).items():
        b = [rnd.randrange(r) for _ in range(n)]
        c = [rnd.randrange(r) for _ in range(n)]
        b[0], b[1], b[2], c[0], c[1], c[2] = 0, 1, r - 1, r - 1, 0, 1
        for op in M.MAPS:
            three = op in ("mul_add", "mul_sub")
            for bb in (b, r - 1, rnd.randrange(r)) + ((0, 1) if name == "random" else ()):
                for cv in ((c, r - 1) + ((0, rnd.randrange(r)) if name == "random" else ()) if three else (None,)):
                    rc, got = run_map(exe, tmp, r, op, a, bb, cv, mont)
                    assert rc == 0 and got == M.map_op(op, a, bb, cv, r), (field, name, op, isinstance(bb, int), isinstance(cv, int))
            rc, got = run_map(exe, tmp, r, op, a, a, a if three else None, mont)  # (the same vector in every place)
            assert rc == 0 and got == M.map_op(op, a, a, a if three else None, r), (field, name, op)


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n,tile", [(1, T), (5, T), (T, T), (2 * T + 3, T), (73, 8), (41, 6)])
def test_inverse_against_the_model(harness, n, tile, mont):
    """the sweeps, the product tree and the Fermat chain; a tile that is no multiple of a lane's four elements; 1 / 0 = 0 beside its neighbours"""
    field, exe, tmp = harness
    r = _r(field)
    for name, a in _inputs(r, n, tile, rng(22 + n)).items():
        rc, got = run_inverse(exe, tmp, r, a, tile, mont)
        assert rc == 0 and got == M.inverse(a, r), (field, name, n, tile)


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n,batch,tile", [(1, 3, T), (T + 1, 2, T), (2 * T + 3, 1, T), (73, 1, 8), (21, 3, 4), (7, 2, 2), (41, 1, 6)])
def test_scans_against_the_model(harness, n, batch, tile, mont):
    """one, two and three levels of totals, rows that end inside a tile, both ops, inclusive and exclusive, the row totals"""
    field, exe, tmp = harness
    r = _r(field)
    for name, a in _inputs(r, n * batch, tile, rng(23 + n)).items():
        if tile == T and name not in ("random", "all r - 1", "zeros at the ends of a tile"):
            continue
        for op in ("sum", "product"):
            for exclusive in (False, True):
                rc, got, totals = run_scan(exe, tmp, r, a, batch, tile, op, exclusive, mont)
                want, want_totals = M.scan(a, op, exclusive, r, batch)
                assert rc == 0 and got == want and totals == want_totals, (field, name, op, exclusive)


def test_the_number_of_levels():
    """what plan_levels gives at the sizes the GPU tests name: t t + t + 1 elements need a second level of totals"""
    def levels(n, t):
        k = 1
        while -(-n // t) > 1:
            n, k = -(-n // t), k + 1
        return k

    assert levels(T, T) == 1 and levels(T + 1, T) == 2 and levels(T * T, T) == 2 and levels(T * T + 1, T) == 3
    for t in (2, 4, 8):
        assert levels(t * t + t + 1, t) == 3


def test_a_value_not_below_r_is_reported(harness):
    field, exe, tmp = harness
    r = _r(field)
    a = [3] * 40
    assert run_inverse(exe, tmp, r, a, 8, False)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        a[17] = bad
        assert run_inverse(exe, tmp, r, a, 8, False)[0] == 3, hex(bad)
        assert run_scan(exe, tmp, r, a, 1, 8, "product", False, False)[0] == 3
        assert run_scan(exe, tmp, r, a, 1, 8, "sum", True, False)[0] == 3
        assert run_map(exe, tmp, r, "add", a, 1, None, False)[0] == 3
        assert run_map(exe, tmp, r, "mul", [1] * 40, a, None, False)[0] == 3
        assert run_map(exe, tmp, r, "mul_add", [1] * 40, 2, a, False)[0] == 3


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the tree, the slots, the levels and the data; shifts)"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r = _r(field)
    rnd = rng(29)
    for n, batch, tile in ((T + 5, 1, T), (73, 2, 8), (7, 3, 2)):
        a = [rnd.randrange(r) for _ in range(n * batch)]
        a[0], a[-1] = 0, r - 1
        rc, got = run_inverse(exe, tmp_path, r, a, tile, True)
        assert rc == 0 and got == M.inverse(a, r)
        for op in ("sum", "product"):
            rc, got, totals = run_scan(exe, tmp_path, r, a, batch, tile, op, True, True)
            assert rc == 0 and (got, totals) == M.scan(a, op, True, r, batch)
        rc, got = run_map(exe, tmp_path, r, "mul_sub", a, a[::-1], 5, True)
        assert rc == 0 and got == M.map_op("mul_sub", a, a[::-1], 5, r)
