"""libmsm_frmat.so's product on the CPU: a stand-alone program (tests/host_harness/frmat_harness.cpp) that runs the checks, the transposed structure,
the levels and the tiles' slots of csrc/frmat_plan.h and, lane by lane and tile by tile, the functions the kernels call (csrc/frmat_kernels.h) --
with the tile passed in --, compiled with g++ -DFQ_CHECK so that every limb and value bound of csrc/fq29.h is asserted, against the pure-Python
model (tests/frmat_model.py).  The five fields, both data forms, both directions.  Host logic only."""
import os
import struct
import subprocess

import pytest

from tests import frmat_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
T = 1024  # the design's tile (csrc/frmat_kernels.h: FRMAT_TILE)
R_MODEL = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
def test_model_products_and_transpose():
    r = R_MODEL
    # [[1, 2, 0], [0, 0, 0], [3, 0, 4 + 5]] with the last row's column 2 given twice, out of order
    ptr, idx, val = [0, 2, 2, 5], [1, 0, 2, 0, 2], [2, 1, 4, 3, 5]
    assert M.matvec(3, 3, ptr, idx, val, [1, 10, 100], r) == [21, 0, 903]
    assert M.matvec(3, 3, ptr, idx, val, [1, 10, 100], r, transpose=True) == [301, 2, 900]
    t_ptr, t_idx, t_val = M.transpose_csr(3, 3, ptr, idx, val)
    assert (t_ptr, t_idx, t_val) == ([0, 2, 3, 5], [0, 2, 0, 2, 2], [1, 3, 2, 4, 5])
    assert M.matvec(3, 3, t_ptr, t_idx, t_val, [1, 10, 100], r) == [301, 2, 900]
    assert M.matvec(1, 2, [0, 2], [0, 1], [r - 1, r - 1], [r - 1, 2], r) == [(1 - 2) % r]
    rnd = rng(3)
    for name in M.SMALL_SHAPES:  # <M x, w> = <x, M^T w>
        _, rows, cols, ptr, idx = M.shape(name, rnd)
        val = [rnd.randrange(r) for _ in idx]
        x, w = [rnd.randrange(r) for _ in range(cols)], [rnd.randrange(r) for _ in range(rows)]
        lhs = sum(a * b for a, b in zip(M.matvec(rows, cols, ptr, idx, val, x, r), w)) % r
        assert lhs == sum(a * b for a, b in zip(x, M.matvec(rows, cols, ptr, idx, val, w, r, transpose=True))) % r


def test_model_levels():
    rnd = rng(4)
    for name, want in M.LEVELS.items():
        tile, _, _, ptr, _ = M.shape(name, rnd)
        assert M.levels(ptr, tile) == want, name
    assert M.levels([0, (1 << 20) + 5] + [(1 << 20) + 5 + k for k in range(1, 1025)], T) == 3  # the large GPU case: 1025 partials, then 2


# ---- the program -----------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frmat_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frt_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frmat_harness.cpp"), "-o", exe])
    return exe


def _words(vals):
    return struct.pack("<%dI" % len(vals), *vals)


def run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val, x, mont=False, transpose=False, y_len=None):
    """-> (status, launches, levels, y) -- y plain integers, y_len of them"""
    out_len = cols if transpose else rows
    y_len = out_len if y_len is None else y_len
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(_words(ptr) + _words(idx) + M.to_bytes(val) + M.to_bytes(M.mont(x, r) if mont else x))
    if fout.exists():
        fout.unlink()
    p = subprocess.run([exe, "mul"] + [str(a) for a in (rows, cols, len(idx), tile, int(transpose), y_len)] + [str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3, 4), (p.returncode, p.stderr[-500:])
    if p.returncode == 4 or not fout.exists():
        return p.returncode, None, None, None
    raw = fout.read_bytes()
    launches, levels = struct.unpack("<2I", raw[:8])
    y = M.from_bytes(raw[32:])
    return p.returncode, launches, levels, (M.mont(y, r, back=True) if mont else y)


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frmat_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _values(r, rnd, n):
    return [(0, 1, r - 1)[rnd.randrange(3)] if rnd.randrange(4) == 0 else rnd.randrange(r) for _ in range(n)]


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("name", M.DESIGN_SHAPES + M.SMALL_SHAPES)
def test_product_against_the_model(harness, name, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(51)
    tile, rows, cols, ptr, idx = M.shape(name, rnd)
    val = _values(r, rnd, len(idx))
    for transpose in (False, True):
        x = _values(r, rnd, rows if transpose else cols)
        out_len = cols if transpose else rows
        rc, launches, levels, y = run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val, x, mont, transpose, y_len=out_len + 3)
        assert rc == 0 and y == M.matvec(rows, cols, ptr, idx, val, x, r, transpose) + [0, 0, 0], (field, name, transpose)
        t_ptr = M.transpose_csr(rows, cols, ptr, idx, val)[0] if transpose else ptr
        assert levels == M.levels(t_ptr, tile) and launches == levels + 1, (field, name, transpose)
        if not transpose and name in M.LEVELS:
            assert levels == M.LEVELS[name], (field, name)


@pytest.mark.parametrize("mont", [False, True])
def test_a_full_tile_of_one_row_at_the_lazy_bound(harness, mont):
    """1024 entries of one row: every lane adds four products lazily (the static_assert of csrc/frmat_kernels.h), the scan adds 256 lane sums;
    all values and all of x r - 1 (the largest products), and all 0, with the program's bound checks on"""
    field, exe, tmp = harness
    r = _r(field)
    for v, xv in ((r - 1, r - 1), (0, 0), (r - 1, 0), (1, r - 1)):
        rc, launches, levels, y = run_mul(exe, tmp, r, T, 1, 3, [0, T], [k % 3 for k in range(T)], [v] * T, [xv] * 3, mont)
        assert (rc, launches, levels) == (0, 2, 1) and y == [T * v * xv % r], (field, v, xv)


def test_a_value_not_below_r_is_reported(harness):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(52)
    tile, rows, cols, ptr, idx = M.shape("9x7 with empty rows", rnd)
    idx = [c % 6 for c in idx]  # column 6 is referenced by no entry
    val = [rnd.randrange(r) for _ in idx]
    x = [rnd.randrange(r) for _ in range(cols)]
    assert run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val, x)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        for at in (0, len(idx) - 1):
            assert run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val[:at] + [bad] + val[at + 1:], x)[0] == 3, hex(bad)
        for at in sorted(set(idx))[:2] + [idx[-1]]:
            assert run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val, x[:at] + [bad] + x[at + 1:])[0] == 3, (hex(bad), at)
        rc, _, _, y = run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val, x[:6] + [bad])  # a column nobody references is not read
        assert rc == 0 and y == M.matvec(rows, cols, ptr, idx, val, x, r)
        w = [rnd.randrange(r) for _ in range(rows)]  # transposed: x has a scalar per row, and the empty rows' are not read
        assert run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val, [bad] + w[1:], transpose=True)[0] == 0
        assert run_mul(exe, tmp, r, tile, rows, cols, ptr, idx, val, w[:2] + [bad] + w[3:], transpose=True)[0] == 3


def test_the_plan_rejects_a_bad_structure(harness):
    field, exe, tmp = harness
    r = _r(field)
    ptr, idx, val, x = [0, 2, 3], [0, 1, 1], [1, 2, 3], [4, 5]
    assert run_mul(exe, tmp, r, 4, 2, 2, ptr, idx, val, x)[0] == 0
    assert run_mul(exe, tmp, r, 4, 2, 2, ptr, [0, 2, 1], val, x)[0] == 4  # a column >= cols
    assert run_mul(exe, tmp, r, 4, 2, 2, ptr, [0, 1, 0xffffffff], val, x)[0] == 4
    assert run_mul(exe, tmp, r, 4, 2, 2, [0, 4, 3], idx, val, x)[0] == 4  # a decreasing row_ptr (whose last word is nnz)
    assert run_mul(exe, tmp, r, 4, 3, 2, [0, 2, 1, 3], idx, val, x)[0] == 4
    assert run_mul(exe, tmp, r, 4, 2, 2, [1, 2, 3], idx, val, x)[0] == 4  # row_ptr[0] != 0
    assert run_mul(exe, tmp, r, 4, 2, 2, [0, 2, 2], idx, val, x)[0] == 4  # row_ptr[rows] != nnz
    assert run_mul(exe, tmp, r, 4, 2, 2, [0, 2, 4], idx, val, x)[0] == 4
    assert run_mul(exe, tmp, r, 4, 2, 2, ptr, [0, 2, 1], [r, 2, 3], x)[0] == 4  # both faults: the structure's is reported


def test_the_transposed_structure_is_the_models(harness):
    field, exe, tmp = harness
    rnd = rng(53)
    for name in M.SMALL_SHAPES + ("one row of 2050", "1x1 empty"):
        _, rows, cols, ptr, idx = M.shape(name, rnd)
        fin, fout = tmp / "t_in.bin", tmp / "t_out.bin"
        fin.write_bytes(_words(ptr) + _words(idx))
        subprocess.check_call([exe, "transpose", str(rows), str(cols), str(len(idx)), str(fin), str(fout)])
        raw = fout.read_bytes()
        got = list(struct.unpack("<%dI" % (len(raw) // 4), raw))
        t_ptr, t_idx, t_from = M.transpose_csr(rows, cols, ptr, idx, list(range(len(idx))))  # (the values are the entries' numbers)
        assert got == t_ptr + t_idx + t_from, name


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the slots, the flags, the levels, the partials and
    the data; shifts) on three of the small shapes, both directions"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r, rnd = _r(field), rng(54)
    for name in ("9x7 with empty rows", "one row of 70", "random tile 2"):
        tile, rows, cols, ptr, idx = M.shape(name, rnd)
        val = _values(r, rnd, len(idx))
        for transpose in (False, True):
            x = _values(r, rnd, rows if transpose else cols)
            rc, _, _, y = run_mul(exe, tmp_path, r, tile, rows, cols, ptr, idx, val, x, True, transpose)
            assert rc == 0 and y == M.matvec(rows, cols, ptr, idx, val, x, r, transpose), (name, transpose)
