"""libmsm_frgate.so's call on the CPU: what the pure-Python model (tests/frgate_model.py) must satisfy, and a stand-alone program
(tests/host_harness/frgate_harness.cpp) that runs the checks, offsets and term records of csrc/frgate_plan.h and, element by element, the function
the kernel calls (csrc/frgate_kernels.h), compiled with g++ -DFQ_CHECK so that every limb and value bound of csrc/fq29.h is asserted, against that
model.  The five fields, both data forms.  Host logic only."""
import os
import subprocess

import pytest

from tests import frgate_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
MONT, ACC = 2, 4  # MSM_FRGATE_MONT256, MSM_FRGATE_ACCUMULATE


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
R_MODEL = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _root(log_n, r=R_MODEL):
    return pow(5, (r - 1) >> log_n, r)


def test_model_apply_is_the_definition():
    r, rnd = R_MODEL, rng(1)
    n = 8
    rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(3)]
    assert M.apply(rows, [(1, (0,))], n, 1, None, None, r) == rows[0]
    assert M.apply(rows, [(1, ((0, 1),))], n, 1, None, None, r) == rows[0][1:] + rows[0][:1]
    assert M.apply(rows, [(1, ((0, -1),))], n, 1, None, None, r) == rows[0][-1:] + rows[0][:-1]
    assert M.apply(rows, [(1, ((0, 1),))], n, 2, None, None, r) == rows[0][2:] + rows[0][:2]
    assert M.apply(rows, [(1, ((0, 9),))], n, 1, None, None, r) == rows[0][1:] + rows[0][:1]
    assert M.apply(rows, [(3, (0, 1)), (r - 1, (2,))], n, 1, [2, 5], rows[1], r) == \
        [(rows[1][i] + (2, 5)[i % 2] * (3 * rows[0][i] * rows[1][i] - rows[2][i])) % r for i in range(n)]


def test_model_quotient_of_a_satisfied_and_of_a_broken_circuit():
    """columns a, b, c with a b = c and c = a(omega X) on all of H, two challenges: the quotient has degree below n, t(z) Z_H(z) is the expression at z,
    and one changed witness element leaves a remainder in the top coefficients"""
    r, rnd = R_MODEL, rng(7)
    log_n, log_ext = 3, 2
    n, big = 1 << log_n, 1 << (log_n + log_ext)
    wn, wbig = _root(log_n), _root(log_n + log_ext)
    assert pow(wbig, 1 << log_ext, r) == wn
    a, b, c = [0] * n, [rnd.randrange(1, r) for _ in range(n)], [0] * n
    a[0] = rnd.randrange(1, r)
    for i in range(n):
        if i == n - 1:
            b[i] = a[0] * pow(a[i], r - 2, r) % r  # the wrap closes: c[n - 1] = a[0]
        c[i] = a[i] * b[i] % r
        if i < n - 1:
            a[i + 1] = c[i]
    cols = [M.interpolate(v, wn, r) for v in (a, b, c)]
    al0, al1 = rnd.randrange(r), rnd.randrange(r)
    terms = [(al0, (0, 1)), ((r - al0) % r, (2,)), (al1, (2,)), ((r - al1) % r, ((0, 1),))]
    t = M.quotient(cols, terms, log_n, log_ext, 7, wbig, r)
    assert len(t) == big and not any(t[n:]) and any(t[:n])
    z = rnd.randrange(r)
    va, vb, vc, vaw = (M.evaluate(cols[0], z, r), M.evaluate(cols[1], z, r), M.evaluate(cols[2], z, r), M.evaluate(cols[0], z * wn % r, r))
    assert M.evaluate(t, z, r) * (pow(z, n, r) - 1) % r == (al0 * (va * vb - vc) + al1 * (vc - vaw)) % r
    c[3] = (c[3] + 1) % r
    cols[2] = M.interpolate(c, wn, r)
    assert any(M.quotient(cols, terms, log_n, log_ext, 7, wbig, r)[n:])


# ---- the program -----------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frgate_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frg_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frgate_harness.cpp"), "-o", exe])
    return exe


def _strided(rows, stride, filler):
    out = []
    for v, row in enumerate(rows):
        out += list(row) + ([filler] * (stride - len(row)) if v + 1 < len(rows) else [])
    return out


def run_apply(exe, tmp, r, rows, terms, n, step=1, scale=None, acc=None, stride=None, mont=False, filler=1, raw_terms=None):
    """-> (status, out as plain integers); rows, scale, acc: plain integers, put into the data's form here; the gaps between rows hold `filler`"""
    stride = n if stride is None else stride
    form = (lambda v: M.mont(v, r)) if mont else list
    flat = _strided([form(row[:n]) for row in rows], stride, filler)
    before = form(acc) if acc is not None else [(1 << 256) - 1] * n  # (without ACCUMULATE the output is not read: all ones is not below r)
    tb = M.term_bytes(terms) if raw_terms is None else raw_terms
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(tb + M.to_bytes(flat) + M.to_bytes(form(scale) if scale is not None else []) + M.to_bytes(before))
    flags = (MONT if mont else 0) | (ACC if acc is not None else 0)
    p = subprocess.run([exe, "apply"] + [str(x) for x in (n, len(rows), stride, step, len(scale) if scale is not None else 0, flags, len(tb) // 100, fin, fout)],
                       capture_output=True, text=True)
    assert p.returncode in (0, 3, 4), (p.returncode, p.stderr[-500:])
    if p.returncode == 4:
        return 4, None
    got = M.from_bytes(fout.read_bytes())
    return p.returncode, M.mont(got, r, back=True) if mont else got


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frgate_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _rows(r, rnd, batch, n):
    rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(batch)]
    for row in rows:  # planted 0 / 1 / r - 1
        for v in (0, 1, r - 1):
            row[rnd.randrange(n)] = v
    return rows


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n", [1, 2, 4, 64, 512])
def test_apply_against_the_model(harness, n, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(60 + n)
    batch = 4
    rows = _rows(r, rnd, batch, max(n, 4))
    rows = [row[:n] for row in rows]
    row = lambda: rnd.randrange(batch)  # noqa: E731
    kinds = {
        "degree 1": [(rnd.randrange(r), (row(),))],
        "degree 8": [(r - 1, tuple((row(), rot) for rot in (0, 1, -1, 3, -3, 0, 2, 5)))],
        "a row repeated with different rotations": [(1, ((0, 0), (0, 1), (0, -1), (0, 0)))],
        "coefficients 0, 1, r - 1": [(0, (0, 1)), (1, ((batch - 1, 1),)), (r - 1, (row(), (row(), -3)))],
        "33 terms": [((1, r - 1, rnd.randrange(r))[j % 3], tuple((row(), rnd.randrange(-3, 4)) for _ in range(1 + j % 3))) for j in range(33)],
    }
    for name, terms in kinds.items():
        for step in sorted({1, min(4, n), n}):
            rc, got = run_apply(exe, tmp, r, rows, terms, n, step=step, mont=mont)
            assert rc == 0 and got == M.apply(rows, terms, n, step, None, None, r), (field, n, name, step)
        for scale_len in sorted({1, min(4, n), n}):
            scale = [(0, 1, r - 1, rnd.randrange(r))[j % 4] for j in range(scale_len)]
            acc = [(r - 1, 0, rnd.randrange(r))[j % 3] for j in range(n)]
            rc, got = run_apply(exe, tmp, r, rows, terms, n, step=min(4, n), scale=scale, acc=acc, stride=n + 3, mont=mont)
            assert rc == 0 and got == M.apply(rows, terms, n, min(4, n), scale, acc, r), (field, n, name, scale_len)


@pytest.mark.parametrize("mont", [False, True])
def test_rotations_wrap_any_number_of_times(harness, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(61)
    n = 16
    rows = _rows(r, rnd, 2, n)
    for rot, step in ((17, 1), (-17, 1), (5, 4), (-5, 4), (1, 16), (2 ** 31 - 1, 16), (-2 ** 31, 15), (2 ** 31 - 1, 7), (-2 ** 31, 1)):
        terms = [(1, ((0, rot), (1, -(rot // 2))))]
        rc, got = run_apply(exe, tmp, r, rows, terms, n, step=step, mont=mont)
        assert rc == 0 and got == M.apply(rows, terms, n, step, None, None, r), (field, rot, step)
        out = subprocess.run([exe, "offset", str(rot), str(step), str(n)], capture_output=True, text=True, check=True).stdout
        assert int(out) == rot * step % n


@pytest.mark.parametrize("mont", [False, True])
def test_apply_at_the_lazy_bounds(harness, mont):
    """64 terms of degree 8 with every element, coefficient and scale r - 1, accumulated onto r - 1 -- and the other extreme values --, with the
    program's bound checks on: the lane's sum reaches its largest value before each tidy"""
    field, exe, tmp = harness
    r = _r(field)
    n = 4
    for value in (r - 1, 1, 0):
        rows = [[value] * n, [r - 1] * n]
        for num_terms in (1, 32, 33, 64):
            terms = [(r - 1, tuple((j % 2, j - 3) for j in range(8)))] * num_terms
            for scale, acc in ((None, None), ([r - 1], [r - 1] * n), ([r - 1] * n, None)):
                rc, got = run_apply(exe, tmp, r, rows, terms, n, scale=scale, acc=acc, mont=mont)
                assert rc == 0 and got == M.apply(rows, terms, n, 1, scale, acc, r), (field, value, num_terms)


def test_a_value_not_below_r_is_reported_where_it_is_read(harness):
    field, exe, tmp = harness
    r = _r(field)
    n, stride = 8, 11
    rows = [[3] * n, [4] * n, [5] * n]
    terms = [(1, (0, (2, 1)))]  # row 1 is not named
    assert run_apply(exe, tmp, r, rows, terms, n, stride=stride)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        assert run_apply(exe, tmp, r, rows, terms, n, stride=stride, filler=bad)[0] == 0  # behind n: not read
        for at in (0, n - 1):
            rows[1][at] = bad
            assert run_apply(exe, tmp, r, rows, terms, n, stride=stride)[0] == 0  # an unnamed row: not read
            rows[1][at] = 4
            rows[2][at] = bad
            assert run_apply(exe, tmp, r, rows, terms, n, stride=stride)[0] == 3
            rows[2][at] = 5
            scale = [1] * 4
            scale[at % 4] = bad
            assert run_apply(exe, tmp, r, rows, terms, n, stride=stride, scale=scale)[0] == 3
            acc = [2] * n
            acc[at] = bad
            assert run_apply(exe, tmp, r, rows, terms, n, stride=stride, acc=acc)[0] == 3
    # (without ACCUMULATE run_apply fills the output with all ones, which is not below r: every call above that returned 0 did not read it)


def test_the_plan_refuses_what_is_out_of_range(harness):
    field, exe, tmp = harness
    r = _r(field)
    rows = [[1] * 8, [2] * 8]
    good = [(1, (0, 1))]
    assert run_apply(exe, tmp, r, rows, good, 8)[0] == 0
    assert run_apply(exe, tmp, r, rows, good, 8, step=0)[0] == 4
    assert run_apply(exe, tmp, r, rows, good, 8, step=9)[0] == 4
    assert run_apply(exe, tmp, r, rows, good, 8, scale=[1, 1, 1])[0] == 4  # not a power of two
    assert run_apply(exe, tmp, r, [[1] * 6], [(1, (0,))], 6)[0] == 4  # n not a power of two
    assert run_apply(exe, tmp, r, rows, [(1, (0, 2))], 8)[0] == 4  # a row outside the batch
    assert run_apply(exe, tmp, r, rows, [(r, (0,))], 8)[0] == 4  # a coefficient not below r
    assert run_apply(exe, tmp, r, rows, good * 65, 8)[0] == 4
    assert run_apply(exe, tmp, r, rows, [], 8)[0] == 4
    assert run_apply(exe, tmp, r, [[1] * 8] * 33, good, 8)[0] == 4  # more than MAX_ROWS rows
    zero_degree = (1).to_bytes(32, "little") + bytes(68)
    nine = (1).to_bytes(32, "little") + (9).to_bytes(4, "little") + bytes(64)
    assert run_apply(exe, tmp, r, rows, None, 8, raw_terms=zero_degree)[0] == 4
    assert run_apply(exe, tmp, r, rows, None, 8, raw_terms=nine)[0] == 4


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the rows, the term records and the scale; the offset
    arithmetic of the largest rotations)"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r = _r(field)
    rnd = rng(69)
    for n, batch, stride in ((512, 2, 512), (64, 32, 67), (1, 1, 1)):
        rows = _rows(r, rnd, batch, max(n, 4))
        rows = [row[:n] for row in rows]
        terms = [(rnd.randrange(r), ((0, 2 ** 31 - 1), (batch - 1, -2 ** 31), 0)), (r - 1, ((batch - 1, -1),))] + [(1, ((0, j),)) for j in range(40)]
        scale = [rnd.randrange(r) for _ in range(min(4, n))]
        acc = [rnd.randrange(r) for _ in range(n)]
        assert run_apply(exe, tmp_path, r, rows, terms, n, step=n, stride=stride, mont=True) == (0, M.apply(rows, terms, n, n, None, None, r))
        assert run_apply(exe, tmp_path, r, rows, terms, n, step=min(3, n), scale=scale, acc=acc, stride=stride, mont=True) == \
            (0, M.apply(rows, terms, n, min(3, n), scale, acc, r))
