"""libmsm_frhash.so's Poseidon2 on the CPU: the two forms of the definition (tests/frhash2_model.py: structured, and dense with explicit M_E and
M_I = J + diag(mu)) against each other, and a stand-alone program (tests/host_harness/frhash2_harness.cpp) that runs the plan of
csrc/frhash_plan.h and, lane by lane in serial order, the functions the kernels call (csrc/frhash_kernels.h) on a slab of the size a Poseidon2
launch requests, compiled with g++ -DFQ_CHECK so that every limb and value bound is asserted, against the model: permutations and sponges, the
five fields, both data forms, t in {2, 3, 4, 8, 12}, R_P = 0, and the pattern that reaches the bounds.  Host logic only."""
import os
import subprocess

import pytest

from tests import frhash2_model as M2
from tests import frhash_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
WIDTHS = M2.WIDTHS


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_external_matrices_are_the_papers():
    assert M2.external_matrix(2) == [[2, 1], [1, 2]] and M2.external_matrix(3) == [[2, 1, 1], [1, 2, 1], [1, 1, 2]]
    assert M2.external_matrix(4) == [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]
    m8 = M2.external_matrix(8)
    assert m8[0] == [10, 14, 2, 6, 5, 7, 1, 3] and m8[5] == [4, 6, 1, 1, 8, 12, 2, 2]
    m12 = M2.external_matrix(12)
    assert all(m12[i][j] == (2 if i // 4 == j // 4 else 1) * M2.M4[i % 4][j % 4] for i in range(12) for j in range(12))
    assert max(sum(row) for row in m12) == 64  # (a row sums to 4 x 16: the factor the kernel's bounds are about)
    x = [3, 1, 4, 1]
    assert M2.m4_chain(x, 1 << 61) == [sum(m * v for m, v in zip(row, x)) for row in M2.M4]


def test_model_semantics():
    r = 97
    p = M2.Poseidon2(r, 3, 2, 1, [1, 2, 3, 4, 5, 6, 7], [10, 20, 30])
    ext = lambda s: [(x + sum(s)) % r for x in s]  # noqa: E731
    s = ext([3, 4, 5])
    s = ext([(x + c) ** 5 % r for x, c in zip(s, (1, 2, 3))])
    s[0] = (s[0] + 4) ** 5 % r  # the internal round: ONE constant, the first element alone
    s = [(m * x + sum(s)) % r for m, x in zip((10, 20, 30), s)]
    s = ext([(x + c) ** 5 % r for x, c in zip(s, (5, 6, 7))])
    assert p.permute([3, 4, 5]) == s
    assert p.hash([10], 0, 0, 0) == p.permute([0, 10, 0])[0]  # the sponge is the first model's
    assert p.hash([10, 20, 30], 5, 1, 2) == p.permute([(a + 30) % r for a in p.permute([10, 5, 20])[:1]] + p.permute([10, 5, 20])[1:])[2]
    with pytest.raises(AssertionError):
        M2.Poseidon2(r, 5, 2, 1, [0] * 11, [0] * 5)  # a width Poseidon2 does not define


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("t", WIDTHS)
def test_the_structured_and_the_dense_form_agree(field, t):
    r, rnd = _r(field), rng(900 + t)
    for rf, rp in ((8, 56), (2, 0), (4, 3)):
        a, b = M2.sample(r, t, rf, rp), M2.sample(r, t, rf, rp, dense=True)
        assert a.rc == b.rc and a.mu == b.mu
        for state in [[r - 1] * t, [0] * t] + [[rnd.randrange(r) for _ in range(t)] for _ in range(3)]:
            assert a.permute(state) == b.permute(state), (field, t, rf, rp)
    worst, dense = [M2.Poseidon2, M2.Poseidon2Dense]
    args = (r, t, 8, 56, [r - 1] * (8 * t + 56), [r - 1] * t)
    assert worst(*args).permute([r - 1] * t) == dense(*args).permute([r - 1] * t)


# ---- the program -----------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frhash2_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frh_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frhash2_harness.cpp"), "-o", exe])
    return exe


def _call(exe, tmp, args, data):
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(M.to_bytes(data))
    if fout.exists():
        fout.unlink()
    p = subprocess.run([exe] + [str(a) for a in args] + [str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3, 4), (p.returncode, p.stderr[-500:])
    return p.returncode, M.from_bytes(fout.read_bytes()) if fout.exists() else None


def permute(exe, tmp, p, stored, mont=False, tile=0):
    return _call(exe, tmp, ("permute", p.t, p.full_rounds, p.partial_rounds, 2 if mont else 0, tile, len(stored) // p.t), p.rc + p.mu + list(stored))


def sponge(exe, tmp, p, stored_rows, length, mont=False, tile=0, gap=()):
    stride = len(stored_rows[0]) + len(gap)
    flat = [x for row in stored_rows for x in list(row) + list(gap)]
    flat = flat[:(len(stored_rows) - 1) * stride + length]
    return _call(exe, tmp, ("hash", p.t, p.full_rounds, p.partial_rounds, 2 if mont else 0, tile, len(stored_rows), length, stride, p.capacity_at, p.out_at),
                 p.rc + p.mu + [p.capacity] + flat)


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frhash2_" + request.param)
    return request.param, _build(tmp, request.param), tmp


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("t", WIDTHS)
def test_permutations_against_the_model(harness, t, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(1000 + t)
    states = [[r - 1] * t, [0] * t, [1] + [0] * (t - 1)] + [[rnd.randrange(r) for _ in range(t)] for _ in range(4)]
    flat = [x for s in states for x in s]
    for rf, rp in ((8, 56), (8, 0), (2, 0), (2, 1)):
        p = M2.sample(r, t, rf, rp)
        want = form([x for s in states for x in p.permute(s)], r, mont)
        for tile in (0, 3):  # one workgroup; three lanes to a workgroup, the last one short
            rc, got = permute(exe, tmp, p, form(flat, r, mont), mont, tile)
            assert rc == 0 and got == want, (field, t, rf, rp, mont, tile)


@pytest.mark.parametrize("t", WIDTHS)
def test_the_worst_case_of_the_bounds(harness, t):
    """state, constants, mu and capacity all r - 1: every lazy sum is as large as it gets, under FQ_CHECK; also without internal rounds, with two
    external rounds alone, and at the limits of both round numbers"""
    field, exe, tmp = harness
    r = _r(field)
    for rf, rp in ((8, 56), (8, 0), (2, 0), (16, 128)):
        p = M2.Poseidon2(r, t, rf, rp, [r - 1] * (rf * t + rp), [r - 1] * t, capacity=r - 1, capacity_at=t - 1, out_at=t - 1)
        states = [[r - 1] * t, [0] * t]
        for mont in (False, True):
            rc, got = permute(exe, tmp, p, form([x for s in states for x in s], r, mont), mont)
            assert rc == 0 and got == form([x for s in states for x in p.permute(s)], r, mont), (field, t, rf, rp, mont)
        rows = [[r - 1] * (2 * (t - 1) + 1)] * 2  # (three permutations a row: what a permutation left, plus an absorbed r - 1, enters the next)
        rc, got = sponge(exe, tmp, p, rows, len(rows[0]))
        assert rc == 0 and got == [p.hash(row) for row in rows], (field, t, rf, rp)


@pytest.mark.parametrize("t", WIDTHS)
def test_sponges_against_the_model(harness, t):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(1100 + t)
    conventions = ((0, 0, 0), ((3 << 64) % r, t - 1, 0), ((1 << (t - 1)) - 1, 0, 1 % t))
    for k, length in enumerate(sorted({1, max(1, t - 2), t - 1, t, 2 * (t - 1), 2 * (t - 1) + 1})):
        capacity, capacity_at, out_at = conventions[k % 3]
        p = M2.sample(r, t, capacity=capacity, capacity_at=capacity_at, out_at=out_at)
        rows = [[rnd.randrange(r) for _ in range(length)] for _ in range(3)]
        mont = bool(k & 1)
        rc, got = sponge(exe, tmp, p, [form(row, r, mont) for row in rows], length, mont, tile=2, gap=(r, (1 << 256) - 1))  # (the gap is not read)
        assert rc == 0 and got == form([p.hash(row) for row in rows], r, mont), (field, t, length)


def test_what_the_plan_refuses_and_reports(harness):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(1200)
    p = M2.sample(r, 3)
    states = [rnd.randrange(r) for _ in range(3 * 5)]
    assert permute(exe, tmp, p, states)[0] == 0
    for at in (0, 7, 14):
        assert permute(exe, tmp, p, states[:at] + [r] + states[at + 1:])[0] == 3, at
    for t in (5, 6, 7, 9, 10, 11, 1, 13):  # widths Poseidon2 does not define
        q = M2.Poseidon2.__new__(M2.Poseidon2)
        q.t, q.full_rounds, q.partial_rounds, q.rc, q.mu = t, 8, 56, [0] * (8 * t + 56), [0] * t
        assert permute(exe, tmp, q, [0] * t)[0] == 4, t
    bad = M2.Poseidon2(r, 3, 8, 56, p.rc[:-1] + [r], p.mu)
    assert permute(exe, tmp, bad, states)[0] == 3
    bad = M2.Poseidon2(r, 3, 8, 56, p.rc, p.mu[:2] + [r])
    assert permute(exe, tmp, bad, states)[0] == 3


def test_the_bench_tools_product_count_follows_the_kernels_tidy_rules(harness):
    """tools/bench_frhash.py restates frh2_tidy_sums, frh2_bound and frh2_tidy_sbox to count a permutation's products: the program prints the
    kernel's own, per width, for this field"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bench_frhash as tool
    finally:
        sys.path.pop(0)
    field, exe, _ = harness
    r = _r(field)
    for t in WIDTHS:
        out = subprocess.run([exe, "rules", str(t)], capture_output=True, text=True, check=True).stdout.split()
        tidy_sums, bound, tidy_sbox, headroom = bool(int(out[0])), int(out[1]), bool(int(out[2])), int(out[3])
        assert headroom == (1 << 261) // r and tool.poseidon2_rules(r, t) == (tidy_sums, bound, tidy_sbox), (field, t)
        layer, sbox = (0 if t < 4 else t + 4 if tidy_sums else t), (4 if tidy_sbox else 3)
        assert tool.products2(r, t, 8, 56) == t + 8 * (t * sbox + layer) + layer + 56 * (sbox + 2 * t), (field, t)
    assert tool.poseidon2_rules(_r("bls12_381"), 12) == (True, 4, False) and tool.poseidon2_rules(_r("bls12_381"), 3) == (False, 8, True)
    assert tool.poseidon2_rules(_r("bn254"), 12) == (False, 8, False) and tool.products2(_r("bn254"), 3, 8, 57) == 588
    assert subprocess.run([exe, "rules", "5"]).returncode == 4


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the table and into a slab that holds ONE copy of the
    state; shifts), run on its own: every width, a short tile, a strided sponge"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r, rnd = _r(field), rng(1300)
    for t in WIDTHS:
        p = M2.sample(r, t, capacity=7, capacity_at=t - 1, out_at=1)
        states = [[rnd.randrange(r) for _ in range(t)] for _ in range(5)] + [[r - 1] * t]
        rc, got = permute(exe, tmp_path, p, [x for s in states for x in s], tile=2)
        assert rc == 0 and got == [x for s in states for x in p.permute(s)], t
        rows = [[rnd.randrange(r) for _ in range(2 * t - 1)] for _ in range(3)]
        rc, got = sponge(exe, tmp_path, p, [M.mont(row, r) for row in rows], 2 * t - 1, mont=True, tile=64, gap=(r,))
        assert rc == 0 and got == M.mont([p.hash(row) for row in rows], r), t
