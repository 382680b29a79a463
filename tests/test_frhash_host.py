"""libmsm_frhash.so's Poseidon on the CPU: the pure-Python model (tests/frhash_model.py) against known answers and against the generator of
msm_webgpu_amd.api, and a stand-alone program (tests/host_harness/frhash_harness.cpp) that runs the plan of csrc/frhash_plan.h and, lane by
lane in serial order, the functions the kernels call (csrc/frhash_kernels.h), compiled with g++ -DFQ_CHECK so that every limb and value bound
is asserted, against the model: permutations, sponges and trees, the five fields, both data forms, t in {2, 3, 5, 9, 12} and, per field, the
widest state that goes into the S-box untidied, the narrowest that is tidied first (4 and 5, 7 and 8, or 9 and 10) and t = 10.  Host logic only."""
import os
import subprocess

import pytest

from tests import frhash_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
WIDTHS = (2, 3, 5, 9, 12)
# frh_permute tidies the S-box input iff (t + 4)^2 > FQ_HEADROOM (70 for BLS12-381, 127 for Pallas and Vesta, 169 for BN254 and Grumpkin, where
# t = 9 meets the bound with equality): the last width that is not tidied and the first that is
EDGE = {"bls12_381": (4, 5), "pallas": (7, 8), "vesta": (7, 8), "bn254": (9, 10), "grumpkin": (9, 10)}
R_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


# ---- the model and the generator ------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    rc, mds = M.parameters(R_BN254, 3, 8, 57)
    assert rc[0] == 0x0ee9a592ba9a9518d05986d656f40c2114c4993c11bb29938d21d47304cd8e6e
    assert mds[0][0] == 0x109b7f411ba0e4c9b2b70caf5c36a7b194be7c11ad24378bfedb68592ba8118b
    assert len(rc) == 65 * 3 and all(0 <= c < R_BN254 for c in rc)
    assert M.standard(R_BN254, 3, 8, 57).hash([1, 2]) == 7853200120776062878684798364095072458815029376092732009249414926327459813530
    assert M.standard(R_BN254, 2, 8, 56).hash([1]) == 18586133768512220936620570745912940619677854269274689475585506675881198879027


def test_the_generator_of_the_package_is_the_models():
    from msm_webgpu_amd import api

    assert api.POSEIDON_PARTIAL_ROUNDS == M.DEFAULT_PARTIAL == dict(zip(range(2, 13), (56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60)))
    for curve, t, rf, rp in (("bn254", 3, 8, None), ("bn254", 2, 8, 56), ("bls12_381", 5, 8, None), ("pallas", 3, 8, 56), ("vesta", 12, 6, 3), ("grumpkin", 4, 2, 0)):
        rc, mds = api.poseidon_parameters(curve, t, rf, rp)
        want_rc, want_mds = M.parameters(api.SCALAR_FIELDS[curve], t, rf, rp)
        assert isinstance(rc, list) and rc == list(want_rc) and mds == [list(row) for row in want_mds], (curve, t)
        r = api.SCALAR_FIELDS[curve]
        assert all((mds[i][j] * (pow(mds[0][0], r - 2, r) - pow(mds[0][j], r - 2, r) - pow(mds[i][0], r - 2, r) + pow(mds[i][j], r - 2, r))) % r == 0
                   for i in range(t) for j in range(t))  # (a Cauchy matrix: 1 / m[i][j] = x_i + y_j)
    assert "subspace" in api.poseidon_parameters.__doc__
    for bad in (lambda: api.poseidon_parameters("bn254", 1), lambda: api.poseidon_parameters("bn254", 13), lambda: api.poseidon_parameters("bn254", 3, 7),
                lambda: api.poseidon_parameters("bn254", 3, 8, 129), lambda: api.poseidon_parameters("nothing", 3)):
        with pytest.raises(ValueError):
            bad()


def test_x5_permutes_every_field_and_x3_none():
    from math import gcd

    for field in FIELDS:
        assert gcd(5, _r(field) - 1) == 1 and gcd(3, _r(field) - 1) == 3, field


def test_model_semantics():
    r = 97  # (5 does not divide 96)
    p = M.Poseidon(r, 3, 2, 1, list(range(1, 10)), [[1, 2, 3], [4, 5, 6], [7, 8, 10]])
    s = [(x + c) ** 5 % r for x, c in zip((3, 4, 5), (1, 2, 3))]
    s = [sum(m * x for m, x in zip(row, s)) % r for row in p.mds]
    s = [(s[0] + 4) ** 5 % r, (s[1] + 5) % r, (s[2] + 6) % r]  # the partial round: the first element alone
    s = [sum(m * x for m, x in zip(row, s)) % r for row in p.mds]
    s = [(x + c) ** 5 % r for x, c in zip(s, (7, 8, 9))]
    assert p.permute([3, 4, 5]) == [sum(m * x for m, x in zip(row, s)) % r for row in p.mds]
    # the sponge: capacity at 1, the inputs onto positions 0 and 2, a short last block, the output from position 2
    assert p.hash([10, 20, 30], 5, 1, 2) == p.permute([(a + 30) % r for a in p.permute([10, 5, 20])[:1]] + p.permute([10, 5, 20])[1:])[2]
    assert p.hash([10], 0, 0, 0) == p.permute([0, 10, 0])[0]
    leaves = list(range(8))
    levels = p.merkle(leaves)
    assert [len(level) for level in levels] == [4, 2, 1] and levels[0][3] == p.hash([6, 7]) and levels[2][0] == p.hash(levels[1])
    for index in (0, 5, 7):
        path = p.path(leaves, levels, index)
        assert len(path) == 3 and all(len(row) == 1 for row in path) and p.verify(leaves[index], index, path, levels[-1][0])
        path[1][0] ^= 1
        assert not p.verify(leaves[index], index, path, levels[-1][0])
    assert M.Poseidon(r, 2, 2, 0, [1, 2, 3, 4], [[1, 2], [3, 5]]).merkle_chain(9, 3)[2] == M.Poseidon(r, 2, 2, 0, [1, 2, 3, 4], [[1, 2], [3, 5]]).hash(
        [M.Poseidon(r, 2, 2, 0, [1, 2, 3, 4], [[1, 2], [3, 5]]).merkle_chain(9, 2)[1]])


# ---- the program -----------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frhash_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frh_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frhash_harness.cpp"), "-o", exe])
    return exe


def _call(exe, tmp, args, data):
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(M.to_bytes(data))
    if fout.exists():
        fout.unlink()
    p = subprocess.run([exe] + [str(a) for a in args] + [str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3, 4), (p.returncode, p.stderr[-500:])
    return p.returncode, M.from_bytes(fout.read_bytes()) if fout.exists() else None


def _params(p):
    return list(p.rc) + [c for row in p.mds for c in row]


def permute(exe, tmp, p, stored, mont=False, tile=0):
    return _call(exe, tmp, ("permute", p.t, p.full_rounds, p.partial_rounds, 2 if mont else 0, tile, len(stored) // p.t), _params(p) + list(stored))


def sponge(exe, tmp, p, stored_rows, length, mont=False, tile=0, gap=()):
    stride = len(stored_rows[0]) + len(gap)
    flat = [x for row in stored_rows for x in list(row) + list(gap)]
    flat = flat[:(len(stored_rows) - 1) * stride + length]
    return _call(exe, tmp, ("hash", p.t, p.full_rounds, p.partial_rounds, 2 if mont else 0, tile, len(stored_rows), length, stride, p.capacity_at, p.out_at),
                 _params(p) + [p.capacity] + flat)


def tree(exe, tmp, p, stored_leaves, n_leaves=None, mont=False, tile=0):
    n_leaves = len(stored_leaves) if n_leaves is None else n_leaves
    return _call(exe, tmp, ("merkle", p.t, p.full_rounds, p.partial_rounds, 2 if mont else 0, tile, n_leaves, p.capacity_at, p.out_at), _params(p) + [p.capacity] + list(stored_leaves))


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frhash_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def edge_widths(field):
    """the field's two widths at the tidy boundary and the even width 10, as far as WIDTHS does not hold them"""
    return sorted(set(EDGE[field] + (10,)) - set(WIDTHS))


def test_the_tidy_boundary_is_where_the_constants_put_it():
    import re

    for field, (last, first) in EDGE.items():
        text = open(os.path.join(ROOT, "msm-webgpu_amd", "csrc", "fr_%s_constants.h" % field)).read()
        headroom = int(re.search(r"constexpr int FQ_HEADROOM = (\d+);", text).group(1))
        assert headroom == (1 << 261) // _r(field) and first == last + 1 and (last + 4) ** 2 <= headroom < (first + 4) ** 2, (field, headroom)
    assert (EDGE["bn254"][0] + 4) ** 2 == (1 << 261) // _r("bn254")  # met with equality
    assert [edge_widths(f) for f in FIELDS] == [[10], [10], [7, 8, 10], [7, 8, 10], [4, 10]]


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("t", WIDTHS)
def test_permutations_against_the_model(harness, t, mont):
    _permutations(harness, t, mont)


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
def test_permutations_at_the_tidy_boundary(harness, mont):
    for t in edge_widths(harness[0]):
        _permutations(harness, t, mont)


def _permutations(harness, t, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(400 + t)
    p = M.standard(r, t)
    states = [[r - 1] * t, [0] * t, [1] + [0] * (t - 1)] + [[rnd.randrange(r) for _ in range(t)] for _ in range(4)]
    flat = [x for s in states for x in s]
    want = form([x for s in states for x in p.permute(s)], r, mont)
    for tile in (0, 3):  # one workgroup; three lanes to a workgroup, the last one short
        rc, got = permute(exe, tmp, p, form(flat, r, mont), mont, tile)
        assert rc == 0 and got == want, (field, t, mont, tile)


@pytest.mark.parametrize("t", WIDTHS)
def test_the_worst_case_of_the_bounds(harness, t):
    """constants, matrix and state all r - 1: every lazy sum is as large as it gets; then no partial rounds, and two full rounds alone"""
    _worst_case(harness, t)


def test_the_worst_case_at_the_tidy_boundary(harness):
    """the same where the S-box input is as large as it may be without being tidied -- (t + 4)^2 = 64 of 70, 121 of 127, 169 of 169 -- and one wider"""
    for t in sorted(set(EDGE[harness[0]] + (10,))):
        _worst_case(harness, t)


def _worst_case(harness, t):
    field, exe, tmp = harness
    r = _r(field)
    for rf, rp in ((8, M.DEFAULT_PARTIAL[t]), (8, 0), (2, 0), (16, 128)):
        p = M.Poseidon(r, t, rf, rp, [r - 1] * ((rf + rp) * t), [[r - 1] * t] * t, capacity=r - 1, capacity_at=t - 1, out_at=t - 1)
        states = [[r - 1] * t, [0] * t]
        for mont in (False, True):
            rc, got = permute(exe, tmp, p, form([x for s in states for x in s], r, mont), mont)
            assert rc == 0 and got == form([x for s in states for x in p.permute(s)], r, mont), (field, t, rf, rp, mont)
        rows = [[r - 1] * (2 * (t - 1) + 1)] * 2
        rc, got = sponge(exe, tmp, p, rows, len(rows[0]))
        assert rc == 0 and got == [p.hash(row) for row in rows], (field, t, rf, rp)


@pytest.mark.parametrize("t", WIDTHS)
def test_sponges_against_the_model(harness, t):
    _sponges(harness, t)


def test_sponges_at_the_tidy_boundary(harness):
    for t in edge_widths(harness[0]):
        _sponges(harness, t)


def _sponges(harness, t):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(500 + t)
    conventions = ((0, 0, 0), ((3 << 64) % r, t - 1, 0), ((1 << (t - 1)) - 1, 0, 1 % t))
    for k, length in enumerate(sorted({1, max(1, t - 2), t - 1, t, 2 * (t - 1), 2 * (t - 1) + 1})):
        capacity, capacity_at, out_at = conventions[k % 3]
        p = M.standard(r, t, capacity=capacity, capacity_at=capacity_at, out_at=out_at)
        rows = [[rnd.randrange(r) for _ in range(length)] for _ in range(3)]
        mont = bool(k & 1)
        rc, got = sponge(exe, tmp, p, [form(row, r, mont) for row in rows], length, mont, tile=2, gap=(r, (1 << 256) - 1))  # (the gap is not read)
        assert rc == 0 and got == form([p.hash(row) for row in rows], r, mont), (field, t, length)


def test_trees_against_the_model(harness):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(600)
    for t, n, tile in ((3, 2, 0), (3, 32, 0), (3, 32, 3), (5, 64, 5), (9, 64, 0), (12, 121, 7)):
        p = M.standard(r, t, capacity=(1 << (t - 1)) - 1, capacity_at=0, out_at=1)
        leaves = [rnd.randrange(r) for _ in range(n)]
        for mont in (False, True):
            rc, got = tree(exe, tmp, p, form(leaves, r, mont), mont=mont, tile=tile)
            assert rc == 0 and got == form([x for level in p.merkle(leaves) for x in level], r, mont), (field, t, n, mont)
    p = M.standard(r, 2)
    rc, got = tree(exe, tmp, p, [5], n_leaves=3)
    assert rc == 0 and got == p.merkle_chain(5, 3)
    for t, n in ((3, 3), (3, 0), (3, 1), (5, 8), (12, 12), (2, 0), (2, 65)):  # no power of the arity; a chain too long
        assert tree(exe, tmp, M.standard(r, t), [1] * max(n, 1), n_leaves=n)[0] == 4, (t, n)


def test_the_levels_of_a_tree(harness):
    _, exe, _ = harness
    for t, n, want in ((3, 2, "1"), (3, 2048, "1024 512 256 128 64 32 16 8 4 2 1"), (5, 1024, "256 64 16 4 1"), (9, 512, "64 8 1"), (12, 121, "11 1"), (2, 3, "1 1 1"),
                       (3, 1 << 26, " ".join(str(1 << k) for k in range(25, -1, -1)))):
        assert subprocess.run([exe, "levels", str(t), str(n)], capture_output=True, text=True).stdout.split() == want.split(), (t, n)
    assert subprocess.run([exe, "levels", "3", str((1 << 26) + 2)]).returncode == 4 and subprocess.run([exe, "levels", "3", "24"]).returncode == 4


def test_a_value_not_below_r_is_reported(harness):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(700)
    p = M.standard(r, 3)
    states = [rnd.randrange(r) for _ in range(3 * 5)]
    assert permute(exe, tmp, p, states)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        for at in (0, 7, 14):
            assert permute(exe, tmp, p, states[:at] + [bad] + states[at + 1:])[0] == 3, (hex(bad), at)
            assert permute(exe, tmp, p, states[:at] + [bad] + states[at + 1:], mont=True)[0] == 3
        for at in (0, 2, 4):
            assert sponge(exe, tmp, p, [states[:5], states[5:10][:at] + [bad] + states[5:10][at + 1:]], 5)[0] == 3, (hex(bad), at)
        assert tree(exe, tmp, p, states[:3] + [bad])[0] == 3
    bad_rc = M.Poseidon(r, 3, 8, 57, list(p.rc[:-1]) + [r], p.mds)
    assert permute(exe, tmp, bad_rc, states)[0] == 3
    bad_cap = M.Poseidon(r, 3, 8, 57, p.rc, p.mds, capacity=r)
    assert sponge(exe, tmp, bad_cap, [states[:2]], 2)[0] == 3


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the table, the slabs and the levels; shifts) on the
    widest state, a short tile, a strided sponge and a tree of several levels"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r, rnd = _r(field), rng(800)
    p = M.standard(r, 12, capacity=7, capacity_at=11, out_at=3)
    states = [[rnd.randrange(r) for _ in range(12)] for _ in range(5)]
    rc, got = permute(exe, tmp_path, p, [x for s in states for x in s], tile=2)
    assert rc == 0 and got == [x for s in states for x in p.permute(s)]
    rows = [[rnd.randrange(r) for _ in range(23)] for _ in range(3)]
    rc, got = sponge(exe, tmp_path, p, rows, 23, tile=64, gap=(r,))
    assert rc == 0 and got == [p.hash(row) for row in rows]
    p = M.standard(r, 3)
    leaves = [rnd.randrange(r) for _ in range(16)]
    rc, got = tree(exe, tmp_path, p, M.mont(leaves, r), mont=True, tile=1)
    assert rc == 0 and got == M.mont([x for level in p.merkle(leaves) for x in level], r)
