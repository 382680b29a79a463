"""libmsm_frlook.so's lookup on the CPU: a stand-alone program (tests/host_harness/frlook_harness.cpp) that runs the plan of csrc/frlook_plan.h and,
lane by lane in serial order, the functions the kernels call (csrc/frlook_kernels.h) through the host definitions of the atomics shim, compiled
with g++ -DFQ_CHECK so that their assertions are on, against the pure-Python model (tests/frlook_model.py): the slot array word by word, the
counts, the indices, the missing elements and m in both forms.  The five fields.  Host logic only."""
import os
import struct
import subprocess

import pytest

from tests import frlook_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
R_MODEL = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def _r(field):
    from msm_webgpu_amd import api

    return api.SCALAR_FIELDS[field]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
def test_model_semantics():
    t = [5, 7, 5, 9, 7, 5]
    counts, idx, missing, first, distinct = M.lookup(t, [[5, 5, 8, 9], [7, 1, 5, 5]])
    assert counts == [4, 1, 0, 1, 0, 0] and idx == [0, 0, M.MISSING, 3, 1, M.MISSING, 0, 0]
    assert (missing, first, distinct) == (2, 2, 3)
    assert M.lookup(t, [[5, 9, 8], [7, 8, 8]], n=2) == ([1, 1, 0, 1, 0, 0], [0, 3, 1, M.MISSING], 1, 3, 3)  # (the tail of a row is not looked up)
    assert M.lookup([3], [[3, 3]])[2:4] == (0, M.NO_MISSING)
    r = R_MODEL
    assert M.multiplicities([0, 1, 3], r) == [0, 1, 3] and M.multiplicities([0, 1, 3], r, True) == [0, pow(2, 256, r), 3 * pow(2, 256, r) % r]
    m, h_f, h_t, s_f, s_t = M.logup([1, 2, 3, 2], [[1, 2, 2, 3], [3, 3, 3, 1]], 10, r)
    assert m == [2, 2, 4, 0] and s_f == s_t and len(h_f) == 4 and h_t[3] == 0


def test_model_hash_and_slots():
    assert M.key_hash(0) != M.key_hash(1) and M.key_hash(1) != M.key_hash(1 << 224)
    assert [M.slot_count(n) for n in (1, 2, 3, 64, 65, 1025, 1 << 24)] == [2, 4, 8, 128, 256, 4096, 1 << 25]
    # every word of the key reaches the LOW bits of the hash: 256 keys that differ in one word only reach all of 16 slots (a hash that
    # spreads leaves one of them empty with probability 16 (15/16)^256 ~ 1e-6; one that ignores the word reaches a single slot)
    for word in range(8):
        assert len({M.key_hash(k << (32 * word)) & 15 for k in range(1, 257)}) == 16, word
    slots, distinct = M.build_slots([5, 7, 5, 9, 7, 5])
    assert distinct == 3 and sorted(s for s in slots if s != M.EMPTY) == [0, 1, 3] and len(slots) == 16
    t = M.table("wrapping chain", R_MODEL, rng(1))
    slots, distinct = M.build_slots(t)
    assert distinct == 8 and slots[15] == 0 and slots[:7] == [1, 2, 3, 4, 5, 6, 7]  # the chain goes round the end, and pushes the chain at 0 on
    assert M.probes(t, slots, t[4]) == 5 and M.probes(t, slots, t[7]) == 7
    one_bit, _ = M.build_slots(list(range(65)), bits=1)
    assert all(s != M.EMPTY for s in one_bit[:65]) and all(s == M.EMPTY for s in one_bit[66:])  # one run from slot 0 (or 1) on


# ---- the program -----------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("frlook_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=frl_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "frlook_harness.cpp"), "-o", exe])
    return exe


def run(exe, tmp, table, rows, bits=0, mont=False, n=None, gap=b""):
    """table, rows: the scalars AS STORED; every row is followed by `gap` (whole scalars that must not be read)
    -> (status, dict of the program's outputs, or None)"""
    n_t, batch = len(table), len(rows)
    width = len(rows[0])
    n = width if n is None else n
    stride = width + len(gap) // 32
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(M.to_bytes(table) + b"".join(M.to_bytes(row) + gap for row in rows))
    if fout.exists():
        fout.unlink()
    p = subprocess.run([exe, "run"] + [str(a) for a in (n_t, bits, int(mont), n, batch, stride)] + [str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3), (p.returncode, p.stderr[-500:])
    raw = fout.read_bytes()
    head = struct.unpack("<8I", raw[:32])
    size, total = head[6], batch * n
    words = struct.unpack("<%dI" % (size + n_t + total), raw[32:32 + 4 * (size + n_t + total)])
    return p.returncode, {"distinct": head[1], "missing": head[2] | head[3] << 32, "first_missing": head[4] | head[5] << 32, "plan_distinct": head[7],
                          "slots": list(words[:size]), "counts": list(words[size:size + n_t]), "idx": list(words[size + n_t:]),
                          "m": M.from_bytes(raw[32 + 4 * (size + n_t + total):])}


def check(out, table, rows, r, bits=0, mont=False, n=None):
    """the program's outputs against the model, for stored table and rows"""
    counts, idx, missing, first, distinct = M.lookup(table, rows, n)
    slots, d = M.build_slots(table, bits)
    assert d == distinct and out["slots"] == slots
    assert (out["distinct"], out["plan_distinct"], out["missing"], out["first_missing"]) == (distinct, distinct, missing, first)
    assert out["counts"] == counts and out["idx"] == idx and out["m"] == M.multiplicities(counts, r, mont)


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frlook_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _looked_up(table, r, rnd, n, foreign=0.1):
    """n values of the table (in the form it is stored in), a tenth of them not in it"""
    have = set(table)
    out = []
    for _ in range(n):
        v = table[rnd.randrange(len(table))]
        if rnd.random() < foreign:
            v = rnd.randrange(r)
            while v in have:
                v = rnd.randrange(r)
        out.append(v)
    return out


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("name", M.TABLES)
def test_tables_against_the_model(harness, name, mont):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(71)
    plain = M.table(name, r, rnd)
    table = M.mont(plain, r) if mont else plain
    for bits in (1, 4, 0) if len(table) <= 65 or name == "random 1025" else (0,):
        rows = [_looked_up(table, r, rnd, 70) for _ in range(2)]
        rc, out = run(exe, tmp, table, rows, bits, mont)
        assert rc == 0, (field, name, bits)
        check(out, table, rows, r, bits, mont)


def test_a_chain_that_wraps_round_the_end_of_the_slots(harness):
    field, exe, tmp = harness
    r = _r(field)
    table = M.table("wrapping chain", r, rng(72))
    slots, _ = M.build_slots(table)
    assert slots[15] == 0 and slots[0] == 1  # (what the case is about)
    rows = [table + [table[0] + 1, 0]]
    rc, out = run(exe, tmp, table, rows)
    assert rc == 0
    check(out, table, rows, r)
    assert out["idx"][:8] == list(range(8))


def test_rows_with_a_gap_and_a_short_n(harness):
    """the elements between n and stride are not read: they hold bytes that are not below r"""
    field, exe, tmp = harness
    r, rnd = _r(field), rng(73)
    table = M.table("random 65", r, rnd)
    rows = [_looked_up(table, r, rnd, 9) for _ in range(3)]
    rc, out = run(exe, tmp, table, rows, gap=b"\xff" * 160)
    assert rc == 0
    check(out, table, rows, r)
    rc, out = run(exe, tmp, table, [row + [r, r + 1] for row in rows], n=9)
    assert rc == 0
    check(out, table, rows, r)


def test_counts_at_the_largest_multiplicity(harness):
    """every element the same key: one count of batch * n, written as a scalar in both forms (the doublings of csrc/frlook_kernels.h)"""
    field, exe, tmp = harness
    r = _r(field)
    for mont in (False, True):
        table = [r - 1, 0, 3] if not mont else M.mont([r - 1, 0, 3], r)
        rows = [[table[0]] * 4097, [table[0]] * 4097]
        rc, out = run(exe, tmp, table, rows, mont=mont)
        assert rc == 0 and out["counts"] == [8194, 0, 0]
        check(out, table, rows, r, mont=mont)


def test_a_value_not_below_r_is_reported(harness):
    field, exe, tmp = harness
    r, rnd = _r(field), rng(74)
    table = M.table("random 64", r, rnd)
    rows = [_looked_up(table, r, rnd, 12)]
    assert run(exe, tmp, table, rows)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        for at in (0, 31, 63):
            assert run(exe, tmp, table[:at] + [bad] + table[at + 1:], rows)[0] == 3, (hex(bad), at)
        for at in (0, 5, 11):
            assert run(exe, tmp, table, [rows[0][:at] + [bad] + rows[0][at + 1:]])[0] == 3, (hex(bad), at)


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the slots, the keys, the counts and the outputs;
    shifts and rotations) on the chains of one hash bit, the wrapping chain, repeated keys and both forms"""
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r, rnd = _r(field), rng(75)
    for name, bits, mont in (("random 65", 1, False), ("wrapping chain", 0, False), ("tripled", 4, True), ("identical", 0, True), ("random 1", 0, False)):
        plain = M.table(name, r, rnd)
        table = M.mont(plain, r) if mont else plain
        rows = [_looked_up(table, r, rnd, 67) for _ in range(2)]
        rc, out = run(exe, tmp_path, table, rows, bits, mont, gap=b"\xff" * 32)
        assert rc == 0, name
        check(out, table, rows, r, bits, mont)
