"""Lookup arguments on the device (include/msm_frlook.h; MsmContext.lookup_table, scalars_multiplicities) against the pure-Python model
(tests/frlook_model.py), byte for byte: m in the data's form, the counts, the index of every element, `missing`, `first_missing` and `distinct`.
The smallest shapes at which the kernels can still go wrong: tables of 1 .. 1025 keys -- the last two also with 1 and 4 hash bits, which gives
probe chains longer than a wave and across workgroups --, 1 .. 4097 looked-up elements, rows with a gap of bytes that must not be read,
repeated and identical table values, a column of one value (one count of 4097 through the aggregated path), waves whose lanes all differ,
missing elements at the first, a middle and the last position, values that are not below r, both forms, the five fields, each output alone,
a second run, a caller's stream, the host form, and one middle shape: a range table of 2^16 under 2 rows of 2^18."""
import ctypes as C

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frlook_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
ERR_NONCANONICAL = -4
R = api.SCALAR_FIELDS["bn254"]
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
FORMS = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])


@pytest.fixture(scope="module")
def contexts(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(curve="bn254", mont=False):
        if curve not in made:
            made[curve] = m.MsmContext(0, curve)
        made[curve].set_scalar_format(mont256=mont)
        return made[curve]

    yield get
    api.frlook_test_hash_bits(0)
    for c in made.values():
        c.close()
    api.frlook_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def stored(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def rows_dev(rows, gap=0):
    """batch rows of stored scalars, each followed by `gap` scalars of 0xFF bytes (not below any r: they must not be read)"""
    return torch.frombuffer(bytearray(b"".join(M.to_bytes(row) + b"\xff" * (32 * gap) for row in rows)), dtype=torch.uint8).reshape(-1, 32).cuda()


def table_of(ctx, vals, bits=0):
    api.frlook_test_hash_bits(bits)
    try:
        return ctx.lookup_table(dev(vals))
    finally:
        api.frlook_test_hash_bits(0)


def looked_up(table, r, rnd, n, foreign=0.1):
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


def check(ctx, r, mont, plain_table, plain_rows, bits=0, gap=0, what=None):
    """everything a count returns against the model; the data go to the device in the context's form"""
    table, rows = stored(plain_table, r, mont), [stored(row, r, mont) for row in plain_rows]
    counts, idx, missing, first, distinct = M.lookup(table, rows)
    n = len(rows[0])
    with table_of(ctx, table, bits) as t:
        assert (t.n, t.distinct, t.mont256) == (len(table), distinct, mont), what
        got_m, got_idx, got_counts, (got_missing, got_first) = ctx.scalars_multiplicities(t, rows_dev(rows, gap), batch=len(rows), n=n, indices=True, counts=True, strict=False)
    assert (got_missing, got_first) == (missing, first if missing else None), what
    assert got_counts.dtype == torch.uint32 and got_counts.cpu().numpy().tolist() == counts, what
    assert got_idx.dtype == torch.int32 and tuple(got_idx.shape) == (len(rows), n), what
    assert got_idx.cpu().numpy().astype(np.uint32).reshape(-1).tolist() == idx, what
    assert tuple(got_m.shape) == (len(table), 32) and raw(got_m) == M.to_bytes(M.multiplicities(counts, r, mont)), what


# ---- tables of every size, short and long chains ---------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("n_t,bits", [(1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (65, 1), (65, 4), (1025, 0), (1025, 1), (1025, 4)])
def test_table_sizes_and_hash_bits(contexts, n_t, bits, mont):
    ctx, rnd = contexts("bn254", mont), rng(900 + n_t)
    table = M.table("random %d" % n_t, R, rnd)
    check(ctx, R, mont, table, [looked_up(table, R, rnd, 130)], bits, what=(n_t, bits, mont))


# ---- every length of a row, one row and three with a gap ----------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 4097])
def test_row_lengths_and_rows_with_a_gap(contexts, n, mont):
    ctx, rnd = contexts("bn254", mont), rng(910 + n)
    table = M.table("random 65", R, rnd)
    check(ctx, R, mont, table, [looked_up(table, R, rnd, n)], what=(n, 1))
    check(ctx, R, mont, table, [looked_up(table, R, rnd, n) for _ in range(3)], gap=5, what=(n, 3))


# ---- repeated table values ------------------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("name", ["tripled", "identical", "zero and r - 1", "range 1025", "word 7 only", "wrapping chain"])
def test_repeated_and_special_tables(contexts, name, mont):
    ctx, rnd = contexts("bn254", mont), rng(920)
    table = M.table(name, R, rnd)
    check(ctx, R, mont, table, [looked_up(table, R, rnd, 200) for _ in range(2)], what=name)
    if name in ("tripled", "identical"):
        check(ctx, R, mont, table, [looked_up(table, R, rnd, 200)], bits=1, what=name)


# ---- what the lanes of a wave hold ------------------------------------------------------------------------------------------------------------------------
@FORMS
def test_one_value_every_lane_different_and_two_alternating(contexts, mont):
    ctx, rnd = contexts("bn254", mont), rng(930)
    table = M.table("random 1025", R, rnd)
    check(ctx, R, mont, table, [[table[700]] * 4097], what="all equal")  # one count of 4097: across waves and workgroups, one atomic per wave
    check(ctx, R, mont, table, [[table[700]] * 1366 for _ in range(3)], gap=5, what="all equal, three rows")
    different = list(table[:1024])
    rnd.shuffle(different)
    check(ctx, R, mont, table, [different + different[:1]], what="every lane different")
    check(ctx, R, mont, table, [[table[3], table[900]] * 600 + [table[3]]], what="two alternating")
    check(ctx, R, mont, table, [([table[5]] * 64 + different[:64]) * 4], what="a wave of one value, a wave of 64")


# ---- missing elements ----------------------------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("where", [(0,), (1500,), (2 * 1025 - 1,), (0, 1500, 2 * 1025 - 1), (1024, 1025), tuple(range(2050))], ids=["first", "middle", "last", "three", "row end", "all"])
def test_missing_elements(contexts, where, mont):
    ctx, rnd = contexts("bn254", mont), rng(940)
    table = M.table("random 65", R, rnd)
    rows = [looked_up(table, R, rnd, 1025, foreign=0) for _ in range(2)]
    for at in where:
        rows[at // 1025][at % 1025] = (table[7] + 1 + at) % R  # (next to a table value; not in the table: checked by the model's count below)
    assert M.lookup(table, rows)[2:4] == (len(where), where[0])
    check(ctx, R, mont, table, rows, what=where)
    t = table_of(ctx, stored(table, R, mont))
    f = rows_dev([stored(row, R, mont) for row in rows])
    with pytest.raises(ValueError, match=r"%d looked-up values are not in the table; the first is element %d \(row %d, position %d\)" % (
            len(where), where[0], where[0] // 1025, where[0] % 1025)):
        ctx.scalars_multiplicities(t, f, batch=2)
    t.close()


# ---- values that are not below r -------------------------------------------------------------------------------------------------------------------------------
def test_noncanonical_values_are_reported_and_the_next_call_is_clean(contexts):
    ctx, rnd = contexts("bn254", False), rng(950)
    table = M.table("random 65", R, rnd)
    rows = [looked_up(table, R, rnd, 300)]
    for bad in (R, (1 << 256) - 1):
        for at in (0, 33, 64):
            with pytest.raises(api.MsmHipError) as e:
                ctx.lookup_table(dev(table[:at] + [bad] + table[at + 1:]))
            assert e.value.code == ERR_NONCANONICAL
        with table_of(ctx, table) as t:
            for at in (0, 150, 299):
                with pytest.raises(api.MsmHipError) as e:
                    ctx.scalars_multiplicities(t, dev(rows[0][:at] + [bad] + rows[0][at + 1:]), strict=False)
                assert e.value.code == ERR_NONCANONICAL
                got = ctx.scalars_multiplicities(t, dev(rows[0]), counts=True, strict=False)  # the same handle, unaffected
                counts, _, missing, first, _ = M.lookup(table, rows)
                assert got[1].cpu().numpy().tolist() == counts and got[2] == (missing, first if missing else None)
    check(ctx, R, False, table, rows)


# ---- the five fields ---------------------------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("curve", FIELDS + ("bn254_g2",))
def test_every_field(contexts, curve, mont):
    ctx, rnd = contexts(curve, mont), rng(960)
    r = api.SCALAR_FIELDS[curve]
    table = M.table("random 65", r, rnd) + [r - 1, 0]
    check(ctx, r, mont, table, [looked_up(table, r, rnd, 65) + [r - 1] for _ in range(3)], bits=1, gap=5, what=curve)
    tripled = M.table("tripled", r, rnd)
    check(ctx, r, mont, tripled, [[0] + looked_up(tripled, r, rnd, 1024, foreign=0.5)], what=curve)


# ---- the C ABI: each output alone, none, a second run, streams, the host form -------------------------------------------------------------------
def test_each_output_alone_none_twice_and_on_a_callers_stream(contexts):
    ctx, rnd = contexts("bn254", False), rng(970)
    L = api.frlook_lib()
    table = M.table("random 1025", R, rnd)
    rows = [looked_up(table, R, rnd, 1000) for _ in range(2)]
    counts, idx, missing, first, _ = M.lookup(table, rows)
    want = {"m": M.to_bytes(counts), "counts": np.asarray(counts, dtype=np.uint32).tobytes(), "idx": np.asarray(idx, dtype=np.uint32).tobytes()}
    f = rows_dev(rows)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with table_of(ctx, table) as t:
        for stream in (None, side.cuda_stream):  # the library's own stream, a caller's
            for asked in (("m",), ("counts",), ("idx",), (), ("m", "counts", "idx"), ("m", "counts", "idx")):  # (the last twice: the same bytes)
                out = {"m": torch.full((1025, 32), 0xEE, dtype=torch.uint8, device="cuda"), "counts": torch.full((1025,), 0x6E6E6E6E, dtype=torch.int32, device="cuda"),
                       "idx": torch.full((2000,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")}
                torch.cuda.synchronize()
                miss, fst = C.c_uint64(5), C.c_uint64(5)
                ptr = [out[k].data_ptr() if k in asked else None for k in ("m", "counts", "idx")]
                assert L.msm_frlook_count_device(t._h, stream, ptr[0], ptr[1], ptr[2], f.data_ptr(), 1000, 2, 1000, 0, C.byref(miss), C.byref(fst)) == 0
                assert (miss.value, fst.value) == (missing, first), asked
                for k in out:  # what was asked for is the model's, the rest is untouched
                    assert (raw(out[k]) == want[k]) if k in asked else bool((out[k].view(torch.uint8) == (0xEE if k == "m" else 0x6E)).all()), (asked, k)
        assert L.msm_frlook_count_device(t._h, None, None, None, None, f.data_ptr(), 1000, 2, 1000, 0, None, None) == 0  # nowhere to report to
        # the host form, staged: the same outputs
        hm, hidx, hcounts, (hmiss, hfirst) = ctx.scalars_multiplicities(t, b"".join(M.to_bytes(row) for row in rows), batch=2, indices=True, counts=True, strict=False)
        assert hm == want["m"] and hidx.tobytes() == want["idx"] and hcounts.tobytes() == want["counts"] and (hmiss, hfirst) == (missing, first)
    with ctx.lookup_table(M.to_bytes(table)) as t:  # a table from host bytes: resident with its first count
        assert t.distinct == 1025
        assert raw(ctx.scalars_multiplicities(t, f, batch=2, strict=False)[0]) == want["m"]
        out = torch.empty((1025, 32), dtype=torch.uint8, device="cuda")
        assert ctx.scalars_multiplicities(t, f, batch=2, out=out, strict=False)[0].data_ptr() == out.data_ptr() and raw(out) == want["m"]


# ---- one middle shape ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_range_table_of_2_16_under_two_rows_of_2_18(contexts):
    """numpy on both sides: the keys are their own indices"""
    ctx = contexts("bn254", False)
    n_t, n, batch = 1 << 16, 1 << 18, 2
    keys = np.zeros((n_t, 8), dtype=np.uint32)
    keys[:, 0] = np.arange(n_t, dtype=np.uint32)
    vals = np.random.default_rng(11).integers(0, n_t + 3, size=batch * n, dtype=np.uint32)  # (three values beyond the table)
    f = np.zeros((batch * n, 8), dtype=np.uint32)
    f[:, 0] = vals
    found = vals < n_t
    with ctx.lookup_table(torch.from_numpy(keys.view(np.uint8)).cuda()) as t:
        assert t.distinct == n_t
        got_m, got_idx, got_counts, (missing, first) = ctx.scalars_multiplicities(t, torch.from_numpy(f.view(np.uint8)).cuda(), batch=batch, indices=True, counts=True, strict=False)
    want = np.bincount(vals[found], minlength=n_t).astype(np.uint32)
    assert np.array_equal(got_counts.cpu().numpy(), want)
    assert np.array_equal(got_idx.cpu().numpy().astype(np.uint32).reshape(-1), np.where(found, vals, np.uint32(0xFFFFFFFF)))
    assert (missing, first) == (int((~found).sum()), int(np.argmax(~found)))
    wide = np.zeros((n_t, 8), dtype=np.uint32)
    wide[:, 0] = want
    assert np.array_equal(got_m.cpu().numpy().reshape(-1).view(np.uint32).reshape(n_t, 8), wide)
