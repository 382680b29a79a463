"""libmsm_frmem.so on the device against the pure-Python model (tests/frmem_model.py) and numpy.argsort(kind="stable"), word for word: the stable
argsort and the access counters over the sizes at which the code takes another path (one lane, one wave, one tile, several, three scan levels
above the keys through the tile hook), ten key sets at eight widths, tables of 1, max key + 1 and 2^16 entries, refusals with the outputs
untouched, every call a second time (the same bytes), in the host form, and once on a caller's stream behind the torch op that makes the keys."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import frmem_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG = -2
SENTINEL = 0xA5
WIDTHS = ((4, 1), (4, 8), (4, 9), (4, 24), (4, 32), (8, 33), (8, 40), (8, 64))  # (key_bytes, bits)
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, (1 << 16) + 1)
WAYS = ("own stream", "again", "host")
MODEL_UP_TO = 1025  # the model's lists up to here; numpy everywhere


@pytest.fixture(scope="module")
def mem(ctx):
    from msm_webgpu_amd import memory

    memory.frmem_test_tile(0)
    yield memory
    memory.frmem_test_tile(0)
    memory.frmem_release()


# ---- numpy's answers --------------------------------------------------------------------------------------------------------------------------------
def _sizes(n, n_t):
    """the bytes of rank, prev, counts, last (a table the library refuses for its size is not allocated)"""
    t = n_t if n_t and n_t <= 1 << 26 else 1 if n_t else 0
    return [4 * n, 4 * n, 4 * t, 4 * t]


def np_keys(keys, key_bytes):
    return np.array(keys, dtype=np.uint32 if key_bytes == 4 else np.uint64)


def np_access(k, n_t):
    """-> rank, prev, counts, last (uint32), distinct; counts and last None without a table"""
    n = len(k)
    perm = np.argsort(k, kind="stable")
    ks = k[perm]
    head = np.r_[True, ks[1:] != ks[:-1]]
    at = np.arange(n)
    start = np.maximum.accumulate(np.where(head, at, 0))
    rank, prev = np.empty(n, np.uint32), np.empty(n, np.uint32)
    rank[perm] = at - start
    prev[perm] = np.where(head, M.MISSING, np.r_[0, perm[:-1]])
    if n_t is None:
        return rank, prev, None, None, int(head.sum())
    tail = np.r_[head[1:], True]
    counts, last = np.zeros(n_t, np.uint32), np.full(n_t, M.MISSING, np.uint32)
    counts[ks[tail].astype(np.int64)] = (at - start + 1)[tail]
    last[ks[tail].astype(np.int64)] = perm[tail]
    return rank, prev, counts, last, int(head.sum())


# ---- the entry points in their ways --------------------------------------------------------------------------------------------------------------------
class Calls:
    """sort and access on the library's stream, again (the same bytes), and in the host form; every output starts as SENTINEL bytes"""

    def __init__(self, mem):
        self.L = mem.frmem_lib()

    @staticmethod
    def _dev(nbytes):
        return torch.full((max(nbytes, 1),), SENTINEL, dtype=torch.uint8, device="cuda")

    def sort(self, k, key_bytes, bits, keys_out=True):
        """-> [(rc, perm bytes, keys_out bytes or None) ..] for the three ways"""
        n = len(k)
        dk = torch.from_numpy(k.view(np.int32 if key_bytes == 4 else np.int64)).cuda()
        got = []
        for way in ("own stream", "again"):
            perm, out = self._dev(4 * n), self._dev(key_bytes * n)
            torch.cuda.synchronize()
            rc = self.L.msm_frmem_sort_device(0, None, perm.data_ptr(), out.data_ptr() if keys_out else None, dk.data_ptr(), key_bytes, bits, n)
            got.append((rc, perm.cpu().numpy().tobytes()[:4 * n], out.cpu().numpy().tobytes()[:key_bytes * n]))
        perm, out = np.full(4 * n, SENTINEL, np.uint8), np.full(key_bytes * n, SENTINEL, np.uint8)
        rc = self.L.msm_frmem_sort(0, perm.ctypes.data, out.ctypes.data if keys_out else None, k.ctypes.data, key_bytes, bits, n)
        got.append((rc, perm.tobytes(), out.tobytes()))
        return got

    def access(self, k, key_bytes, bits, n_t, mask=15, ways=WAYS):
        """-> [(rc, [rank, prev, counts, last bytes], distinct) ..]; an output outside `mask` is NULL (and keeps its sentinel bytes here)"""
        n = len(k)
        sizes, n_t = _sizes(n, n_t), min(n_t or 0, 1 << 40)
        dk = torch.from_numpy(k.view(np.int32 if key_bytes == 4 else np.int64)).cuda()
        got = []
        for way in ways:
            distinct = C.c_uint64(12345)
            if way == "host":
                outs = [np.full(max(s, 1), SENTINEL, np.uint8) for s in sizes]
                ptr = [o.ctypes.data if mask >> b & 1 else None for b, o in enumerate(outs)]
                rc = self.L.msm_frmem_access(0, ptr[0], ptr[1], ptr[2], ptr[3], n_t or 0, k.ctypes.data, key_bytes, bits, n, C.byref(distinct))
                raw = [o.tobytes()[:s] for o, s in zip(outs, sizes)]
            else:
                outs = [self._dev(s) for s in sizes]
                ptr = [o.data_ptr() if mask >> b & 1 else None for b, o in enumerate(outs)]
                torch.cuda.synchronize()
                rc = self.L.msm_frmem_access_device(0, None, ptr[0], ptr[1], ptr[2], ptr[3], n_t or 0, dk.data_ptr(), key_bytes, bits, n, C.byref(distinct))
                raw = [o.cpu().numpy().tobytes()[:s] for o, s in zip(outs, sizes)]
            got.append((rc, raw, distinct.value))
        return got


@pytest.fixture(scope="module")
def calls(mem):
    return Calls(mem)


def _untouched(nbytes):
    return bytes([SENTINEL]) * nbytes


def _check_sort(calls, keys, key_bytes, bits, where):
    k = np_keys(keys, key_bytes)
    perm = np.argsort(k, kind="stable").astype(np.uint32)
    if len(keys) <= MODEL_UP_TO:
        assert perm.tolist() == M.argsort(keys), where
    runs = k[perm]
    assert np.all((runs[1:] != runs[:-1]) | (perm[1:] > perm[:-1]))  # stability: inside a run the indices ascend
    got = calls.sort(k, key_bytes, bits)
    assert all(g == (0, perm.tobytes(), runs.tobytes()) for g in got), where  # (twice on the device: the same bytes; the host form agrees)


def _check_access(calls, keys, key_bytes, bits, n_t, where, mask=15, ways=WAYS):
    k = np_keys(keys, key_bytes)
    n = len(keys)
    table = n_t if mask & 12 else None
    sizes = _sizes(n, n_t)
    got = calls.access(k, key_bytes, bits, n_t, mask, ways)
    if table is not None and (table > 1 << 26 or max(keys) >= table):  # refused, by the argument checks or on the device: nothing is written
        assert all(g == (ERR_INVALID_ARG, [_untouched(s) for s in sizes], 12345) for g in got), where
        return False
    want = np_access(k, table)
    if n <= MODEL_UP_TO and (table or 0) < 1 << 16:
        model = M.access(keys, table)
        assert all(w is None and m is None or w.tolist() == m for w, m in zip(want[:4], model[:4])) and want[4] == model[4], where
    raw = [want[b].tobytes() if mask >> b & 1 else _untouched(sizes[b]) for b in range(4)]
    assert all(g == (0, raw, want[4]) for g in got), where
    return True


def _all_sets(mem, calls, n, tile, seed):
    rnd = rng(seed)
    for name in M.KEY_SETS:
        for key_bytes, bits in WIDTHS:
            keys = M.keys(name, n, bits, rnd)
            where = (n, name, key_bytes, bits)
            _check_sort(calls, keys, key_bytes, bits, where)
            assert mem.frmem_last() == (M.launches(n, bits, tile), len(M.levels(n, tile))), where
            for n_t in (1, max(keys) + 1, 1 << 16):
                ok = _check_access(calls, keys, key_bytes, bits, n_t, where + (n_t,), ways=WAYS if n_t < 1 << 16 else WAYS[::2] if n_t == 1 << 16 else WAYS[:1])  # (a table of megabytes: once)
                if ok:
                    assert mem.frmem_last() == (M.launches(n, bits, tile, access=True, table=True), len(M.levels(n, tile))), where


@pytest.mark.parametrize("n", SIZES)
def test_sort_and_access_at_the_design_tile(mem, calls, n):
    mem.frmem_test_tile(0)
    _all_sets(mem, calls, n, M.TILE, 200 + n)


@pytest.mark.parametrize("n", [n for n in SIZES if n <= 4097])
def test_several_scan_levels_through_the_tile_hook(mem, calls, n):
    mem.frmem_test_tile(64)
    try:
        _all_sets(mem, calls, n, 64, 300 + n)
        if n == 4097:  # 65 * 256 digit counts: four levels with the keys
            assert M.levels(n, 64) == [4097, 65 * 256, 260, 5] and mem.frmem_last()[1] == 4
    finally:
        mem.frmem_test_tile(0)


def test_every_output_alone(mem, calls):
    rnd = rng(401)
    for tile, n in ((0, 1500), (64, 700)):
        mem.frmem_test_tile(tile)
        try:
            for name in M.KEY_SETS:
                keys = M.keys(name, n, 11, rnd)
                for mask in (1, 2, 4, 8):
                    assert _check_access(calls, keys, 4, 11, max(keys) + 1, (n, name, mask), mask=mask)
                    assert mem.frmem_last()[0] == M.launches(n, 11, tile or M.TILE, access=True, table=mask >= 4)
        finally:
            mem.frmem_test_tile(0)


def test_a_refused_key_leaves_the_outputs_and_the_next_call_alone(mem, calls):
    """a key at or above 2^bits, or at or above n_t, in the first, a middle and the last position: INVALID_ARG, sentinel bytes everywhere, and
    the call after it is right"""
    rnd = rng(402)
    for key_bytes, bits, n in ((4, 9, 1), (4, 9, 3000), (4, 24, 70), (8, 33, 1025), (8, 40, 5000)):
        for at in sorted({0, n // 2, n - 1}):
            keys = M.keys("uniform", n, bits, rnd)
            good = list(keys)
            keys[at] = 1 << bits
            k = np_keys(keys, key_bytes)
            assert all(g == (ERR_INVALID_ARG, _untouched(4 * n), _untouched(key_bytes * n)) for g in calls.sort(k, key_bytes, bits)), (bits, n, at)
            assert all(g == (ERR_INVALID_ARG, [_untouched(4 * n)] * 2 + [_untouched(4 * 64)] * 2, 12345) for g in calls.access(k, key_bytes, bits, 64)), (bits, n, at)
            _check_sort(calls, good, key_bytes, bits, "after a refusal")
    for n in (1, 1500):
        for at in sorted({0, n // 2, n - 1}):
            keys = [rnd.randrange(40) for _ in range(n)]
            keys[at] = 40
            assert not _check_access(calls, keys, 4, 16, 40, (n, at))
            assert _check_access(calls, keys, 4, 16, 40, (n, at), mask=3)  # (without counts and last the table's size does not bind)
            assert _check_access(calls, keys, 4, 16, 41, (n, at))


def test_on_a_callers_stream_behind_the_op_that_makes_the_keys(ctx, mem):
    """the Python functions on a side stream: the keys come out of a torch op enqueued just before on that stream"""
    side = torch.cuda.Stream()
    n = (1 << 16) + 1
    base = torch.arange(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        keys = ((base * 2654435761) % 5003).to(torch.int32)
        perm, sorted_keys = mem.argsort(ctx, keys, bits=13, sorted_keys=True)
        rank, prev, counts, last, distinct = mem.access_counters(ctx, keys, table_size=5003, bits=13)
    k = keys.cpu().numpy().astype(np.uint32)
    want = np.argsort(k, kind="stable")
    assert np.array_equal(perm.cpu().numpy(), want) and np.array_equal(sorted_keys.cpu().numpy(), k[want])
    w = np_access(k, 5003)
    for got, exp in zip((rank, prev, counts, last), w[:4]):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp)
    assert distinct == w[4]
    wide = torch.from_numpy(np.random.default_rng(5).integers(0, 1 << 63, size=3000, dtype=np.int64)).cuda()
    assert np.array_equal(mem.argsort(ctx, wide).cpu().numpy(), np.argsort(wide.cpu().numpy(), kind="stable"))
    with pytest.raises(ValueError, match="not below 2\\^12"):
        mem.argsort(ctx, keys, bits=12)
    with pytest.raises(ValueError, match="table"):
        mem.access_counters(ctx, keys, table_size=5002)
    with pytest.raises(ValueError, match="bits"):
        mem.argsort(ctx, keys, bits=33)
    with pytest.raises(TypeError, match="keys"):
        mem.argsort(ctx, keys.float())
    with pytest.raises(TypeError, match="addr"):
        mem.access_counters(ctx, keys.cpu())
    with pytest.raises(ValueError, match="keys"):
        mem.argsort(ctx, torch.stack([keys, keys], 1)[:, 0])  # not contiguous
