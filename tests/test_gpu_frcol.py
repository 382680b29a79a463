"""libmsm_frcol.so on the device against the pure-Python model (tests/frcol_model.py), byte for byte: run expansion at both biases, halo2's permuted
pair and gather, over the sizes at which the code takes another path (one tile, two, three scan levels through the tile hook), count sets
that put one run across several workgroups or a stretch of zeros across several tiles, output lengths that are no multiple of anything,
refused totals with the outputs untouched, and every call a second time, on a caller's stream and in the host form."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import frcol_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG = -2


@pytest.fixture(scope="module")
def col(ctx):
    from msm_webgpu_amd import columns

    columns.frcol_test_tile(0)
    yield columns
    columns.frcol_test_tile(0)
    columns.frcol_release()


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _words(v):
    return np.array(v, dtype=np.uint32)


def _scalars(n, rnd):
    return [rnd.getrandbits(256) for _ in range(n)]


def _bytes(t):
    return t.cpu().numpy().tobytes()


SENTINEL = 0xA5


class Calls:
    """the three entry points in their four ways: the library's stream, again (the same bytes), a caller's stream, the host form"""

    def __init__(self, col):
        self.L = col.frcol_lib()
        self.side = torch.cuda.Stream()

    def _ways(self, device_call, host_call, outs_bytes):
        """-> [(rc, [output bytes ..]) ..] for the four ways; every output starts as SENTINEL bytes"""
        got = []
        for way in ("own stream", "again", "caller's stream"):
            outs = [torch.full((nb,), SENTINEL, dtype=torch.uint8, device="cuda") for nb in outs_bytes]
            torch.cuda.synchronize()
            if way == "caller's stream":
                with torch.cuda.stream(self.side):
                    rc = device_call(self.side.cuda_stream, [o.data_ptr() for o in outs])
            else:
                rc = device_call(None, [o.data_ptr() for o in outs])
            got.append((rc, [_bytes(o) for o in outs]))  # (the call returns after its stream has completed)
        bufs = [C.create_string_buffer(bytes([SENTINEL]) * nb, nb) for nb in outs_bytes]
        rc = host_call([C.addressof(b) for b in bufs])
        got.append((rc, [b.raw for b in bufs]))
        return got

    def expand(self, t, counts, n_out, bias):
        tb, cw = M.to_bytes(t), _words(counts)
        dt, dc = _dev(tb), torch.from_numpy(cw.view(np.int32)).cuda()
        totals = []

        def device_call(stream, outs):
            total = C.c_uint64(12345)
            rc = self.L.msm_frcol_expand_device(0, stream, outs[0], dt.data_ptr(), dc.data_ptr(), len(t), bias, n_out, C.byref(total))
            totals.append(total.value)
            return rc

        def host_call(outs):
            total = C.c_uint64(12345)
            rc = self.L.msm_frcol_expand(0, outs[0], tb, cw.ctypes.data, len(t), bias, n_out, C.byref(total))
            totals.append(total.value)
            return rc

        return self._ways(device_call, host_call, [32 * n_out]), totals

    def pair(self, t, counts):
        n = len(t)
        tb, cw = M.to_bytes(t), _words(counts)
        dt, dc = _dev(tb), torch.from_numpy(cw.view(np.int32)).cuda()
        totals = []

        def device_call(stream, outs):
            total, used = C.c_uint64(12345), C.c_uint64(12345)
            rc = self.L.msm_frcol_pair_device(0, stream, outs[0], outs[1], dt.data_ptr(), dc.data_ptr(), n, C.byref(total), C.byref(used))
            totals.append((total.value, used.value))
            return rc

        def host_call(outs):
            total, used = C.c_uint64(12345), C.c_uint64(12345)
            rc = self.L.msm_frcol_pair(0, outs[0], outs[1], tb, cw.ctypes.data, n, C.byref(total), C.byref(used))
            totals.append((total.value, used.value))
            return rc

        return self._ways(device_call, host_call, [32 * n, 32 * n]), totals

    def gather(self, a, idx):
        n = len(idx)
        ab, iw = M.to_bytes(a), _words(idx)
        da, di = _dev(ab), torch.from_numpy(iw.view(np.int32)).cuda()
        return self._ways(lambda stream, outs: self.L.msm_frcol_gather_device(0, stream, outs[0], da.data_ptr(), len(a), di.data_ptr(), n),
                          lambda outs: self.L.msm_frcol_gather(0, outs[0], ab, len(a), iw.ctypes.data, n), [32 * n])


@pytest.fixture(scope="module")
def calls(col):
    return Calls(col)


def _check_expand(calls, t, c, n_out, bias, where):
    got, totals = calls.expand(t, c, n_out, bias)
    want = M.to_bytes(M.expand(t, c, bias))
    assert totals == [M.total(c, bias)] * 4, where
    for rc, (out,) in got:
        assert rc == 0 and out == want, where


def _check_pair(calls, t, c, where):
    got, totals = calls.pair(t, c)
    a, s, used = M.pair(t, c)
    assert totals == [(len(t), used)] * 4, where
    for rc, outs in got:
        assert rc == 0 and outs == [M.to_bytes(a), M.to_bytes(s)], where


def _all_sets(col, calls, sizes, tile, seed):
    rnd = rng(seed)
    for n_t in sizes:
        t = _scalars(n_t, rnd)
        for name in M.COUNT_SETS:
            _check_pair(calls, t, M.counts(name, n_t, n_t, rnd), (n_t, name))
            assert col.frcol_last() == (M.launches(n_t, tile), len(M.levels(n_t, tile))), (n_t, name)
            for bias, n in ((0, n_t), (1, 2 * n_t), (0, 2 * n_t + 1)):
                _check_expand(calls, t, M.counts(name, n_t, n - bias * n_t, rnd), n, bias, (n_t, name, bias, n))


@pytest.mark.parametrize("n_t", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_expand_and_pair_at_the_design_tile(col, calls, n_t):
    col.frcol_test_tile(0)
    _all_sets(col, calls, [n_t], M.TILE, 100 + n_t)


def test_three_scan_levels_through_the_tile_hook(col, calls):
    col.frcol_test_tile(64)
    try:
        _all_sets(col, calls, [64, 65, 4096, 4097], 64, 111)
        assert [len(M.levels(n, 64)) for n in (64, 65, 4096, 4097)] == [2, 2, 2, 3] and col.frcol_last() == (6, 3)  # (4097: the table, 65 nodes, 2 nodes)
    finally:
        col.frcol_test_tile(0)


def test_output_lengths_1_to_4097(col, calls):
    rnd = rng(112)
    t = _scalars(9, rnd)
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097):
        for bias in (0, 1):
            if n - 9 * bias >= 0:
                _check_expand(calls, t, M.counts("random", 9, n - 9 * bias, rnd), n, bias, (n, bias))


def test_all_used_and_one_used(col, calls):
    rnd = rng(113)
    t = _scalars(1500, rnd)
    got, totals = calls.pair(t, [1] * 1500)
    assert totals == [(1500, 1500)] * 4 and all(rc == 0 and outs == [M.to_bytes(t)] * 2 for rc, outs in got)  # no fillers: A' = S' = t
    for at in (0, 700, 1499):
        c = [0] * 1500
        c[at] = 1500
        got, totals = calls.pair(t, c)
        assert totals == [(1500, 1)] * 4
        for rc, outs in got:
            assert rc == 0 and outs == [M.to_bytes([t[at]] * 1500), M.to_bytes([t[at]] + t[:at] + t[at + 1:])], at  # the fillers are all the others, ascending


def test_a_total_that_does_not_match_is_refused_and_the_next_call_is_unaffected(col, calls):
    rnd = rng(114)
    for n_t in (4, 1500):
        t = _scalars(n_t, rnd)
        untouched = bytes([SENTINEL]) * (32 * n_t)
        for c in ([0x80000000, 0x80000000, n_t - 1, 0] + [0] * (n_t - 4), [0xFFFFFFFF] * n_t, [0] * (n_t - 1) + [n_t + 1], [n_t - 1] + [0] * (n_t - 1), [0] * n_t):
            got, totals = calls.expand(t, c, n_t, 0)
            assert totals == [sum(c)] * 4 and all(rc == ERR_INVALID_ARG and out == [untouched] for rc, out in got), c[:4]
            got, totals = calls.pair(t, c)
            assert [x[0] for x in totals] == [sum(c)] * 4 and all(rc == ERR_INVALID_ARG and outs == [untouched] * 2 for rc, outs in got), c[:4]
            if sum(c):  # (with bias 1 the sum is n_t more: n_t for the counts that are all zero, and out is then the table)
                got, totals = calls.expand(t, c, n_t, 1)
                assert totals == [sum(c) + n_t] * 4 and all(rc == ERR_INVALID_ARG and out == [untouched] for rc, out in got), c[:4]
            else:
                _check_expand(calls, t, c, n_t, 1, "all zero, bias 1")
            _check_pair(calls, t, M.counts("random", n_t, n_t, rnd), "after a refusal")


@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_gather(col, calls, n):
    rnd = rng(115 + n)
    for n_a in (1, 7, 1030):
        a = _scalars(n_a, rnd)
        idx = [rnd.randrange(n_a) for _ in range(n)]
        for at in range(0, n, 5):
            idx[at] = M.MISSING
        want, ok = M.gather(a, idx)
        assert ok and all(rc == 0 and out == [M.to_bytes(want)] for rc, out in calls.gather(a, idx)), n_a
        idx[n // 2] = n_a + rnd.randrange(3)  # one index out of range: refused, that element zero, the others as usual
        want, ok = M.gather(a, idx)
        assert not ok and want[n // 2] == 0
        assert all(rc == ERR_INVALID_ARG and out == [M.to_bytes(want)] for rc, out in calls.gather(a, idx)), n_a
        idx[n // 2] = 0
        assert all(rc == 0 for rc, _ in calls.gather(a, idx))  # the next call is unaffected


def test_a_middle_shape_through_the_python_functions(ctx, col):
    """n_t = 2^16 into n_out = 2^18, on device tensors and numpy (the model's lists would take seconds): expand at bias 0, and the pair at 2^16"""
    n_t, n_out = 1 << 16, 1 << 18
    g = np.random.default_rng(116)
    t = g.integers(0, 256, size=(n_t, 32), dtype=np.uint8)
    c = np.bincount(np.concatenate([g.integers(0, n_t, size=n_out // 2), g.integers(0, 50, size=n_out // 4), np.full(n_out // 4, 40000)]), minlength=n_t).astype(np.uint32)
    dt, dc = torch.from_numpy(t).cuda(), torch.from_numpy(c.view(np.int32)).cuda()
    out = col.expand(ctx, dt, dc, n_out)
    assert np.array_equal(out.cpu().numpy(), np.repeat(t, c, axis=0))
    with pytest.raises(ValueError):
        col.expand(ctx, dt, dc, n_out - 1)
    s = col.expand(ctx, dt, dc, n_out + n_t, bias=1, out=torch.empty((n_out + n_t, 32), dtype=torch.uint8, device="cuda"))
    assert np.array_equal(s.cpu().numpy(), np.repeat(t, c + 1, axis=0))
    c2 = np.bincount(np.concatenate([g.integers(0, n_t, size=n_t // 2), np.full(n_t // 2, 77)]), minlength=n_t).astype(np.uint32)
    a_perm, s_perm = col.permuted_pair(ctx, dt, torch.from_numpy(c2.view(np.int32)).cuda())
    assert np.array_equal(a_perm.cpu().numpy(), np.repeat(t, c2, axis=0))
    heads = (np.cumsum(c2.astype(np.int64)) - c2)[c2 > 0]
    want_s = np.empty_like(t)
    filler = np.ones(n_t, dtype=bool)
    filler[heads] = False
    want_s[heads], want_s[filler] = t[c2 > 0], t[c2 == 0]
    assert np.array_equal(s_perm.cpu().numpy(), want_s)
    idx = torch.from_numpy(g.integers(-1, n_t, size=n_out).astype(np.int32)).cuda()
    got = col.gather(ctx, dt, idx).cpu().numpy()
    i = idx.cpu().numpy()
    assert np.array_equal(got, np.where((i < 0)[:, None], 0, t[np.maximum(i, 0)]))
    with pytest.raises(ValueError):
        col.gather(ctx, dt, torch.full((5,), n_t, dtype=torch.int32, device="cuda"))
