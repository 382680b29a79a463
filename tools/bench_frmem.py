#!/usr/bin/env python3
"""Timing of the memory-checking columns (msm_webgpu_amd.memory: libmsm_frmem.so) on one GPU: the stable argsort and the access counters at
n = 2^16, 2^20, 2^24 keys, declared widths of 16, 24, 32 and 64 bits, and three distributions -- `uniform` over the whole width, `all-equal`, and
`hot` (90 % one address, the rest uniform).

Yardsticks, in the same process -- what gave the same result before: torch.sort(stable=True) for the argsort, and for the counters that sort plus
the torch ops that derive rank, prev and (where there is a table: widths of 16 and 24 bits, n_t = 2^bits) counts from it.  Keys of 16 .. 32 bits are
int32 words for the library and, so that torch orders them as unsigned, int64 for torch; keys of 64 bits are int64 below 2^63 for both.  No bar is
set: a line gives both times and their ratio (new / old: below 1 the library is faster).  Per n, access is also put beside the
scalars_multiplicities (a table of 2^16) and the scalars_inverse of n scalars that a memory argument pays anyway.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream
has completed), old and new ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  The outputs are checked against the
yardstick's in the run.

usage: tools/bench_frmem.py [--log-n 16,20,24] [--bits 16,24,32,64] [--calls 20] [--rounds 3] [--no-check] [--no-prover]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402
from msm_webgpu_amd import api, memory  # noqa: E402

KINDS = ("uniform", "all-equal", "hot")


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def keys_of(kind, n, bits, gen):
    """-> (the keys as the library takes them, the same values as torch orders them: int64)"""
    top = 1 << min(bits, 63)
    if kind == "uniform":
        v = gen.integers(0, top, size=n, dtype=np.int64)
    elif kind == "all-equal":
        v = np.full(n, int(gen.integers(0, top)), dtype=np.int64)
    else:  # hot: 90 % one address
        v = np.where(gen.random(n) < 0.9, int(gen.integers(0, top)), gen.integers(0, top, size=n, dtype=np.int64))
    wide = torch.from_numpy(v).cuda()
    return (wide if bits > 32 else torch.from_numpy(v.astype(np.uint32).view(np.int32)).cuda()), wide


def torch_access(wide, n_t):
    """rank, prev and counts with torch: the stable sort, the runs' heads, a running maximum of their positions, two scatters, a bincount"""
    sk, perm = torch.sort(wide, stable=True)
    n = wide.numel()
    at = torch.arange(n, device=wide.device)
    head = torch.ones(n, dtype=torch.bool, device=wide.device)
    head[1:] = sk[1:] != sk[:-1]
    start = torch.cummax(torch.where(head, at, 0), 0).values
    rank, prev = torch.empty_like(at), torch.empty_like(at)
    rank[perm] = at - start
    prev[perm] = torch.where(head, -1, torch.roll(perm, 1))
    counts = torch.bincount(wide, minlength=n_t) if n_t else None
    return rank, prev, counts


def line(label, name, new, old, old_name, rounds, calls):
    mn, mo = statistics.mean(new), statistics.mean(old)
    print("%s %-30s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)  against %s %9.3f (%.3f .. %.3f)  new / old = %.2f x" % (
        label, name, mn * 1e3, min(new) * 1e3, max(new) * 1e3, rounds, calls, old_name, mo * 1e3, min(old) * 1e3, max(old) * 1e3, mn / mo), flush=True)
    return mn / mo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", default="16,20,24")
    ap.add_argument("--bits", default="16,24,32,64")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-prover", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    c = m.MsmContext(0, curve="bn254")
    gen = np.random.default_rng(47)
    ratios = {}
    for log_n in [int(s) for s in a.log_n.split(",")]:
        n = 1 << log_n
        for bits in [int(s) for s in a.bits.split(",")]:
            n_t = 1 << bits if bits <= 24 else None
            label = "n = 2^%-2d bits = %-2d" % (log_n, bits)
            for kind in KINDS:
                keys, wide = keys_of(kind, n, bits, gen)
                new_sort = lambda: memory.argsort(c, keys, bits=bits, sorted_keys=True)  # noqa: E731
                old_sort = lambda: torch.sort(wide, stable=True)  # noqa: E731
                new_acc = lambda: memory.access_counters(c, keys, table_size=n_t, bits=bits)  # noqa: E731
                old_acc = lambda: torch_access(wide, n_t)  # noqa: E731
                (perm, sk), (wk, wperm) = new_sort(), old_sort()
                (rank, prev, counts, _, _), (wrank, wprev, wcounts) = new_acc(), old_acc()
                verdict = "unchecked"
                if not a.no_check:
                    ok = torch.equal(perm.to(torch.int64), wperm) and torch.equal(wide[wperm], wk) and torch.equal(sk.view(keys.dtype), keys[wperm])
                    ok = ok and torch.equal(rank.to(torch.int64), wrank) and torch.equal(prev.to(torch.int64), wprev) and (n_t is None or torch.equal(counts.to(torch.int64), wcounts))
                    verdict = "ok" if ok else "WRONG"
                del perm, sk, wk, wperm, rank, prev, counts, wrank, wprev, wcounts
                ts, tso, ta, tao = [], [], [], []
                for _ in range(a.rounds):
                    tso.append(timed(old_sort, a.calls))
                    ts.append(timed(new_sort, a.calls))
                    tao.append(timed(old_acc, a.calls))
                    ta.append(timed(new_acc, a.calls))
                ratios["argsort", log_n, bits, kind] = line(label, "argsort, %s [%s]" % (kind, verdict), ts, tso, "torch.sort(stable)", a.rounds, a.calls)
                ratios["access", log_n, bits, kind] = line(label, "access%s, %s [%s]" % (" + counts" if n_t else "", kind, verdict), ta, tao, "torch sort + ops", a.rounds, a.calls)
                del keys, wide
                torch.cuda.empty_cache()
        if not a.no_prover:  # what a memory argument pays anyway, at this n: the lookup's count into 2^16 entries, and a batch inversion
            words = gen.integers(0, 1 << 32, size=(1 << 16, 8), dtype=np.uint64).astype(np.uint32)
            words[:, 7] &= 0x0FFFFFFF
            words[:, 0] = np.arange(1 << 16, dtype=np.uint32)
            table_values = torch.from_numpy(words.view(np.uint8).reshape(-1, 32)).cuda()
            addr = torch.from_numpy(gen.integers(0, 1 << 16, size=n)).cuda()
            f = table_values[addr].contiguous()
            addr32 = addr.to(torch.int32)
            table = c.lookup_table(table_values)
            m_out, inv_out = torch.empty((1 << 16, 32), dtype=torch.uint8, device="cuda"), torch.empty_like(f)
            acc = lambda: memory.access_counters(c, addr32, table_size=1 << 16, bits=16)  # noqa: E731
            count = lambda: c.scalars_multiplicities(table, f, out=m_out)  # noqa: E731
            inverse = lambda: c.scalars_inverse(f, out=inv_out)  # noqa: E731
            acc(), count(), inverse()
            ta, tc, ti = [], [], []
            for _ in range(a.rounds):
                ta.append(timed(acc, a.calls))
                tc.append(timed(count, a.calls))
                ti.append(timed(inverse, a.calls))
            label = "n = 2^%-2d bits = 16" % log_n
            line(label, "access + counts, uniform", ta, tc, "scalars_multiplicities", a.rounds, a.calls)
            line(label, "access + counts, uniform", ta, ti, "scalars_inverse", a.rounds, a.calls)
            table.close()
            del table_values, addr, f, addr32, m_out, inv_out
            torch.cuda.empty_cache()
    for what in ("argsort", "access"):
        r = [v for k, v in ratios.items() if k[0] == what]
        worst = max((v, k) for k, v in ratios.items() if k[0] == what)
        best = min((v, k) for k, v in ratios.items() if k[0] == what)
        print("%s: new / old from %.2f x (n = 2^%d, %d bits, %s) to %.2f x (n = 2^%d, %d bits, %s); the library is faster in %d of %d shapes" % (
            what, best[0], best[1][1], best[1][2], best[1][3], worst[0], worst[1][1], worst[1][2], worst[1][3], sum(v < 1 for v in r), len(r)), flush=True)
    c.close()
    memory.frmem_release()
    api.frlook_release()
    api.frvec_release()


if __name__ == "__main__":
    main()
