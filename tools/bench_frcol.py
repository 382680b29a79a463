#!/usr/bin/env python3
"""Timing of the lookup columns (msm_webgpu_amd.columns: libmsm_frcol.so) on one GPU, BN254, n = 2^20 looked-up elements: halo2's permuted pair
at n = n_t = 2^20, and the run expansion of n = 2^20 over n_t = 2^16 and 2^20 at bias 0 (halo2's A') and bias 1 (plookup's s, n + n_t outputs).
Yardsticks, in the same process: the scalars_multiplicities count of the same column -- what every caller pays immediately before -- and a
device-to-device copy of the output bytes.  A verdict line says MET (the call's mean is no longer than the count's) or NOT MET.

Count columns: `uniform` (every element a uniformly drawn table entry), `one-entry` (everything in one entry: one run of n), `all-ones` (every
entry n / n_t times: once each at n_t = n) and `witness-like` (90 % in entry 0, the rest uniform).

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream
has completed), the candidate and its yardsticks ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  The outputs are
checked in the run against torch.repeat_interleave (and, for S', the heads and fillers laid out with torch).  Also one halo2_lookup at 2^20 next
to ctx.msm of that length.

usage: tools/bench_frcol.py [--log-n 20] [--calls 20] [--rounds 3] [--no-check] [--no-prover]"""
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
from msm_webgpu_amd import api, columns  # noqa: E402

CURVE = "bn254"
KINDS = ("uniform", "one-entry", "all-ones", "witness-like")


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def table_keys(n_t, gen):
    """n_t x 32 bytes on the device: distinct random keys below r (top word below 2^28; word 0 is the index)"""
    words = gen.integers(0, 1 << 32, size=(n_t, 8), dtype=np.uint64).astype(np.uint32)
    words[:, 7] &= 0x0FFFFFFF
    words[:, 0] = np.arange(n_t, dtype=np.uint32)
    return torch.from_numpy(words.view(np.uint8).reshape(n_t, 32)).cuda()


def column(kind, keys, n, gen):
    """-> (the indices the column was drawn with, the column)"""
    n_t = keys.shape[0]
    if kind == "uniform":
        idx = gen.integers(0, n_t, size=n)
    elif kind == "one-entry":
        idx = np.full(n, 12345 % n_t)
    elif kind == "all-ones":
        idx = np.arange(n) % n_t
    else:  # witness-like: 90 % in entry 0
        idx = np.where(gen.random(n) < 0.9, 0, gen.integers(0, n_t, size=n))
    idx = torch.from_numpy(idx.astype(np.int64)).cuda()
    return idx, keys[idx].contiguous()


def line(label, name, new, rounds, calls, refs=()):
    mn = statistics.mean(new)
    text = "%s %-34s %8.3f ms/call (%.3f .. %.3f over %d rounds of %d)" % (label, name, mn * 1e3, min(new) * 1e3, max(new) * 1e3, rounds, calls)
    for ref_name, ref, judged in refs:
        mr = statistics.mean(ref)
        text += "  against %s %8.3f (%.3f .. %.3f) = %.2f x%s" % (ref_name, mr * 1e3, min(ref) * 1e3, max(ref) * 1e3, mn / mr, ("  MET" if mn <= mr else "  NOT MET") if judged else "")
    print(text, flush=True)
    return new


def want_pair(keys, cnt):
    """(A', S') by the definition, laid out with torch"""
    n = keys.shape[0]
    a = torch.repeat_interleave(keys, cnt, dim=0)
    heads = (torch.cumsum(cnt, 0) - cnt)[cnt > 0]
    s = torch.empty_like(keys)
    filler = torch.ones(n, dtype=torch.bool, device=keys.device)
    filler[heads] = False
    s[heads], s[filler] = keys[cnt > 0], keys[cnt == 0]
    return a, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--log-tables", default="16,20")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-prover", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    c = m.MsmContext(0, curve=CURVE)
    gen = np.random.default_rng(43)
    n = 1 << a.log_n
    for log_t in [int(s) for s in a.log_tables.split(",")]:
        n_t = 1 << log_t
        keys = table_keys(n_t, gen)
        table = c.lookup_table(keys)
        label = "%-6s n_t = 2^%-2d n = 2^%-2d" % (CURVE, log_t, a.log_n)
        m_out = torch.empty((n_t, 32), dtype=torch.uint8, device="cuda")
        outs = [torch.empty((n + n_t, 32), dtype=torch.uint8, device="cuda") for _ in range(4)]
        shapes = [("expand, bias 0", 0), ("expand, bias 1", 1)] + ([("pair", None)] if n_t == n else [])
        means = {}
        for kind in KINDS:
            idx, f = column(kind, keys, n, gen)
            _, cnt = c.scalars_multiplicities(table, f, counts=True)
            cnt64 = cnt.view(torch.int32).to(torch.int64)
            assert a.no_check or torch.equal(cnt64, torch.bincount(idx, minlength=n_t))
            for name, bias in shapes:
                n_out = n if bias is None else n + bias * n_t
                if bias is None:
                    call = lambda: columns.permuted_pair(c, keys, cnt, out=(outs[0][:n], outs[1][:n]))  # noqa: E731
                    nbytes = 2 * 32 * n_out
                else:
                    call = lambda: columns.expand(c, keys, cnt, n_out, bias=bias, out=outs[0][:n_out])  # noqa: E731
                    nbytes = 32 * n_out
                count = lambda: c.scalars_multiplicities(table, f, out=m_out)  # noqa: E731
                src, dst = outs[2].view(-1)[:nbytes], outs[3].view(-1)[:nbytes]  # (the pair writes two columns: a copy of as many bytes)
                copy = lambda: dst.copy_(src)  # noqa: E731
                call(), count(), copy()
                verdict = "unchecked"
                if not a.no_check:
                    if bias is None:
                        wa, ws = want_pair(keys, cnt64)
                        ok = torch.equal(outs[0][:n], wa) and torch.equal(outs[1][:n], ws)
                    else:
                        ok = torch.equal(outs[0][:n_out], torch.repeat_interleave(keys, cnt64 + bias, dim=0))
                    verdict = "ok" if ok else "WRONG"
                tn, tc, tm = [], [], []
                for _ in range(a.rounds):
                    tn.append(timed(call, a.calls))
                    tc.append(timed(count, a.calls))
                    tm.append(timed(copy, a.calls))
                line(label, "%s, %s [%s]" % (name, kind, verdict), tn, a.rounds, a.calls,
                     [("the count", tc, True), ("a copy of %d MiB" % (nbytes >> 20), tm, False)])
                means[name, kind] = tn
            del idx, f, cnt
        for name, _ in shapes:
            u = means[name, "uniform"]
            print("%s %s: %s; the uniform rounds spread %.3f .. %.3f ms" % (label, name, ", ".join(
                "%s / uniform = %.2f x" % (k, statistics.mean(means[name, k]) / statistics.mean(u)) for k in KINDS[1:]), min(u) * 1e3, max(u) * 1e3), flush=True)
        if not a.no_prover and n_t == n:  # the whole argument next to the commitment of the same length
            _, f = column("witness-like", keys, n, gen)
            c.set_bases(c.sample_points(n, 41), endomorphism=None)
            x = c.sample_scalars(n, 62)
            beta, gamma = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA0987654321
            _, _, _, total = columns.halo2_lookup(c, keys, f, beta, gamma)
            c.msm(x)
            th, tm = [], []
            for _ in range(a.rounds):
                th.append(timed(lambda: columns.halo2_lookup(c, keys, f, beta, gamma), a.calls))
                tm.append(timed(lambda: c.msm(x), a.calls))
            line(label, "halo2_lookup [%s]" % ("closes at one" if int.from_bytes(total, "little") == 1 else "WRONG"), th, a.rounds, a.calls, [("msm of 2^%d" % a.log_n, tm, False)])
            del f, x
        table.close()
        del keys, m_out, outs
        torch.cuda.empty_cache()
    c.close()
    columns.frcol_release()
    api.frlook_release()
    api.frvec_release()


if __name__ == "__main__":
    main()
