#!/usr/bin/env python3
"""Timing of the lookup step of a logUp argument (MsmContext.lookup_table, scalars_multiplicities: libmsm_frlook.so) on one GPU, BN254, 2^20 looked-up
elements, against the inversion that logUp pays per looked-up element anyway (scalars_inverse of the same 2^20 elements), in the same process.
A verdict line says MET (the count's mean is no longer than the inversion's) or NOT MET.

Tables: n_t = 2^16, a range table (keys 0 .. 2^16 - 1: 2 MiB of keys), and n_t = 2^20, random keys with key 0 = 0 (32 MiB of keys).  Looked-up
columns f of n = 2^20: `uniform` (every element a uniformly drawn table entry), `all-equal` (one table entry, the worst case for atomics that
are not aggregated) and `witness-like` (90 % zeros -- table entry 0 --, the rest uniform).

Reported per table and column: create (msm_frlook_create_device: copy, clear, build, one synchronisation), count into m (count + finish, one
synchronisation), the count against the inversion, and all-equal against uniform.  Also a whole MsmContext.logup over one column and the 2^16
table next to ctx.msm of 2^20 scalars.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the
count and the inversion ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  The counts are checked in the run against
torch.bincount of the indices the column was drawn with.

usage: tools/bench_frlook.py [--log-n 20] [--calls 20] [--rounds 3] [--no-check] [--no-prover]"""
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
from msm_webgpu_amd import api  # noqa: E402

CURVE = "bn254"


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def table_keys(log_t, gen):
    """n_t x 32 bytes on the device: a range table at 2^16, else random keys below r (top word below 2^28) with key 0 = 0"""
    n_t = 1 << log_t
    words = np.zeros((n_t, 8), dtype=np.uint32)
    if log_t <= 16:
        words[:, 0] = np.arange(n_t, dtype=np.uint32)
    else:
        words[:] = gen.integers(0, 1 << 32, size=(n_t, 8), dtype=np.uint64).astype(np.uint32)
        words[:, 7] &= 0x0FFFFFFF
        words[0] = 0
    return torch.from_numpy(words.view(np.uint8).reshape(n_t, 32)).cuda()


def column(kind, keys, n, gen):
    """-> (the indices the column was drawn with, the column)"""
    n_t = keys.shape[0]
    if kind == "uniform":
        idx = gen.integers(0, n_t, size=n)
    elif kind == "all-equal":
        idx = np.full(n, 12345 % n_t)
    else:  # witness-like: 90 % zeros
        idx = np.where(gen.random(n) < 0.9, 0, gen.integers(0, n_t, size=n))
    idx = torch.from_numpy(idx.astype(np.int64)).cuda()
    return idx, keys[idx].contiguous()


def line(label, name, new, rounds, calls, ref=None, ref_name="", judged=False):
    mn = statistics.mean(new)
    text = "%s %-28s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)" % (label, name, mn * 1e3, min(new) * 1e3, max(new) * 1e3, rounds, calls)
    if ref is not None:
        mr = statistics.mean(ref)
        text += "  against %-24s %9.3f ms/call (%.3f .. %.3f)  = %.2f x  %s" % (ref_name, mr * 1e3, min(ref) * 1e3, max(ref) * 1e3, mn / mr,
                                                                               ("MET" if mn <= mr else "NOT MET") if judged else "(reported)")
    print(text, flush=True)
    return mn


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
    gen = np.random.default_rng(41)
    n = 1 << a.log_n
    scratch = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    for log_t in [int(s) for s in a.log_tables.split(",")]:
        keys = table_keys(log_t, gen)
        n_t = keys.shape[0]
        label = "%-6s n_t = 2^%-2d n = 2^%-2d" % (CURVE, log_t, a.log_n)
        made = []

        def create():
            made.append(c.lookup_table(keys))
            if len(made) > 1:
                made.pop(0).close()

        create()
        line(label, "create", [timed(create, a.calls) for _ in range(a.rounds)], a.rounds, a.calls)
        table = made[0]
        assert table.distinct == n_t
        m_out = torch.empty((n_t, 32), dtype=torch.uint8, device="cuda")
        means = {}
        for kind in ("uniform", "all-equal", "witness-like"):
            idx, f = column(kind, keys, n, gen)

            def count():
                c.scalars_multiplicities(table, f, out=m_out)

            def inverse():
                c.scalars_inverse(f, out=scratch)

            count(), inverse()
            verdict = "unchecked"
            if not a.no_check:
                _, got = c.scalars_multiplicities(table, f, counts=True)
                ok = torch.equal(got.view(torch.int32).to(torch.int64), torch.bincount(idx, minlength=n_t))
                ok = ok and torch.equal(m_out.view(torch.int32).view(n_t, 8)[:, 0].to(torch.int64), torch.bincount(idx, minlength=n_t))
                verdict = "ok" if ok else "WRONG"
            tc, ti = [], []
            for _ in range(a.rounds):
                tc.append(timed(count, a.calls))
                ti.append(timed(inverse, a.calls))
            means[kind] = line(label, "count, %s [%s]" % (kind, verdict), tc, a.rounds, a.calls, ti, "scalars_inverse of 2^%d" % a.log_n, judged=True)
            del idx, f
        print("%s all-equal / uniform = %.2f x, witness-like / uniform = %.2f x" % (label, means["all-equal"] / means["uniform"], means["witness-like"] / means["uniform"]),
              flush=True)
        if not a.no_prover and log_t <= 16:  # the whole column preparation next to the commitment of the same length
            _, f = column("witness-like", keys, n, gen)
            c.set_bases(c.sample_points(n, 41), endomorphism=None)
            x = c.sample_scalars(n, 62)
            beta = 0x1234567890ABCDEF1234567890ABCDEF
            c.logup(keys, f, beta), c.msm(x)
            tl, tm = [], []
            for _ in range(a.rounds):
                tl.append(timed(lambda: c.logup(keys, f, beta), a.calls))
                tm.append(timed(lambda: c.msm(x), a.calls))
            line(label, "logup (one column)", tl, a.rounds, a.calls, tm, "msm of 2^%d" % a.log_n)
            del f, x
        table.close()
        del keys, m_out
        torch.cuda.empty_cache()
    c.close()
    api.frlook_release()
    api.frvec_release()


if __name__ == "__main__":
    main()
