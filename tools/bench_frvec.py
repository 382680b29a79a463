#!/usr/bin/env python3
"""Timing of the scalar-field vector operations (MsmContext.scalars_add .. scalars_scan: libmsm_frvec.so) on one GPU against three yardsticks timed
in the same process, none of them the code under test:
  (a) a device-to-device copy that moves the bytes the operation moves (its reads plus its writes);
  (b) the forward NTT of the same length (scalars_fft) -- the step before these operations in a prover;
  (c) ctx.msm of 2^20 scalars on a context with default bases -- the step after them.
The conditions (the issue's): map and scan at 2^20 take no longer than the 2^20 NTT; the inverse's streaming part per element -- (t(2^24) -
t(2^20)) / (2^24 - 2^20) -- stays at or below the NTT's, its fixed part (the time at n = one tile, one Fermat chain) is reported apart; the whole
grand-product chain (add, 2 x mul_add, inverse, mul, exclusive product scan) at 2^20 stays below the MSM of 2^20 scalars.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the
operations and the yardsticks ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  Every operation runs in place on its own
output again and again (an output is a valid input).  Each timed shape is checked in the run on sampled elements against Python integers (a map
directly; an inverse by out * a = 1; a scan by out[i] = out[i - 1] o a[i]).  Kernel times proper come from a run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_frvec.py ...`.

usage: tools/bench_frvec.py [--shapes bn254:16,bn254:20,bn254:24,pallas:20,...] [--calls 20] [--rounds 3] [--no-check] [--no-msm]"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402
from msm_webgpu_amd import api  # noqa: E402

MSM_LOG_N = 20
TILE = 1024


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def at(t, idx):
    return [int.from_bytes(t[i].cpu().numpy().tobytes(), "little") for i in idx]


def check(c, r, n, a, b, cc, rnd):
    """every operation once on copies, sampled elements against Python integers -> list of the operations that are wrong"""
    idx = sorted(set(rnd.sample(range(1, n), min(4, n - 1)) + [n - 1])) if n > 1 else [0]
    prev = [i - 1 for i in idx]
    va, vb, vc, vp = at(a, idx), at(b, idx), at(cc, idx), at(a, prev)
    bad = []
    k = 0x1234567
    for name, got, want in (("add", c.scalars_add(a.clone(), b), [(x + y) % r for x, y in zip(va, vb)]),
                            ("mul", c.scalars_mul(a.clone(), b), [x * y % r for x, y in zip(va, vb)]),
                            ("mul_add", c.scalars_mul_add(a.clone(), b, cc), [(x * y + z) % r for x, y, z in zip(va, vb, vc)]),
                            ("mul_add const", c.scalars_mul_add(a.clone(), k, k + 1), [(x * k + k + 1) % r for x in va])):
        if at(got, idx) != want:
            bad.append(name)
    inv = c.scalars_inverse(a.clone())
    if [x * y % r for x, y in zip(at(inv, idx), va)] != [1 if x else 0 for x in va]:
        bad.append("inverse")
    for op, f in (("sum", lambda x, y: (x + y) % r), ("product", lambda x, y: x * y % r)):
        s = c.scalars_scan(a.clone(), op=op)
        if [f(x, y) for x, y in zip(at(s, prev), va)] != at(s, idx) or at(s, [0]) != at(a, [0]):
            bad.append("scan " + op)
    s, tot = c.scalars_scan(a.clone(), op="product", exclusive=True, totals=True)
    if [x * y % r for x, y in zip(at(s, prev), vp)] != at(s, idx) or at(s, [0]) != [1] or at(s, [n - 1])[0] * at(a, [n - 1])[0] % r != int.from_bytes(tot, "little"):
        bad.append("scan product exclusive")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bn254:10,bn254:16,bn254:20,bn254:24,pallas:20,vesta:20,bls12_381:20")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-msm", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    rnd = random.Random(27)
    ctxs = {}
    means = {}
    for shape in a.shapes.split(","):
        curve, log_n = shape.split(":")
        log_n = int(log_n)
        n = 1 << log_n
        r = api.SCALAR_FIELDS[curve]
        if curve not in ctxs:
            c = m.MsmContext(0, curve=curve)
            msm_s = None
            if not a.no_msm and curve == "bn254":  # the MSM yardstick: 2^20 default bases and 2^20 scalars
                c.set_bases(c.sample_points(1 << MSM_LOG_N, 41), endomorphism=None)
                msm_s = c.sample_scalars(1 << MSM_LOG_N, 42)
            ctxs[curve] = (c, msm_s)
        c, msm_s = ctxs[curve]
        va, vb, vc = (c.sample_scalars(n, 43 + k) for k in range(3))
        nt = va.clone()
        bad = [] if a.no_check else check(c, r, n, va, vb, vc, rnd)
        k1, k2 = rnd.randrange(r), rnd.randrange(r)
        # name -> (call, vectors moved: reads + writes)
        ops = {"add  a + b": (lambda: c.scalars_add(va, vb), 3), "mul  a * b": (lambda: c.scalars_mul(va, vb), 3),
               "mul_add  a * b + c": (lambda: c.scalars_mul_add(va, vb, vc), 4), "mul_add  a * k1 + k2": (lambda: c.scalars_mul_add(va, k1, k2), 2),
               "inverse": (lambda: c.scalars_inverse(va), 2), "scan sum": (lambda: c.scalars_scan(va, op="sum"), 3 if n > TILE else 2),
               "scan product": (lambda: c.scalars_scan(va, op="product"), 3 if n > TILE else 2),
               "scan product, exclusive": (lambda: c.scalars_scan(va, op="product", exclusive=True, totals=True), 3 if n > TILE else 2)}

        def chain():  # the permutation argument's grand product, from f, id, sigma (here: va, vb, vc) to z
            c.scalars_add(va, k2)
            c.scalars_mul_add(vb, k1, va)
            c.scalars_mul_add(vc, k1, va)
            c.scalars_inverse(vc)
            c.scalars_mul(vb, vc)
            c.scalars_scan(vb, op="product", exclusive=True, totals=True)

        ops["grand-product chain (6 calls)"] = (chain, (2, 3, 3, 2, 3, 3))  # (every call's own vectors)
        copies = {}
        for moved in sorted({v[1] for v in ops.values() if isinstance(v[1], int)}):  # a copy of moved / 2 vectors reads and writes `moved` vectors' bytes
            src = torch.empty(moved * n * 16, dtype=torch.uint8, device="cuda")
            copies[moved] = (src, torch.empty_like(src))
        runs = {name: fn for name, (fn, _) in ops.items()}
        for moved, (src, dst) in copies.items():
            runs["copy %d" % moved] = (lambda s=src, d=dst: d.copy_(s))
        runs["ntt"] = lambda: c.scalars_fft(nt, log_n)
        if msm_s is not None:
            runs["msm"] = lambda: c.msm(msm_s)
        for fn in runs.values():
            fn()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(timed(fn, a.calls))
        mean = {k: statistics.mean(v) for k, v in t.items()}
        means[(curve, log_n)] = mean
        label = "%-10s 2^%-2d" % (curve, log_n)
        print("%s %-30s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)" % (label, "ntt forward, in place", mean["ntt"] * 1e3, min(t["ntt"]) * 1e3, max(t["ntt"]) * 1e3,
                                                                             a.rounds, a.calls))
        if "msm" in t:
            print("%s %-30s %9.3f ms/call (%.3f .. %.3f)" % (label, "msm 2^20, default bases", mean["msm"] * 1e3, min(t["msm"]) * 1e3, max(t["msm"]) * 1e3))
        for name, (_, moved) in ops.items():
            cp = mean["copy %d" % moved] if isinstance(moved, int) else sum(mean["copy %d" % k] for k in moved)
            line = "%s %-30s %9.3f ms/call (%.3f .. %.3f)  = %.2f x copy of its %d vectors (%.3f ms)  = %.2f x ntt" % (
                label, name, mean[name] * 1e3, min(t[name]) * 1e3, max(t[name]) * 1e3, mean[name] / cp, moved if isinstance(moved, int) else sum(moved), cp * 1e3,
                mean[name] / mean["ntt"])
            if "msm" in t:
                line += "  = %.3f x msm(2^20)" % (mean[name] / mean["msm"])
            print(line)
        print("%s checked on sampled elements: %s; last call (launches, levels) %s" % (label, "unchecked" if a.no_check else ("ok" if not bad else "WRONG: " + ", ".join(bad)),
                                                                                       api.frvec_last()), flush=True)
        del va, vb, vc, nt, copies, runs, ops
        torch.cuda.empty_cache()
    # the conditions
    for curve in sorted({k[0] for k in means}):
        m20 = means.get((curve, 20))
        if m20:
            for name in m20:
                if name.startswith(("add", "mul", "scan")):
                    print("verdict %-10s %-30s at 2^20 <= ntt at 2^20 (%.3f <= %.3f ms): %s" % (curve, name, m20[name] * 1e3, m20["ntt"] * 1e3,
                                                                                             "MET" if m20[name] <= m20["ntt"] else "NOT MET"))
            if "msm" in m20:
                ch = m20["grand-product chain (6 calls)"]
                print("verdict %-10s grand-product chain at 2^20 < msm of 2^20 (%.3f < %.3f ms): %s" % (curve, ch * 1e3, m20["msm"] * 1e3, "MET" if ch < m20["msm"] else "NOT MET"))
        m24, m10 = means.get((curve, 24)), means.get((curve, 10))
        if m10:
            print("inverse   %-10s fixed part (n = one tile of %d: one Fermat chain): %.3f ms" % (curve, TILE, m10["inverse"] * 1e3))
        if m20 and m24:
            per = lambda k: (m24[k] - m20[k]) / ((1 << 24) - (1 << 20)) * 1e12  # noqa: E731
            print("verdict %-10s inverse streaming %.1f ps/element <= ntt streaming %.1f ps/element: %s" % (curve, per("inverse"), per("ntt"),
                                                                                                         "MET" if per("inverse") <= per("ntt") else "NOT MET"))
    for c, _ in ctxs.values():
        c.close()
    api.frvec_release()
    api.fr_release()


if __name__ == "__main__":
    main()
