#!/usr/bin/env python3
"""Timing of the polynomial-opening operations (MsmContext.scalars_eval .. scalars_powers, kzg_open: libmsm_frpoly.so) on one GPU, each against what
gives the same result on the other libraries, timed in the same process:
  eval                    scalars_scan(op="sum") of the same length (a sum costs a scan there)
  divide                  scalars_scan(op="product") of the same length (the same two-phase shape)
  dot                     scalars_mul, then scalars_scan(op="sum", totals=True)
  combine of 4 / 16 rows  scalars_mul, then 3 / 15 calls of scalars_mul_add
  powers                  a torch fill, then scalars_scan(op="product", exclusive=True)
  kzg_open at 2^20        the ctx.msm it ends in (BN254, 2^20 default bases)
The expectation in every pair is "the new call takes no longer" (kzg_open: stays below twice its MSM); a verdict line says MET or NOT MET.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the
new calls and their yardsticks ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  In-place operations run on their own
output again and again (an output is a valid input).  Each shape is checked in the run on sampled elements against Python integers.

usage: tools/bench_frpoly.py [--shapes bn254:10,bn254:16,bn254:20,bn254:24,pallas:20,...] [--calls 20] [--rounds 3] [--no-check] [--no-msm]"""
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
MAX_ELEMENTS = 1 << 26


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def at(t, idx):
    return [int.from_bytes(t[i].cpu().numpy().tobytes(), "little") for i in idx]


def check(c, r, n, a, b, rows, coeffs, rnd):
    """every operation once, sampled elements against Python integers -> list of the operations that are wrong"""
    idx = sorted(set(rnd.sample(range(1, n), min(4, n - 1)) + [n - 1])) if n > 1 else [0]
    bad = []
    z = rnd.randrange(r)
    q, y = c.scalars_divide(a, z, out=torch.empty_like(a), values=True)
    va, vq, vp = at(a, idx), at(q, idx), at(q, [i - 1 for i in idx])
    if [(x + z * h) % r for x, h in zip(va, vq)] != vp or at(q, [n - 1]) != [0] or (at(a, [0])[0] + z * at(q, [0])[0]) % r != int.from_bytes(y, "little"):
        bad.append("divide")
    if c.scalars_eval(a, z) != y:
        bad.append("eval")
    pw = c.scalars_powers(z, n, scale=3)
    if at(pw, idx) != [3 * pow(z, i, r) % r for i in idx]:
        bad.append("powers")
    if int.from_bytes(c.scalars_dot(a, pw), "little") != 3 * int.from_bytes(y, "little") % r:  # sum a[i] 3 z^i
        bad.append("dot")
    k = len(coeffs)
    got = c.scalars_combine(rows, coeffs)
    if at(got, idx) != [sum(cf * x for cf, x in zip(coeffs, at(rows, [j * n + i for j in range(k)]))) % r for i in idx]:
        bad.append("combine")
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
    rnd = random.Random(28)
    ctxs = {}
    for shape in a.shapes.split(","):
        curve, log_n = shape.split(":")
        log_n = int(log_n)
        n = 1 << log_n
        r = api.SCALAR_FIELDS[curve]
        if curve not in ctxs:
            ctxs[curve] = m.MsmContext(0, curve=curve)
        c = ctxs[curve]
        z, g = rnd.randrange(2, r), rnd.randrange(2, r)
        va, vb, vd, vs, vp, vm = (c.sample_scalars(n, 43 + k) for k in range(6))
        acc, pw = torch.empty_like(va), torch.empty_like(va)
        fill = torch.frombuffer(bytearray(g.to_bytes(32, "little")), dtype=torch.uint8).cuda()
        pairs = [("eval", lambda: c.scalars_eval(va, z), "scan sum", lambda: c.scalars_scan(vs, op="sum")),
                 ("divide, in place", lambda: c.scalars_divide(vd, z), "scan product", lambda: c.scalars_scan(vp, op="product")),
                 ("dot", lambda: c.scalars_dot(va, vb), "mul + scan sum with totals", lambda: c.scalars_scan(c.scalars_mul(vm, vb), op="sum", totals=True)),
                 ("powers", lambda: c.scalars_powers(g, n, out=pw), "fill + exclusive scan product",
                  lambda: c.scalars_scan(acc.copy_(fill.expand(n, 32)), op="product", exclusive=True))]
        rows, coeffs = {}, {}
        for k in (4, 16):
            if k * n > MAX_ELEMENTS:
                print("%-10s 2^%-2d combine of %d rows: %d x 2^%d scalars are more than a call takes (2^26): not timed" % (curve, log_n, k, k, log_n))
                continue
            rows[k] = c.sample_scalars(k * n, 60 + k)
            coeffs[k] = [rnd.randrange(r) for _ in range(k)]

            def chain(k=k):
                t, cf = rows[k], coeffs[k]
                c.scalars_mul(t[:n], cf[0], out=acc)
                for j in range(1, k):
                    c.scalars_mul_add(t[j * n:(j + 1) * n], cf[j], acc, out=acc)

            pairs.append(("combine of %d rows" % k, lambda k=k: c.scalars_combine(rows[k], coeffs[k], out=acc), "mul + %d x mul_add" % (k - 1), chain))
        bad = [] if a.no_check else check(c, r, n, va, vb, rows.get(4, va), coeffs.get(4, [5]), rnd)
        if curve == "bn254" and log_n == MSM_LOG_N and not a.no_msm:  # the whole opening against the MSM it ends in
            c.set_bases(c.sample_points(n, 41), endomorphism=None)
            pairs.append(("kzg_open (divide + msm)", lambda: c.kzg_open(va, z), "msm", lambda: c.msm(va)))
        for _, fn, _, ref in pairs:
            fn(), ref()
        t = {}
        for _ in range(a.rounds):
            for name, fn, ref_name, ref in pairs:
                t.setdefault(name, []).append(timed(fn, a.calls))
                t.setdefault(name + " / ref", []).append(timed(ref, a.calls))
        label = "%-10s 2^%-2d" % (curve, log_n)
        for name, _, ref_name, _ in pairs:
            new, ref = t[name], t[name + " / ref"]
            mn, mr = statistics.mean(new), statistics.mean(ref)
            bound = 2 * mr if name.startswith("kzg_open") else mr
            print("%s %-24s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)  against %-30s %9.3f ms/call (%.3f .. %.3f)  = %.2f x  %s" % (
                label, name, mn * 1e3, min(new) * 1e3, max(new) * 1e3, a.rounds, a.calls, ref_name, mr * 1e3, min(ref) * 1e3, max(ref) * 1e3, mn / mr,
                "MET" if mn <= bound else "NOT MET"))
        print("%s checked on sampled elements: %s" % (label, "unchecked" if a.no_check else ("ok" if not bad else "WRONG: " + ", ".join(bad))), flush=True)
        del va, vb, vd, vs, vp, vm, acc, pw, rows, pairs
        torch.cuda.empty_cache()
    for c in ctxs.values():
        c.close()
    api.frpoly_release()
    api.frvec_release()


if __name__ == "__main__":
    main()
