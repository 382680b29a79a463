#!/usr/bin/env python3
"""Timing of Poseidon on one GPU (MsmContext.scalars_permute, scalars_hash, merkle_tree: libmsm_frhash.so) against two yardsticks, neither of
them the code under test:

  the chain    the same permutation put together from scalars_gate calls, which is what a user did before: per round t gates for u = s + c (the
               round constant as the coefficient of a row of ones) and t gates for sum_j M[i][j] u_j^5 (u_j outside the S-box in a partial
               round) -- 2 t launches a round, on states stored column by column, which the chain needs and which is prepared OUTSIDE the timed
               region.  Its result is compared with the fused kernel's in the run.
  the ceiling  the multiplier's issue rate: products per permutation, R_F (3 t + t^2) + R_P (3 + t^2), times the time per product that
               tools/ubench_fqmul.hip measures in the same session (--ubench <binary>, built with hipcc -O3 -std=c++17 --offload-arch=gfx950
               tools/ubench_fqmul.hip -o <binary>; the inline-assembly multiplier at 3 waves per SIMD).
               The kernel pairs the matrix step's products under one reduction, so it issues fewer multiply-adds than that many single
               products: a fraction above 1 is possible and means just that.

A tree is reported against (n - 1) / (A - 1) permutations at the batch rate; a sponge against its permutations at the batch rate.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the
call and its chain ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.

usage: tools/bench_frhash.py [--log-n 20] [--widths 3,5,9,12] [--calls 10] [--chain-calls 1] [--rounds 3] [--ubench build/ubench_fqmul] [--no-chain]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402
from msm_webgpu_amd import api  # noqa: E402


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def spread(v):
    return "%9.3f ms (%.3f .. %.3f)" % (statistics.mean(v) * 1e3, min(v) * 1e3, max(v) * 1e3)


def products(t, rf, rp):
    return rf * (3 * t + t * t) + rp * (3 + t * t)


def ubench(path):
    """ns per product per lane over the whole GPU, from the micro-benchmark's line for the assembly multiplier at 3 waves per SIMD"""
    if not path or not os.path.exists(path):
        return None, "no micro-benchmark binary (%s): no ceiling" % path
    out = subprocess.run([path], capture_output=True, text=True, timeout=120).stdout
    hit = re.search(r"int29_asm.*waves/SIMD=3\s+[\d.]+ ms\s+([\d.]+) ns per wave-multiplication per SIMD\s+\(([\d.]+) G modmul/s per GPU\)", out)
    if not hit:
        return None, "the micro-benchmark's output has no int29_asm line at 3 waves per SIMD"
    return 1.0 / float(hit.group(2)), "tools/ubench_fqmul.hip, this session: int29_asm at 3 waves/SIMD %s ns per wave-multiplication per SIMD, %s G products/s" % (
        hit.group(1), hit.group(2))


def chain(c, cols, u, t, rf, rp, rc, mds):
    """the permutation of the states in cols[0 .. t) (cols[t]: ones) by 2 t gates a round; the result is in cols[0 .. t)"""
    for k in range(rf + rp):
        full = k < rf // 2 or k >= rf // 2 + rp
        for i in range(t):
            c.scalars_gate(cols, [(1, (i,)), (rc[k * t + i], (t,))], batch=t + 1, out=u[i])
        for i in range(t):
            c.scalars_gate(u, [(mds[i][j], (j,) * 5 if full or j == 0 else (j,)) for j in range(t)], batch=t + 1, out=cols[i])


def bench_permute(c, curve, t, n, a, ns_per_product):
    rf, rp = 8, api.POSEIDON_PARTIAL_ROUNDS[t]
    rc, mds = api.poseidon_parameters(curve, t, rf, rp)
    label = "%-9s permute t = %-2d n = 2^%d" % (curve, t, n.bit_length() - 1)
    states = c.sample_scalars(n * t, 71).view(n, t, 32)
    out = torch.empty_like(states)
    h = c.poseidon(t, rf, rp)
    fused = lambda: c.scalars_permute(h, states, out=out)  # noqa: E731
    fused()
    tc = None
    if not a.no_chain:
        one = int(1).to_bytes(32, "little")
        cols = torch.empty((t + 1, n, 32), dtype=torch.uint8, device="cuda")
        cols[:t] = states.transpose(0, 1)
        cols[t] = torch.frombuffer(bytearray(one), dtype=torch.uint8).cuda()
        u = cols.clone()
        chain(c, cols, u, t, rf, rp, rc, mds)
        same = torch.equal(cols[:t].transpose(0, 1).contiguous(), out)
        print("%s the chain of %d gates and the fused kernel agree on all %d states: %s" % (label, 2 * t * (rf + rp), n, "ok" if same else "WRONG"), flush=True)
        tc = []
    tf = []
    for _ in range(a.rounds):
        tf.append(timed(fused, a.calls))
        if tc is not None:
            tc.append(timed(lambda: chain(c, cols, u, t, rf, rp, rc, mds), a.chain_calls))
    mean = statistics.mean(tf)
    line = "%s %s = %.2f ns per permutation" % (label, spread(tf), mean / n * 1e9)
    if tc is not None:
        beaten = max(tf) < min(tc)
        line += "  against the chain %s = %.4f x  %s" % (spread(tc), mean / statistics.mean(tc), "BEATEN beyond the spread of both" if beaten else "NOT BEATEN")
    if ns_per_product:
        ceiling = products(t, rf, rp) * n * ns_per_product * 1e-9
        line += "  ceiling (%d products) %.3f ms: fraction %.2f" % (products(t, rf, rp), ceiling * 1e3, ceiling / mean)
    print(line, flush=True)
    h.close()
    return mean / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--widths", default="3,5,9,12")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--chain-calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ubench", default=os.path.join(ROOT, "build", "ubench_fqmul"))
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    ns_per_product, note = ubench(a.ubench)
    print(note, flush=True)
    n = 1 << a.log_n
    c = m.MsmContext(0, curve="bn254")
    rate = {}
    for t in [int(s) for s in a.widths.split(",")]:
        rate[t] = bench_permute(c, "bn254", t, n, a, ns_per_product)
        torch.cuda.empty_cache()
    # sponges: rows of length 2 (one permutation each, t = 3) and of length 64 (32 permutations each)
    if 3 in rate:
        h = c.poseidon(3)
        for rows, length in ((n, 2), (n >> 4, 64)):
            data = c.sample_scalars(rows * length, 72)
            out = torch.empty((rows, 32), dtype=torch.uint8, device="cuda")
            c.scalars_hash(h, data, length, batch=rows, out=out)
            th = [timed(lambda: c.scalars_hash(h, data, length, batch=rows, out=out), a.calls) for _ in range(a.rounds)]
            perms = rows * ((length + 1) // 2)
            print("bn254     hash    t = 3  %d rows of %d: %s  against %d permutations at the batch rate %.3f ms = %.2f x" % (
                rows, length, spread(th), perms, perms * rate[3] * 1e3, statistics.mean(th) / (perms * rate[3])), flush=True)
        h.close()
    # trees: 2^log_n leaves at arity 2, 4^(log_n / 2) at arity 4
    for t, leaves in ((3, n), (5, 1 << (a.log_n & ~1))):
        if t not in rate:
            continue
        h = c.poseidon(t, capacity=(1 << (t - 1)) - 1, out_at=1)
        data = c.sample_scalars(leaves, 73)
        count = (leaves - 1) // (t - 2)
        nodes = torch.empty((count, 32), dtype=torch.uint8, device="cuda")
        c.merkle_tree(h, data, out=nodes)
        tm = [timed(lambda: c.merkle_tree(h, data, out=nodes), a.calls) for _ in range(a.rounds)]
        levels = len(c._merkle_levels(h, leaves))
        print("bn254     merkle  arity %d  %d leaves, %d levels: %s  against %d permutations at the batch rate %.3f ms = %.2f x" % (
            t - 1, leaves, levels, spread(tm), count, count * rate[t] * 1e3, statistics.mean(tm) / (count * rate[t])), flush=True)
        h.close()
    c.close()
    c = m.MsmContext(0, curve="bls12_381")
    bench_permute(c, "bls12_381", 3, n, a, ns_per_product)
    c.close()
    api.frhash_release()
    api.frgate_release()


if __name__ == "__main__":
    main()
