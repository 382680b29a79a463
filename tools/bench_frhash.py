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

Poseidon2 (MsmContext.poseidon2; --poseidon2-widths, empty: none) is timed against the EXISTING Poseidon kernel of the same t, R_F = 8 and the
same R_P, on the same states, the two ALTERNATED in one process; beside the measured ratio stand the ratio of the two product counts (what to
expect where the multiplier bounds both) and each kernel's fraction of the ceiling.  Its products, a pair under one reduction counted as 2:
t + R_F (t S + L) + L + R_P (S + 2 t), S = 3 or 4 products an S-box, L = 0, t or t + 4 products a layer (csrc/frhash_kernels.h).  Its constants
are drawn from a seeded generator: the time does not depend on them.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the
call and its chain ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.

usage: tools/bench_frhash.py [--log-n 20] [--widths 3,5,9,12] [--poseidon2-widths 3,4,8,12] [--calls 10] [--chain-calls 1] [--rounds 3]
                             [--ubench build/ubench_fqmul] [--no-chain]"""
import argparse
import os
import random
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


def poseidon2_rules(r, t):
    """(frh2_tidy_sums(t), frh2_bound(t), frh2_tidy_sbox(t)) of csrc/frhash_kernels.h over the field of order r, restated;
    tests/test_frhash2_host.py compares them with the kernel's own for every field and width"""
    headroom = (1 << 261) // r
    tidy_sums = t >= 8 and ((t // 2 + 3) ** 2 > headroom or t * (t // 2 + 2) + 2 > headroom)
    bound = 2 * t + 2 if t < 4 else 2 if t == 4 else 4 if tidy_sums else t // 2 + 2
    return tidy_sums, bound, (bound + 1) ** 2 > headroom


def products2(r, t, rf, rp):
    """the products of one Poseidon2 permutation as csrc/frhash_kernels.h issues them over the field of order r, a pair of fq_mul2 counted as 2"""
    tidy_sums, _, tidy_sbox = poseidon2_rules(r, t)
    sbox = 4 if tidy_sbox else 3
    layer = 0 if t < 4 else t + 4 if tidy_sums else t
    return t + rf * (t * sbox + layer) + layer + rp * (sbox + 2 * t)


def bench_poseidon2(c, curve, t, n, a, ns_per_product):
    """Poseidon2 against the existing Poseidon kernel: the same t, R_F, R_P and states, alternated"""
    rf, rp = 8, api.POSEIDON_PARTIAL_ROUNDS[t]
    r = api.SCALAR_FIELDS[curve]
    rnd = random.Random(74 + t)
    label = "%-9s poseidon2 t = %-2d R_P = %d n = 2^%d" % (curve, t, rp, n.bit_length() - 1)
    states = c.sample_scalars(n * t, 71).view(n, t, 32)
    out_old, out_new = torch.empty_like(states), torch.empty_like(states)
    old = c.poseidon(t, rf, rp)
    new = c.poseidon2(t, rf, rp, [rnd.randrange(r) for _ in range(rf * t + rp)], [rnd.randrange(r) for _ in range(t)])
    run_old = lambda: c.scalars_permute(old, states, out=out_old)  # noqa: E731
    run_new = lambda: c.scalars_permute(new, states, out=out_new)  # noqa: E731
    run_old(), run_new()
    t_old, t_new = [], []
    for _ in range(a.rounds):
        t_new.append(timed(run_new, a.calls))
        t_old.append(timed(run_old, a.calls))
    p_old, p_new = products(t, rf, rp), products2(r, t, rf, rp)
    faster = max(t_new) < min(t_old)
    line = "%s %s = %.2f ns per permutation  against poseidon %s = %.4f x  %s  products %d against %d = %.4f x" % (
        label, spread(t_new), statistics.mean(t_new) / n * 1e9, spread(t_old), statistics.mean(t_new) / statistics.mean(t_old),
        "FASTER beyond the spread of both" if faster else "NOT FASTER", p_new, p_old, p_new / p_old)
    if ns_per_product:
        line += "  fraction of the ceiling %.2f (poseidon %.2f)" % (p_new * n * ns_per_product * 1e-9 / statistics.mean(t_new), p_old * n * ns_per_product * 1e-9 / statistics.mean(t_old))
    print(line, flush=True)
    old.close()
    new.close()


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
    ap.add_argument("--poseidon2-widths", default="3,4,8,12")
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
    widths2 = [int(s) for s in a.poseidon2_widths.split(",") if s]
    for t in widths2:
        bench_poseidon2(c, "bn254", t, n, a, ns_per_product)
        torch.cuda.empty_cache()
    c.close()
    c = m.MsmContext(0, curve="bls12_381")
    bench_permute(c, "bls12_381", 3, n, a, ns_per_product)
    for t in widths2[-1:]:  # the widest: the one width at which this field tidies the position sums
        bench_poseidon2(c, "bls12_381", t, n, a, ns_per_product)
    c.close()
    api.frhash_release()
    api.frgate_release()


if __name__ == "__main__":
    main()
