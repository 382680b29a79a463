#!/usr/bin/env python3
"""Timing of the batch scalar multiplication calls (msm_hip_mul_each_device / msm_hip_mul_base_device) on one GPU.

Protocol: device-resident scalars and output, every shape warmed up, then `--calls` calls timed back to back (each call returns when its
output is complete) and the variants of a shape ALTERNATED `--rounds` times in one process, so that a drift of the clocks falls on all of them;
the spread over the rounds is printed beside every mean.  Run the command again for the spread between processes.

Per shape it prints ms per call, ns per output, the multiply-adds per output counted from the path taken (csrc/g1.h, csrc/scalar_mul.h), and the
share of the v_mad_u64_u32 issue ceiling (profiles/r01_ubench_valu_rates.txt: 2.35 ns per wave instruction and SIMD at two or more waves) that
this amounts to.  For comparison the same share is printed for k_smvp_chunks, from the stage timer of an MSM at 2^20 in the same process.
Kernel times proper come from a run of this script under `rocprofv3 --kernel-trace --stats -- python tools/bench_mul.py ...`.

usage: tools/bench_mul.py [--curves bn254,bls12_381,bn254_g2] [--logn 16,20,22] [--calls 20] [--rounds 3] [--oracle] [--crossover]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402

MAD_NS = 2.35  # ns per v_mad_u64_u32 wave instruction and SIMD (measured issue ceiling)
LIMBS = {"bn254": 9, "grumpkin": 9, "pallas": 9, "vesta": 9, "bls12_381": 14, "bn254_g2": 9, "bls12_381_g2": 14}
G2 = ("bn254_g2", "bls12_381_g2")
PRIME_ORDER = ("bn254", "grumpkin", "pallas", "vesta")


def mads(curve):
    """multiply-adds of one field product / square / two-product sum (L limbs: 2 L^2, L (L + 1) / 2 + L^2, 3 L^2; in Fq2 a product is two
    two-product sums, a square two products, a two-product sum two four-product sums of 5 L^2)"""
    L = LIMBS[curve]
    mul, sqr, mul2 = 2 * L * L, L * (L + 1) // 2 + L * L, 3 * L * L
    if curve in G2:
        return 2 * mul2, 2 * mul, 2 * 5 * L * L
    return mul, sqr, mul2


def path_mads(curve, endo):
    """(issued, useful) multiply-adds per output: a wave issues the ladder's addition in every step, a lane needs it in 3 of 4 (endomorphism)
    or 1 of 2 (plain) steps; + the normalisation (9 products, 2 conversions, 1 / 16 of a Fermat inversion)"""
    mul, sqr, mul2 = mads(curve)
    dbl = 3 * sqr + 6 * mul
    madd = 6 * mul + 2 * sqr + mul2
    bits = {"bls12_381": 381, "bls12_381_g2": 381}.get(curve, 254)
    inv = bits * sqr + (bits // 2) * mul
    norm = 13 * mul + inv // 16
    if endo:
        setup = madd + 9 * mul
        return 127 * (dbl + madd) + setup + norm, 127 * dbl + 95 * madd + setup + norm
    rb = 254 if curve in ("bn254", "bn254_g2", "grumpkin") else 255  # the plain ladder's steps: r's bit length
    return rb * (dbl + madd) + norm, rb * dbl + (rb // 2) * madd + norm


def ceiling_share(total_mads, seconds, cus):
    return total_mads * MAD_NS * 1e-9 / (cus * 4 * 64) / seconds


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def crossover(curve, calls):
    """mul_base through the broadcast ladder against the table forced at every even digit width, n = 2^10 .. 2^20: per (n, C) the time of a call
    with the table held, and of the call that builds it -- the figures the table threshold and the C-by-n policy are set from"""
    c = m.MsmContext(0, curve=curve)
    pts = c.sample_points(16, 21)
    c.set_bases(pts, endomorphism=None if curve in PRIME_ORDER else False)
    print("%s: mul_base crossover, ms per call (ladder | per C: held / first call with the build)" % curve)
    for logn in (10, 12, 13, 14, 16, 18, 20):
        n = 1 << logn
        s = c.sample_scalars(n, 22)
        out = torch.empty((n, c.pb), dtype=torch.uint8, device="cuda")
        k = max(3, min(calls, (1 << 22) // n))
        c.mul_policy("never")
        c.mul_base(0, s, out=out)
        row = ["2^%-2d ladder %8.3f" % (logn, timed(lambda: c.mul_base(0, s, out=out), k) * 1e3)]
        for bits in (8, 10, 12, 14, 16):
            c.mul_policy(1, bits)
            c.set_bases(pts, endomorphism=None if curve in PRIME_ORDER else False)  # drops the table
            first = timed(lambda: c.mul_base(0, s, out=out), 1)
            held = timed(lambda: c.mul_base(0, s, out=out), k)
            row.append("C=%-2d %8.3f / %8.3f" % (bits, held * 1e3, first * 1e3))
        c.mul_policy(0, 0)
        c.set_bases(pts, endomorphism=None if curve in PRIME_ORDER else False)
        c.mul_base(0, s, out=out)
        row.append("policy: path %d C=%d" % c.mul_last()[:2])
        print("   ".join(row), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254")
    ap.add_argument("--logn", default="16,20")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--oracle", action="store_true", help="also time the CPU oracle's scalar multiplication on 2048 of the inputs (context, one thread)")
    ap.add_argument("--crossover", action="store_true", help="only the mul_base ladder / table crossover table of each curve")
    a = ap.parse_args()
    if a.crossover:
        for curve in a.curves.split(","):
            crossover(curve, a.calls)
        return
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), cus))
    for curve in a.curves.split(","):
        for logn in (int(x) for x in a.logn.split(",")):
            n = 1 << logn
            c = m.MsmContext(0, curve=curve)
            pts = c.sample_points(n, 11)
            s = c.sample_scalars(n, 12)
            out = torch.empty((n, c.pb), dtype=torch.uint8, device="cuda")
            c.set_bases(pts, endomorphism=None if curve in PRIME_ORDER else False)
            # variants: (name, call, endomorphism ladder?)
            def base_ladder():
                c.mul_policy("never")
                try:
                    c.mul_base(0, s, out=out)
                finally:
                    c.mul_policy(0, 0)
            # (mul_base by the policy: the table is held after the warm-up call, so the timed calls do not build it; the first call is timed apart)
            variants = [("mul_each", lambda: c.mul_each(s, out=out), curve in PRIME_ORDER),
                        ("mul_base broadcast ladder (forced)", base_ladder, curve in PRIME_ORDER),
                        ("mul_base policy (table held)", lambda: c.mul_base(0, s, out=out), "table")]
            if curve not in PRIME_ORDER and curve != "bls12_381":  # (the G2 samplers draw from the subgroup: the caller may vouch for the order;
                variants.append(("mul_each order_r", lambda: c.mul_each(s, bases_order_r=True, out=out), True))  # BLS12-381 G1's sampler does not promise it)
            if curve in PRIME_ORDER and hasattr(c, "mul_force_ladder"):
                def plain():
                    c.mul_force_ladder(1)
                    try:
                        c.mul_each(s, out=out)
                    finally:
                        c.mul_force_ladder(0)
                variants.append(("mul_each plain ladder (forced)", plain, False))
            t_first = timed(lambda: c.mul_base(0, s, out=out), 1)  # builds the table
            first_bits = c.mul_last()[1]
            for _, fn, _ in variants:
                fn()
            times = {name: [] for name, _, _ in variants}
            for _ in range(a.rounds):
                for name, fn, _ in variants:
                    times[name].append(timed(fn, a.calls))
            for name, _, endo in variants:
                t = times[name]
                mean = statistics.mean(t)
                if endo == "table":
                    mul, sqr, mul2 = mads(curve)
                    rb = 254 if curve in ("bn254", "bn254_g2", "grumpkin") else 255
                    w = (rb + 1 + first_bits) // first_bits if first_bits else 0
                    issued = useful = w * (6 * mul + 2 * sqr + mul2) + 13 * mul
                    name = "%s C=%d" % (name, first_bits)
                else:
                    issued, useful = path_mads(curve, endo)
                print("%-13s 2^%d %-32s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)  %8.1f ns/output  mads/output issued %d useful %d  ceiling share issued %.2f useful %.2f"
                      % (curve, logn, name, mean * 1e3, min(t) * 1e3, max(t) * 1e3, a.rounds, a.calls, mean / n * 1e9, issued, useful,
                         ceiling_share(issued * n, mean, cus), ceiling_share(useful * n, mean, cus)))
            print("%-13s 2^%d %-32s %9.3f ms: the first mul_base call, which builds the table (C = %d)" % (curve, logn, "mul_base first call", t_first * 1e3, first_bits))
            if curve == "bn254" and logn == 20:  # the yardstick: the SMVP kernel of an MSM over the same bases, from the stage timer
                c.set_stage_timing(2)
                c.set_bases(pts, endomorphism=True)
                c.msm(s)
                smvp = [0.0] * a.rounds
                for k in range(a.rounds):
                    c.msm(s)
                    smvp[k] = c.stage_ms()["smvp"] * 1e-3
                mul, sqr, mul2 = mads(curve)
                adds = 16 * n  # 2n inputs x 8 half-length windows
                t = statistics.mean(smvp)
                print("%-13s 2^%d %-32s %9.3f ms (%.3f .. %.3f)  ceiling share %.2f" % (curve, logn, "k_smvp_chunks (stage timer, 16 n additions assumed)", t * 1e3, min(smvp) * 1e3,
                      max(smvp) * 1e3, ceiling_share(adds * (6 * mul + 2 * sqr + mul2), t, cus)))
            if a.oracle:
                import importlib
                orc = importlib.import_module("oracle.cpu" if curve == "bn254" else "oracle.cpu_" + curve)
                k = min(n, 2048)
                ph, sh = pts[:k].cpu().numpy().tobytes(), s[:k].cpu().numpy().tobytes()
                t0 = time.perf_counter()
                orc.g1_scalar_mul(ph, sh)
                dt = time.perf_counter() - t0
                print("%-13s oracle g1_scalar_mul: %.0f us per point on one CPU thread (%d points): %.1f s for 2^%d" % (curve, dt / k * 1e6, k, dt / k * n, logn))
            c.close()


if __name__ == "__main__":
    main()
