#!/usr/bin/env python3
"""Timing of the group FFT over the resident bases (msm_hip_bases_fft_device) on one GPU, against its yardstick: msm_hip_mul_each_device at the
same n in the same process.

Protocol, as tools/bench_mul.py: device-resident output, every shape warmed up, then `--calls` calls timed back to back (each call returns when
its output is complete), the transform and mul_each ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.

The ladder work of a transform is (n / 2) (log_n - 1) outputs of mul_each (stage 0 has no ladder), so the bound printed per shape is
    time(fft) <= 1.15 * (log_n - 1) / 2 * time(mul_each, n)
(two mixed additions per butterfly ~ 1 %, the normalisation between stages ~ 3 %, strided and bit-reversed loads); the scale pass of the Lagrange
form is n more ladders, (log_n - 1) / 2 + 1 in the same units.

Every timed shape is checked in the run through a random sparse combination of its outputs:
    sum_i rho_i out[i] == msm(P, [sum_i rho_i omega^(i j)])      four nonzero rho_i at random positions i
(left: a sparse MSM over the output as a base set; right: one MSM over the input bases with scalars from Python integers).
The bases are random multiples of the generator (msm_hip_mul_base_device), points of order r on every curve.
Kernel times proper come from a run under `rocprofv3 --kernel-trace --stats -- python tools/bench_fft.py ...`.

usage: tools/bench_fft.py [--shapes bn254:16,bn254:18,bn254:20,bn254:22,bls12_381:20] [--calls 20] [--rounds 3] [--no-check]"""
import argparse
import importlib
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402
from msm_webgpu_amd import api  # noqa: E402

PRIME_ORDER = ("bn254", "grumpkin", "pallas", "vesta")


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def b32(v):
    return int(v).to_bytes(32, "little")


def check(c, curve, log_n, omega, scale, out, bases_dev, rnd):
    """the random sparse combination; `c` holds the input bases, and holds them again afterwards"""
    r = api.SCALAR_FIELDS[curve]
    n = 1 << log_n
    idx = rnd.sample(range(n), 4) if n >= 4 else list(range(n))
    rho = [rnd.randrange(1, r) for _ in idx]
    acc = [0] * n
    for i, rh in zip(idx, rho):
        z, x = pow(omega, i, r), rh
        for j in range(n):
            acc[j] += x
            x = x * z % r
    k = pow(n, r - 2, r) if scale else 1
    want = c.msm(b"".join(b32(v * k % r) for v in acc))
    c.set_bases(out, zero_is_identity=True)
    got = c.msm_sparse(np.asarray(idx, dtype=np.uint32), b"".join(b32(v) for v in rho))
    c.set_bases(bases_dev, endomorphism=None if curve in PRIME_ORDER else False)
    return got == want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bn254:16,bn254:18,bn254:20,bn254:22,bls12_381:20")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    rnd = random.Random(20)
    for shape in a.shapes.split(","):
        curve, log_n = shape.split(":")
        log_n = int(log_n)
        n = 1 << log_n
        ref = importlib.import_module("oracle.%s_ref" % curve)
        omega = api.root_of_unity(curve, log_n, inverse=True)
        c = m.MsmContext(0, curve=curve)
        c.set_bases(ref.points_to_bytes([ref.G]))
        s = c.sample_scalars(n, 31)
        bases_dev = c.mul_base(0, s, bases_order_r=True)  # n random multiples of the generator
        c.set_bases(bases_dev, endomorphism=None if curve in PRIME_ORDER else False)
        out = torch.empty((n, c.pb), dtype=torch.uint8, device="cuda")
        out_mul = torch.empty((n, c.pb), dtype=torch.uint8, device="cuda")
        # variants: (name, call, the flag for the yardstick's ladder)
        variants = [("lagrange (omega^-1, 1/n)", lambda: c.bases_fft(omega, log_n, scale=True, out=out), False),
                    ("forward (no scale)", lambda: c.bases_fft(omega, log_n, out=out), False)]
        if curve not in PRIME_ORDER:
            variants.append(("lagrange, bases_order_r", lambda: c.bases_fft(omega, log_n, scale=True, bases_order_r=True, out=out), True))
        yard = {False: lambda: c.mul_each(s, out=out_mul), True: lambda: c.mul_each(s, bases_order_r=True, out=out_mul)}
        flags = sorted({f for _, _, f in variants})
        t_first = timed(variants[0][1], 1)  # builds the twiddle table on the host and uploads it
        for _, fn, _ in variants:
            fn()
        for f in flags:
            yard[f]()
        t_fft = {name: [] for name, _, _ in variants}
        t_mul = {f: [] for f in flags}
        for _ in range(a.rounds):
            for name, fn, _ in variants:
                t_fft[name].append(timed(fn, a.calls))
            for f in flags:
                t_mul[f].append(timed(yard[f], a.calls))
        for f in flags:
            t = t_mul[f]
            print("%-10s 2^%d %-28s %10.3f ms/call (%.3f .. %.3f over %d rounds of %d)" % (curve, log_n, "mul_each" + (" order_r" if f else ""), statistics.mean(t) * 1e3,
                  min(t) * 1e3, max(t) * 1e3, a.rounds, a.calls))
        for name, fn, f in variants:
            t = t_fft[name]
            mean, mul = statistics.mean(t), statistics.mean(t_mul[f])
            ladders = (log_n - 1) / 2 + (1 if "lagrange" in name else 0)  # in units of n ladders: the twiddled stages, + the scale pass
            bound = 1.15 * ladders * mul  # (the acceptance bound proper is the forward transform's: no scale pass)
            fn()  # (the variant's own output: the variants share `out`)
            ok = "unchecked" if a.no_check else ("combination ok" if check(c, curve, log_n, omega, "lagrange" in name, out, bases_dev, rnd) else "COMBINATION WRONG")
            print("%-10s 2^%d %-28s %10.3f ms/call (%.3f .. %.3f)  = %.2f x mul_each = %.3f x its %.1f n ladders; bound 1.15 x %.1f x mul_each = %.3f ms: %s  [%s, stages/ladder %s]"
                  % (curve, log_n, name, mean * 1e3, min(t) * 1e3, max(t) * 1e3, mean / mul, mean / (ladders * mul), ladders, ladders, bound * 1e3,
                     "MET" if mean <= bound else "NOT MET", ok, c.fft_last()), flush=True)
        print("%-10s 2^%d %-28s %10.3f ms: the first call, which builds the twiddle table (%d entries) on the host" % (curve, log_n, "first call", t_first * 1e3, n // 2), flush=True)
        c.close()


if __name__ == "__main__":
    main()
