"""Signed and 128-bit narrow scalar formats (MSM_HIP_SCALAR_SIGNED, MSM_HIP_SCALAR_U128) against the forms a caller had before them, on the same
context, in the same process, alternating.

    python tools/signed_scalar_timing.py [log2 sizes, default 20,22] [repeats, default 15]

For every size and base mode (the default -- the endomorphism on BN254 -- and plain bases) and every new format, uniform values of the format as
device scalars through msm_hip_run_device (single-MSM latency: median, min, interquartile range, max of the timed runs):
  (a) I8 .. I64 against the unsigned format of the same width on the magnitudes |v| (I128: against U128 on |v|) -- what the sign costs;
  (b) every new format against the same values as 32-byte canonical scalars v mod r -- for negative values that form is full width;
  (c) U128 against its 32-byte form -- 9 windows of n entries instead of 16 (or 2 n x 8 with the endomorphism).
Each form gets one untimed run first; then the forms alternate, and every run is timed.  The signed and the 32-byte results must agree."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402
from oracle import bn254_ref  # noqa: E402

FORMATS = [("i8", 1, True), ("i16", 2, True), ("i32", 4, True), ("i64", 8, True), ("u128", 16, False), ("i128", 16, True)]
STAGES = ["recode_count", "coarse_scan", "coarse_scatter", "fine_sort", "smvp", "smvp_stitch", "bucket_reduce", "device_total"]
R_LIMBS = [(bn254_ref.R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def limbs_of(raw, width):
    """n x width little-endian bytes -> (lo, hi) uint64 limbs of the two's-complement value sign-extended to 128 bits, and the sign"""
    n = raw.shape[0]
    ext = np.zeros((n, 16), dtype=np.uint8)
    ext[:, :width] = raw
    neg = (raw[:, width - 1] >> 7).astype(bool)
    ext[neg, width:] = 0xFF
    l = ext.view(np.uint64)
    return l[:, 0].copy(), l[:, 1].copy(), neg


def forms(raw, width, signed):
    """the magnitudes as n x width bytes, and v mod r as n x 32 bytes"""
    lo, hi, neg = limbs_of(raw, width)
    if not signed:
        if width < 16:
            hi[:] = 0
        neg = np.zeros_like(neg)
    one = np.uint64(1)
    mlo = np.where(neg, ~lo + one, lo)  # |v| = ~v + 1 over 128 bits
    mhi = np.where(neg, ~hi + (mlo == 0).astype(np.uint64), hi)
    mag = np.stack([mlo, mhi], axis=1).view(np.uint8)[:, :width].copy()
    # r - |v| for the negative values: a 256-bit subtraction with borrows (|v| <= 2^127 < r)
    r0, r1, r2, r3 = (np.uint64(x) for x in R_LIMBS)
    d0 = r0 - mlo
    b0 = (mlo > r0).astype(np.uint64)
    d1 = r1 - mhi - b0
    b1 = ((mhi > r1) | ((mhi == r1) & (b0 == 1))).astype(np.uint64)
    d2 = r2 - b1  # (r's upper limbs are far from zero: no further borrow)
    zero = np.zeros_like(mlo)
    s32 = np.stack([np.where(neg, d0, mlo), np.where(neg, d1, mhi), np.where(neg, d2, zero), np.where(neg, r3, zero)], axis=1)
    return mag, s32.view(np.uint8).copy()


def timed(ctx, width, signed, scalars):
    """one MSM in the given format: (latency in ms, stage times, result)"""
    ctx.set_scalar_format(width=width, signed=signed)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ctx.msm(scalars)
        return (time.perf_counter() - t0) * 1e3, ctx.stage_ms(), r
    finally:
        ctx.set_scalar_format(width=32)


def spread(xs):
    """median [min, quartiles, max] of a list of latencies"""
    q = statistics.quantiles(xs, n=4) if len(xs) > 1 else [xs[0]] * 3
    return "%7.3f ms [min %.3f, IQR %.3f - %.3f, max %.3f]" % (statistics.median(xs), min(xs), q[0], q[2], max(xs))


def fmt_stages(st):
    return " ".join("%s=%.3f" % (k, st.get(k, 0.0)) for k in STAGES)


def main():
    sizes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [20, 22]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    print("device:", torch.cuda.get_device_name(0), " repeats:", reps)
    for logn in sizes:
        n = 1 << logn
        for mode in ("default", "plain"):
            ctx = m.MsmContext(0)
            ctx.set_bases(ctx.sample_points(n, 1), endomorphism=None if mode == "default" else False)
            rng = np.random.default_rng(logn)
            print("\n== n = 2^%d, bases: %s (uses endomorphism: %s)" % (logn, mode, ctx.uses_endomorphism()))
            for name, width, signed in FORMATS:
                raw = rng.integers(0, 256, size=(n, width), dtype=np.uint8)
                mag, s32 = forms(raw, width, signed)
                runs = [(name, width, signed, torch.from_numpy(raw).cuda().reshape(-1))]
                if signed:  # (a): the unsigned format of the width on |v|
                    runs.append(("u%d on |v|" % (8 * width), width, False, torch.from_numpy(mag).cuda().reshape(-1)))
                runs.append(("32-byte v mod r", 32, False, torch.from_numpy(s32).cuda().reshape(-1)))
                for _, w, sg, t in runs:  # one untimed run of each form (pools; the adaptive k_fine_hist of 32-byte series)
                    timed(ctx, w, sg, t)
                got = [[] for _ in runs]
                for _ in range(reps):
                    for k, (_, w, sg, t) in enumerate(runs):
                        got[k].append(timed(ctx, w, sg, t))
                assert all(x[2] == got[-1][0][2] for x in got[0] + got[-1]), "%s and its 32-byte form differ" % name
                med = [statistics.median([x[0] for x in g]) for g in got]
                for k, (label, _, _, _) in enumerate(runs):
                    rel = "" if k == 0 else "   %s is %5.2fx of this form's median (this / %s = %5.2f)" % (name, med[0] / med[k], name, med[k] / med[0])
                    print("%-16s %s%s" % (label, spread([x[0] for x in got[k]]), rel))
                for k, (label, _, _, _) in enumerate(runs):
                    mid = sorted(got[k], key=lambda x: x[0])[len(got[k]) // 2]
                    print("      %-16s stages (median run): %s" % (label, fmt_stages(mid[1])))
                sys.stdout.flush()
            ctx.close()


if __name__ == "__main__":
    main()
