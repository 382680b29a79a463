"""Narrow scalar formats (MSM_HIP_SCALARS_U8 .. U64) against the same values in 32-byte form, on the same context, in the same process, alternating.

    python tools/narrow_scalar_timing.py [log2 sizes, default 20,22] [repeats, default 15]

For every size and base mode (the default -- the endomorphism on BN254 -- and plain bases) and every input kind (bool at density 1/2, u8, u16,
u32, u64 uniform): device scalars through msm_hip_run_device (single-MSM latency: median, min, interquartile range, max of the timed runs, and the
stage times of the median run), then host scalars through msm_hip_run (the narrow form uploads n x width bytes, the 32-byte form n x 32).  Each form
gets one untimed run first; every other run is timed."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402

DT = {1: torch.uint8, 2: torch.uint16, 4: torch.uint32, 8: torch.uint64}
STAGES = ["recode_count", "coarse_scan", "coarse_scatter", "fine_sort", "smvp", "smvp_stitch", "bucket_reduce", "device_total"]


def inputs(kind, n, g):
    if kind == "bool":
        return 1, (torch.rand(n, device="cuda", generator=g) < 0.5).to(torch.uint8)
    width = int(kind[1:]) // 8
    return width, torch.randint(0, 256, (n, width), dtype=torch.uint8, device="cuda", generator=g).view(DT[width]).reshape(-1)


def widen(t, width):
    out = torch.zeros((t.numel(), 32), dtype=torch.uint8, device="cuda")
    out[:, :width] = t.view(torch.uint8).reshape(-1, width)
    return out


def timed(ctx, width, scalars):
    """one MSM in the given width: (latency in ms, stage times, result)"""
    ctx.set_scalar_format(width=width)
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
            g = torch.Generator(device="cuda").manual_seed(logn)
            print("\n== n = 2^%d, bases: %s (uses endomorphism: %s)" % (logn, mode, ctx.uses_endomorphism()))
            for kind in ("bool", "u8", "u16", "u32", "u64"):
                width, t = inputs(kind, n, g)
                w32 = widen(t, width)
                # device scalars: one untimed run of each form first (pools; the adaptive k_fine_hist that a skewed 32-byte series arms),
                # then the two forms alternate so that clocks and neighbours affect both alike; every run below is timed and reported
                timed(ctx, width, t)
                timed(ctx, 32, w32)
                nar, wide = [], []
                for _ in range(reps):
                    nar.append(timed(ctx, width, t))
                    wide.append(timed(ctx, 32, w32))
                assert all(x[2] == wide[0][2] for x in nar + wide), "narrow and 32-byte results differ (%s)" % kind
                mn = sorted(nar, key=lambda x: x[0])[len(nar) // 2]
                mw = sorted(wide, key=lambda x: x[0])[len(wide) // 2]
                print("%-5s device  narrow  %s" % (kind, spread([x[0] for x in nar])))
                print("              32-byte %s   speed-up of the medians %5.2fx" % (spread([x[0] for x in wide]), mw[0] / mn[0]))
                print("      narrow  stages (median run): %s" % fmt_stages(mn[1]))
                print("      32-byte stages (median run): %s" % fmt_stages(mw[1]))
                # host scalars through msm_hip_run
                hb, hw = t.view(torch.uint8).cpu().numpy().tobytes(), w32.cpu().numpy().tobytes()
                timed(ctx, width, hb)
                timed(ctx, 32, hw)
                hn, hwd = [], []
                for _ in range(max(3, reps // 3)):
                    hn.append(timed(ctx, width, hb)[0])
                    hwd.append(timed(ctx, 32, hw)[0])
                print("      host    narrow  %s" % spread(hn))
                print("              32-byte %s   speed-up of the medians %5.2fx" % (spread(hwd), statistics.median(hwd) / statistics.median(hn)))
                sys.stdout.flush()
            ctx.close()


if __name__ == "__main__":
    main()
