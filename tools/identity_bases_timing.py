"""Base sets with identity records (MSM_HIP_BASES_ZERO_IS_IDENTITY) against the unflagged engine, on the same device, in one process, alternating.

    python tools/identity_bases_timing.py [log2 base counts, default 20,22] [repeats, default 15] [--mask-only]  > profiles/identity_bases.txt

For every base count and base mode (endomorphism and plain bases), 32-byte device scalars, single MSMs (msm_hip_run_device):
  (a) unflagged  vs  flagged on the same identity-free set: the same kernels, so the same time within noise
  (b) one identity base (record n / 3)  vs  unflagged: the cost of the mask pass (k_mask_identity: one read and write of the scalars)
  (c) 50 % identities  vs  the unflagged dense MSM of the same vector with those scalars zeroed
Each form gets one untimed run first; the forms then alternate.  The results of every pair are asserted equal in every run.  Latency: median,
min, interquartile range, max; stage 0 (recode + coarse histogram, where the mask pass runs) of the median run.  --mask-only: only (b), three runs
each, for a `rocprofv3 --kernel-trace --stats` run that takes the mask kernel's own time."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402


def spread(xs):
    q = statistics.quantiles(xs, n=4) if len(xs) > 1 else [xs[0]] * 3
    return "%7.3f ms [min %.3f, IQR %.3f - %.3f, max %.3f]" % (statistics.median(xs), min(xs), q[0], q[2], max(xs))


def timed(ctx, s):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ctx.msm(s)
    return (time.perf_counter() - t0) * 1e3, ctx.stage_ms().get("recode_count", 0.0), r.to_affine_bytes(), ctx.env_report()["last_identity_mask"]


def compare(title, a_label, a_ctx, a_s, b_label, b_ctx, b_s, reps, want_mask):
    timed(a_ctx, a_s)
    timed(b_ctx, b_s)
    ra, rb = [], []
    for _ in range(reps):
        ra.append(timed(a_ctx, a_s))
        rb.append(timed(b_ctx, b_s))
    assert all(x[2] == ra[0][2] for x in ra + rb), "%s: results differ" % title
    assert all(x[3] == 0 for x in ra) and all(x[3] == want_mask for x in rb), "%s: mask pass where it should not be (or missing)" % title
    ma = statistics.median(x[0] for x in ra)
    mb = statistics.median(x[0] for x in rb)
    sa = sorted(ra)[len(ra) // 2][1]
    sb = sorted(rb)[len(rb) // 2][1]
    print("%s" % title)
    print("   %-30s %s  stage 0 %.3f ms" % (a_label, spread([x[0] for x in ra]), sa))
    print("   %-30s %s  stage 0 %.3f ms   difference of the medians %+.3f ms (%+.1f %%)" % (b_label, spread([x[0] for x in rb]), sb, mb - ma,
                                                                                         100.0 * (mb - ma) / ma))
    sys.stdout.flush()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mask_only = "--mask-only" in sys.argv
    sizes = [int(x) for x in args[0].split(",")] if args else [20, 22]
    reps = 3 if mask_only else int(args[1]) if len(args) > 1 else 15
    print("device:", torch.cuda.get_device_name(0), " repeats:", reps)
    for logn in sizes:
        n = 1 << logn
        for endo in (True, False):
            print("\n== n = 2^%d, %s bases, 32-byte device scalars" % (logn, "endomorphism" if endo else "plain"))
            plain = m.MsmContext(0)
            pts = plain.sample_points(n, 11)
            plain.set_bases(pts, endomorphism=endo)
            s = plain.sample_scalars(n, 12)
            flagged = m.MsmContext(0)
            if not mask_only:  # (a)
                flagged.set_bases(pts, endomorphism=endo, zero_is_identity=True)
                compare("(a) identity-free set", "unflagged", plain, s, "flagged", flagged, s, reps, 0)
            # (b)
            one = pts.clone()
            one[n // 3] = 0
            flagged.set_bases(one, endomorphism=endo, zero_is_identity=True)
            s_one = s.clone()
            s_one[n // 3] = 0
            compare("(b) one identity base", "unflagged, that scalar zeroed", plain, s_one, "flagged, one identity", flagged, s, reps, 1)
            if not mask_only:  # (c)
                half = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(13)) < 0.5
                zeroed = pts.clone()
                zeroed[half] = 0
                flagged.set_bases(zeroed, endomorphism=endo, zero_is_identity=True)
                s_half = s.clone()
                s_half[half] = 0
                compare("(c) 50 %% identities (%d)" % int(half.sum()), "unflagged, their scalars zeroed", plain, s_half, "flagged, 50 % identities",
                        flagged, s, reps, 1)
            plain.close()
            flagged.close()


if __name__ == "__main__":
    main()
