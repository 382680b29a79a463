"""Sparse MSMs (msm_hip_run_sparse_device) against the densified form of the same terms, on the same context, in the same process, alternating.

    python tools/sparse_msm_timing.py [log2 base counts, default 20,22] [repeats, default 15]

For every base count and base mode (the default -- the endomorphism on BN254 -- and plain bases) and every case -- nnz = 2^10, 2^14, 2^18 distinct
random indices with uniform 32-byte scalars, a full permutation of all bases, and a one-hot vector (one U8 one per row of 16 bases) --:
  sparse     msm_sparse(indices, scalars) from device tensors
  densified  a device scatter of the scalars into a zeroed n x 32 B vector, then the dense msm of all n bases (the scatter is timed with it)
  dense nnz  for reference: a dense msm of nnz points (the first nnz bases), what the sparse call is expected to cost
Latency of single MSMs: median, min, interquartile range, max of the timed runs, and the stage times of the sparse form's median run.  Each form
gets one untimed run first; the forms then alternate.  Sparse and densified results are asserted equal in every run."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402

STAGES = ["recode_count", "coarse_scan", "coarse_scatter", "fine_sort", "smvp", "smvp_stitch", "bucket_reduce", "device_total"]


def spread(xs):
    """median [min, quartiles, max] of a list of latencies"""
    q = statistics.quantiles(xs, n=4) if len(xs) > 1 else [xs[0]] * 3
    return "%7.3f ms [min %.3f, IQR %.3f - %.3f, max %.3f]" % (statistics.median(xs), min(xs), q[0], q[2], max(xs))


def fmt_stages(st):
    return " ".join("%s=%.3f" % (k, st.get(k, 0.0)) for k in STAGES)


def timed(ctx, fn, width=32):
    ctx.set_scalar_format(width=width)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, ctx.stage_ms(), r
    finally:
        ctx.set_scalar_format(width=32)


def case_inputs(case, n, g):
    """(label, indices, scalars, scalar width)"""
    if case == "one-hot":
        rows = n // 16
        col = torch.randint(0, 16, (rows,), device="cuda", generator=g)
        idx = torch.arange(rows, device="cuda") * 16 + col
        return "one-hot u8 (%d rows x 16)" % rows, idx.to(torch.int32), torch.ones(rows, dtype=torch.uint8, device="cuda"), 1
    nnz = n if case == "perm" else 1 << case
    idx = torch.randperm(n, device="cuda", generator=g)[:nnz].to(torch.int32)
    s = torch.randint(0, 256, (nnz, 32), dtype=torch.uint8, device="cuda", generator=g)
    s[:, 31] &= 0x0F  # below r
    return ("full permutation" if case == "perm" else "nnz 2^%d" % case), idx, s, 32


def densify(idx, s, width, n):
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    out[idx.long(), :width] = s.view(torch.uint8).reshape(-1, width)
    return out


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
            print("\n== n_bases = 2^%d, bases: %s (uses endomorphism: %s)" % (logn, mode, ctx.uses_endomorphism()))
            for case in (10, 14, 18, "perm", "one-hot"):
                label, idx, s, width = case_inputs(case, n, g)
                nnz = idx.numel()
                sparse = lambda: ctx.msm_sparse(idx, s)  # noqa: E731
                dense_of = lambda: ctx.msm(densify(idx, s, width, n))  # noqa: E731
                first = s if width == 32 else densify(torch.arange(nnz, device="cuda"), s, width, nnz)
                dense_nnz = lambda: ctx.msm(first)  # noqa: E731
                timed(ctx, sparse, width)
                timed(ctx, dense_of)
                timed(ctx, dense_nnz)
                sp, de, dn = [], [], []
                for _ in range(reps):
                    sp.append(timed(ctx, sparse, width))
                    de.append(timed(ctx, dense_of))
                    dn.append(timed(ctx, dense_nnz))
                assert all(x[2] == de[0][2] for x in sp + de), "sparse and densified results differ (%s)" % label
                ms = sorted(sp, key=lambda x: x[0])[len(sp) // 2]
                md = sorted(de, key=lambda x: x[0])[len(de) // 2]
                print("%-26s sparse     %s" % (label, spread([x[0] for x in sp])))
                print("%-26s densified  %s   speed-up of the medians %5.2fx" % ("", spread([x[0] for x in de]), md[0] / ms[0]))
                print("%-26s dense nnz  %s" % ("", spread([x[0] for x in dn])))
                print("      sparse    stages (median run): %s" % fmt_stages(ms[1]))
                print("      densified stages (median run): %s" % fmt_stages(md[1]))
                sys.stdout.flush()
            ctx.close()


if __name__ == "__main__":
    main()
