#!/usr/bin/env python3
"""Timing of the scalar-field NTT (MsmContext.scalars_fft: msm_fr_ntt_device, libmsm_fr.so) on one GPU against two yardsticks timed in the same
process, neither of them the code under test:
  (a) a device-to-device copy of the same bytes -- one read plus one write of the data, so a transform's passes can be counted in copies;
  (b) ctx.msm of 2^20 scalars of the same field on a context with default bases -- a prover's NTT -> MSM step is lengthened by exactly the ratio.
The bound: time(NTT, 2^20) <= 0.25 * time(MSM, 2^20), per field.

Protocol: device data, every shape warmed up (the warm-up call builds and uploads the twiddle tables), then `--calls` calls timed back to back
(each call returns when its stream has completed), the transform, the copy and the MSM ALTERNATED `--rounds` times; min .. max over the rounds
beside every mean.  The transform runs in place on its own output again and again (an output is a valid input).

Every timed shape is checked in the run against four outputs computed from the definition, out[i] = sum_j omega^(i j) a[j], over Python integers:
on the timed vector itself up to 2^20 elements; beyond, on a vector of the same shape with 4096 nonzero entries (the definition's sum over 2^24
terms is minutes of Python).  Kernel times proper come from a run under `rocprofv3 --kernel-trace --stats -- python tools/bench_ntt.py ...`.

usage: tools/bench_ntt.py [--shapes bn254:16:1,bn254:20:1,...] [--calls 20] [--rounds 3] [--no-check] [--no-msm]"""
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


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def scalars_at(t, idx):
    return [int.from_bytes(t[i].cpu().numpy().tobytes(), "little") for i in idx]


def check(c, curve, log_n, batch, data, rnd):
    """four outputs of one transform of this shape against the definition -> (ok, what was checked)"""
    r = api.SCALAR_FIELDS[curve]
    n = 1 << log_n
    omega = api.root_of_unity(curve, log_n)
    v = rnd.randrange(batch)
    if n <= 1 << 20:
        work = data.clone()
        a = [int.from_bytes(b, "little") for b in (lambda raw: (raw[k:k + 32] for k in range(0, len(raw), 32)))(work[v * n:(v + 1) * n].cpu().numpy().tobytes())]
        support = range(n)
        what = "dense"
    else:
        work = torch.zeros_like(data)
        support = sorted(rnd.sample(range(n), 4096))
        vals = [rnd.randrange(r) for _ in support]
        rows = torch.frombuffer(bytearray(b"".join(x.to_bytes(32, "little") for x in vals)), dtype=torch.uint8).reshape(-1, 32).cuda()
        work[torch.tensor([v * n + j for j in support], device="cuda")] = rows
        a = dict(zip(support, vals))
        what = "4096 nonzero inputs"
    c.scalars_fft(work, log_n, batch=batch)
    idx = rnd.sample(range(n), 4) if n >= 4 else list(range(n))
    got = scalars_at(work, [v * n + i for i in idx])
    for i, g in zip(idx, got):
        z = pow(omega, i, r)
        if what == "dense":
            acc, x = 0, 1
            for j in support:
                acc += a[j] * x
                x = x * z % r
        else:
            acc = sum(a[j] * pow(z, j, r) for j in support)
        if acc % r != g:
            return False, what
    return True, what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bn254:16:1,bn254:20:1,bn254:22:1,bn254:24:1,bn254:16:64,pallas:20:1,vesta:20:1,bls12_381:20:1")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-msm", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    rnd = random.Random(26)
    ctxs = {}
    verdicts = []
    for shape in a.shapes.split(","):
        curve, log_n, batch = shape.split(":")
        log_n, batch = int(log_n), int(batch)
        n = 1 << log_n
        if curve not in ctxs:  # the field's context: 2^20 default bases and 2^20 scalars for the MSM yardstick
            c = m.MsmContext(0, curve=curve)
            msm_s = None
            if not a.no_msm:
                c.set_bases(c.sample_points(1 << MSM_LOG_N, 41), endomorphism=None)
                msm_s = c.sample_scalars(1 << MSM_LOG_N, 42)
            ctxs[curve] = (c, msm_s)
        c, msm_s = ctxs[curve]
        data = c.sample_scalars(batch * n, 43)
        other = torch.empty_like(data)
        runs = {"ntt": lambda: c.scalars_fft(data, log_n, batch=batch), "copy": lambda: other.copy_(data)}
        if msm_s is not None:
            runs["msm"] = lambda: c.msm(msm_s)
        t_first = timed(runs["ntt"], 1)  # builds the tables of this (field, log_n, omega) on the host and uploads them
        ok = ("unchecked", "") if a.no_check else check(c, curve, log_n, batch, data, rnd)
        for fn in runs.values():
            fn()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(timed(fn, a.calls))
        mean = {k: statistics.mean(v) for k, v in t.items()}
        label = "%-10s %3d x 2^%-2d" % (curve, batch, log_n)
        for k in ("copy", "msm"):
            if k in t:
                print("%s %-22s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)" % (label, "d2d copy, same bytes" if k == "copy" else "msm 2^20, default bases", mean[k] * 1e3,
                      min(t[k]) * 1e3, max(t[k]) * 1e3, a.rounds, a.calls))
        line = "%s %-22s %9.3f ms/call (%.3f .. %.3f)  = %.2f x copy" % (label, "ntt forward, in place", mean["ntt"] * 1e3, min(t["ntt"]) * 1e3, max(t["ntt"]) * 1e3,
                                                                        mean["ntt"] / mean["copy"])
        if "msm" in t:
            line += "  = %.3f x msm(2^20)" % (mean["ntt"] / mean["msm"])
            if log_n == MSM_LOG_N and batch == 1:
                met = mean["ntt"] <= 0.25 * mean["msm"]
                verdicts.append((curve, met))
                line += "; bound 0.25 x msm = %.3f ms: %s" % (0.25 * mean["msm"] * 1e3, "MET" if met else "NOT MET")
        line += "  [%s%s; passes, widest %s; first call %.3f ms]" % ("unchecked" if a.no_check else ("4 outputs ok" if ok[0] else "OUTPUTS WRONG"), ", " + ok[1] if ok[1] else "",
                                                                   api.fr_last(), t_first * 1e3)
        print(line, flush=True)
        del data, other
    for curve, met in verdicts:
        print("verdict %-10s time(NTT, 2^20) <= 0.25 * time(MSM, 2^20): %s" % (curve, "MET" if met else "NOT MET"))
    for c, _ in ctxs.values():
        c.close()
    api.fr_release()


if __name__ == "__main__":
    main()
