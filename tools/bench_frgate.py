#!/usr/bin/env python3
"""Timing of constraint evaluation (MsmContext.scalars_gate: libmsm_frgate.so) on one GPU against the same expression put together from the
unchanged libraries, in the same process.  A verdict line says MET (the new call's mean is no longer than the yardstick's) or NOT MET.

The expression is a PLONK identity over the extended coset domain, log_ext = 2, nine terms:
  the gate         qM a b + qL a + qR b + qO c + qC                                  (five terms, rows 0 .. 7)
  the permutation  alpha (z(omega X) u1 u2 u3 - z v1 v2 v3)                         (two terms of degree 4, rows 8 .. 14; one rotation)
  the first row    alpha^2 (L1 z - L1)                                               (two terms, rows 8 and 15)
times 1 / Z_H, a scale of period 4.  Those nine terms name 16 distinct rows: 8 for the gate, z, six permutation factors and L1.

The YARDSTICK: per term, a scalars_mul for every factor after the first into a scratch vector, then a scalars_mul_add with the coefficient broadcast
onto the sum (the first term a scalars_mul); at the end a scalars_mul by the scale tiled to N elements.  The rolled copy of z and the tiled scale
are prepared OUTSIDE the timed region, which favours the yardstick.

Also: the whole MsmContext.quotient (16 columns of n = N / 4 coefficients -> the N coefficients of t) next to the ctx.msm of length N.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the
product and its yardstick ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  Sampled outputs are checked in the run
against Python integers.

usage: tools/bench_frgate.py [--log-big 20,22] [--calls 20] [--rounds 3] [--no-check] [--no-prover]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402
from msm_webgpu_amd import api  # noqa: E402

CURVE = "bn254"
LOG_EXT = 2
SHIFT = 7
ROWS = 16
A, B, C_, QM, QL, QR, QO, QC, Z, U1, U2, U3, V1, V2, V3, L1 = range(ROWS)


def identity(r, alpha):
    a2 = alpha * alpha % r
    return [(1, (QM, A, B)), (1, (QL, A)), (1, (QR, B)), (1, (QO, C_)), (1, (QC,)),
            (alpha, ((Z, 1), U1, U2, U3)), ((r - alpha) % r, (Z, V1, V2, V3)),
            (a2, (L1, Z)), ((r - a2) % r, (L1,))]


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def ints(t, idx):
    """the scalars of t at idx as Python integers (one gather on the device, one copy)"""
    raw = t[torch.as_tensor(np.asarray(idx, dtype=np.int64), device=t.device)].cpu().numpy().tobytes()
    return [int.from_bytes(raw[k:k + 32], "little") for k in range(0, len(raw), 32)]


def check(rows, terms, step, scale, out, r, sample):
    """out on the sampled elements against Python integers"""
    big = rows.shape[1]
    sc = ints(scale, list(range(scale.shape[0])))
    for i in sample:
        e = 0
        for coeff, factors in terms:
            p = coeff
            for f in factors:
                row, rot = (f, 0) if isinstance(f, int) else f
                p = p * ints(rows[row], [(i + rot * step) % big])[0] % r
            e += p
        if ints(out, [i]) != [e * sc[i % len(sc)] % r]:
            return False
    return True


def report(label, name, new, ref, rounds, calls, useful, judged=True, ref_name="mul / mul_add chain"):
    mn, mr = statistics.mean(new), statistics.mean(ref)
    tail = "   useful %.0f GB/s" % (useful / mn / 1e9) if useful else ""
    print("%s %-22s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)  against %-20s %9.3f ms/call (%.3f .. %.3f)  = %.2f x  %s%s" % (
        label, name, mn * 1e3, min(new) * 1e3, max(new) * 1e3, rounds, calls, ref_name, mr * 1e3, min(ref) * 1e3, max(ref) * 1e3, mn / mr,
        ("MET" if mn <= mr else "NOT MET") if judged else "(reported)", tail), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-big", default="20,22")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-prover", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    r = api.SCALAR_FIELDS[CURVE]
    c = m.MsmContext(0, curve=CURVE)
    gen = np.random.default_rng(37)
    terms = identity(r, 0x1234567890ABCDEF1234567890ABCDEF)
    named = len({(f if isinstance(f, int) else f[0]) for _, fs in terms for f in fs})
    step = 1 << LOG_EXT
    for k in [int(s) for s in a.log_big.split(",")]:
        big = 1 << k
        label = "%-6s N = 2^%-2d" % (CURVE, k)
        rows = c.sample_scalars(ROWS * big, 61).view(ROWS, big, 32)
        scale = c.vanishing_inverse(k - LOG_EXT, LOG_EXT, SHIFT)
        out = torch.empty((big, 32), dtype=torch.uint8, device="cuda")
        # the yardstick's inputs, prepared outside the timed region: the rolled copy of z, the scale tiled to N elements
        rolled = {(Z, 1): torch.roll(rows[Z], -step, 0).contiguous()}
        tiled = scale.repeat(big // scale.shape[0], 1).contiguous()
        tmp, acc = torch.empty_like(out), torch.empty_like(out)

        def factor(f):
            return rows[f] if isinstance(f, int) else rolled[f]

        def yardstick():
            for j, (coeff, factors) in enumerate(terms):
                cur = factor(factors[0])
                for f in factors[1:]:
                    c.scalars_mul(cur, factor(f), out=tmp)
                    cur = tmp
                if j == 0:
                    c.scalars_mul(cur, coeff, out=acc)
                else:
                    c.scalars_mul_add(cur, coeff, acc, out=acc)
            c.scalars_mul(acc, tiled, out=acc)

        def gate():
            c.scalars_gate(rows, terms, batch=ROWS, step=step, scale=scale, out=out)

        gate(), yardstick()
        passes = sum(len(fs) - 1 for _, fs in terms) + len(terms) + 1
        verdict = "unchecked"
        if not a.no_check:
            sample = sorted({0, 1, step - 1, big - step, big - 1} | {int(v) for v in gen.integers(0, big, size=6)})
            ok = check(rows, terms, step, scale, out, r, sample)
            verdict = "ok" if ok and torch.equal(out, acc) else "WRONG"
        print("%s %d terms over %d distinct rows; the yardstick makes %d passes; checked on sampled elements against Python integers, and the two routes "
              "against each other on all: %s" % (label, len(terms), named, passes, verdict), flush=True)
        tn, tr = [], []
        for _ in range(a.rounds):
            tn.append(timed(gate, a.calls))
            tr.append(timed(yardstick, a.calls))
        report(label, "scalars_gate", tn, tr, a.rounds, a.calls, (named + 1) * 32 * big)
        del rolled, tiled, tmp, acc, out
        if not a.no_prover:  # the whole quotient next to the commitment of the same length
            n = big >> LOG_EXT
            cols = rows[:, :n].contiguous()
            c.set_bases(c.sample_points(big, 41), endomorphism=None)
            x = c.sample_scalars(big, 62)
            c.quotient(cols, terms, ROWS, k - LOG_EXT, LOG_EXT, SHIFT), c.msm(x)
            tq, tm = [], []
            for _ in range(a.rounds):
                tq.append(timed(lambda: c.quotient(cols, terms, ROWS, k - LOG_EXT, LOG_EXT, SHIFT), a.calls))
                tm.append(timed(lambda: c.msm(x), a.calls))
            report(label, "quotient (16 columns)", tq, tm, a.rounds, a.calls, 0, judged=False, ref_name="msm of 2^%d" % k)
            del cols, x
        del rows
        torch.cuda.empty_cache()
    c.close()
    api.frgate_release()
    api.frvec_release()
    api.fr_release()


if __name__ == "__main__":
    main()
