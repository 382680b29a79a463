#!/usr/bin/env python3
"""Timing of the sumcheck operations (MsmContext.scalars_mle_fold .. sumcheck_prove: libmsm_frmle.so) on one GPU, each against what gives the same
result on the other four libraries, timed in the same process:
  fold                    scalars_sub on the halves, then scalars_mul_add (2 calls)
  eval                    scalars_dot with a prebuilt eq table
  eq                      k doubling steps of maps: scalars_mul into the upper half, scalars_sub in the lower (2 k calls)
  round, degree 2         g(0), g(1), g(2) of A B: two scalars_mul_sub for the values at t = 2, three scalars_dot (5 calls)
  round with fold_by      scalars_mle_fold, then scalars_sumcheck_round (both new: what the fusion saves)
  sumcheck_prove at 2^20  20 rounds of eq A B - eq C over four rows (restored from a copy before every run), next to the ctx.msm of 2^20
  the floor               scalars_sumcheck_round and scalars_mle_eval at n = 2, next to scalars_dot at n = 2
The expectation in every pair is "the new call takes no longer"; a verdict line says MET or NOT MET (the prover and the floor are reported, not judged).

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the new
calls and their yardsticks ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  Each shape is checked in the run: the new
and the old results against each other, the eq table on sampled elements against Python integers.

--order low (or both) adds, for every shape, the calls of msm-webgpu_amd/multilinear.py under MSM_FRMLE_LOW_FIRST next to the same calls top first,
alternated in the same way: the fold apart and in place, the round of degree 2 over two rows and of degree 3 over four, the fused round, and
at 2^20 the whole proof.  The ratio low / top is reported, not judged; the bytes say parity for the fold apart and the plain round, and the copy
of a quarter of every row for the two in-place binds.  A last line sets the in-place fold's schedule (a quarter of
every row through scratch) against the other one put together from calls: all outputs apart, then half of every row copied home.
--order low leaves the yardstick pairs above out.

usage: tools/bench_frmle.py [--shapes bn254:16,bn254:20,bn254:24] [--calls 20] [--rounds 3] [--no-check] [--no-prover] [--order top|low|both]"""
import argparse
import hashlib
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
from msm_webgpu_amd import multilinear as ml  # noqa: E402

PROVER_LOG_N = 20


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def at(t, idx):
    return [int.from_bytes(t[i].cpu().numpy().tobytes(), "little") for i in idx]


def report(label, name, new, ref_name, ref, rounds, calls, judged=True):
    mn, mr = statistics.mean(new), statistics.mean(ref)
    print("%s %-26s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)  against %-34s %9.3f ms/call (%.3f .. %.3f)  = %.2f x  %s" % (
        label, name, mn * 1e3, min(new) * 1e3, max(new) * 1e3, rounds, calls, ref_name, mr * 1e3, min(ref) * 1e3, max(ref) * 1e3, mn / mr,
        ("MET" if mn <= mr else "NOT MET") if judged else "(reported)"), flush=True)


def orders_section(c, label, k, r, a, rnd):
    """the low-first calls against the same calls top first, on four rows of 2^k scalars"""
    n = 1 << k
    rows = c.sample_scalars(4 * n, 61)
    work, out = torch.empty_like(rows), torch.empty_like(rows)
    work.copy_(rows)
    ch = rnd.randrange(2, r)
    t2, t3 = [(1, (0, 1))], [(1, (0, 1, 2)), (r - 1, (0, 3))]

    def challenge(j, values):
        return int.from_bytes(hashlib.sha256(values).digest(), "little") % r

    def prove(order):
        work.copy_(rows)
        return ml.sumcheck_prove(c, work, t3, 4, challenge, order=order)

    def both(fn):
        return (lambda: fn("low")), (lambda: fn("top"))

    cases = [("fold apart, 4 rows", a.calls) + both(lambda o: ml.fold(c, rows, ch, batch=4, out=out, order=o)),
             ("fold in place, 4 rows", a.calls) + both(lambda o: ml.fold(c, work, ch, batch=4, order=o)),
             ("round, degree 2, 2 rows", a.calls) + both(lambda o: ml.sumcheck_round(c, rows[:2 * n], t2, batch=2, order=o)),
             ("round, degree 3, 4 rows", a.calls) + both(lambda o: ml.sumcheck_round(c, rows, t3, batch=4, order=o)),
             ("fused round, degree 3", a.calls) + both(lambda o: ml.sumcheck_round(c, work, t3, batch=4, fold=ch, order=o))]
    if k == PROVER_LOG_N and not a.no_prover:
        cases.append(("sumcheck_prove, %d rounds" % k, max(a.calls // 4, 1)) + both(prove))

    # the schedule the library did not take, put together from calls: ALL n / 2 outputs of every row to another buffer in one launch, then n / 2
    # scalars of every row copied home -- against the one it took (n / 4 to scratch, n / 4 in place, n / 4 copied)
    def all_through_scratch():
        ml.fold(c, work, ch, batch=4, out=out)
        work.reshape(4, n, 32)[:, :n // 2].copy_(out.reshape(4, n, 32)[:, :n // 2])
        torch.cuda.synchronize()

    cases.append(("in place vs all via scratch", a.calls, lambda: ml.fold(c, work, ch, batch=4), all_through_scratch))
    for _, _, low, top in cases:
        low(), top()
    t = {}
    for _ in range(a.rounds):
        for name, calls, low, top in cases:
            t.setdefault(name, []).append(timed(low, calls))
            t.setdefault(name + " / top", []).append(timed(top, calls))
    for name, calls, _, _ in cases:
        other = "fold apart + copy of n / 2 (low first)" if " vs " in name else "the same call top first"
        report(label, "low: " + name, t[name], other, t[name + " / top"], a.rounds, calls, judged=False)
    del rows, work, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bn254:16,bn254:20,bn254:24")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-prover", action="store_true")
    ap.add_argument("--order", choices=("top", "low", "both"), default="top")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    rnd = random.Random(29)
    ctxs = {}
    for shape in a.shapes.split(","):
        curve, k = shape.split(":")
        k = int(k)
        n, h = 1 << k, 1 << (k - 1)
        r = api.SCALAR_FIELDS[curve]
        if curve not in ctxs:
            ctxs[curve] = m.MsmContext(0, curve=curve)
        c = ctxs[curve]
        if a.order != "top":
            orders_section(c, "%-10s 2^%-2d" % (curve, k), k, r, a, rnd)
            if a.order == "low":
                continue
        point = [rnd.randrange(2, r) for _ in range(k)]
        ch = rnd.randrange(2, r)
        ab = c.sample_scalars(2 * n, 51)  # rows A and B of every round below
        va, vb = ab[:n], ab[n:]
        work, tmp, tmp2 = torch.empty_like(ab), torch.empty_like(va), torch.empty_like(va)
        eq_new, eq_old = torch.empty_like(va), torch.empty_like(va)
        one = torch.frombuffer(bytearray((1).to_bytes(32, "little")), dtype=torch.uint8).cuda()
        terms = [(1, (0, 1))]

        def fold_old():
            c.scalars_sub(work[h:n], work[:h], out=tmp[:h])
            c.scalars_mul_add(tmp[:h], ch, work[:h], out=work[:h])

        def eq_old_fn():
            eq_old[:1].copy_(one.reshape(1, 32))
            size = 1
            for z in reversed(point):  # (the variable bound last is the lowest bit: every step puts its variable on top)
                c.scalars_mul(eq_old[:size], z, out=eq_old[size:2 * size])
                c.scalars_sub(eq_old[:size], eq_old[size:2 * size], out=eq_old[:size])
                size *= 2

        def round_old():
            c.scalars_mul_sub(va[h:], 2, va[:h], out=tmp[:h])
            c.scalars_mul_sub(vb[h:], 2, vb[:h], out=tmp2[:h])
            return c.scalars_dot(va[:h], vb[:h]) + c.scalars_dot(va[h:], vb[h:]) + c.scalars_dot(tmp[:h], tmp2[:h])

        def fused():
            return c.scalars_sumcheck_round(work, terms, batch=2, fold=ch)

        def separate():
            c.scalars_mle_fold(work, ch, batch=2)
            return c.scalars_sumcheck_round(work, terms, batch=2, n=h)

        work.copy_(ab)
        c.scalars_eq(point, out=eq_new)
        pairs = [("fold, in place", lambda: c.scalars_mle_fold(work[:n], ch), "sub + mul_add on the halves", fold_old),
                 ("eval", lambda: c.scalars_mle_eval(va, point), "dot with a prebuilt eq table", lambda: c.scalars_dot(va, eq_new)),
                 ("eq", lambda: c.scalars_eq(point, out=eq_new), "%d map calls" % (2 * k), eq_old_fn),
                 ("round, degree 2", lambda: c.scalars_sumcheck_round(ab, terms, batch=2), "2 mul_sub + 3 dot", round_old),
                 ("round with fold_by", fused, "fold, then round (both new)", separate)]
        bad = []
        if not a.no_check:
            eq_old_fn()
            idx = sorted({0, 1, n // 2, n - 1} | {rnd.randrange(n) for _ in range(4)})
            want = []
            for i in idx:
                v = 1
                for j, z in enumerate(point):
                    v = v * (z if (i >> (k - 1 - j)) & 1 else 1 - z) % r
                want.append(v)
            if at(eq_new, idx) != want or at(eq_old, idx) != want:
                bad.append("eq")
            if c.scalars_mle_eval(va, point) != c.scalars_dot(va, eq_new):
                bad.append("eval")
            if c.scalars_sumcheck_round(ab, terms, batch=2) != round_old():
                bad.append("round")
            work.copy_(ab)
            fold_old()
            first = at(work, [0, 1, h - 1])
            work.copy_(ab)
            v_fused = fused()
            if at(work, [0, 1, h - 1]) != first:
                bad.append("fold")
            work.copy_(ab)
            if separate() != v_fused:
                bad.append("round with fold_by")
            work.copy_(ab)
        for _, fn, _, ref in pairs:
            fn(), ref()
        t = {}
        for _ in range(a.rounds):
            for name, fn, ref_name, ref in pairs:
                t.setdefault(name, []).append(timed(fn, a.calls))
                t.setdefault(name + " / ref", []).append(timed(ref, a.calls))
        label = "%-10s 2^%-2d" % (curve, k)
        for name, _, ref_name, _ in pairs:
            report(label, name, t[name], ref_name, t[name + " / ref"], a.rounds, a.calls)
        print("%s checked (new against old, eq on sampled elements against Python integers): %s" % (
            label, "unchecked" if a.no_check else ("ok" if not bad else "WRONG: " + ", ".join(bad))), flush=True)
        if k == PROVER_LOG_N and not a.no_prover:  # the whole proof next to the MSM of the same length
            rows = c.sample_scalars(4 * n, 61)
            c.scalars_eq(point, out=rows[:n])
            table = torch.empty_like(rows)
            prover_terms = [(1, (0, 1, 2)), (r - 1, (0, 3))]
            c.set_bases(c.sample_points(n, 41), endomorphism=None)

            def challenge(j, values):
                return int.from_bytes(hashlib.sha256(values).digest(), "little") % r

            def prove():
                table.copy_(rows)
                return c.sumcheck_prove(table, prover_terms, 4, challenge)

            prove(), c.msm(va)
            tp, tm = [], []
            for _ in range(a.rounds):
                tp.append(timed(prove, max(a.calls // 4, 1)))
                tm.append(timed(lambda: c.msm(va), a.calls))
            report(label, "sumcheck_prove, %d rounds" % k, tp, "msm of 2^%d" % k, tm, a.rounds, a.calls, judged=False)
            del rows, table
        del ab, va, vb, work, tmp, tmp2, eq_new, eq_old, pairs
        torch.cuda.empty_cache()
    c = next(iter(ctxs.values()))
    two = c.sample_scalars(4, 71)
    floor = [("round at n = 2", lambda: c.scalars_sumcheck_round(two, [(1, (0, 1))], batch=2)), ("eval at n = 2", lambda: c.scalars_mle_eval(two[:2], [5])),
             ("dot at n = 2 (two copies)", lambda: c.scalars_dot(two[:2], two[2:]))]
    for _, fn in floor:
        fn()
    t = {}
    for _ in range(a.rounds):
        for name, fn in floor:
            t.setdefault(name, []).append(timed(fn, 10 * a.calls))
    for name, _ in floor:
        print("the floor  %-26s %9.1f us/call (%.1f .. %.1f over %d rounds of %d)" % (name, statistics.mean(t[name]) * 1e6, min(t[name]) * 1e6, max(t[name]) * 1e6, a.rounds,
                                                                                     10 * a.calls))
    for c in ctxs.values():
        c.close()
    api.frmle_release()
    api.frpoly_release()
    api.frvec_release()


if __name__ == "__main__":
    main()
