#!/usr/bin/env python3
"""Timing of the sparse matrix-vector product (MsmContext.scalars_matvec: libmsm_frmat.so) on one GPU.  There is no earlier route on the device
that gives the same result, so every shape is timed against a YARDSTICK from the unchanged libraries, in the same process: scalars_mul over nnz
elements and scalars_scan(op="sum") over nnz elements -- the same multiplications and the same additions on contiguous data, without a gather.
A verdict line says MET (the product's mean is no longer than the yardstick's) or NOT MET.

Shapes, rows = cols = 2^k, nnz = 4 rows in all three:
  (a) uniform             4 entries a row, random columns
  (b) R1CS-like           a quarter of the rows reference column 0 (the constant one), 8 rows hold rows / 16 entries each, the others 3 or 4
  (c) the transpose of (b)   column 0 is now a ROW of rows / 4 entries
and the ratio (b) / (a) at equal nnz -- the balancing claim -- and the gathered bytes per second (nnz x 32 bytes of x per product).
At 2^20: r1cs_tables (three products) next to the ctx.msm of the same length and next to sumcheck_prove over its output.

Protocol: device data, every shape warmed up, then `--calls` calls timed back to back (each call returns when its stream has completed), the
product and its yardstick ALTERNATED `--rounds` times; min .. max over the rounds beside every mean.  Every shape's result is checked in the
run, on sampled rows against Python integers.

usage: tools/bench_frmat.py [--log-rows 16,20,22] [--calls 20] [--rounds 3] [--no-check] [--no-prover]"""
import argparse
import hashlib
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

PROVER_LOG_N = 20
CURVE = "bn254"


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


def random_values(gen, n):
    """n canonical scalars of BN254 as n x 32 bytes: the top byte below 0x30, the top byte of r"""
    v = gen.integers(0, 256, size=(n, 32), dtype=np.uint8)
    v[:, 31] &= 0x1F
    return v


def uniform(gen, rows):
    ptr = 4 * np.arange(rows + 1, dtype=np.int64)
    return ptr, gen.integers(0, rows, size=4 * rows, dtype=np.int64)


def r1cs_like(gen, rows):
    """4 rows entries: 8 rows of rows / 16, the others 3 each and one more in as many as it takes; column 0 in every fourth row"""
    lengths = np.full(rows, 3, dtype=np.int64)
    heavy = (np.arange(8) * (rows // 8) + rows // 16).astype(np.int64)
    lengths[heavy] = rows // 16
    light = np.setdiff1d(np.arange(rows), heavy)
    lengths[light[:4 * rows - int(lengths.sum())]] += 1
    assert int(lengths.sum()) == 4 * rows
    ptr = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lengths)])
    idx = gen.integers(1, rows, size=4 * rows, dtype=np.int64)
    idx[ptr[:-1][::4]] = 0
    return ptr, idx


def check_rows(ptr, idx, val, x, y, r, sample, transpose_of=None):
    """y on the sampled rows against Python integers; transpose_of: y is M^T x, the sample are columns"""
    if transpose_of is None:
        for i in sample:
            e = np.arange(ptr[i], ptr[i + 1])
            xs = ints(x, idx[e])
            want = sum(int.from_bytes(val[k].tobytes(), "little") * v for k, v in zip(e, xs)) % r
            if ints(y, [i]) != [want]:
                return False
        return True
    row_of = transpose_of
    for j in sample:
        e = np.nonzero(idx == j)[0]
        xs = ints(x, row_of[e])
        want = sum(int.from_bytes(val[k].tobytes(), "little") * v for k, v in zip(e, xs)) % r
        if ints(y, [j]) != [want]:
            return False
    return True


def report(label, name, new, ref, rounds, calls, nnz, judged=True, ref_name="mul + scan(sum) over nnz"):
    mn, mr = statistics.mean(new), statistics.mean(ref)
    print("%s %-24s %9.3f ms/call (%.3f .. %.3f over %d rounds of %d)  against %-26s %9.3f ms/call (%.3f .. %.3f)  = %.2f x  %s   gathered %.0f GB/s" % (
        label, name, mn * 1e3, min(new) * 1e3, max(new) * 1e3, rounds, calls, ref_name, mr * 1e3, min(ref) * 1e3, max(ref) * 1e3, mn / mr,
        ("MET" if mn <= mr else "NOT MET") if judged else "(reported)", 32 * nnz / mn / 1e9), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", default="16,20,22")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-prover", action="store_true")
    a = ap.parse_args()
    print("device: %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    r = api.SCALAR_FIELDS[CURVE]
    c = m.MsmContext(0, curve=CURVE)
    gen = np.random.default_rng(31)
    for k in [int(s) for s in a.log_rows.split(",")]:
        rows = 1 << k
        nnz = 4 * rows
        label = "%-6s 2^%-2d" % (CURVE, k)
        val = random_values(gen, nnz)
        t0 = time.perf_counter()
        pa, ia = uniform(gen, rows)
        pb, ib = r1cs_like(gen, rows)
        ma = c.scalars_matrix(rows, rows, pa, ia, val)
        mb = c.scalars_matrix(rows, rows, pb, ib, val, transpose=True)
        x = c.sample_scalars(rows, 51)
        y = torch.empty_like(x)
        flat, prod = c.sample_scalars(nnz, 52), torch.empty((nnz, 32), dtype=torch.uint8, device="cuda")
        flat2 = c.sample_scalars(nnz, 53)

        def yardstick():
            c.scalars_mul(flat, flat2, out=prod)
            c.scalars_scan(prod, op="sum", out=prod)

        shapes = [("(a) uniform", lambda: c.scalars_matvec(ma, x, out=y)), ("(b) R1CS-like", lambda: c.scalars_matvec(mb, x, out=y)),
                  ("(c) transpose of (b)", lambda: c.scalars_matvec(mb, x, out=y, transpose=True))]
        for _, fn in shapes:  # (the first product on a side also takes the matrix to the device)
            fn()
        yardstick()
        print("%s set-up (arrays, create, first products): %.2f s; launches and levels: %s" % (
            label, time.perf_counter() - t0, ", ".join("%s %s" % (name, (fn(), api.frmat_last())[1]) for name, fn in shapes)), flush=True)
        bad = []
        if not a.no_check:
            sample = sorted({0, 1, rows // 16, rows - 1} | {int(v) for v in gen.integers(0, rows, size=6)})
            shapes[0][1]()
            if not check_rows(pa, ia, val, x, y, r, sample):
                bad.append("(a)")
            shapes[1][1]()
            if not check_rows(pb, ib, val, x, y, r, sample):
                bad.append("(b)")
            shapes[2][1]()
            row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(pb))
            if not check_rows(pb, ib, val, x, y, r, sample, transpose_of=row_of):
                bad.append("(c)")
        t = {}
        for _ in range(a.rounds):
            for name, fn in shapes:
                t.setdefault(name, []).append(timed(fn, a.calls))
                t.setdefault(name + " / ref", []).append(timed(yardstick, a.calls))
        for name, _ in shapes:
            report(label, name, t[name], t[name + " / ref"], a.rounds, a.calls, nnz)
        print("%s (b) / (a) at equal nnz = %d: %.2f x;  checked on sampled rows against Python integers: %s" % (
            label, nnz, statistics.mean(t["(b) R1CS-like"]) / statistics.mean(t["(a) uniform"]), "unchecked" if a.no_check else ("ok" if not bad else "WRONG: " + ", ".join(bad))),
            flush=True)
        if k == PROVER_LOG_N and not a.no_prover:  # the three tables next to the commitment before them and the sumcheck behind them
            buf = torch.empty((4, rows, 32), dtype=torch.uint8, device="cuda")
            point = [int(v) for v in gen.integers(2, 1 << 62, size=k)]
            c.scalars_eq(point, out=buf[0])
            c.set_bases(c.sample_points(rows, 41), endomorphism=None)
            terms = [(1, (0, 1, 2)), (r - 1, (0, 3))]

            def challenge(j, values):
                return int.from_bytes(hashlib.sha256(values).digest(), "little") % r

            def tables():
                c.r1cs_tables(ma, mb, ma, x, out=buf, first_row=1)

            work = torch.empty_like(buf)

            def prove():
                work.copy_(buf)
                return c.sumcheck_prove(work, terms, 4, challenge)

            tables(), c.msm(x), prove()
            tt, tm, tp = [], [], []
            for _ in range(a.rounds):
                tt.append(timed(tables, a.calls))
                tm.append(timed(lambda: c.msm(x), a.calls))
                tp.append(timed(prove, max(a.calls // 4, 1)))
            report(label, "r1cs_tables (3 products)", tt, tm, a.rounds, a.calls, 3 * nnz, judged=False, ref_name="msm of 2^%d" % k)
            report(label, "r1cs_tables (3 products)", tt, tp, a.rounds, a.calls, 3 * nnz, judged=False, ref_name="sumcheck_prove, %d rounds" % k)
            del buf, work
        ma.close(), mb.close()
        del x, y, flat, flat2, prod, val
        torch.cuda.empty_cache()
    c.close()
    api.frmat_release()
    api.frmle_release()
    api.frvec_release()


if __name__ == "__main__":
    main()
