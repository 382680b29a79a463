"""Child driver of tests/test_gpu_env_paths.py: runs one seeded workload of MSMs in a FRESH process -- the library reads its MSM_HIP_*
settings once, so each setting needs a process of its own -- checks every result bit-exactly against the CPU oracle, and prints one JSON
line: {"workload", "cases", "failures", "evidence"}.  `evidence` is what the test hook msm_hip_test_env_report (api.env_report) read back:
the resolved settings and, per case, the shape the launch took.  Exit status 0 only if every case matched.
Usage: python tests/env_child.py WORKLOAD SEED   (test infrastructure: uses the oracle)

Points: a pool of distinct sampled points, tiled to n (P_i = pool[i mod K]); the oracle folds the scalars onto the pool -- sum_i s_i P_i =
sum_k (sum_{i = k mod K} s_i mod r) pool[k] -- and runs the CPU MSM over the K pool points (exact on groups of prime order r: BLS12-381's
pool is cofactor-cleared, G2's pool holds known multiples of the generator and is checked in closed form, as tools/fuzz_gpu.py does)."""
import ctypes
import importlib
import json
import os
import random
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import msm_webgpu_amd as m  # noqa: E402
from msm_webgpu_amd.api import env_report  # noqa: E402
from msm_webgpu_amd.sharding import window_range  # noqa: E402

ORACLE_THREADS = 16
BLS12_381_COFACTOR = 0x396C8C005555E1568C00AAAB0000AAAB
MAXLW = 64


def nwin(bits, halves=False):
    return ((127 if halves else 254) + bits) // bits


def pick_window_bits(forced, n, nvec, halves):
    """msm_plan.h: pick_window_bits, for a forced width (the bump of grouped launches whose windows would not fit MAXLW)"""
    bits = forced or ((14 if n <= 1 << 16 else 16) if nvec > 1 else (12 if n <= 1 << 12 else 16))
    while bits < 16 and nvec * nwin(bits, halves) > MAXLW:
        bits += 2
    return bits


class Curve:
    """the pool of distinct points of one curve, tiled inputs and the folded oracle"""

    def __init__(self, name, pool=1 << 13, seed=7):
        self.name = name
        if name == "bls12_381":
            pool = min(pool, 1 << 11)  # (one CPU scalar multiplication per pool point)
        self.ref = importlib.import_module("oracle." + ("bn254_ref" if name == "bn254" else name + "_ref"))
        self.R = self.ref.R
        if name.endswith("_g2"):
            pool = 1 << 12
            self.pts = self.ref.sample_points(pool, 99)
            self.mult = self.ref.sample_multipliers(pool, 99)
            self.pool = self.ref.points_to_bytes(self.pts)
        else:
            self.cpu = importlib.import_module("oracle.cpu" if name == "bn254" else "oracle.cpu_" + name)
            raw = self.cpu.sample_points(seed, pool)
            if name == "bls12_381":  # h P: the sampler's points lie outside the subgroup of order r, where folding mod r would not be exact
                pb = len(raw) // pool
                h = self.ref.scalars_to_bytes([BLS12_381_COFACTOR])
                raw = b"".join(self.cpu.to_affine64(self.cpu.cpu_msm(raw[pb * k:pb * k + pb], h)) for k in range(pool))
                r = self.ref.scalars_to_bytes([self.R])
                assert self.cpu.to_affine64(self.cpu.cpu_msm(raw[:pb], r)) == self.cpu.to_affine64(self.cpu.cpu_msm(raw[:pb], bytes(32)))
            self.pool = raw
        self.K = pool
        self.pb = len(self.pool) // pool

    def points(self, n):
        full, rest = divmod(n, self.K)
        return self.pool * full + self.pool[:rest * self.pb]

    def oracle(self, scalars):
        n = len(scalars)
        k = min(n, self.K)
        folded = [0] * k
        for i, s in enumerate(scalars):
            folded[i % k] += s
        folded = [f % self.R for f in folded]
        if self.name.endswith("_g2"):
            t = sum(f * mu for f, mu in zip(folded, self.mult)) % self.R
            return self.ref.affine_to_bytes(self.ref.mul(t, self.ref.G))
        return self.cpu.to_affine64(self.cpu.cpu_msm(self.pool[:k * self.pb], self.ref.scalars_to_bytes(folded), ORACLE_THREADS))

    def scalars(self, rnd, n, kind="uniform"):
        R = self.R
        if kind == "equal":
            return [rnd.randrange(R)] * n
        if kind == "three":
            vals = [rnd.randrange(R) for _ in range(3)]
            return [vals[rnd.randrange(3)] for _ in range(n)]
        if kind == "half_equal":
            v = rnd.randrange(R)
            return [v if i % 2 else rnd.randrange(R) for i in range(n)]
        if kind == "skewed":  # a few large buckets: small values
            return [rnd.randrange(1 << 17) for _ in range(n)]
        return [rnd.randrange(R) for _ in range(n)]

    def enc(self, scalars):
        return self.ref.scalars_to_bytes(scalars)


class Run:
    def __init__(self, workload):
        self.workload = workload
        self.cases = 0
        self.failures = []
        self.evidence = {"settings": env_report()}

    def check(self, label, got, want):
        self.cases += 1
        gb = got.to_affine_bytes() if hasattr(got, "to_affine_bytes") else got
        if gb != want:
            self.failures.append(label)
            print("MISMATCH %s" % label, file=sys.stderr, flush=True)

    def expect(self, label, ok):
        """a 'took effect' condition: counted like a wrong result when it does not hold"""
        if not ok:
            self.failures.append("effect: " + label)
            print("EFFECT NOT SEEN %s" % label, file=sys.stderr, flush=True)

    def note(self, key, value):
        self.evidence.setdefault(key, []).append(value)


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def shares(ctx, t, n, nwindows, size, curve):
    """every share of `size` windows of one vector, gathered and combined (16-bit windows); the first share is launched last, so that the
    context's last launch is a share of `size` windows"""
    parts = [ctx.msm_windows(t, b, min(b + size, nwindows)) for b in reversed(range(0, nwindows, size))][::-1]
    return m.MsmContext.combine_windows(torch.cat(parts, dim=0), curve=curve)


def half_shares(ctx, t, n, size, curve):
    """the 8 half-length windows of endomorphism bases in shares of `size`, one vector per launch"""
    parts = []
    for b in range(0, 8, size):
        e = min(b + size, 8)
        out = torch.empty((e - b, 3 * ctx.cb), dtype=torch.uint8, device="cuda")
        ctx.launch_half_windows_batch(t, n, b, e, 1, out)
        ctx.slot_sync(1)
        parts.append(out)
    return m.MsmContext.combine_windows(torch.cat(parts, dim=0), curve=curve)


def grouped(ctx, vecs, n, world, curve):
    """a group of vectors through every rank's launch_windows_batch; returns the combined MSM of each vector"""
    g = len(vecs)
    t = dev(b"".join(vecs))
    outs = []
    for r in range(world):
        b, e = window_range(r, world)
        out = torch.empty((g * (e - b), 3 * ctx.cb), dtype=torch.uint8, device="cuda")
        ctx.launch_windows_batch(t, n, b, e, r % 4, out)
        ctx.slot_sync(r % 4)
        outs.append((b, e, out))
    res = []
    for v in range(g):
        parts = [out[v * (e - b):(v + 1) * (e - b)] for b, e, out in outs]
        res.append(m.MsmContext.combine_windows(torch.cat(parts, dim=0), curve=curve))
    return res


def vwindow_shares(ctx, sb, n, world, curve):
    nv = ctx.virtual_windows()
    t = dev(sb)
    pairs = []
    for r in range(world):
        b, e = window_range(r, world, nv)
        if e == b:
            continue
        out = torch.empty(((e - b) * 2, 3 * ctx.cb), dtype=torch.uint8, device="cuda")
        ctx.launch_vwindows_batch(t, n, b, e, r % 4, out)
        ctx.slot_sync(r % 4)
        pairs.append(out)
    return m.MsmContext.combine_vwindows_batch(torch.cat(pairs, dim=0).cpu(), nv, curve)[0]


def oneshot(ctx_curve_id, cb, points, sb, n, modulus):
    out = ctypes.create_string_buffer(3 * cb)
    rc = m.lib().msm_hip_msm_curve(ctx_curve_id, points, sb, n, out)
    if rc:
        raise m.MsmHipError(rc, "msm_hip_msm_curve")
    return m.G1(out.raw, modulus)


# ---- workloads: one per row family of tests/test_gpu_env_paths.py


def w_window_bits(run, rnd):
    """sync host / device, slot, a batch of 9 and 16-bit window shares, plain and endomorphism bases, n in {1, 4097, 70000}"""
    cv = Curve("bn254")
    forced = run.evidence["settings"]["window_bits"]
    ctx = m.MsmContext(0)
    for n in (1, 4097, 70000):
        pts = cv.points(n)
        vecs = [cv.scalars(rnd, n, k) for k in ("uniform", "three", "equal")]
        wants = [cv.oracle(v) for v in vecs]
        sbs = [cv.enc(v) for v in vecs]
        for endo in (False, True):
            ctx.set_bases(pts, endomorphism=endo)
            tag = "n%d/%s" % (n, "endo" if endo else "plain")
            single = pick_window_bits(forced, n, 1, endo)
            run.check(tag + "/host", ctx.msm(sbs[0]), wants[0])
            run.note("single_wbits", [n, endo, ctx.last_window_bits()])
            run.expect(tag + "/host wbits", ctx.last_window_bits() == single)
            run.check(tag + "/device", ctx.msm(dev(sbs[1])), wants[1])
            run.expect(tag + "/device wbits", ctx.last_window_bits() == single)
            ctx.launch_host(sbs[2], slot=2)
            run.check(tag + "/slot", ctx.finish(2), wants[2])
            run.expect(tag + "/slot wbits", ctx.last_window_bits() == single)
            # a batch of 9: groups of batch_group_size, the last one's window bits by the bump rule
            g = ctx.batch_group_size(n)
            fit = MAXLW // nwin(pick_window_bits(forced, n, 2, endo), endo)
            run.expect(tag + "/group size", g == max(1, min((1 << 20) // n, fit, MAXLW)))
            blob = b"".join(sbs[j % 3] for j in range(9))
            res = ctx.msm_batch(blob if endo else dev(blob), n)
            for j in range(9):
                run.check(tag + "/batch%d" % j, res[j], wants[j % 3])
            last_nvec = 9 - g * ((9 - 1) // g)
            run.note("batch_wbits", [n, endo, g, ctx.last_window_bits()])
            run.expect(tag + "/batch wbits", ctx.last_window_bits() == pick_window_bits(forced, n, last_nvec, endo))
            if not endo:  # window shares index the reference's 16 windows: always 16 bits
                run.check(tag + "/shares", shares(ctx, dev(sbs[0]), n, 16, 8, "bn254"), wants[0])
                run.expect(tag + "/share wbits", ctx.last_window_bits() == 16)
    ctx.close()


CHUNK_CURVES = ("bn254", "bls12_381", "bn254_g2")


def w_chunk(run, rnd):
    """2^16 uniform, all-equal and 3-value scalars, a batch and 17-bit (BLS12-381: 19-bit) wide tables on three curves"""
    n = 1 << 16
    for name in CHUNK_CURVES:
        cv = Curve(name)
        ctx = m.MsmContext(0, curve=name)
        pts = cv.points(n)
        ctx.set_bases(pts)
        for kind in ("uniform", "equal", "three"):
            v = cv.scalars(rnd, n, kind)
            want = cv.oracle(v)
            run.check("%s/%s" % (name, kind), ctx.msm(cv.enc(v)), want)
            rep = ctx.env_report()
            run.note("chunk_len", [name, kind, rep["last_chunk_len"], rep["last_w_count"]])
        vs = [cv.scalars(rnd, n) for _ in range(2)]
        res = ctx.msm_batch(dev(b"".join(cv.enc(v) for v in vs)), n)
        for j, v in enumerate(vs):
            run.check("%s/batch%d" % (name, j), res[j], cv.oracle(v))
        run.note("chunk_len_batch", [name, ctx.env_report()["last_chunk_len"]])
        ctx.set_wide_bits(19 if name == "bls12_381" else 17)
        ctx.set_bases(pts, precompute="wide")
        v = cv.scalars(rnd, n)
        run.check("%s/wide" % name, ctx.msm(cv.enc(v)), cv.oracle(v))
        run.note("chunk_len_wide", [name, ctx.env_report()["last_chunk_len"]])
        ctx.close()


def w_bpr(run, rnd):
    """single launches at widths 12, 14 and 16, batches, grouped launches and 2-window shares on BN254, BLS12-381 and BN254 G2"""
    n = 4097
    for name in CHUNK_CURVES:
        cv = Curve(name)
        ctx = m.MsmContext(0, curve=name)
        ctx.set_bases(cv.points(n))
        vs = [cv.scalars(rnd, n, k) for k in ("uniform", "three", "uniform")]
        wants = [cv.oracle(v) for v in vs]
        sbs = [cv.enc(v) for v in vs]
        for bits in (12, 14, 16):
            ctx.set_window_bits(bits)
            run.check("%s/w%d" % (name, bits), ctx.msm(sbs[0]), wants[0])
            rep = ctx.env_report()
            run.note("logr", [name, "single", rep["last_wbits"], rep["last_w_count"], rep["last_logr"]])
            res = ctx.msm_batch(dev(b"".join(sbs)), n)
            for j in range(3):
                run.check("%s/w%d/batch%d" % (name, bits, j), res[j], wants[j])
            rep = ctx.env_report()
            run.note("logr", [name, "batch", rep["last_wbits"], rep["last_w_count"], rep["last_logr"]])
        ctx.set_window_bits(0)
        res = grouped(ctx, sbs, n, 2, name)
        for j in range(3):
            run.check("%s/grouped%d" % (name, j), res[j], wants[j])
        rep = ctx.env_report()
        run.note("logr", [name, "grouped", rep["last_wbits"], rep["last_w_count"], rep["last_logr"]])
        run.check("%s/shares2" % name, shares(ctx, dev(sbs[1]), n, 16, 2, name), wants[1])
        rep = ctx.env_report()
        run.note("logr", [name, "share2", rep["last_wbits"], rep["last_w_count"], rep["last_logr"]])
        ctx.close()


def w_planes(run, rnd):
    """window shares of 1, 2, 8 and 15 windows, half-window shares, whole MSMs in both base modes, batches"""
    cv = Curve("bn254")
    n = 4097
    ctx = m.MsmContext(0)
    pts = cv.points(n)
    vs = [cv.scalars(rnd, n, k) for k in ("uniform", "three")]
    wants = [cv.oracle(v) for v in vs]
    sbs = [cv.enc(v) for v in vs]
    ctx.set_bases(pts)
    for size in (1, 2, 8, 15):
        run.check("share%d" % size, shares(ctx, dev(sbs[size % 2]), n, 16, size, "bn254"), wants[size % 2])
        run.note("planes", ["share", size, ctx.env_report()["last_planes"]])
    run.check("whole/plain", ctx.msm(sbs[0]), wants[0])
    run.note("planes", ["whole", 16, ctx.env_report()["last_planes"]])
    res = ctx.msm_batch(dev(b"".join(sbs)), n)
    for j in range(2):
        run.check("batch/plain%d" % j, res[j], wants[j])
    run.note("planes", ["batch", 16, ctx.env_report()["last_planes"]])
    ctx.set_bases(pts, endomorphism=True)
    for size in (1, 2, 8):
        run.check("half_share%d" % size, half_shares(ctx, dev(sbs[size % 2]), n, size, "bn254"), wants[size % 2])
        run.note("planes", ["half_share", size, ctx.env_report()["last_planes"]])
    run.check("whole/endo", ctx.msm(sbs[1]), wants[1])
    run.note("planes", ["whole_endo", 8, ctx.env_report()["last_planes"]])
    res = ctx.msm_batch(b"".join(sbs), n)
    for j in range(2):
        run.check("batch/endo%d" % j, res[j], wants[j])
    ctx.close()


def w_pipeline(run, rnd):
    """sync launches and pipelined launches across all slots, host and device scalars"""
    cv = Curve("bn254")
    ctx = m.MsmContext(0)
    for n in (4097, 70000):
        ctx.set_bases(cv.points(n), endomorphism=n > 5000)
        vs = [cv.scalars(rnd, n, k) for k in ("uniform", "three", "equal", "uniform")]
        wants = [cv.oracle(v) for v in vs]
        sbs = [cv.enc(v) for v in vs]
        run.check("n%d/sync" % n, ctx.msm(sbs[0]), wants[0])
        run.note("inline", ["sync", n, ctx.env_report()["last_inline_reduce"]])
        ts = [dev(b) for b in sbs]
        for rounds in range(2):
            for slot in range(4):
                if slot % 2:
                    ctx.launch_host(sbs[slot], slot=slot)
                else:
                    ctx.launch(ts[slot], slot=slot)
            for slot in range(4):
                run.check("n%d/pipe%d/slot%d" % (n, rounds, slot), ctx.finish(slot), wants[slot])
        run.note("inline", ["pipelined", n, ctx.env_report()["last_inline_reduce"]])
    ctx.close()


def w_fine_hist(run, rnd):
    """uniform, all-equal and half-equal scalars at 2^17"""
    cv = Curve("bn254")
    n = 1 << 17
    ctx = m.MsmContext(0)
    ctx.set_bases(cv.points(n))
    for kind in ("uniform", "equal", "half_equal", "uniform"):
        v = cv.scalars(rnd, n, kind)
        run.check(kind, ctx.msm(cv.enc(v)), cv.oracle(v))
        run.note("fine_hist", [kind, ctx.env_report()["last_fine_hist"]])
    ctx.close()


def w_bases_auto(run, rnd):
    """set_bases with flags 0 on BN254 and Grumpkin, then dense, batch, sparse and one-shot"""
    for name in ("bn254", "grumpkin"):
        cv = Curve(name)
        ctx = m.MsmContext(0, curve=name)
        n = 4097
        pts = cv.points(n)
        ctx.set_bases(pts, endomorphism=None)
        run.note("uses_endomorphism", [name, ctx.uses_endomorphism()])
        v = cv.scalars(rnd, n)
        want = cv.oracle(v)
        run.check(name + "/dense", ctx.msm(cv.enc(v)), want)
        res = ctx.msm_batch(dev(cv.enc(v) * 2), n)
        run.check(name + "/batch", res[1], want)
        idx = [rnd.randrange(n) for _ in range(3000)]
        sv = cv.scalars(rnd, len(idx))
        gathered = [0] * n
        for i, s in zip(idx, sv):
            gathered[i] = (gathered[i] + s) % cv.R
        run.check(name + "/sparse", ctx.msm_sparse(idx, cv.enc(sv)), cv.oracle(gathered))
        run.check(name + "/oneshot", oneshot(ctx.curve_id, ctx.cb, pts, cv.enc(v), n, ctx.modulus), want)
        ctx.close()
    m.lib().msm_hip_oneshot_release()


def w_oneshot_chunks(run, rnd):
    """msm_hip_msm_curve at n in {1, 1023, 1025, 70001} and 2^19 + 3 on BN254 (endomorphism bases) and BLS12-381 (plain bases)"""
    for name in ("bn254", "bls12_381"):
        cv = Curve(name)
        ctx = m.MsmContext(0, curve=name)
        for n in (1, 1023, 1025, 70001, (1 << 19) + 3):
            v = cv.scalars(rnd, n)
            run.check("%s/n%d" % (name, n), oneshot(ctx.curve_id, ctx.cb, cv.points(n), cv.enc(v), n, ctx.modulus), cv.oracle(v))
            rep = env_report()
            run.note("upload", [name, n, rep["upload_parts"], rep["upload_chunks"]])
        ctx.close()
    m.lib().msm_hip_oneshot_release()


def w_parts(run, rnd):
    """one-shot and msm_hip_run with host scalars at 2^19 + 3 and 2^20 + 5, each called twice (the kept contexts)"""
    cv = Curve("bn254")
    ctx = m.MsmContext(0)
    for n in ((1 << 19) + 3, (1 << 20) + 5):
        pts = cv.points(n)
        ctx.set_bases(pts)
        for call in range(2):
            v = cv.scalars(rnd, n, "uniform" if call == 0 else "three")
            want = cv.oracle(v)
            sb = cv.enc(v)
            run.check("n%d/oneshot%d" % (n, call), oneshot(ctx.curve_id, ctx.cb, pts, sb, n, ctx.modulus), want)
            rep = env_report()
            run.note("parts", ["oneshot", n, rep["upload_parts"], rep["upload_chunks"]])
            run.check("n%d/run%d" % (n, call), ctx.msm(sb), want)
            run.note("parts", ["run", n, env_report()["upload_parts"], 0])
    ctx.close()
    m.lib().msm_hip_oneshot_release()


def w_wide(run, rnd):
    """wide tables: whole MSMs, a batch, virtual-window shares at world 1 / 2 / 8, all-equal scalars; BN254 and BLS12-381"""
    forced = run.evidence["settings"]["wide_bits"]
    for name in ("bn254", "bls12_381"):
        cv = Curve(name)
        ctx = m.MsmContext(0, curve=name)
        n = 4097
        pts = cv.points(n)
        widths = [forced] if forced else [16, 17, 19, 20]
        for bits in widths:
            if name == "bls12_381" and bits == 17:  # (15 x 17 bits cannot hold BLS12-381's scalars)
                continue
            if forced:
                ctx.set_bases(pts, precompute="wide")  # the width from MSM_HIP_WIDE_BITS
            else:
                ctx.set_wide_bits(bits)
                ctx.set_bases(pts, precompute="wide")
                ctx.set_wide_bits(0)
            run.note("wide_bits", [name, bits, ctx.wide_bits()])
            run.expect("%s/%d wide_bits" % (name, bits), ctx.wide_bits() == bits)
            vs = [cv.scalars(rnd, n, k) for k in ("uniform", "equal", "skewed")]
            wants = [cv.oracle(v) for v in vs]
            sbs = [cv.enc(v) for v in vs]
            tag = "%s/w%d" % (name, bits)
            for j in range(3):
                run.check(tag + "/whole%d" % j, ctx.msm(sbs[j]), wants[j])
            rep = ctx.env_report()
            run.note("top_shift", [name, bits, rep["last_wide_top_shift"]])
            res = ctx.msm_batch(dev(b"".join(sbs[:2])), n)
            for j in range(2):
                run.check(tag + "/batch%d" % j, res[j], wants[j])
            for world in (1, 2, 8):
                for j in (0, 2):
                    run.check(tag + "/shares%d/%d" % (world, j), vwindow_shares(ctx, sbs[j], n, world, name), wants[j])
                    rep = ctx.env_report()
                    run.note("share_lists", [name, bits, world, rep["last_list_path"]])
        if forced:  # msm_hip_set_wide_bits takes precedence over the environment
            other = 16 if forced != 16 else 18
            ctx.set_wide_bits(other)
            ctx.set_bases(pts, precompute="wide")
            ctx.set_wide_bits(0)
            run.expect("%s set_wide_bits precedence" % name, ctx.wide_bits() == other)
            run.note("precedence", [name, other, ctx.wide_bits()])
            v = cv.scalars(rnd, n)
            run.check("%s/precedence" % name, ctx.msm(cv.enc(v)), cv.oracle(v))
        ctx.close()


def w_combine(run, rnd):
    """batches, grouped launches and MultiGpuMsm([0] * 8): the host window combines of several MSMs"""
    cv = Curve("bn254")
    n = 4097
    ctx = m.MsmContext(0)
    pts = cv.points(n)
    ctx.set_bases(pts)
    vs = [cv.scalars(rnd, n, "uniform" if j % 2 else "three") for j in range(4)]
    wants = [cv.oracle(v) for v in vs]
    sbs = [cv.enc(v) for v in vs]
    res = ctx.msm_batch(b"".join(sbs), n)
    for j in range(4):
        run.check("batch%d" % j, res[j], wants[j])
    res = grouped(ctx, sbs, n, 4, "bn254")
    for j in range(4):
        run.check("grouped%d" % j, res[j], wants[j])
    ctx.close()
    mg = m.MultiGpuMsm([0] * 8, "host")
    mg.set_bases(pts)
    run.check("mgpu/msm", mg.msm(sbs[0]), wants[0])
    g = min(4, mg.group_size)
    mg.launch_batch(b"".join(sbs[:g]), n, 1)
    res = mg.finish_batch(1, g)
    for j in range(g):
        run.check("mgpu/batch%d" % j, res[j], wants[j])
    mg.close()
    rep = env_report()
    run.note("combine", [rep["combine_helpers"], rep["combine_started"]])


def w_debug_sync(run, rnd):
    """one short pass over every workload family"""
    w_window_bits(run, rnd)
    w_planes(run, rnd)
    w_pipeline(run, rnd)
    w_bases_auto(run, rnd)
    w_combine(run, rnd)


WORKLOADS = {
    "window_bits": w_window_bits,
    "chunk": w_chunk,
    "bpr": w_bpr,
    "planes": w_planes,
    "pipeline": w_pipeline,
    "fine_hist": w_fine_hist,
    "bases_auto": w_bases_auto,
    "oneshot_chunks": w_oneshot_chunks,
    "parts": w_parts,
    "wide": w_wide,
    "combine": w_combine,
    "debug_sync": w_debug_sync,
}


def main(argv):
    workload, seed = argv[1], int(argv[2])
    run = Run(workload)
    try:
        WORKLOADS[workload](run, random.Random(seed))
    except Exception:  # a library error is a failed case, reported like a wrong result
        traceback.print_exc()
        run.failures.append("exception: " + traceback.format_exc().strip().splitlines()[-1])
    run.evidence["settings_after"] = env_report()
    print(json.dumps({"workload": workload, "cases": run.cases, "failures": run.failures, "evidence": run.evidence}), flush=True)
    return 0 if not run.failures and run.cases else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
