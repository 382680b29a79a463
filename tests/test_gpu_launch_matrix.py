"""Every launch shape plan_launch can make, checked bit-exact against the CPU oracle: scalar format (canonical, MONT256, U8 .. U64) x base mode
(plain, endomorphism, 16-bit tables, wide tables) x window setting (auto, 12, 14, 16) x shape (dense, sparse), through every whole-MSM entry point
(sync host, sync device, launch + finish on a non-zero slot, and for dense vectors the host and device batch).  Nothing is sampled: every run
reaches every cell, and after every call last_window_bits() must be the width the documented rules give (include/msm_hip.h; modelled by
tests/launch_model.py), which proves the cell was reached.  The pairs the API rejects are asserted as rejections.

Values plant the edges of the signed recode at the width that runs (tests/edge_scalars.py); each oracle answer is computed once per (points,
integers, indices) and shared by every cell that takes the same input.  A long-lived context then runs a seeded walk through the matrix with
base-set, window and format changes between steps, and checks the skew credit (msm_hip_test_skew_credit) after each step."""
import importlib
import random
import zlib

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import cpu
from tests.edge_scalars import edge_vector
from tests.launch_model import NB, batch_groups, run_bits  # the documented rules

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG = -2
FORMATS = ["canonical", "mont256", "u8", "u16", "u32", "u64"]
MODES = ["plain", "endomorphism", "tables", "wide"]
WINDOWS = [0, 12, 14, 16]
NP_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
TORCH_DTYPES = {1: torch.uint8, 2: torch.uint16, 4: torch.uint32, 8: torch.uint64}
OTHER_CURVES = ["grumpkin", "pallas", "vesta", "bls12_381", "bn254_g2", "bls12_381_g2"]


def oracle_module(curve):
    return cpu if curve == "bn254" else importlib.import_module("oracle.cpu_" + curve)


def scalar_order(curve):
    return importlib.import_module("oracle.%s_ref" % curve).R


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def plant_bits(fmt, mode, fixed, n):
    """the window width whose recode edges a cell's values plant: the one that runs (byte windows: the 8-bit edges)"""
    return 8 if NB[fmt] in (1, 2) else run_bits(fmt, mode, fixed, n)


def base_flags(mode):
    return dict(endomorphism=mode == "endomorphism", precompute="wide" if mode == "wide" else mode == "tables")


def set_format(c, fmt):
    c.set_scalar_format(mont256=fmt == "mont256", width=NB[fmt] or 32)


# ---------------------------------------------------------------------------------------------------------------- one context's checks
class Matrix:
    """A context, its points (host wire bytes; every base set is a prefix), the oracle answers so far, and the failures met.  Failures are
    collected, not raised, so that one run names every cell that differs."""

    def __init__(self, c, curve, points):
        self.c, self.curve, self.points = c, curve, points
        self.orc, self.r = oracle_module(curve), scalar_order(curve)
        self.answers, self.vectors = {}, {}
        self.failures, self.reached = [], set()
        self.slot = 0

    def next_slot(self):
        self.slot = self.slot % 3 + 1  # slots 1 .. 3 (the sync calls use slot 0)
        return self.slot

    # -- inputs
    def values(self, fmt, c, n, kind="edges"):
        """n integers of the format planting the C-bit edges; "equal": all of them the longest carry chain; "reversed": the edges last"""
        nb = NB[fmt]
        key = (nb, c, n, kind)
        if key not in self.vectors:
            seed = zlib.crc32(repr((self.curve, nb, c, n)).encode())
            v = edge_vector(8 * nb, c, n, seed) if nb else edge_vector(self.r.bit_length(), c, n, seed, r=self.r)
            self.vectors[key] = [v[0]] * n if kind == "equal" else v[::-1] if kind == "reversed" else v
        return self.vectors[key]

    def encode(self, fmt, ints):
        nb = NB[fmt]
        if nb:
            return np.array(ints, dtype=np.uint64).astype(NP_DTYPES[nb]).tobytes()
        if fmt == "mont256":
            ints = [(v << 256) % self.r for v in ints]
        return b"".join(v.to_bytes(32, "little") for v in ints)

    def device(self, fmt, host):
        t = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
        nb = NB[fmt]
        return t.view(TORCH_DTYPES[nb]) if nb > 1 else t

    def want(self, key, ints, idx=None):
        """the oracle's sum_j ints[j] * P[idx[j]] (idx None: the first len(ints) points), once per key"""
        if key not in self.answers:
            pb = self.c.pb
            if idx is None:
                pts = self.points[:pb * len(ints)]
            else:
                pts = np.frombuffer(self.points, dtype=np.uint8).reshape(-1, pb)[np.asarray(idx, dtype=np.int64)].tobytes()
            s32 = b"".join(v.to_bytes(32, "little") for v in ints)
            self.answers[key] = self.orc.to_affine64(self.orc.cpu_msm(pts, s32, n_threads=16))
        return self.answers[key]

    # -- checks
    def check(self, where, call, want, bits):
        try:
            got = call()
        except (m.MsmHipError, ValueError, TypeError) as e:
            self.failures.append("%s: raised %r" % (where, e))
            return
        got = [g.to_affine_bytes() for g in got] if isinstance(got, list) else got.to_affine_bytes()
        if got != want:
            self.failures.append("%s: differs from the oracle" % where)
        ran = self.c.last_window_bits()
        if ran != bits:
            self.failures.append("%s: ran at %d bits, the rules say %d" % (where, ran, bits))

    def rejected(self, where, call, exc, code=None, slot=None):
        try:
            call()
        except exc as e:
            if code is not None and e.code != code:
                self.failures.append("%s: rejected with %d, not %d" % (where, e.code, code))
            return
        except Exception as e:  # noqa: BLE001 (recorded: the wrong kind of rejection)
            self.failures.append("%s: raised %r, not %s" % (where, e, exc.__name__))
            return
        self.failures.append("%s: accepted, the API documents a rejection" % where)
        if slot is not None:
            self.c.slot_sync(slot)  # (collect what was launched, so that the slot stays usable)

    # -- cells
    def dense(self, fmt, mode, fixed, n, batch=3):
        c, nb = self.c, NB[fmt]
        cb = plant_bits(fmt, mode, fixed, n)
        ints = self.values(fmt, cb, n)
        want = self.want(("dense", nb, cb, n, "edges"), ints)
        host = self.encode(fmt, ints)
        dev = self.device(fmt, host)
        bits = run_bits(fmt, mode, fixed, n)
        where = "%s %s/%s/%d dense n=%d" % (self.curve, fmt, mode, fixed, n)
        self.check(where + " host", lambda: c.msm(host), want, bits)
        self.check(where + " device", lambda: c.msm(dev), want, bits)
        slot = self.next_slot()
        self.check(where + " slot %d" % slot, lambda: (c.launch(dev, slot=slot), c.finish(slot))[1], want, bits)
        if batch:
            kinds = ["edges", "equal", "reversed"][:batch]
            vecs = [self.values(fmt, cb, n, k) for k in kinds]
            wants = [self.want(("dense", nb, cb, n, k), v) for k, v in zip(kinds, vecs)]
            blob = b"".join(self.encode(fmt, v) for v in vecs)
            groups = batch_groups(fmt, mode, fixed, n, batch, self.c.virtual_windows() or 1)
            bbits = run_bits(fmt, mode, fixed, n, groups[-1])
            self.check(where + " batch host", lambda: c.msm_batch(blob, n), wants, bbits)
            self.check(where + " batch device", lambda: c.msm_batch(self.device(fmt, blob), n), wants, bbits)
        self.reached.add((fmt, mode, fixed, "dense"))

    def sparse_inputs(self, fmt, mode, fixed, nnz, n_bases, tag):
        """nnz entries over n_bases bases: repeats, the last base, and (32-byte formats) an opposite pair (s, r - s) on the last base"""
        nb = NB[fmt]
        cb = plant_bits(fmt, mode, fixed, nnz)
        ints = list(self.values(fmt, cb, nnz))
        rng = np.random.default_rng(zlib.crc32(repr((self.curve, nnz, n_bases, tag)).encode()))
        idx = rng.integers(0, n_bases, size=nnz, dtype=np.int64)
        idx[nnz // 2] = n_bases - 1
        if nnz >= 4:
            idx[-2:] = n_bases - 1
            if not nb:
                ints[-2:] = [ints[0], self.r - ints[0]]
        key = ("sparse", nb, cb, nnz, n_bases, tag)
        return idx, ints, self.want(key, ints, idx)

    def sparse(self, fmt, mode, fixed, nnz, n_bases, tag=""):
        c = self.c
        where = "%s %s/%s/%d sparse nnz=%d over %d" % (self.curve, fmt, mode, fixed, nnz, n_bases)
        idx, ints, want = self.sparse_inputs(fmt, mode, fixed, nnz, n_bases, tag)
        host = self.encode(fmt, ints)
        dev = self.device(fmt, host)
        di = torch.from_numpy(idx).to(torch.int32 if nnz % 2 else torch.int64).cuda()
        if mode == "wide":  # sparse MSMs over wide tables: MSM_HIP_ERR_INVALID_ARG from every entry point (include/msm_hip.h)
            self.rejected(where + " host", lambda: c.msm_sparse(idx, host), m.MsmHipError, ERR_INVALID_ARG)
            self.rejected(where + " device", lambda: c.msm_sparse(di, dev), m.MsmHipError, ERR_INVALID_ARG)
            slot = self.next_slot()
            self.rejected(where + " slot", lambda: c.launch_sparse(di, dev, slot=slot), m.MsmHipError, ERR_INVALID_ARG, slot=slot)
        else:
            bits = run_bits(fmt, mode, fixed, nnz)
            self.check(where + " host", lambda: c.msm_sparse(idx, host), want, bits)
            self.check(where + " device", lambda: c.msm_sparse(di, dev), want, bits)
            slot = self.next_slot()
            self.check(where + " slot %d" % slot, lambda: (c.launch_sparse(di, dev, slot=slot), c.finish(slot))[1], want, bits)
        self.reached.add((fmt, mode, fixed, "sparse"))

    def narrow_rejections(self, fmt, where):
        """a narrow format with the window-sharding calls (MSM_HIP_ERR_INVALID_ARG), and with mont256 (ValueError)"""
        c = self.c
        n = min(1000, c.n_bases)
        t = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        out = torch.zeros((16, c.jb), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.rejected(where + " msm_windows", lambda: c.msm_windows(t, 0, 4, out[:4]), m.MsmHipError, ERR_INVALID_ARG)
        self.rejected(where + " launch_windows_batch", lambda: c.launch_windows_batch(t, n, 0, 2, 1, out[:2]), m.MsmHipError, ERR_INVALID_ARG, slot=1)
        self.rejected(where + " launch_half_windows_batch", lambda: c.launch_half_windows_batch(t, n, 0, 8, 2, out[:8]), m.MsmHipError,
                      ERR_INVALID_ARG, slot=2)
        self.rejected(where + " launch_vwindows_batch", lambda: c.launch_vwindows_batch(t, n, 0, 1, 3, out[:2]), m.MsmHipError, ERR_INVALID_ARG,
                      slot=3)
        self.rejected(where + " mont256", lambda: c.set_scalar_format(mont256=True, width=NB[fmt]), ValueError)

    def report(self):
        assert not self.failures, "%d failures:\n%s" % (len(self.failures), "\n".join(self.failures[:60]))


# ---------------------------------------------------------------------------------------------------------------- the BN254 matrix
N_BIG, N_SMALL = 16384, 1000  # sparse: a few thousand entries over 16384 bases (the indices outrun the width choice), and more entries than bases
DENSE_N = [1, 4096, 4097]  # both sides of the automatic 12 / 16-bit threshold
SPARSE_BIG = [1, 4096, 4097]
SPARSE_SMALL = [4096, 4097]


@pytest.fixture(scope="module")
def bn254(gpu):
    c = m.MsmContext(0)
    points = c.sample_points(N_BIG, 9101).cpu().numpy().tobytes()
    M = Matrix(c, "bn254", points)
    yield M
    c.close()


@pytest.mark.parametrize("mode", MODES)
def test_bn254_matrix(bn254, mode):
    M, c = bn254, bn254.c
    M.failures, M.reached = [], set()
    c.set_bases(M.points[:N_BIG * c.pb], **base_flags(mode))
    try:
        for fmt in FORMATS:
            set_format(c, fmt)
            for fixed in WINDOWS:
                c.set_window_bits(fixed)
                for n in DENSE_N:
                    M.dense(fmt, mode, fixed, n)
                for nnz in SPARSE_BIG:
                    M.sparse(fmt, mode, fixed, nnz, N_BIG)
                if NB[fmt]:
                    M.narrow_rejections(fmt, "bn254 %s/%s/%d" % (fmt, mode, fixed))
        c.set_bases(M.points[:N_SMALL * c.pb], **base_flags(mode))  # a shrink: the base buffer keeps its capacity
        for fmt in FORMATS:
            set_format(c, fmt)
            for fixed in WINDOWS:
                c.set_window_bits(fixed)
                for nnz in SPARSE_SMALL:
                    M.sparse(fmt, mode, fixed, nnz, N_SMALL)
    finally:
        c.set_window_bits(0)
        set_format(c, "canonical")
    assert M.reached == {(f, mode, w, s) for f in FORMATS for w in WINDOWS for s in ("dense", "sparse")}
    M.report()


# ---------------------------------------------------------------------------------------------------------------- the other curves: a slice
# each format once, each base mode at least once, widths other than the default, dense and sparse (sparse on wide tables: the rejection)
SLICE = [("canonical", "endomorphism", 14), ("mont256", "tables", 0), ("u8", "wide", 0), ("u16", "plain", 0), ("u32", "plain", 14),
         ("u64", "endomorphism", 16)]


def subgroup_points_bls12_381(seed, n):
    """n BLS12-381 G1 points of order r (multiples of the generator): the endomorphism mode is exact for such points only"""
    from oracle import bls12_381_ref as ref

    orc = oracle_module("bls12_381")
    jac = orc.g1_scalar_mul(ref.points_to_bytes([ref.G]) * n, orc.sample_scalars(seed, n))
    return b"".join(orc.to_affine64(jac[144 * i:144 * (i + 1)]) for i in range(n))


@pytest.mark.parametrize("curve", OTHER_CURVES)
def test_other_curves_slice(gpu, curve):
    n_bases = 600 if curve.endswith("_g2") else 1024
    c = m.MsmContext(0, curve=curve)
    try:
        # (the G2 samplers draw multiples of the generator: order r, as the endomorphism mode needs)
        points = subgroup_points_bls12_381(9102, n_bases) if curve == "bls12_381" else c.sample_points(n_bases, 9102).cpu().numpy().tobytes()
        M = Matrix(c, curve, points)
        for mode in MODES:
            c.set_bases(points, **base_flags(mode))
            for fmt, cell_mode, fixed in SLICE:
                if cell_mode != mode:
                    continue
                set_format(c, fmt)
                c.set_window_bits(fixed)
                try:
                    for n in (1, n_bases):
                        M.dense(fmt, mode, fixed, n)
                    for nnz in (1, n_bases // 2 + 1, 2 * n_bases + 1):
                        M.sparse(fmt, mode, fixed, nnz, n_bases)
                finally:
                    c.set_window_bits(0)
                    set_format(c, "canonical")
        assert M.reached == {(f, mo, w, s) for f, mo, w in SLICE for s in ("dense", "sparse")}
        M.report()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- one long-lived context
N_SEQ = 40000  # > FINE_BIG (32768): an all-equal 32-byte vector of this length fills one huge coarse bin and arms the skew credit
SEQ_BASES = [1000, 5000, 16384, N_SEQ]


def test_long_lived_context_sequence(gpu):
    """A seeded walk of 72 steps through the matrix on ONE context: base sets that grow and shrink (sparse indices just below the new n_bases),
    window and format changes between steps.  After every step: the oracle's answer, the rules' window width, and the skew credit -- a narrow
    launch leaves it alone, a 32-byte launch lowers it by one per launch unless that launch re-arms it to 64 (include/msm_hip.h)."""
    c = m.MsmContext(0)
    try:
        points = c.sample_points(N_SEQ, 9103).cpu().numpy().tobytes()
        M = Matrix(c, "bn254", points)
        rnd = random.Random(20261016)
        ops = ["dense_host", "dense_device", "dense_slot", "batch", "sparse_host", "sparse_device", "sparse_slot", "equal", "sparse_top"] * 8
        rnd.shuffle(ops)
        mode, n_bases, fmt, fixed = "plain", 0, "canonical", 0
        armed, narrow_steps = 0, 0  # (steps whose credit rule was checked: some must arm it, some must be narrow)
        for step, op in enumerate(ops):
            if step == 0 or rnd.random() < 0.3:
                mode = rnd.choice(MODES)
                n_bases = rnd.choice([b for b in SEQ_BASES if b != n_bases])
                c.set_bases(points[:n_bases * c.pb], **base_flags(mode))
            if rnd.random() < 0.3:
                fixed = rnd.choice(WINDOWS)
                c.set_window_bits(fixed)
            if rnd.random() < 0.5:
                fmt = rnd.choice(FORMATS + ["canonical", "mont256"])  # (32-byte formats weighted up: the credit rules need both kinds of step)
                set_format(c, fmt)
            before = c.skew_credit()
            launches, arms = 1, False
            where = "step %d (%s, %s bases x %d, %s, window %d)" % (step, op, mode, n_bases, fmt, fixed)
            n_fail = len(M.failures)
            if op.startswith("dense") or op == "batch":
                n = rnd.choice([x for x in (1, 4096, 4097, n_bases) if x <= n_bases])
                cb = plant_bits(fmt, mode, fixed, n)
                ints = M.values(fmt, cb, n)
                want = M.want(("dense", NB[fmt], cb, n, "edges"), ints)
                host = M.encode(fmt, ints)
                bits = run_bits(fmt, mode, fixed, n)
                if op == "dense_host":
                    M.check(where, lambda: c.msm(host), want, bits)
                elif op == "dense_device":
                    M.check(where, lambda: c.msm(M.device(fmt, host)), want, bits)
                elif op == "dense_slot":
                    slot = M.next_slot()
                    M.check(where, lambda: (c.launch(M.device(fmt, host), slot=slot), c.finish(slot))[1], want, bits)
                else:
                    groups = batch_groups(fmt, mode, fixed, n, 3, c.virtual_windows() or 1)
                    launches = len(groups)
                    blob = host * 3
                    M.check(where, lambda: c.msm_batch(M.device(fmt, blob) if step % 2 else blob, n), [want] * 3, run_bits(fmt, mode, fixed, n, groups[-1]))
            elif op == "equal":  # N_SEQ equal values: dense when the bases allow, else sparse over them
                cb = plant_bits(fmt, mode, fixed, N_SEQ)
                ints = M.values(fmt, cb, N_SEQ, "equal")
                host = M.encode(fmt, ints)
                bits = run_bits(fmt, mode, fixed, N_SEQ)
                if n_bases >= N_SEQ:
                    M.check(where, lambda: c.msm(M.device(fmt, host)), M.want(("dense", NB[fmt], cb, N_SEQ, "equal"), ints), bits)
                    arms = not NB[fmt]
                else:
                    idx = np.random.default_rng(step).integers(0, n_bases, size=N_SEQ, dtype=np.int64)
                    if mode == "wide":
                        M.rejected(where, lambda: c.msm_sparse(idx, host), m.MsmHipError, ERR_INVALID_ARG)
                        launches = 0
                    else:
                        M.check(where, lambda: c.msm_sparse(idx, host), M.want(("equal", NB[fmt], cb, n_bases, step), ints, idx), bits)
                        arms = not NB[fmt]
            else:
                nnz = rnd.choice([1, 4096, 4097, 2 * n_bases + 1])
                idx, ints, want = M.sparse_inputs(fmt, mode, fixed, nnz, n_bases, "seq")
                if op == "sparse_top":  # indices just below n_bases: what a stale base set would get wrong
                    idx = n_bases - 1 - np.random.default_rng(step).integers(0, min(64, n_bases), size=nnz, dtype=np.int64)
                    want = M.want(("top", NB[fmt], nnz, n_bases, step), ints, idx)
                host = M.encode(fmt, ints)
                bits = run_bits(fmt, mode, fixed, nnz)
                di = torch.from_numpy(idx).cuda()
                if mode == "wide":
                    M.rejected(where, lambda: c.msm_sparse(di, M.device(fmt, host)), m.MsmHipError, ERR_INVALID_ARG)
                    launches = 0
                elif op == "sparse_host":
                    M.check(where, lambda: c.msm_sparse(idx, host), want, bits)
                elif op == "sparse_slot":
                    slot = M.next_slot()
                    M.check(where, lambda: (c.launch_sparse(di, M.device(fmt, host), slot=slot), c.finish(slot))[1], want, bits)
                else:
                    M.check(where, lambda: c.msm_sparse(di, M.device(fmt, host)), want, bits)
            after = c.skew_credit()
            if len(M.failures) > n_fail:
                continue  # (a call that failed says nothing about the credit)
            armed += arms
            narrow_steps += NB[fmt] > 0
            if NB[fmt] or not launches:
                if after != before:
                    M.failures.append("%s: skew credit %d -> %d, a narrow or rejected launch must leave it alone" % (where, before, after))
            elif arms:
                if after != 64:
                    M.failures.append("%s: skew credit %d -> %d, an all-equal 32-byte launch of %d entries arms it to 64" % (where, before, after, N_SEQ))
            elif after not in (max(before - launches, 0), 64):
                M.failures.append("%s: skew credit %d -> %d after %d 32-byte launches" % (where, before, after, launches))
        assert len(ops) >= 60 and armed >= 2 and narrow_steps >= 10, (armed, narrow_steps)
        M.report()
    finally:
        c.close()
