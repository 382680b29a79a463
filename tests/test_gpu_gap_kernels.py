"""The kernels between two SMVPs: the first sort pass that also places every tile inside its coarse bins (no scan launch of its own), the
cue that turns the sub-range histograms of huge coarse bins on (skew, not the endomorphism's top window), and the stitch over buckets of
1, 2, 3, 5 ... pieces up to the queued and the shared ones.  Every result is compared bit-exactly with the CPU oracle of its curve."""
import importlib
import random

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import bn254_ref as ref
from oracle import cpu

pytestmark = pytest.mark.gpu
N_MAX = (1 << 14) + 3
MODES = [False, True]
MODE_IDS = ["plain", "endomorphism"]


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def dev(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def small(gpu):
    """one context, N_MAX points and scalars, and the oracle's answer for every prefix length a test asks for (computed once)"""
    points, scalars = cpu.sample_points(601, N_MAX), cpu.sample_scalars(602, N_MAX)
    want = {}

    def oracle(n):
        if n not in want:
            want[n] = cpu.to_affine64(cpu.cpu_msm(points[:64 * n], scalars[:32 * n], 16))
        return want[n]

    c = m.MsmContext(0)
    yield c, points, scalars, oracle
    c.close()


# ---------------------------------------------------------------------------------------------------------------- the tile prefix inside k_count
# one tile, a tile boundary, several tiles: 1, 2 and many workgroups add to a bin's fill word
@pytest.mark.parametrize("endo", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 3 * 2048 + 5, (1 << 14) + 3])
def test_tile_prefix_sizes_and_slot_reuse(small, n, endo):
    c, points, scalars, oracle = small
    c.set_bases(points[:64 * n], endomorphism=endo)
    s = dev(scalars[:32 * n])
    # twice into the same slot, then two slots alternating: a fill word that is not back at zero corrupts the launch after it
    for slot in (0, 0, 1, 0, 1):
        c.launch(s, slot)
        assert c.finish(slot).to_affine_bytes() == oracle(n), slot
    c.launch(s, 0)
    c.launch(s, 1)
    assert c.finish(0).to_affine_bytes() == oracle(n) and c.finish(1).to_affine_bytes() == oracle(n)


@pytest.mark.parametrize("endo", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,n", [(12, 1 << 12), (14, 1 << 14), (16, 1 << 14)])
def test_tile_prefix_window_sizes(small, bits, n, endo):
    # 8 and 32 coarse bins per window instead of 128: the fill words of the bins a window does not have stay zero
    c, points, scalars, oracle = small
    c.set_bases(points[:64 * n], endomorphism=endo)
    c.set_window_bits(bits)
    try:
        for _ in range(2):
            assert c.msm(scalars[:32 * n]).to_affine_bytes() == oracle(n)
            assert c.last_window_bits() == bits
    finally:
        c.set_window_bits(0)
    assert c.msm(scalars[:32 * n]).to_affine_bytes() == oracle(n)  # (12 bits at 2^12 by itself)


@pytest.mark.parametrize("endo", MODES, ids=MODE_IDS)
def test_tile_prefix_grouped_launch(small, endo):
    # several whole 2^14-point MSMs per launch: grid (tiles, vectors), every vector fills its own windows' words
    c, points, scalars, oracle = small
    n, nv = 1 << 14, 5
    vecs = [cpu.sample_scalars(610 + k, n) for k in range(nv - 1)] + [scalars[:32 * n]]
    want = [cpu.to_affine64(cpu.cpu_msm(points[:64 * n], v, 16)) for v in vecs[:-1]] + [oracle(n)]
    c.set_bases(points[:64 * n], endomorphism=endo)
    batch = dev(b"".join(vecs))
    for _ in range(2):
        assert [g.to_affine_bytes() for g in c.msm_batch(batch, n)] == want


# ---------------------------------------------------------------------------------------------------------------- when the sub-range histograms run
def fine_hist(c):
    return bool(c.env_report()["last_fine_hist"])


def test_skew_arms_the_histograms_and_uniform_does_not(gpu):
    n = 1 << 16
    c = m.MsmContext(0)
    try:
        pts = c.sample_points(n, 620)
        pb = pts.cpu().numpy().tobytes()
        c.set_bases(pts, endomorphism=True)
        uni = c.sample_scalars(n, 621)
        want_uni = cpu.to_affine64(cpu.cpu_msm(pb, uni.cpu().numpy().tobytes(), 16))
        for _ in range(3):  # a fresh context, uniform scalars: never
            assert c.msm(uni).to_affine_bytes() == want_uni
            assert not fine_hist(c) and c.skew_credit() == 0
        # every scalar equal: one coarse bin per window holds a half's 2^16 entries.  The launch itself runs without the histograms (every sharer
        # of the bin sweeps it) and must be right; its report arms them for the launches that follow
        s = 0x1234_5678_9ABC_DEF0_1357_9BDF_2468_ACE0_FEDC_BA98_7654_3210 % ref.R
        total = c.msm((1).to_bytes(32, "little") * n)
        c2 = m.MsmContext(0)  # (the vector of ones has armed c already: the all-equal launch goes to a context that has seen nothing)
        try:
            c2.set_bases(pts, endomorphism=True)
            got = c2.msm(s.to_bytes(32, "little") * n)
            assert not fine_hist(c2)
            assert got.to_affine() == ref.mul(s, total.to_affine())
            assert c2.skew_credit() == 64
            assert c2.msm(uni).to_affine_bytes() == want_uni
            assert fine_hist(c2) and c2.skew_credit() == 63
            assert c2.msm(s.to_bytes(32, "little") * n) == got and fine_hist(c2)  # with the histograms: the same sum
            assert c2.skew_credit() == 64
        finally:
            c2.close()
    finally:
        c.close()


@pytest.mark.parametrize("endo", MODES, ids=MODE_IDS)
def test_witness_like_vector_arms_the_histograms(gpu, endo):
    # 40 % zeros, 30 % ones at 2^17: slot 1 of the lowest window holds 39 Ki entries, 38 mean bins
    n = 1 << 17
    rnd = random.Random(13)
    c = m.MsmContext(0)
    try:
        pts = c.sample_points(n, 630)
        base = ref.bytes_to_scalars(c.sample_scalars(n, 631).cpu().numpy().tobytes())
        sb = ref.scalars_to_bytes([0 if (u := rnd.random()) < 0.4 else 1 if u < 0.7 else base[i] for i in range(n)])
        c.set_bases(pts, endomorphism=endo)
        want = cpu.to_affine64(cpu.cpu_msm(pts.cpu().numpy().tobytes(), sb, 16))
        assert c.msm(sb).to_affine_bytes() == want and not fine_hist(c)
        assert c.skew_credit() == 64
        assert c.msm(sb).to_affine_bytes() == want and fine_hist(c)
    finally:
        c.close()


def test_uniform_endomorphism_launches_at_2p20_run_no_histograms(gpu):
    # the headline shape: the top window's coarse bins reach twice the mean, which is the 32 Ki threshold here.  They are shared by eight
    # workgroups each (right with or without histograms), and they are not skew: no launch of the series runs k_fine_hist
    n = 1 << 20
    c = m.MsmContext(0)
    try:
        pts = c.sample_points(n, 640)
        c.set_bases(pts, endomorphism=True)
        sc = c.sample_scalars(n, 641)
        want = cpu.to_affine64(cpu.cpu_msm(pts.cpu().numpy().tobytes(), sc.cpu().numpy().tobytes(), 16))
        for _ in range(3):
            assert c.msm(sc).to_affine_bytes() == want
            assert not fine_hist(c) and c.skew_credit() == 0
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- the stitch
def runs_vector(orc, n, seed, lengths):
    """uniform scalars among which, for every r of `lengths`, two values are repeated r times: with the SMVP's shortest chunk (8 entries) their
    buckets are stitched from about r / 8 + 1 pieces"""
    rnd = random.Random(seed)
    sb = orc.sample_scalars(seed, n)
    sc = [int.from_bytes(sb[32 * i:32 * i + 32], "little") for i in range(n)]
    pos = list(range(n))
    rnd.shuffle(pos)
    k = 0
    for r in lengths:
        for _ in range(2):
            v = sc[pos[k]]
            for i in pos[k:k + r]:
                sc[i] = v
            k += r
    assert k <= n
    return b"".join(v.to_bytes(32, "little") for v in sc)


PIECES = [9, 12, 17, 20, 25, 33, 41, 64, 300, 1100]  # 2, 3, 4, 5 ... pieces; 300 and 1100 entries: past the 32 pieces of the big queue


@pytest.mark.parametrize("endo", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("curve", ["bn254", "grumpkin"])
@pytest.mark.parametrize("kind", ["uniform", "runs", "10_values", "all_equal"])
def test_stitch_piece_counts(gpu, curve, kind, endo):
    orc = cpu if curve == "bn254" else importlib.import_module("oracle.cpu_" + curve)
    n = 1 << 15 if kind == "10_values" else 1 << 14
    c = m.MsmContext(0, curve=curve)
    try:
        pts = c.sample_points(n, 650).cpu().numpy().tobytes()
        if kind == "uniform":  # 16-bit windows at 2^14: hardly a run reaches into a second chunk
            sb = orc.sample_scalars(651, n)
        elif kind == "runs":
            sb = runs_vector(orc, n, 652, PIECES)
        elif kind == "10_values":  # runs of thousands of entries: the queue of big buckets
            vals = [orc.sample_scalars(653, 10)[32 * i:32 * i + 32] for i in range(10)]
            rnd = random.Random(654)
            sb = b"".join(vals[rnd.randrange(10)] for _ in range(n))
        else:  # one bucket per window with every entry: the shared huge bucket
            sb = orc.sample_scalars(655, 1) * n
        c.set_bases(pts, endomorphism=endo)
        c.set_window_bits(16)
        want = orc.to_affine64(orc.cpu_msm(pts, sb, 16))
        assert c.msm(sb).to_affine_bytes() == want
        assert c.msm(sb).to_affine_bytes() == want  # the slot's queue and counters are back at zero
    finally:
        c.close()


@pytest.mark.parametrize("curve", ["bls12_381", "bn254_g2"])
def test_stitch_of_the_wide_units(gpu, curve):
    # 14 limbs and Fq2: the same kernel source in the units of the wide fields, against their own oracles
    orc = importlib.import_module("oracle.cpu_" + curve)
    n = 1200
    c = m.MsmContext(0, curve=curve)
    try:
        pts = c.sample_points(n, 660).cpu().numpy().tobytes()
        sb = runs_vector(orc, n, 661, [9, 17, 25, 41, 300])
        c.set_bases(pts)
        c.set_window_bits(16)
        assert c.msm(sb).to_affine_bytes() == orc.to_affine64(orc.cpu_msm(pts, sb, 16))
    finally:
        c.close()
