"""Sparse MSMs over the resident bases (include/msm_hip.h: msm_hip_run_sparse ...): sum_j s_j * P[idx_j].  Every result is checked against
the CPU oracle over the gathered pairs (P[idx_j], s_j) -- repeats need no special treatment there -- or, at 2^20 points, against the same
context's dense MSM of the scattered scalars, which the other suites pin against the oracle."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import cpu

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG = -2
CURVES = ["bn254", "grumpkin", "pallas", "vesta", "bls12_381", "bn254_g2", "bls12_381_g2"]
SMALL = ("bls12_381", "bn254_g2", "bls12_381_g2")  # slower oracles: small shapes
BN254_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BLS12_381_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def oracle_module(curve):
    return cpu if curve == "bn254" else importlib.import_module("oracle.cpu_" + curve)


def gather(points, pb, idx):
    return np.frombuffer(points, dtype=np.uint8).reshape(-1, pb)[np.asarray(idx, dtype=np.int64)].tobytes()


def widen(v):
    """narrow values -> n x 32 B, zero-extended"""
    out = np.zeros((v.size, 32), dtype=np.uint8)
    out[:, :v.dtype.itemsize] = np.ascontiguousarray(v).view(np.uint8).reshape(v.size, -1)
    return out.tobytes()


def want(orc, points, pb, idx, scalars32):
    if len(idx) == 0:
        return bytes(2 * (pb // 2))
    return orc.to_affine64(orc.cpu_msm(gather(points, pb, idx), scalars32, n_threads=16))


def dev_u8(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def dev_idx(idx, dtype=torch.int64):
    return torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dtype).cuda()


def sampled_points(c, n, seed):
    """n points of the context's curve, drawn on the device (the host sampler takes seconds at 2^16) -> host wire bytes"""
    return c.sample_points(n, seed).cpu().numpy().tobytes()


def subgroup_points_bls12_381(seed, n):
    """n BLS12-381 G1 points of order r (multiples of the generator): the curve's cofactor is not 1, and the endomorphism mode and r - s = -s
    hold for such points only -- what every valid input is"""
    from oracle import bls12_381_ref as ref

    orc = oracle_module("bls12_381")
    jac = orc.g1_scalar_mul(ref.points_to_bytes([ref.G]) * n, orc.sample_scalars(seed, n))
    return b"".join(orc.to_affine64(jac[144 * i:144 * (i + 1)]) for i in range(n))


def points_for(curve, c, n, seed):
    if curve == "bls12_381":
        return subgroup_points_bls12_381(seed, n)
    return sampled_points(c, n, seed) if n > 4096 else oracle_module(curve).sample_points(seed, n)


def random_indices(rng, n_bases, nnz):
    """random indices with repeats, and the last base among them"""
    idx = rng.integers(0, n_bases, size=nnz, dtype=np.int64)
    if nnz:
        idx[nnz // 2] = n_bases - 1
    return idx


# ---------------------------------------------------------------------------------------------------------------- shapes on every curve
@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endomorphism"])
@pytest.mark.parametrize("curve", CURVES)
def test_shapes_against_the_oracle(gpu, curve, endo):
    orc = oracle_module(curve)
    small = curve in SMALL
    sizes = [1, 1000] if small else [1, 1000, (1 << 16) + 3]
    counts = [0, 1, 2, 255] + ([] if small else [4097])
    rng = np.random.default_rng(601 + CURVES.index(curve) + (100 if endo else 0))
    c = m.MsmContext(0, curve=curve)
    try:
        points = points_for(curve, c, sizes[-1], 600 + CURVES.index(curve))
        for n_bases in sizes:
            c.set_bases(points[:n_bases * c.pb], endomorphism=endo)
            for k, nnz in enumerate(counts):
                idx = random_indices(rng, n_bases, nnz)
                s = orc.sample_scalars(7000 + nnz + n_bases, nnz)
                if k % 2:  # host and device inputs alternate
                    got = c.msm_sparse(idx, s)
                else:
                    got = c.msm_sparse(dev_idx(idx, torch.int32 if k % 4 else torch.int64), dev_u8(s))
                assert got.to_affine_bytes() == want(orc, points, c.pb, idx, s), (n_bases, nnz)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- tables and formats
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_fixed_base_tables(gpu, curve):
    orc = oracle_module(curve)
    n_bases = 1000
    points = orc.sample_points(610, n_bases)
    rng = np.random.default_rng(611)
    c = m.MsmContext(0, curve=curve)
    try:
        c.set_bases(points, precompute=True)
        for nnz in (1, 255, 4097):
            idx = random_indices(rng, n_bases, nnz)
            s = orc.sample_scalars(612 + nnz, nnz)
            assert c.msm_sparse(dev_idx(idx), dev_u8(s)).to_affine_bytes() == want(orc, points, c.pb, idx, s), nnz
    finally:
        c.close()


def test_mont256_scalars(gpu):
    n_bases, nnz = 1000, 777
    points = cpu.sample_points(620, n_bases)
    rng = np.random.default_rng(621)
    idx = random_indices(rng, n_bases, nnz)
    s = cpu.sample_scalars(622, nnz)
    mont = b"".join((int.from_bytes(s[32 * j:32 * j + 32], "little") * (1 << 256) % BN254_R).to_bytes(32, "little") for j in range(nnz))
    c = m.MsmContext(0)
    try:
        c.set_bases(points, endomorphism=None)
        c.set_scalar_format(mont256=True)
        assert c.msm_sparse(dev_idx(idx), dev_u8(mont)).to_affine_bytes() == want(cpu, points, c.pb, idx, s)
        assert c.msm_sparse(idx, mont).to_affine_bytes() == want(cpu, points, c.pb, idx, s)
    finally:
        c.close()


NP_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
TORCH_DTYPES = {1: torch.uint8, 2: torch.uint16, 4: torch.uint32, 8: torch.uint64}


@pytest.mark.parametrize("width", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_narrow_formats(gpu, curve, width):
    orc = oracle_module(curve)
    n_bases, nnz = 1000, 3000
    points = orc.sample_points(630, n_bases)
    rng = np.random.default_rng(631 + width)
    idx = random_indices(rng, n_bases, nnz)
    v = rng.integers(0, 1 << (8 * width), size=nnz, dtype=np.uint64).astype(NP_DTYPES[width])
    v[:3] = [0, 1, (1 << (8 * width)) - 1]
    c = m.MsmContext(0, curve=curve)
    try:
        c.set_bases(points, endomorphism=None)  # (the default mode: narrow entries read the plain records idx_j)
        c.set_scalar_format(width=width)
        t = torch.from_numpy(v.view(np.uint8).copy()).cuda().view(TORCH_DTYPES[width])
        w = want(orc, points, c.pb, idx, widen(v))
        assert c.msm_sparse(dev_idx(idx), t).to_affine_bytes() == w
        assert c.msm_sparse(idx, v).to_affine_bytes() == w
    finally:
        c.close()


def test_one_hot_rows_as_u8_ones(gpu):
    """A Lasso-style one-hot matrix of 4096 rows x 16 columns, committed as U8 ones at index row * 16 + column"""
    rows, cols = 4096, 16
    col = np.random.default_rng(641).integers(0, cols, size=rows)
    idx = np.arange(rows) * cols + col
    c = m.MsmContext(0)
    try:
        points = sampled_points(c, rows * cols, 640)
        c.set_bases(points, endomorphism=None)
        c.set_scalar_format(width=1)
        got = c.msm_sparse(dev_idx(idx, torch.int32), torch.ones(rows, dtype=torch.uint8, device="cuda"))
        assert got.to_affine_bytes() == want(cpu, points, c.pb, idx, widen(np.ones(rows, dtype=np.uint8)))
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- what stresses the new paths
@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endomorphism"])
def test_every_index_equal(gpu, endo):
    """One base nnz times: with one scalar as well every bucket that fills holds nnz copies of one point (the doubling inside accumulation)"""
    n_bases, nnz = 1000, 4097
    points = cpu.sample_points(650, n_bases)
    idx = np.full(nnz, 617)
    c = m.MsmContext(0)
    try:
        c.set_bases(points, endomorphism=endo)
        for s in (cpu.sample_scalars(651, 1) * nnz, cpu.sample_scalars(652, nnz)):
            assert c.msm_sparse(dev_idx(idx), dev_u8(s)).to_affine_bytes() == want(cpu, points, c.pb, idx, s)
    finally:
        c.close()


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endomorphism"])
@pytest.mark.parametrize("curve,r", [("bn254", BN254_R), ("bls12_381", BLS12_381_R)])
def test_opposite_pairs_cancel(gpu, curve, r, endo):
    n_bases = 1000
    rng = np.random.default_rng(661)
    idx = rng.integers(0, n_bases, size=100)
    s = [int(x) % r for x in rng.integers(1, 1 << 62, size=100)]
    s = [x * 0x1F2E3D4C5B6A7988 % r for x in s]
    pairs_idx = np.concatenate([idx, idx[::-1]])
    pairs_s = b"".join(x.to_bytes(32, "little") for x in s) + b"".join(((r - x) % r).to_bytes(32, "little") for x in s[::-1])
    c = m.MsmContext(0, curve=curve)
    try:
        c.set_bases(points_for(curve, c, n_bases, 660), endomorphism=endo)
        assert c.msm_sparse(dev_idx(pairs_idx), dev_u8(pairs_s)).is_identity()
        assert c.msm_sparse(pairs_idx, pairs_s).is_identity()
    finally:
        c.close()


@pytest.fixture(scope="module")
def big(gpu):
    """2^20 bases with their endomorphism images, generated on the device"""
    n = 1 << 20
    c = m.MsmContext(0)
    pts = c.sample_points(n, 670)
    c.set_bases(pts, endomorphism=True)
    host_points = pts.cpu().numpy().tobytes()
    yield c, n, host_points
    c.close()


def test_full_permutation_equals_the_dense_msm(big):
    c, n, points = big
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(671)).cuda()
    s = c.sample_scalars(n, 672)
    dense = torch.empty_like(s)
    dense[perm] = s  # entry j (scalar s_j at base perm_j) is dense position perm_j
    assert c.msm_sparse(perm, s).to_affine_bytes() == c.msm(dense).to_affine_bytes()
    k = 2048  # the oracle on a slice of the same entries
    head = perm[:k].cpu().numpy()
    assert c.msm_sparse(perm[:k], s[:k]).to_affine_bytes() == want(cpu, points, c.pb, head, s[:k].cpu().numpy().tobytes())


def test_2_14_entries_over_2_20_bases(big):
    c, n, points = big
    idx = random_indices(np.random.default_rng(673), n, 1 << 14)
    s = cpu.sample_scalars(674, 1 << 14)
    assert c.msm_sparse(dev_idx(idx), dev_u8(s)).to_affine_bytes() == want(cpu, points, c.pb, idx, s)


# ---------------------------------------------------------------------------------------------------------------- asynchrony
@pytest.fixture(scope="module")
def mid(gpu):
    n_bases = 4000
    points = cpu.sample_points(680, n_bases)
    c = m.MsmContext(0)
    c.set_bases(points, endomorphism=None)
    yield c, n_bases, points
    c.close()


def test_slots_finished_out_of_order(mid):
    c, n_bases, points = mid
    rng = np.random.default_rng(681)
    i0, i2 = random_indices(rng, n_bases, 3000), random_indices(rng, n_bases, 9000)
    s0, s1, s2 = cpu.sample_scalars(682, 3000), cpu.sample_scalars(683, n_bases), cpu.sample_scalars(684, 9000)
    c.launch_sparse(dev_idx(i0), dev_u8(s0), slot=0)
    c.launch(dev_u8(s1), slot=1)
    c.launch_sparse(dev_idx(i2), dev_u8(s2), slot=2)
    assert c.finish(2).to_affine_bytes() == want(cpu, points, c.pb, i2, s2)
    assert c.finish(0).to_affine_bytes() == want(cpu, points, c.pb, i0, s0)
    assert c.finish(1).to_affine_bytes() == cpu.to_affine64(cpu.cpu_msm(points, s1, n_threads=16))


def test_scalar_format_changed_before_finish(mid):
    c, n_bases, points = mid
    rng = np.random.default_rng(685)
    idx = random_indices(rng, n_bases, 5000)
    v = rng.integers(0, 256, size=5000).astype(np.uint8)
    c.set_scalar_format(width=1)
    try:
        c.launch_sparse(dev_idx(idx), torch.from_numpy(v).cuda(), slot=1)
    finally:
        c.set_scalar_format(width=32)
    s = cpu.sample_scalars(686, 5000)
    c.launch_sparse(dev_idx(idx), dev_u8(s), slot=0)
    c.set_scalar_format(width=2)
    try:
        assert c.finish(1).to_affine_bytes() == want(cpu, points, c.pb, idx, widen(v))
        assert c.finish(0).to_affine_bytes() == want(cpu, points, c.pb, idx, s)
    finally:
        c.set_scalar_format(width=32)


# ---------------------------------------------------------------------------------------------------------------- errors
def test_host_index_out_of_range_enqueues_nothing(mid):
    c, n_bases, points = mid
    idx = np.array([5, n_bases, 7], dtype=np.uint32)
    s = cpu.sample_scalars(690, 3)
    out = C.create_string_buffer(c.jb)
    assert m.lib().msm_hip_run_sparse(c._h, idx.ctypes.data, s, 3, out) == ERR_INVALID_ARG
    with pytest.raises(ValueError):
        c.msm_sparse(idx.astype(np.int64), s)
    with pytest.raises(ValueError):
        c.msm_sparse(np.array([5, -1, 7]), s)
    idx[1] = n_bases - 1
    assert c.msm_sparse(idx, s).to_affine_bytes() == want(cpu, points, c.pb, idx, s)


@pytest.mark.parametrize("mode", ["plain", "endomorphism", "precompute", "u8", "u32"])
def test_device_index_out_of_range(gpu, mode):
    """The guard in the count and scatter passes.  The context first holds 4096 bases, then 1000: the base buffer keeps its capacity (grow never
    shrinks it), so indices in [1000, 4096) would read allocated records if a guard were missing -- a wrong answer, not a fault."""
    points = cpu.sample_points(700, 4096)
    flags = dict(endomorphism=mode == "endomorphism", precompute=mode == "precompute")
    width = {"u8": 1, "u32": 4}.get(mode, 32)
    rng = np.random.default_rng(701)
    c = m.MsmContext(0)
    try:
        c.set_bases(points, **flags)
        c.set_bases(points[:1000 * c.pb], **flags)
        c.set_scalar_format(width=width)
        idx = random_indices(rng, 1000, 2000)
        idx[::7] = rng.integers(1000, 4096, size=idx[::7].size)
        v = rng.integers(1, 200, size=2000).astype(np.uint8 if width == 1 else np.uint32)
        s = cpu.sample_scalars(702, 2000) if width == 32 else torch.from_numpy(v.view(np.uint8).copy()).cuda().view(TORCH_DTYPES[width])
        with pytest.raises(m.MsmHipError) as e:
            c.msm_sparse(dev_idx(idx), dev_u8(s) if width == 32 else s)
        assert e.value.code == ERR_INVALID_ARG
        c.launch_sparse(dev_idx(idx), dev_u8(s) if width == 32 else s, slot=3)
        with pytest.raises(m.MsmHipError) as e:
            c.finish(3)
        assert e.value.code == ERR_INVALID_ARG
        good = idx % 1000
        w = want(cpu, points, c.pb, good, s if width == 32 else widen(v))
        assert c.msm_sparse(dev_idx(good), dev_u8(s) if width == 32 else s).to_affine_bytes() == w  # the context stays usable
        c.launch_sparse(dev_idx(good), dev_u8(s) if width == 32 else s, slot=3)
        assert c.finish(3).to_affine_bytes() == w  # ... and so does the slot
    finally:
        c.close()


def test_wide_tables_are_out_of_scope(gpu):
    points = cpu.sample_points(710, 1000)
    c = m.MsmContext(0)
    try:
        c.set_bases(points, precompute="wide")
        s = cpu.sample_scalars(711, 2)
        out = C.create_string_buffer(c.jb)
        idx = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
        assert m.lib().msm_hip_run_sparse_device(c._h, idx.data_ptr(), dev_u8(s).data_ptr(), 2, out) == ERR_INVALID_ARG
        assert m.lib().msm_hip_run_sparse(c._h, np.array([1, 2], dtype=np.uint32).ctypes.data, s, 2, out) == ERR_INVALID_ARG
        assert m.lib().msm_hip_launch_sparse_device(c._h, idx.data_ptr(), dev_u8(s).data_ptr(), 2, 0) == ERR_INVALID_ARG
        assert c.msm(cpu.sample_scalars(712, 1000)).to_affine_bytes() == cpu.to_affine64(cpu.cpu_msm(points, cpu.sample_scalars(712, 1000), n_threads=16))
    finally:
        c.close()


def test_skew_credit_follows_the_scalar_format(gpu):
    """a sparse launch follows the dense rule of its format -- 32-byte entries that fill a huge coarse bin arm the adaptive
    k_fine_hist credit and 32-byte launches use it, narrow ones neither arm nor use it"""
    n_bases, nnz = (1 << 16) + 3, 1 << 16  # > FINE_BIG equal entries in one coarse bin
    rng = np.random.default_rng(721)
    idx = dev_idx(random_indices(rng, n_bases, nnz))
    c = m.MsmContext(0)
    try:
        points = sampled_points(c, n_bases, 720)
        c.set_bases(points, endomorphism=False)
        c.set_scalar_format(width=1)
        for _ in range(2):
            c.msm_sparse(idx, torch.ones(nnz, dtype=torch.uint8, device="cuda"))
        c.set_scalar_format(width=32)
        assert c.skew_credit() == 0
        ones = torch.zeros((nnz, 32), dtype=torch.uint8, device="cuda")
        ones[:, 0] = 1
        c.msm_sparse(idx, ones)
        armed = c.skew_credit()
        assert armed > 0
        s = cpu.sample_scalars(722, 3000)
        i2 = random_indices(rng, n_bases, 3000)
        assert c.msm_sparse(dev_idx(i2), dev_u8(s)).to_affine_bytes() == want(cpu, points, c.pb, i2, s)
        assert c.skew_credit() == armed - 1
        c.set_scalar_format(width=1)
        c.msm_sparse(idx, torch.ones(nnz, dtype=torch.uint8, device="cuda"))
        c.set_scalar_format(width=32)
        assert c.skew_credit() == armed - 1
    finally:
        c.close()
