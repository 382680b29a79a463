"""Base sets that hold the point at infinity as an all-zero record (include/msm_hip.h: MSM_HIP_BASES_ZERO_IS_IDENTITY), as Groth16 proving keys do.
Every expected value comes from the CPU oracle over the pairs whose base is not the identity (the identities and their scalars dropped), or, at
2^20 points, from the same context's dense MSM over real points with those scalars set to zero, which the other suites pin against the oracle."""
import importlib

import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import bn254_ref, cpu

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_NOT_ON_CURVE = -2, -5
CURVES = ["bn254", "grumpkin", "pallas", "vesta", "bls12_381", "bn254_g2", "bls12_381_g2"]
SMALL = ("bls12_381", "bn254_g2", "bls12_381_g2")  # slower oracles: small shapes
MODES = {"plain": dict(endomorphism=False), "endomorphism": dict(endomorphism=True), "tables": dict(precompute=True),
         "wide": dict(precompute="wide")}
NP_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
BN254_P, BN254_R = bn254_ref.P, bn254_ref.R


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


def oracle_module(curve):
    return cpu if curve == "bn254" else importlib.import_module("oracle.cpu_" + curve)


def identity_positions(n, seed, frac=0.1):
    """the edges of bitmap words and waves (0, 1, 63, 64, 255, 256, n - 1) and about `frac` of the rest at random"""
    rng = np.random.default_rng(seed)
    fixed = [i for i in (0, 1, 63, 64, 255, 256, n - 1) if i < n]
    return np.unique(np.concatenate([np.asarray(fixed, dtype=np.int64), np.flatnonzero(rng.random(n) < frac)]))


def with_identities(points, pb, ids):
    a = np.frombuffer(points, dtype=np.uint8).reshape(-1, pb).copy()
    a[ids] = 0
    return a.tobytes()


def widen(v):
    """narrow values -> n x 32 B, zero-extended"""
    out = np.zeros((v.size, 32), dtype=np.uint8)
    out[:, :v.dtype.itemsize] = np.ascontiguousarray(v).view(np.uint8).reshape(v.size, -1)
    return out.tobytes()


def want(orc, points, pb, scalars32, idx, ids):
    """the oracle over the entries (scalars32[j], P[idx[j]]) whose base is not an identity"""
    idx = np.asarray(idx, dtype=np.int64)
    keep = ~np.isin(idx, ids)
    if not keep.any():
        return bytes(pb)
    pts = np.frombuffer(points, dtype=np.uint8).reshape(-1, pb)[idx[keep]].tobytes()
    sc = np.frombuffer(scalars32, dtype=np.uint8).reshape(-1, 32)[keep].tobytes()
    return orc.to_affine64(orc.cpu_msm(pts, sc, n_threads=16))


def dense_want(orc, points, pb, scalars32, ids):
    return want(orc, points, pb, scalars32, np.arange(len(scalars32) // 32), ids)


def subgroup_points_bls12_381(seed, n):
    """BLS12-381 G1 points of order r (multiples of the generator): what the endomorphism mode needs"""
    from oracle import bls12_381_ref as ref

    orc = oracle_module("bls12_381")
    jac = orc.g1_scalar_mul(ref.points_to_bytes([ref.G]) * n, orc.sample_scalars(seed, n))
    return b"".join(orc.to_affine64(jac[144 * i:144 * (i + 1)]) for i in range(n))


def points_for(curve, c, n, seed):
    return subgroup_points_bls12_381(seed, n) if curve == "bls12_381" else c.sample_points(n, seed).cpu().numpy().tobytes()


def dev_u8(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def mask_used(c):
    return c.env_report()["last_identity_mask"]


# ---------------------------------------------------------------------------------------------------------------- every curve x base mode
@pytest.mark.parametrize("curve", CURVES)
def test_every_curve_and_base_mode(gpu, curve):
    orc = oracle_module(curve)
    n = 600 if curve in SMALL else 4097
    c = m.MsmContext(0, curve=curve)
    try:
        points = points_for(curve, c, n, 900 + CURVES.index(curve))
        ids = identity_positions(n, 901)
        bases = with_identities(points, c.pb, ids)
        scalars = orc.sample_scalars(902 + CURVES.index(curve), n)
        w = dense_want(orc, points, c.pb, scalars, ids)
        for mode, flags in MODES.items():
            c.set_bases(bases, zero_is_identity=True, **flags)
            assert c.msm(scalars).to_affine_bytes() == w, mode
            assert mask_used(c) == 1
            assert c.msm(dev_u8(scalars)).to_affine_bytes() == w, mode
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- scalar formats, dense and sparse
def mont(b, mod, width=32):
    return b"".join((int.from_bytes(b[k:k + width], "little") * (1 << 256) % mod).to_bytes(32, "little") for k in range(0, len(b), width))


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endomorphism"])
def test_scalar_formats_dense_and_sparse(gpu, endo):
    n = 4097
    points = cpu.sample_points(910, n)
    ids = identity_positions(n, 911)
    rng = np.random.default_rng(912)
    s = bytearray(cpu.sample_scalars(913, n))
    s[32 * ids[0]:32 * ids[0] + 32] = b"\xff" * 32  # rejected anywhere else; ignored at an identity
    s = bytes(s)
    idx = rng.integers(0, n, size=3000)
    idx[:40] = np.repeat(ids[:20], 2)  # identities, repeated ...
    idx[40:45] = ids[20:25]            # ... and not
    idx[45] = ids[0]                   # (the 2^256 - 1 of entry 45 sits at an identity)
    sparse_s = bytearray(cpu.sample_scalars(914, idx.size))
    sparse_s[32 * 45:32 * 46] = b"\xff" * 32
    sparse_s = bytes(sparse_s)
    c = m.MsmContext(0)
    try:
        c.set_bases(with_identities(points, 64, ids), endomorphism=endo, zero_is_identity=True)
        cases = [("canonical", 32, s, sparse_s, s, sparse_s)]
        # MONT256: the value at the identity is >= r in that form too
        cases.append(("mont256", 32, mont(s, BN254_R)[:32 * ids[0]] + b"\xff" * 32 + mont(s, BN254_R)[32 * ids[0] + 32:],
                      mont(sparse_s, BN254_R)[:32 * 45] + b"\xff" * 32 + mont(sparse_s, BN254_R)[32 * 46:], s, sparse_s))
        for width in (1, 2, 4, 8):
            v = rng.integers(0, 1 << min(8 * width, 63), size=n, dtype=np.uint64).astype(NP_DTYPES[width])
            vs = rng.integers(0, 1 << min(8 * width, 63), size=idx.size, dtype=np.uint64).astype(NP_DTYPES[width])
            cases.append(("u%d" % (8 * width), width, v.tobytes(), vs.tobytes(), widen(v), widen(vs)))
        for fmt, width, dense_in, sparse_in, dense32, sparse32 in cases:
            c.set_scalar_format(mont256=fmt == "mont256", width=width)
            wd = dense_want(cpu, points, 64, dense32, ids)
            ws = want(cpu, points, 64, sparse32, idx, ids)
            assert c.msm(dense_in).to_affine_bytes() == wd, fmt
            assert c.msm(dev_u8(dense_in)).to_affine_bytes() == wd, fmt
            assert mask_used(c) == 1
            assert c.msm_sparse(idx, sparse_in).to_affine_bytes() == ws, fmt
            assert c.msm_sparse(torch.from_numpy(idx).cuda(), dev_u8(sparse_in)).to_affine_bytes() == ws, fmt
            bad = idx.copy()
            bad[7] = n  # one index beyond the bases: still the kernels' INVALID_ARG
            with pytest.raises(m.MsmHipError) as e:
                c.msm_sparse(torch.from_numpy(bad).cuda(), dev_u8(sparse_in))
            assert e.value.code == ERR_INVALID_ARG
        c.set_scalar_format()
        assert c.msm(s).to_affine_bytes() == dense_want(cpu, points, 64, s, ids)  # (the context is still usable)
    finally:
        c.close()


def test_mont256_bases(gpu):
    """coordinates x * 2^256 mod p: zero is zero in that form too"""
    n = 2000
    points = cpu.sample_points(915, n)
    ids = identity_positions(n, 916)
    s = cpu.sample_scalars(917, n)
    c = m.MsmContext(0)
    try:
        c.set_bases(with_identities(mont(points, BN254_P), 64, ids), mont256=True, check_on_curve=True, zero_is_identity=True)
        assert c.msm(s).to_affine_bytes() == dense_want(cpu, points, 64, s, ids)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- entry points
@pytest.fixture(scope="module")
def bn254_set(gpu):
    n = 4097
    points = cpu.sample_points(920, n)
    ids = identity_positions(n, 921)
    return n, points, ids, with_identities(points, 64, ids)


@pytest.mark.parametrize("mode", ["plain", "endomorphism"])
def test_whole_msm_entry_points(bn254_set, mode):
    n, points, ids, bases = bn254_set
    vecs = [cpu.sample_scalars(922 + k, n) for k in range(3)]
    wants = [dense_want(cpu, points, 64, v, ids) for v in vecs]
    c = m.MsmContext(0)
    try:
        c.set_bases(dev_u8(bases), zero_is_identity=True, **MODES[mode])  # (from a CUDA tensor)
        assert c.msm(vecs[0]).to_affine_bytes() == wants[0]
        assert c.msm(dev_u8(vecs[1])).to_affine_bytes() == wants[1]
        t = dev_u8(vecs[2])
        c.launch(t, slot=2)
        assert c.finish(2).to_affine_bytes() == wants[2]
        c.launch_host(vecs[0], slot=1)
        assert c.finish(1).to_affine_bytes() == wants[0]
        assert [g.to_affine_bytes() for g in c.msm_batch(b"".join(vecs), n)] == wants
        assert [g.to_affine_bytes() for g in c.msm_batch(dev_u8(b"".join(vecs)), n)] == wants
    finally:
        c.close()


def test_window_ranges_combine_to_the_whole_msm(bn254_set):
    n, points, ids, bases = bn254_set
    s = cpu.sample_scalars(930, n)
    w = dense_want(cpu, points, 64, s, ids)
    t = dev_u8(s)
    two = dev_u8(s + cpu.sample_scalars(931, n))
    w2 = dense_want(cpu, points, 64, cpu.sample_scalars(931, n), ids)
    c = m.MsmContext(0)
    try:
        # 16-bit windows of the plain set
        c.set_bases(bases, zero_is_identity=True)
        sums = torch.cat([c.msm_windows(t, 0, 5), c.msm_windows(t, 5, 16)])
        assert m.MsmContext.combine_windows(sums).to_affine_bytes() == w
        # half windows of the endomorphism set: two vectors per launch, two shares
        c.set_bases(bases, endomorphism=True, zero_is_identity=True)
        out = [torch.empty((2 * k, 96), dtype=torch.uint8, device="cuda") for k in (3, 5)]
        c.launch_half_windows_batch(two, n, 0, 3, 0, out[0])
        c.launch_half_windows_batch(two, n, 3, 8, 1, out[1])
        c.slot_sync(0)
        c.slot_sync(1)
        per_vec = torch.cat([out[0].view(2, 3, 96), out[1].view(2, 5, 96)], dim=1).cpu()
        got = m.MsmContext.combine_windows_batch(per_vec.contiguous(), 8)
        assert [g.to_affine_bytes() for g in got] == [w, w2]
        # (window sum, plain total) pairs of the wide tables' virtual windows
        c.set_wide_bits(19)
        c.set_bases(bases, precompute="wide", zero_is_identity=True)
        nv = c.virtual_windows()
        assert nv == 8
        out = [torch.empty((2 * k * 2, 96), dtype=torch.uint8, device="cuda") for k in (3, 5)]
        c.launch_vwindows_batch(two, n, 0, 3, 2, out[0])
        c.launch_vwindows_batch(two, n, 3, 8, 3, out[1])
        c.slot_sync(2)
        c.slot_sync(3)
        pairs = torch.cat([out[0].view(2, 3 * 2, 96), out[1].view(2, 5 * 2, 96)], dim=1).cpu()
        got = m.MsmContext.combine_vwindows_batch(pairs.contiguous(), nv)
        assert [g.to_affine_bytes() for g in got] == [w, w2]
        assert mask_used(c) == 1
    finally:
        c.close()


def test_multi_gpu_object_on_one_device(bn254_set):
    n, points, ids, bases = bn254_set
    vecs = [cpu.sample_scalars(940 + k, n) for k in range(2)]
    wants = [dense_want(cpu, points, 64, v, ids) for v in vecs]
    g = m.MultiGpuMsm([0], gather="host")
    try:
        for endo in (False, True):
            g.set_bases(bases, endomorphism=endo, zero_is_identity=True)
            assert g.msm(vecs[0]).to_affine_bytes() == wants[0]
            assert [x.to_affine_bytes() for x in g.msm_batch(b"".join(vecs), n)] == wants
    finally:
        g.close()


def test_host_run_parts_carry_the_base_offset(gpu):
    """msm_hip_run splits host scalars into sub-MSMs over ranges of the bases: the mask must index base (part offset + j)"""
    L = m.lib()
    n = 70001
    c = m.MsmContext(0)
    try:
        points = c.sample_points(n, 950).cpu().numpy().tobytes()
        ids = identity_positions(n, 951)
        s = cpu.sample_scalars(952, n)
        w = dense_want(cpu, points, 64, s, ids)
        for endo in (False, True):
            c.set_bases(with_identities(points, 64, ids), endomorphism=endo, zero_is_identity=True)
            for parts in (2, 3):
                assert L.msm_hip_test_oneshot_parts(parts, 1) == 0
                assert c.msm(s).to_affine_bytes() == w, (endo, parts)
                assert c.env_report()["upload_parts"] == parts
    finally:
        assert L.msm_hip_test_oneshot_parts(0, 0) == 0
        c.close()


# ---------------------------------------------------------------------------------------------------------------- edges
def test_edge_cases(gpu):
    n = 1000
    points = cpu.sample_points(960, n)
    s = cpu.sample_scalars(961, n)
    c = m.MsmContext(0)
    try:
        # every base the identity: the identity (z = 0), whatever the scalars
        c.set_bases(bytes(64 * n), zero_is_identity=True)
        assert c.msm(s).is_identity()
        assert c.msm(b"\xff" * 32 * n).is_identity()
        # one base, the identity
        c.set_bases(bytes(64), zero_is_identity=True)
        assert c.msm(s[:32]).is_identity()
        # 2^256 - 1 at an identity: OK and the oracle's value
        ids = np.array([3, 500])
        big = bytearray(s)
        big[32 * 3:32 * 4] = b"\xff" * 32
        c.set_bases(with_identities(points, 64, ids), zero_is_identity=True, endomorphism=None)
        assert c.msm(bytes(big)).to_affine_bytes() == dense_want(cpu, points, 64, s, ids)
        with pytest.raises(m.MsmHipError):  # ... and still rejected at a real point
            big[32 * 4:32 * 5] = b"\xff" * 32
            c.msm(bytes(big))
        # CHECK_ON_CURVE with the flag accepts (0, 0) and still rejects an off-curve point
        c.set_bases(with_identities(points, 64, ids), check_on_curve=True, zero_is_identity=True)
        off = bytearray(with_identities(points, 64, ids))
        off[64 * 7 + 32] ^= 1
        with pytest.raises(m.MsmHipError) as e:
            c.set_bases(bytes(off), check_on_curve=True, zero_is_identity=True)
        assert e.value.code == ERR_NOT_ON_CURVE
        # without the flag, (0, 0) is an off-curve point as before
        with pytest.raises(m.MsmHipError) as e:
            c.set_bases(with_identities(points, 64, ids), check_on_curve=True)
        assert e.value.code == ERR_NOT_ON_CURVE
        # the flag alone resolves as flags = 0 does (the curve's default mode: the endomorphism images on BN254)
        c.set_bases(points, endomorphism=None, zero_is_identity=True)
        assert c.uses_endomorphism()
    finally:
        c.close()


def test_no_extra_pass_without_identities(gpu):
    n = 4097
    points = cpu.sample_points(970, n)
    s = cpu.sample_scalars(971, n)
    c = m.MsmContext(0)
    try:
        c.set_bases(points, endomorphism=True)
        plain = c.msm(s).to_affine_bytes()
        assert mask_used(c) == 0
        c.set_bases(points, endomorphism=True, zero_is_identity=True)
        assert c.msm(s).to_affine_bytes() == plain
        assert mask_used(c) == 0
        c.set_bases(with_identities(points, 64, [17]), endomorphism=True, zero_is_identity=True)
        assert c.msm(s).to_affine_bytes() == dense_want(cpu, points, 64, s, [17])
        assert mask_used(c) == 1
    finally:
        c.close()


def test_2_20_bases_half_identities(gpu):
    """2^20 endomorphism bases, half of them identities: the same context's dense MSM over the real points with those scalars zeroed"""
    n = 1 << 20
    c = m.MsmContext(0)
    try:
        pts = c.sample_points(n, 980)
        ids = torch.rand(n, generator=torch.Generator().manual_seed(981)) < 0.5
        ids_dev = ids.cuda()
        zeroed = pts.clone()
        zeroed[ids_dev] = 0
        s = c.sample_scalars(n, 982)
        c.set_bases(zeroed, endomorphism=True, zero_is_identity=True)
        got = c.msm(s).to_affine_bytes()
        assert mask_used(c) == 1
        s0 = s.clone()
        s0[ids_dev] = 0
        c.set_bases(pts, endomorphism=True)
        assert got == c.msm(s0).to_affine_bytes()
    finally:
        c.close()
