"""libmsm_frhash.so in the C ABI (include/msm_frhash.h) and its Python mirror, without a GPU: the symbols are declared and exported at ABI version 1
beside the unchanged other eight libraries, create checks its shape and its constants on the host and touches no device, every bad argument of
a call is answered before a device is asked for, a call without a device fails with the no-device code and leaves its buffers alone, and the
Python methods raise before any library is reached."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import frhash_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG, ERR_NONCANONICAL = -1, -2, -4
MONT256 = 2


def _header():
    with open(os.path.join(ROOT, "include", "msm_frhash.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_are_declared_and_exported(built):
    from msm_webgpu_amd import api

    text = _header()
    for name, value in (("MONT256", "2u"), ("MAX_WIDTH", "12"), ("MAX_FULL_ROUNDS", "16"), ("MAX_PARTIAL_ROUNDS", "128"), ("MAX_ELEMENTS", r"\(1u << 26\)"), ("MAX_LEVELS", "64")):
        assert re.search(r"#define MSM_FRHASH_%s %s\s" % (name, value), text), name
    assert re.search(r"\bint msm_frhash_create\s*\(int curve, int device, uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, uint32_t alpha, "
                     r"const uint8_t\* round_constants,\s*const uint8_t\* mds, uint32_t flags, msm_frhash\*\* out\)", text)
    assert re.search(r"\bint msm_frhash_info\s*\(const msm_frhash\* h, uint32_t\* t, uint32_t\* full_rounds, uint32_t\* partial_rounds\)", text)
    assert re.search(r"\bint msm_frhash_permute_device\s*\(const msm_frhash\* h, void\* stream, void\* out, const void\* state, size_t n, uint32_t flags\)", text)
    assert re.search(r"\bint msm_frhash_permute\s*\(const msm_frhash\* h, uint8_t\* out, const uint8_t\* state, size_t n, uint32_t flags\)", text)
    tail = r"const uint8_t\* capacity,\s*uint32_t capacity_at,\s*uint32_t out_at,\s*uint32_t flags\)"
    assert re.search(r"\bint msm_frhash_hash_device\s*\(const msm_frhash\* h, void\* stream, void\* out, const void\* a, size_t rows, size_t len, size_t stride, " + tail, text)
    assert re.search(r"\bint msm_frhash_hash\s*\(const msm_frhash\* h, uint8_t\* out, const uint8_t\* a, size_t rows, size_t len, size_t stride, " + tail, text)
    assert re.search(r"\bint msm_frhash_merkle_device\s*\(const msm_frhash\* h, void\* stream, void\* nodes, const void\* leaves, size_t n_leaves, " + tail, text)
    assert re.search(r"\bint msm_frhash_merkle\s*\(const msm_frhash\* h, uint8_t\* nodes, const uint8_t\* leaves, size_t n_leaves, " + tail, text)
    assert re.search(r"\bvoid msm_frhash_destroy\s*\(msm_frhash\* h\)", text) and re.search(r"\bvoid msm_frhash_release\s*\(void\)", text)
    assert re.search(r"\bint msm_frhash_abi_version\s*\(void\)", text) and re.search(r"\bint msm_frhash_test_tile\s*\(int lanes\)", text)
    full = open(os.path.join(ROOT, "include", "msm_frhash.h")).read()
    for word in ("Grumpkin", "MSM_HIP_ERR_INVALID_ARG", "MSM_HIP_ERR_NONCANONICAL", "THE HASH IS OF THE VALUES", "ONE device-to-host copy", "circomlib", "halo2", "neptune",
                 "No kernel waits for another workgroup", "reads no environment setting"):  # (the conventions are stated)
        assert word in full, word
    L = api.frhash_lib()
    for name in ("msm_frhash_create", "msm_frhash_info", "msm_frhash_destroy", "msm_frhash_permute", "msm_frhash_permute_device", "msm_frhash_hash", "msm_frhash_hash_device",
                 "msm_frhash_merkle", "msm_frhash_merkle_device", "msm_frhash_release", "msm_frhash_abi_version", "msm_frhash_test_tile"):
        assert hasattr(L, name), name
    assert L.msm_frhash_abi_version() == 1
    assert api.lib().msm_hip_abi_version() == 7 and api.fr_lib().msm_fr_abi_version() == 1 and api.frvec_lib().msm_frvec_abi_version() == 1
    assert api.frpoly_lib().msm_frpoly_abi_version() == 1 and api.frmle_lib().msm_frmle_abi_version() == 1 and api.frmat_lib().msm_frmat_abi_version() == 1
    assert api.frgate_lib().msm_frgate_abi_version() == 1 and api.frlook_lib().msm_frlook_abi_version() == 1
    X = api.MsmContext
    assert (X.FRHASH_MONT256, X.FRHASH_MAX_WIDTH, X.FRHASH_MAX_FULL_ROUNDS, X.FRHASH_MAX_PARTIAL_ROUNDS, X.FRHASH_MAX_ELEMENTS, X.FRHASH_MAX_LEVELS) == (2, 12, 16, 128, 1 << 26, 64)
    for name in ("poseidon", "scalars_permute", "scalars_hash", "merkle_tree", "merkle_path"):
        assert callable(getattr(X, name)), name
    for name in ("frhash_lib", "lib_frhash", "frhash_release", "frhash_test_tile", "poseidon_parameters"):
        assert callable(getattr(api, name)), name
    assert api.lib_frhash is api.frhash_lib
    for name in ("close", "__enter__", "__exit__"):
        assert callable(getattr(api.FrHash, name)), name


def _create(L, p, curve=0, device=0, t=None, rf=None, rp=None, alpha=5, flags=0, rc=True, mds=True):
    h = C.c_void_p()
    code = L.msm_frhash_create(curve, device, p.t if t is None else t, p.full_rounds if rf is None else rf, p.partial_rounds if rp is None else rp, alpha,
                               M.to_bytes(p.rc) if rc else None, M.to_bytes([c for row in p.mds for c in row]) if mds else None, flags, C.byref(h))
    return code, h


def test_create_checks_its_shape_and_its_constants_on_the_host(built):
    from msm_webgpu_amd import api

    L = api.frhash_lib()
    inval = ERR_INVALID_ARG
    for curve, field in ((0, "bn254"), (1, "grumpkin"), (2, "pallas"), (3, "vesta"), (4, "bls12_381"), (5, "bn254"), (6, "bls12_381")):
        r = api.SCALAR_FIELDS[field]
        for t, rf, rp in ((2, 8, 56), (3, 8, 57), (12, 16, 128), (5, 2, 0)):
            p = M.standard(r, t, rf, rp)
            code, h = _create(L, p, curve)
            assert code == 0 and h.value, (field, t)
            got = [C.c_uint32() for _ in range(3)]
            assert L.msm_frhash_info(h, *[C.byref(g) for g in got]) == 0 and [g.value for g in got] == [t, rf, rp]
            assert L.msm_frhash_info(h, None, None, None) == 0
            L.msm_frhash_destroy(h)
        p = M.standard(r, 3)
        for at in (0, 100, len(p.rc) - 1):  # a round constant that is not below r: first, in the middle, last
            for bad in (r, (1 << 256) - 1):
                q = M.Poseidon(r, 3, 8, 57, list(p.rc[:at]) + [bad] + list(p.rc[at + 1:]), p.mds)
                code, h = _create(L, q, curve)
                assert code == ERR_NONCANONICAL and not h.value, (field, at)
        for i, j in ((0, 0), (1, 2), (2, 2)):  # ... and a matrix entry
            mds = [list(row) for row in p.mds]
            mds[i][j] = r
            code, h = _create(L, M.Poseidon(r, 3, 8, 57, p.rc, mds), curve)
            assert code == ERR_NONCANONICAL and not h.value
        q = M.Poseidon(r, 3, 8, 57, [r - 1] * len(p.rc), [[r - 1] * 3] * 3)  # (r - 1 is below r)
        code, h = _create(L, q, curve)
        assert code == 0
        L.msm_frhash_destroy(h)
    p = M.standard(api.SCALAR_FIELDS["bn254"], 3)
    assert _create(L, p, curve=7)[0] == inval and _create(L, p, curve=-1)[0] == inval and _create(L, p, device=-1)[0] == inval
    assert _create(L, p, t=1)[0] == inval and _create(L, p, t=13)[0] == inval and _create(L, p, t=0)[0] == inval  # the width
    assert _create(L, p, rf=7)[0] == inval and _create(L, p, rf=0)[0] == inval and _create(L, p, rf=18)[0] == inval and _create(L, p, rf=1)[0] == inval  # full rounds
    assert _create(L, p, rp=129)[0] == inval
    assert _create(L, p, alpha=3)[0] == inval and _create(L, p, alpha=0)[0] == inval and _create(L, p, alpha=7)[0] == inval  # x^3 permutes none of the fields
    for flags in (1, 4, 8, 1 << 31, 3):
        assert _create(L, p, flags=flags)[0] == inval
    code, h = _create(L, p, flags=MONT256)  # (without effect)
    assert code == 0
    L.msm_frhash_destroy(h)
    assert _create(L, p, rc=False)[0] == inval and _create(L, p, mds=False)[0] == inval
    assert L.msm_frhash_create(0, 0, 3, 8, 57, 5, M.to_bytes(p.rc), M.to_bytes([c for row in p.mds for c in row]), 0, None) == inval  # nowhere to put it
    assert L.msm_frhash_info(None, None, None, None) == inval
    L.msm_frhash_destroy(None)  # (nothing)
    for lanes in (-1, 65, 1 << 20):
        assert L.msm_frhash_test_tile(lanes) == inval
    for lanes in (1, 64, 4, 0):
        assert L.msm_frhash_test_tile(lanes) == 0


def test_the_c_abi_checks_its_arguments_and_needs_a_device(built):
    from msm_webgpu_amd import api

    L = api.frhash_lib()
    inval = ERR_INVALID_ARG
    r = api.SCALAR_FIELDS["bn254"]
    code, h = _create(L, M.standard(r, 3))
    assert code == 0
    code, h5 = _create(L, M.standard(r, 5))
    assert code == 0
    code, h2 = _create(L, M.standard(r, 2))
    assert code == 0
    n = 4
    bufs = [C.create_string_buffer(b"\x01" * (32 * 3 * n), 32 * 3 * n), C.create_string_buffer(b"\x07" * (32 * 3 * n), 32 * 3 * n)]
    a, out = [C.cast(x, C.c_void_p) for x in bufs]
    cap = M.to_bytes([5])
    A, O = 1 << 20, 1 << 16  # device addresses that are never touched: every check below comes first

    # ---- permute
    def pdev(t=h, out=O, state=A, n=n, flags=0):
        return L.msm_frhash_permute_device(t, None, C.c_void_p(out) if out else None, C.c_void_p(state) if state else None, n, flags)

    def phost(t=h, out=out, state=a, n=n, flags=0):
        return L.msm_frhash_permute(t, out, state, n, flags)

    assert pdev(t=None) == inval and phost(t=None) == inval  # the handle
    assert pdev(n=0) == inval and phost(n=0) == inval and pdev(n=(1 << 26) // 3 + 1) == inval and pdev(n=1 << 63) == inval  # n t <= 2^26
    for flags in (1, 4, 1 << 31):
        assert pdev(flags=flags) == inval and phost(flags=flags) == inval
    assert pdev(out=0) == inval and pdev(state=0) == inval and phost(out=None) == inval and phost(state=None) == inval
    assert pdev(out=O + 8) == inval and pdev(state=A + 4) == inval  # unaligned device pointers
    assert pdev(out=A + 32) == inval and pdev(out=A - 32) == inval and pdev(out=A + 32 * (3 * n - 1)) == inval  # overlapping, yet not in place
    assert phost(out=C.c_void_p(a.value + 32)) == inval

    # ---- hash
    def hdev(t=h, out=O, a=A, rows=2, length=5, stride=6, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_hash_device(t, None, C.c_void_p(out) if out else None, C.c_void_p(a) if a else None, rows, length, stride, capacity, capacity_at, out_at, flags)

    def hhost(t=h, out=out, a=a, rows=2, length=5, stride=6, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_hash(t, out, a, rows, length, stride, capacity, capacity_at, out_at, flags)

    def hboth(**kw):
        return [hdev(**kw), hhost(**kw)]

    assert hboth(t=None) == [inval] * 2
    assert hboth(rows=0) == [inval] * 2 and hboth(length=0) == [inval] * 2 and hboth(stride=4) == [inval] * 2
    assert hdev(rows=2, length=1, stride=1 << 26) == inval and hdev(rows=1, length=(1 << 26) + 1, stride=(1 << 26) + 1) == inval  # (rows - 1) stride + len > 2^26
    assert hdev(rows=1 << 63, length=2, stride=2) == inval and hdev(rows=3, length=2, stride=1 << 63) == inval  # (... with a product that wraps)
    assert hboth(capacity_at=3) == [inval] * 2 and hboth(out_at=3) == [inval] * 2 and hboth(capacity_at=1 << 31) == [inval] * 2  # capacity_at = t
    assert hdev(t=h5, capacity_at=5) == inval and hdev(t=h5, out_at=5) == inval
    for flags in (1, 4, 1 << 31):
        assert hboth(flags=flags) == [inval] * 2
    assert hdev(out=0) == inval and hdev(a=0) == inval and hhost(out=None) == inval and hhost(a=None) == inval
    assert hdev(out=O + 8) == inval and hdev(a=A + 4) == inval
    assert hdev(out=A) == inval and hdev(out=A + 32 * 10) == inval and hdev(out=A - 32) == inval  # out inside a's span of 11, or reaching into it
    assert hhost(out=a) == inval
    assert hboth(capacity=M.to_bytes([r])) == [ERR_NONCANONICAL] * 2 and hboth(capacity=M.to_bytes([(1 << 256) - 1])) == [ERR_NONCANONICAL] * 2  # r itself

    # ---- merkle
    def mdev(t=h, nodes=O, leaves=A, n_leaves=8, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_merkle_device(t, None, C.c_void_p(nodes) if nodes else None, C.c_void_p(leaves) if leaves else None, n_leaves, capacity, capacity_at, out_at, flags)

    def mhost(t=h, nodes=out, leaves=a, n_leaves=8, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_merkle(t, nodes, leaves, n_leaves, capacity, capacity_at, out_at, flags)

    def mboth(**kw):
        return [mdev(**kw), mhost(**kw)]

    assert mboth(t=None) == [inval] * 2
    for bad in (0, 1, 3, 6, 12, (1 << 26) + 2, 1 << 27, 1 << 63):  # no power of the arity 2 with k >= 1, or too many
        assert mdev(n_leaves=bad) == inval, bad
    assert mhost(n_leaves=6) == inval and mhost(n_leaves=0) == inval
    assert mdev(t=h5, n_leaves=8) == inval and mdev(t=h5, n_leaves=2) == inval  # arity 4
    assert mdev(t=h2, n_leaves=0) == inval and mdev(t=h2, n_leaves=65) == inval  # arity 1: the levels of a chain
    assert mboth(capacity_at=3) == [inval] * 2 and mboth(out_at=3) == [inval] * 2
    for flags in (1, 4, 1 << 31):
        assert mboth(flags=flags) == [inval] * 2
    assert mdev(nodes=0) == inval and mdev(leaves=0) == inval and mdev(nodes=O + 8) == inval and mdev(leaves=A + 4) == inval
    assert mdev(nodes=A) == inval and mdev(nodes=A + 32 * 7) == inval and mdev(nodes=A - 32 * 6) == inval  # 7 nodes, 8 leaves
    assert mhost(nodes=a) == inval
    assert mboth(capacity=M.to_bytes([r])) == [ERR_NONCANONICAL] * 2

    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        assert pdev() == ERR_NO_DEVICE and phost() == ERR_NO_DEVICE and pdev(flags=MONT256) == ERR_NO_DEVICE
        assert pdev(out=A) == ERR_NO_DEVICE and phost(out=a) == ERR_NO_DEVICE  # in place
        assert pdev(out=A + 32 * 3 * n) == ERR_NO_DEVICE and pdev(out=A - 32 * 3 * n) == ERR_NO_DEVICE  # (apart: right behind, right before)
        assert pdev(n=(1 << 26) // 3, out=1 << 40) == ERR_NO_DEVICE and pdev(n=(1 << 26) // 3, out=O) == inval  # (the largest call; O lies inside its states)
        assert hboth() == [ERR_NO_DEVICE] * 2 and hboth(capacity=None) == [ERR_NO_DEVICE] * 2 and hboth(flags=MONT256, capacity_at=2, out_at=2) == [ERR_NO_DEVICE] * 2
        assert hboth(capacity=M.to_bytes([r - 1])) == [ERR_NO_DEVICE] * 2
        assert hdev(out=A + 32 * 11) == ERR_NO_DEVICE and hdev(out=A - 64) == ERR_NO_DEVICE  # (the span is 11 elements: the gap behind the last row is free)
        assert hdev(rows=1, length=1 << 26, stride=1 << 26) == ERR_NO_DEVICE and hdev(rows=1 << 26, length=1, stride=1, out=1 << 40) == ERR_NO_DEVICE  # 2^26 exactly
        assert mboth() == [ERR_NO_DEVICE] * 2 and mboth(n_leaves=2) == [ERR_NO_DEVICE] * 2 and mdev(n_leaves=1 << 26, nodes=1 << 40) == ERR_NO_DEVICE
        assert mdev(nodes=A + 32 * 8) == ERR_NO_DEVICE and mdev(nodes=A - 32 * 7) == ERR_NO_DEVICE
        assert mdev(t=h2, n_leaves=64) == ERR_NO_DEVICE and mhost(t=h2, n_leaves=3) == ERR_NO_DEVICE and mdev(t=h5, n_leaves=16) == ERR_NO_DEVICE
        assert hdev(t=h5, capacity_at=4, out_at=4) == ERR_NO_DEVICE
        assert [x.raw for x in bufs] == before
    for handle in (h, h5, h2):
        L.msm_frhash_destroy(handle)
    L.msm_frhash_release()  # (nothing held: a no-op)


def _bare_context(curve="bn254", width=32, mont=False):
    """An MsmContext that never touched the library (no device needed)"""
    from msm_webgpu_amd import api

    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.scalar_width, ctx.scalar_signed, ctx.scalar_mont256, ctx.n_bases, ctx._keepalive = curve, width, False, mont, 0, {}
    ctx.curve_id, ctx.modulus = api.CURVES[curve]
    ctx.device = 0
    return ctx


def test_python_handles_and_bad_arguments(built):
    from msm_webgpu_amd import api

    r = api.SCALAR_FIELDS["bn254"]
    ctx = _bare_context()
    with ctx.poseidon() as h:  # no device is touched
        assert (h.t, h.full_rounds, h.partial_rounds, h.arity, h.curve, h.capacity, h.capacity_at, h.out_at) == (3, 8, 57, 2, "bn254", 0, 0, 0) and h._h
        for bad in (lambda: ctx.scalars_permute(h, bytes(33)), lambda: ctx.scalars_permute(h, b""), lambda: ctx.scalars_permute(h, bytes(32 * 4)),  # no whole states
                    lambda: ctx.scalars_hash(h, bytes(32 * 6), 0), lambda: ctx.scalars_hash(h, bytes(32 * 6), 7), lambda: ctx.scalars_hash(h, bytes(32 * 6), 2, batch=4),
                    lambda: ctx.scalars_hash(h, bytes(32 * 6), 4, batch=2), lambda: ctx.scalars_hash(h, bytes(32 * 6), 2, batch=3, stride=3),
                    lambda: ctx.merkle_tree(h, bytes(32 * 6)), lambda: ctx.merkle_tree(h, bytes(32)), lambda: ctx.merkle_tree(h, bytes(64), levels=1),
                    lambda: _bare_context("pallas").scalars_permute(h, bytes(96)),  # another field
                    lambda: _bare_context(width=8).scalars_permute(h, bytes(96)),  # another scalar format
                    lambda: ctx.merkle_path(h, bytes(32 * 4), bytes(32 * 2), 0), lambda: ctx.merkle_path(h, bytes(32 * 4), bytes(32 * 3), 4)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(TypeError):  # out belongs to device vectors
            ctx.scalars_permute(h, bytes(96), out=bytearray(96))
        assert _bare_context("bn254_g2")._frhash_handle(h) == 0 and _bare_context(mont=True)._frhash_handle(h) == 2  # a G2 context takes its G1's field
        path = ctx.merkle_path(h, M.to_bytes([1, 2, 3, 4]), M.to_bytes([5, 6, 7]), 2)  # plain indexing
        assert path == [[M.to_bytes([4])], [M.to_bytes([5])]]
        if not torch.cuda.is_available():
            for call in (lambda: ctx.scalars_permute(h, bytes(96)), lambda: ctx.scalars_hash(h, bytes(64), 2), lambda: ctx.merkle_tree(h, bytes(128))):
                with pytest.raises(api.MsmHipError) as e:
                    call()
                assert e.value.code == ERR_NO_DEVICE
    assert not h._h
    for call in (lambda: ctx.scalars_permute(h, bytes(96)), lambda: ctx.scalars_permute(None, bytes(96)), lambda: ctx.merkle_tree(None, bytes(64))):
        with pytest.raises(TypeError):  # a closed handle, no handle
            call()
    g = _bare_context("grumpkin", mont=True).poseidon(t=5, capacity=(1 << 4) - 1, out_at=1)  # every curve's field
    assert (g.t, g.partial_rounds, g.arity, g.capacity, g.out_at) == (5, 60, 4, 15, 1)
    g.close()
    two = ctx.poseidon(t=2)
    with pytest.raises(ValueError):
        ctx.merkle_tree(two, bytes(32))  # a chain needs its levels
    two.close()
    rc, mds = api.poseidon_parameters("bn254", 3, 8, 4)
    own = ctx.poseidon(3, 8, 4, round_constants=rc, mds=mds)
    assert own.partial_rounds == 4
    own.close()
    for bad in (lambda: ctx.poseidon(t=1), lambda: ctx.poseidon(t=13), lambda: ctx.poseidon(full_rounds=7), lambda: ctx.poseidon(partial_rounds=129),
                lambda: ctx.poseidon(capacity_at=3), lambda: ctx.poseidon(out_at=3), lambda: ctx.poseidon(capacity=r), lambda: ctx.poseidon(round_constants=rc),
                lambda: ctx.poseidon(3, 8, 5, round_constants=rc, mds=mds), lambda: ctx.poseidon(3, 8, 4, round_constants=[r] + rc[1:], mds=mds),
                lambda: ctx.poseidon(3, 8, None, round_constants=rc, mds=mds), lambda: _bare_context(width=8).poseidon()):
        with pytest.raises(ValueError):
            bad()
