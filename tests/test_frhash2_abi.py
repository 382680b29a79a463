"""MSM_FRHASH_POSEIDON2 in the C ABI of libmsm_frhash.so (include/msm_frhash.h) and its Python mirror, without a GPU: create under the flag checks
the width, the flags and the constants on the host and touches no device, the per-call entry points take such a handle and still refuse every
bad argument first, and a call without a device fails with the no-device code."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import frhash2_model as M2
from tests import frhash_model as M
from tests.test_frhash_abi import _bare_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_INVALID_ARG, ERR_NONCANONICAL = -1, -2, -4
MONT256, POSEIDON2 = 2, 16


def _create(L, r, t, rf=8, rp=56, curve=0, flags=POSEIDON2, rc=None, mu=None, null_rc=False, null_mu=False):
    p_rc, p_mu = M2.random_parameters(r, t if t in M2.WIDTHS else 12, rf, rp)
    rc = (p_rc + [0] * (rf * t + rp))[:rf * t + rp] if rc is None else rc
    mu = (p_mu + [0] * t)[:t] if mu is None else mu
    h = C.c_void_p()
    code = L.msm_frhash_create(curve, 0, t, rf, rp, 5, None if null_rc else M.to_bytes(rc), None if null_mu else M.to_bytes(mu), flags, C.byref(h))
    return code, h


def test_the_header_names_the_flag_its_value_and_the_mu_convention():
    full = open(os.path.join(ROOT, "include", "msm_frhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define MSM_FRHASH_POSEIDON2 16u\s", text)
    for word in ("Poseidon2", "mat_internal_diag_m_1", "internal_matrix_diagonal", "mu[i] + 1", "MINUS ONE", "M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]",
                 "circ(2, 1, 1)", "circ(2 M4, M4, ..)", "{2, 3, 4, 8, 12}", "J + diag(mu)"):
        assert word in full, word
    assert re.search(r"\bint msm_frhash_abi_version\s*\(void\)", text)


def test_create_under_the_flag(built):
    from msm_webgpu_amd import api

    L = api.frhash_lib()
    assert L.msm_frhash_abi_version() == 1  # (the change is additive)
    inval = ERR_INVALID_ARG
    for curve, field in ((0, "bn254"), (1, "grumpkin"), (2, "pallas"), (3, "vesta"), (4, "bls12_381"), (5, "bn254"), (6, "bls12_381")):
        r = api.SCALAR_FIELDS[field]
        for t in (2, 3, 4, 8, 12):
            for rf, rp in ((8, 56), (2, 0), (16, 128)):
                code, h = _create(L, r, t, rf, rp, curve)
                assert code == 0 and h.value, (field, t, rf, rp)
                got = [C.c_uint32() for _ in range(3)]
                assert L.msm_frhash_info(h, *[C.byref(g) for g in got]) == 0 and [g.value for g in got] == [t, rf, rp]
                L.msm_frhash_destroy(h)
        for t in (5, 6, 7, 9, 10, 11, 1, 13):  # widths Poseidon2 does not define
            code, h = _create(L, r, t, curve=curve)
            assert code == inval and not h.value, (field, t)
        n_rc = 8 * 3 + 56
        rc, mu = M2.random_parameters(r, 3, 8, 56)
        for bad in (r, (1 << 256) - 1):
            for at in (0, 40, n_rc - 1):  # a round constant that is not below r: the first, one in the middle, the last
                code, h = _create(L, r, 3, curve=curve, rc=rc[:at] + [bad] + rc[at + 1:])
                assert code == ERR_NONCANONICAL and not h.value, (field, at)
            for at in (0, 1, 2):  # ... and an entry of mu
                code, h = _create(L, r, 3, curve=curve, mu=mu[:at] + [bad] + mu[at + 1:])
                assert code == ERR_NONCANONICAL and not h.value, (field, at)
        for t in (3, 12):  # (r - 1 is below r)
            code, h = _create(L, r, t, curve=curve, rc=[r - 1] * (8 * t + 56), mu=[r - 1] * t)
            assert code == 0
            L.msm_frhash_destroy(h)
        # the table is as long as Poseidon2's: R_F t + R_P constants are read, not (R_F + R_P) t -- a value >= r right behind them is not seen
        code, h = _create(L, r, 3, curve=curve, rc=rc + [r])
        assert code == 0
        L.msm_frhash_destroy(h)
    r = api.SCALAR_FIELDS["bn254"]
    for flags in (POSEIDON2 | 1, POSEIDON2 | 4, POSEIDON2 | 8, POSEIDON2 | 1 << 31, 1, 3, 4, 8, 1 << 31, 32):
        assert _create(L, r, 3, flags=flags)[0] == inval, flags
    code, h = _create(L, r, 3, flags=POSEIDON2 | MONT256)  # (MONT256 without effect, as before)
    assert code == 0
    L.msm_frhash_destroy(h)
    assert _create(L, r, 3, null_rc=True)[0] == inval and _create(L, r, 3, null_mu=True)[0] == inval
    assert _create(L, r, 3, curve=7)[0] == inval and _create(L, r, 3, rf=7)[0] == inval and _create(L, r, 3, rf=18)[0] == inval and _create(L, r, 3, rp=129)[0] == inval
    rc, mu = M2.random_parameters(r, 3, 8, 56)
    assert L.msm_frhash_create(0, 0, 3, 8, 56, 5, M.to_bytes(rc), M.to_bytes(mu), POSEIDON2, None) == inval
    assert L.msm_frhash_create(0, 0, 3, 8, 56, 3, M.to_bytes(rc), M.to_bytes(mu), POSEIDON2, C.byref(C.c_void_p())) == inval  # alpha
    assert L.msm_frhash_create(0, -1, 3, 8, 56, 5, M.to_bytes(rc), M.to_bytes(mu), POSEIDON2, C.byref(C.c_void_p())) == inval  # the device


def test_the_calls_take_a_poseidon2_handle_and_need_a_device(built):
    from msm_webgpu_amd import api

    L = api.frhash_lib()
    inval = ERR_INVALID_ARG
    r = api.SCALAR_FIELDS["bn254"]
    code, h = _create(L, r, 3)
    assert code == 0
    code, h4 = _create(L, r, 4)
    assert code == 0
    code, h2 = _create(L, r, 2)
    assert code == 0
    n = 4
    bufs = [C.create_string_buffer(b"\x01" * (32 * 3 * n), 32 * 3 * n), C.create_string_buffer(b"\x07" * (32 * 3 * n), 32 * 3 * n)]
    a, out = [C.cast(x, C.c_void_p) for x in bufs]
    cap = M.to_bytes([5])
    A, O = 1 << 20, 1 << 16  # device addresses that are never touched: every check below comes first

    def pdev(t=h, out=O, state=A, n=n, flags=0):
        return L.msm_frhash_permute_device(t, None, C.c_void_p(out) if out else None, C.c_void_p(state) if state else None, n, flags)

    def phost(t=h, out=out, state=a, n=n, flags=0):
        return L.msm_frhash_permute(t, out, state, n, flags)

    def hdev(t=h, out=O, a=A, rows=2, length=5, stride=6, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_hash_device(t, None, C.c_void_p(out) if out else None, C.c_void_p(a) if a else None, rows, length, stride, capacity, capacity_at, out_at, flags)

    def hhost(t=h, out=out, a=a, rows=2, length=5, stride=6, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_hash(t, out, a, rows, length, stride, capacity, capacity_at, out_at, flags)

    def mdev(t=h, nodes=O, leaves=A, n_leaves=8, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_merkle_device(t, None, C.c_void_p(nodes) if nodes else None, C.c_void_p(leaves) if leaves else None, n_leaves, capacity, capacity_at, out_at, flags)

    def mhost(t=h, nodes=out, leaves=a, n_leaves=8, capacity=cap, capacity_at=0, out_at=0, flags=0):
        return L.msm_frhash_merkle(t, nodes, leaves, n_leaves, capacity, capacity_at, out_at, flags)

    # bad ranges, overlaps and flags are refused first, as for a Poseidon handle; the create flag is no flag of a call
    assert pdev(n=0) == inval and phost(n=0) == inval and pdev(n=(1 << 26) // 3 + 1) == inval
    for flags in (1, 4, POSEIDON2, POSEIDON2 | MONT256, 1 << 31):
        assert pdev(flags=flags) == inval and phost(flags=flags) == inval and hdev(flags=flags) == inval and hhost(flags=flags) == inval
        assert mdev(flags=flags) == inval and mhost(flags=flags) == inval
    assert pdev(out=0) == inval and pdev(state=0) == inval and pdev(out=O + 8) == inval and pdev(state=A + 4) == inval
    assert pdev(out=A + 32) == inval and pdev(out=A - 32) == inval and phost(out=C.c_void_p(a.value + 32)) == inval  # overlapping, yet not in place
    assert hdev(rows=0) == inval and hdev(length=0) == inval and hdev(stride=4) == inval and hhost(stride=4) == inval
    assert hdev(capacity_at=3) == inval and hdev(out_at=3) == inval and hdev(t=h4, capacity_at=4) == inval and hdev(t=h4, out_at=4) == inval
    assert hdev(out=A) == inval and hdev(out=A + 32 * 10) == inval and hhost(out=a) == inval
    assert hdev(capacity=M.to_bytes([r])) == ERR_NONCANONICAL and hhost(capacity=M.to_bytes([r])) == ERR_NONCANONICAL
    for bad in (0, 1, 3, 6, 12, (1 << 26) + 2):
        assert mdev(n_leaves=bad) == inval, bad
    assert mdev(t=h4, n_leaves=8) == inval and mdev(t=h2, n_leaves=0) == inval and mdev(t=h2, n_leaves=65) == inval  # arity 3; a chain's levels
    assert mdev(nodes=A) == inval and mdev(nodes=A + 32 * 7) == inval and mhost(nodes=a) == inval
    assert mdev(capacity=M.to_bytes([r])) == ERR_NONCANONICAL

    if not torch.cuda.is_available():
        before = [x.raw for x in bufs]
        assert pdev() == ERR_NO_DEVICE and phost() == ERR_NO_DEVICE and pdev(flags=MONT256) == ERR_NO_DEVICE and pdev(out=A) == ERR_NO_DEVICE and phost(out=a) == ERR_NO_DEVICE
        assert hdev() == ERR_NO_DEVICE and hhost() == ERR_NO_DEVICE and hdev(capacity=None) == ERR_NO_DEVICE and hhost(flags=MONT256, capacity_at=2, out_at=2) == ERR_NO_DEVICE
        assert hdev(t=h4, capacity_at=3, out_at=3) == ERR_NO_DEVICE
        assert mdev() == ERR_NO_DEVICE and mhost() == ERR_NO_DEVICE and mdev(t=h4, n_leaves=27) == ERR_NO_DEVICE and mdev(t=h2, n_leaves=64) == ERR_NO_DEVICE
        assert [x.raw for x in bufs] == before
    for handle in (h, h4, h2):
        L.msm_frhash_destroy(handle)
    assert L.msm_frhash_test_tile(4) == 0 and L.msm_frhash_test_tile(0) == 0


def test_python_handles_and_bad_arguments(built):
    from msm_webgpu_amd import api

    r = api.SCALAR_FIELDS["bn254"]
    ctx = _bare_context()
    assert (api.MsmContext.FRHASH_POSEIDON2, api.MsmContext.POSEIDON2_WIDTHS) == (16, (2, 3, 4, 8, 12))
    rc, mu = M2.random_parameters(r, 4, 8, 56)
    with ctx.poseidon() as old:
        assert old.kind == "poseidon"
    with ctx.poseidon2(4, 8, 56, rc, mu, capacity=(2 << 64), capacity_at=3) as h:  # no device is touched
        assert (h.kind, h.t, h.full_rounds, h.partial_rounds, h.arity, h.curve, h.capacity, h.capacity_at, h.out_at) == ("poseidon2", 4, 8, 56, 3, "bn254", 2 << 64, 3, 0) and h._h
        for bad in (lambda: ctx.scalars_permute(h, bytes(32 * 5)), lambda: ctx.scalars_hash(h, bytes(32 * 6), 7), lambda: ctx.merkle_tree(h, bytes(32 * 8)),
                    lambda: _bare_context("pallas").scalars_permute(h, bytes(128))):
            with pytest.raises(ValueError):
                bad()
        assert ctx.merkle_path(h, M.to_bytes(range(9)), M.to_bytes([9, 10, 11, 12]), 4) == [[M.to_bytes([3]), M.to_bytes([5])], [M.to_bytes([9]), M.to_bytes([11])]]
        if not torch.cuda.is_available():
            for call in (lambda: ctx.scalars_permute(h, bytes(128)), lambda: ctx.scalars_hash(h, bytes(64), 2), lambda: ctx.merkle_tree(h, bytes(96))):
                with pytest.raises(api.MsmHipError) as e:
                    call()
                assert e.value.code == ERR_NO_DEVICE
    assert not h._h
    with pytest.raises(TypeError):
        ctx.scalars_permute(h, bytes(128))  # a closed handle
    g = _bare_context("grumpkin", mont=True).poseidon2(12, 2, 0, [1] * 24, [2] * 12)  # every curve's field
    assert (g.kind, g.t, g.arity) == ("poseidon2", 12, 11)
    g.close()
    for bad in (lambda: ctx.poseidon2(5, 8, 56, [0] * 96, [0] * 5), lambda: ctx.poseidon2(4, 7, 56, rc, mu), lambda: ctx.poseidon2(4, 8, 129, rc, mu),
                lambda: ctx.poseidon2(4, 8, 56, rc[:-1], mu), lambda: ctx.poseidon2(4, 8, 56, rc + [0] * (56 * 3), mu),  # (Poseidon's count of constants)
                lambda: ctx.poseidon2(4, 8, 56, rc, mu[:3]), lambda: ctx.poseidon2(4, 8, 56, [r] + rc[1:], mu), lambda: ctx.poseidon2(4, 8, 56, rc, mu[:3] + [r]),
                lambda: ctx.poseidon2(4, 8, 56, rc, mu, capacity_at=4), lambda: ctx.poseidon2(4, 8, 56, rc, mu, out_at=4), lambda: ctx.poseidon2(4, 8, 56, rc, mu, capacity=r),
                lambda: _bare_context(width=8).poseidon2(4, 8, 56, rc, mu)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ctx.poseidon2(4, 8, 56)  # no default constants
