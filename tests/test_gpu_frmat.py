"""Sparse matrix-vector products on the device (include/msm_frmat.h; MsmContext.scalars_matrix, scalars_matvec, r1cs_tables) against the pure-Python
model (tests/frmat_model.py), byte for byte: every shape of the host test (tests/test_frmat_host.py) -- under the tile hook and at the design tile
T = 1024 --, both directions, the transposed product also through a matrix made from the transposed arrays; the five fields, both scalar formats
and a G2 context; the zero tail, a row view as output, the planned launches and levels, the rejection of an element of x that is not below r
where -- and only where -- an entry references it, identical bytes on a second run, ordering behind torch's stream, the host form, and one
three-level case at the design tile checked against closed forms, without a big-integer loop on the host."""
import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frmat_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
T = 1024  # csrc/frmat_kernels.h: FRMAT_TILE
ERR_NONCANONICAL, ERR_INVALID_ARG = -4, -2
R = api.SCALAR_FIELDS["bn254"]
FIELDS = ("bn254", "grumpkin", "pallas", "vesta", "bls12_381")
SHAPES = M.DESIGN_SHAPES + M.SMALL_SHAPES


@pytest.fixture(scope="module")
def contexts(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(curve="bn254", mont=False):
        if curve not in made:
            made[curve] = m.MsmContext(0, curve)
        made[curve].set_scalar_format(mont256=mont)
        return made[curve]

    yield get
    api.frmat_test_tile(0)
    for c in made.values():
        c.close()
    api.frmat_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def host(t):
    return M.from_bytes(raw(t))


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def planted(r, n, rnd):
    """random values with 0, 1 and r - 1 among them"""
    return [(0, 1, r - 1)[rnd.randrange(3)] if rnd.randrange(4) == 0 else rnd.randrange(r) for _ in range(n)]


def matrix(ctx, name, rnd, r, transpose=True):
    """-> (FrMatrix made under the shape's tile, its arrays)"""
    tile, rows, cols, ptr, idx = M.shape(name, rnd)
    val = planted(r, len(idx), rnd)
    api.frmat_test_tile(0 if tile == T else tile)
    mat = ctx.scalars_matrix(rows, cols, ptr, idx, val, transpose=transpose)
    api.frmat_test_tile(0)
    return mat, (tile, rows, cols, ptr, idx, val)


# ---- every shape, field and form, both directions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "mont256"])
@pytest.mark.parametrize("curve", FIELDS + ("bn254_g2",))
def test_every_shape_both_directions(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    rnd = rng(600)
    for name in SHAPES:
        mat, (tile, rows, cols, ptr, idx, val) = matrix(ctx, name, rnd, r)
        assert (mat.rows, mat.cols, mat.nnz, mat.has_transpose) == (rows, cols, len(idx), True)
        what = (curve, mont, name)
        x, w = planted(r, cols, rnd), planted(r, rows, rnd)
        y = ctx.scalars_matvec(mat, dev(form(x, r, mont)))
        assert tuple(y.shape) == (rows, 32) and host(y) == form(M.matvec(rows, cols, ptr, idx, val, x, r), r, mont), what
        lv = M.levels(ptr, tile)
        assert api.frmat_last() == (lv + 1, lv) and (name not in M.LEVELS or lv == M.LEVELS[name]), what
        want = form(M.matvec(rows, cols, ptr, idx, val, w, r, transpose=True), r, mont)
        yt = ctx.scalars_matvec(mat, dev(form(w, r, mont)), transpose=True)
        assert tuple(yt.shape) == (cols, 32) and host(yt) == want, what + ("transposed",)
        t_ptr, t_idx, t_val = M.transpose_csr(rows, cols, ptr, idx, val)
        lt = M.levels(t_ptr, tile)
        assert api.frmat_last() == (lt + 1, lt), what
        api.frmat_test_tile(0 if tile == T else tile)
        other = ctx.scalars_matrix(cols, rows, t_ptr, t_idx, M.to_bytes(t_val))  # (the values as bytes, no transposed structure)
        api.frmat_test_tile(0)
        assert not other.has_transpose and raw(ctx.scalars_matvec(other, dev(form(w, r, mont)))) == raw(yt), what + ("from the transposed arrays",)
        other.close()
        mat.close()
        assert not mat._h


# ---- the tail, a row view, two runs ----------------------------------------------------------------------------------------------------------------
def test_pad_to_zeroes_the_tail_and_out_is_a_row_of_a_larger_buffer(contexts):
    ctx = contexts()
    rnd = rng(610)
    for name in ("one row of 2050", "9x7 with empty rows"):
        mat, (tile, rows, cols, ptr, idx, val) = matrix(ctx, name, rnd, R)
        x = planted(R, cols, rnd)
        want = M.matvec(rows, cols, ptr, idx, val, x, R)
        n = 16
        buf = torch.full((3, n, 32), 0xFF, dtype=torch.uint8, device="cuda")
        assert ctx.scalars_matvec(mat, dev(x), out=buf[1], pad_to=n).data_ptr() == buf[1].data_ptr()
        assert host(buf[1]) == want + [0] * (n - rows) and raw(buf[0]) == raw(buf[2]) == b"\xff" * (32 * n), name
        first = raw(ctx.scalars_matvec(mat, dev(x), pad_to=n))
        assert first == raw(buf[1]) and raw(ctx.scalars_matvec(mat, dev(x), pad_to=n)) == first  # the same bytes on every run
        wt = planted(R, rows, rnd)
        yt = ctx.scalars_matvec(mat, dev(wt), transpose=True, pad_to=cols + 5)
        assert host(yt) == M.matvec(rows, cols, ptr, idx, val, wt, R, transpose=True) + [0] * 5
        with pytest.raises(ValueError):
            ctx.scalars_matvec(mat, dev(x), pad_to=rows - 1)
        with pytest.raises(ValueError):
            ctx.scalars_matvec(mat, dev(x), out=buf[1])  # (out of 16, the exact length asked for)
        with pytest.raises(ValueError):
            ctx.scalars_matvec(mat, dev(x + [1]))
        mat.close()


def test_r1cs_tables_fill_three_rows_and_leave_the_others(contexts):
    ctx = contexts()
    rnd = rng(620)
    tile, rows, cols, ptr, idx = M.shape("random tile 8", rnd)
    api.frmat_test_tile(tile)
    vals = [planted(R, len(idx), rnd) for _ in range(3)]
    mats = [ctx.scalars_matrix(rows, cols, ptr, idx, v) for v in vals]
    api.frmat_test_tile(0)
    z = planted(R, cols, rnd)
    want = [M.matvec(rows, cols, ptr, idx, v, z, R) + [0] * (16 - rows) for v in vals]
    buf = torch.full((5, 16, 32), 0xAB, dtype=torch.uint8, device="cuda")
    assert ctx.r1cs_tables(*mats, dev(z), out=buf, first_row=1) is buf
    assert [host(buf[k]) for k in (1, 2, 3)] == want and raw(buf[0]) == raw(buf[4]) == b"\xab" * (32 * 16)
    fresh = ctx.r1cs_tables(*mats, dev(z))
    assert tuple(fresh.shape) == (3, 16, 32) and [host(fresh[k]) for k in range(3)] == want
    wide = ctx.r1cs_tables(*mats, dev(z), n=32)
    assert [host(wide[k]) for k in range(3)] == [w + [0] * 16 for w in want]
    with pytest.raises(ValueError):
        ctx.r1cs_tables(*mats, dev(z), n=8)


# ---- errors, ordering, the host form ---------------------------------------------------------------------------------------------------------------
def test_an_element_of_x_not_below_r_is_refused_where_it_is_read(contexts):
    ctx = contexts()
    rnd = rng(630)
    rows, cols = 2100, 40
    ptr = list(range(rows + 1))
    idx = [rnd.randrange(cols - 1) for _ in range(rows)]  # the last column is referenced by no entry; three tiles
    val = planted(R, rows, rnd)
    mat = ctx.scalars_matrix(rows, cols, ptr, idx, val, transpose=True)
    x = planted(R, cols, rnd)
    want = M.to_bytes(M.matvec(rows, cols, ptr, idx, val, x, R))
    for bad in (R, (1 << 256) - 1):
        for at in (idx[0], idx[-1], idx[1500]):
            b = list(x)
            b[at] = bad
            for call in (lambda: ctx.scalars_matvec(mat, dev(b)), lambda: ctx.scalars_matvec(mat, M.to_bytes(b))):
                with pytest.raises(m.MsmHipError) as e:
                    call()
                assert e.value.code == ERR_NONCANONICAL
                assert raw(ctx.scalars_matvec(mat, dev(x))) == want  # the next call is unaffected
        assert raw(ctx.scalars_matvec(mat, dev(x[:-1] + [bad]))) == want  # a column nobody references is not read
        w = planted(R, rows, rnd)
        w[1234] = bad
        with pytest.raises(m.MsmHipError) as e:
            ctx.scalars_matvec(mat, dev(w), transpose=True)
        assert e.value.code == ERR_NONCANONICAL
    with pytest.raises(ValueError):  # the matrix itself: checked on the host
        ctx.scalars_matrix(2, 2, [0, 1, 2], [0, 1], [1, R])
    with pytest.raises(ValueError):
        ctx.scalars_matrix(2, 2, [0, 1, 2], [0, 2], [1, 1])
    with pytest.raises(ValueError):
        ctx.scalars_matrix(2, 2, [0, 2, 1], [0], [1])
    L, h = api.frmat_lib(), api.C.c_void_p()
    p, i = np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32)
    assert L.msm_frmat_create(0, 0, 1, 1, 1, p.ctypes.data, i.ctypes.data, api.C.cast(api.C.c_char_p(R.to_bytes(32, "little")), api.C.c_void_p), 0, api.C.byref(h)) == ERR_NONCANONICAL
    plain = ctx.scalars_matrix(rows, cols, ptr, idx, val)
    with pytest.raises(ValueError):
        ctx.scalars_matvec(plain, dev(x[:1] * rows), transpose=True)
    t = dev(x + x)
    assert L.msm_frmat_mul_device(plain._h, None, t.data_ptr(), rows, t.data_ptr() + 32 * 8, cols, 0) == ERR_INVALID_ARG  # y over x
    assert L.msm_frmat_mul_device(plain._h, None, t.data_ptr() + 8, rows, t.data_ptr(), cols, 0) == ERR_INVALID_ARG  # unaligned
    assert L.msm_frmat_mul_device(plain._h, None, t.data_ptr(), rows, t.data_ptr(), cols, api.MsmContext.FRMAT_TRANSPOSE) == ERR_INVALID_ARG
    assert host(t) == x + x


def test_a_vector_with_pending_work_on_a_torch_stream(contexts):
    ctx = contexts()
    rnd = rng(640)
    mat, (tile, rows, cols, ptr, idx, val) = matrix(ctx, "one row of 2050", rnd, R)
    x = planted(R, cols, rnd)
    src = dev(x)
    want = M.matvec(rows, cols, ptr, idx, val, x, R)
    big = torch.ones(1 << 24, device="cuda")
    t = torch.zeros(cols, 32, dtype=torch.uint8, device="cuda")
    for _ in range(8):  # work that is still running on torch's stream when the call is made ...
        big = big * 1.0001 + 1.0
    t.copy_(src, non_blocking=True)  # ... and behind it the vector the call reads
    assert host(ctx.scalars_matvec(mat, t)) == want
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        u = torch.zeros(cols, 32, dtype=torch.uint8, device="cuda")
        for _ in range(8):
            big = big * 1.0001 + 1.0
        u.copy_(src, non_blocking=True)
        got = ctx.scalars_matvec(mat, u)
    assert host(got) == want


def test_host_form(contexts):
    rnd = rng(650)
    for mont in (False, True):
        ctx = contexts("bn254", mont)
        mat, (tile, rows, cols, ptr, idx, val) = matrix(ctx, "one row of 2050", rnd, R)
        x, w = planted(R, cols, rnd), planted(R, rows, rnd)
        assert ctx.scalars_matvec(mat, M.to_bytes(form(x, R, mont)), pad_to=8) == M.to_bytes(form(M.matvec(rows, cols, ptr, idx, val, x, R) + [0, 0], R, mont))
        api.frmat_release()  # the staging buffer gone, and back with the next call; the matrix stays
        assert ctx.scalars_matvec(mat, M.to_bytes(form(w, R, mont)), transpose=True) == M.to_bytes(form(M.matvec(rows, cols, ptr, idx, val, w, R, transpose=True), R, mont))
        with pytest.raises(TypeError):
            ctx.scalars_matvec(mat, M.to_bytes(x), out=torch.zeros(rows, 32, dtype=torch.uint8, device="cuda"))


# ---- the design tile over three levels, against closed forms ---------------------------------------------------------------------------------------
def _small(v, n):
    """integers below 2^63 as n x 32 canonical little-endian bytes"""
    out = np.zeros((n, 32), dtype=np.uint8)
    out[:, :8] = np.asarray(v, dtype="<u8").reshape(n, 1).view(np.uint8)
    return out


def test_three_levels_at_the_design_tile_against_closed_forms(contexts):
    """one row of 2^20 + 5 entries -- 1025 tiles hold a part of it, their partials are two tiles of the second pass, whose two are the third --
    and 2^10 rows of one entry behind it; every value 1, x[j] = j + 1: row 0 is the sum 1 + .. + n, row 1 + i is i + 1.  Transposed, with
    w[i] = i + 1: column j is 1 + (j + 2 for j < 2^10).  No loop over the entries on the host."""
    ctx = contexts()
    n, tail = (1 << 20) + 5, 1 << 10
    rows, cols, nnz = 1 + tail, n, n + tail
    ptr = np.concatenate([np.zeros(1, dtype=np.int64), n + np.arange(tail + 1, dtype=np.int64)])
    idx = np.concatenate([np.arange(n, dtype=np.int64), np.arange(tail, dtype=np.int64)])
    mat = ctx.scalars_matrix(rows, cols, ptr, torch.from_numpy(idx), _small(np.ones(nnz, dtype=np.uint64), nnz), transpose=True)
    assert (mat.rows, mat.cols, mat.nnz) == (rows, cols, nnz)
    x = torch.from_numpy(_small(np.arange(1, n + 1, dtype=np.uint64), n)).cuda()
    y = ctx.scalars_matvec(mat, x, pad_to=2048)
    assert api.frmat_last() == (4, 3)
    assert host(y) == [n * (n + 1) // 2 % R] + list(range(1, tail + 1)) + [0] * (2048 - rows)
    w = torch.from_numpy(_small(np.arange(1, rows + 1, dtype=np.uint64), rows)).cuda()
    yt = ctx.scalars_matvec(mat, w, transpose=True)
    assert api.frmat_last() == (2, 1)  # (columns of one or two entries: no row of the transposed matrix is longer)
    want = np.ones(n, dtype=np.uint64)
    want[:tail] += np.arange(2, tail + 2, dtype=np.uint64)
    assert np.array_equal(yt.cpu().numpy(), _small(want, n))
    mat.close()
