"""The columns of a lookup argument on the device (libmsm_frcol.so, include/msm_frcol.h; msm-webgpu_amd/build.py's AUX_LIBRARIES): halo2's permuted
pair A', S' and plookup's sorted vector, from the counts that MsmContext.scalars_multiplicities(counts=True) writes -- an integer prefix sum,
a run expansion and a compaction instead of a sort of 32-byte values on the host.

Module-level functions that take a context (an MsmContext); neither api.py nor scalars.py imports this module.  Every vector is a CUDA uint8
tensor of 32-byte scalars in the context's scalar format (canonical or mont256: the library moves scalars as stored, so the form does not
matter to it).  A call runs on the context's stream, ordered behind torch's work on its first operand as ScalarFieldOps._fr_call orders the
scalars_* methods -- through what that mixin asks of a context: _order_after_torch and the handle _h --, and returns when it is complete."""
import ctypes as C
import importlib
import os

import torch

from ._core import _as_device_u8, _check, lib

_build = importlib.import_module(__package__ + ".build")  # (the module: the package's attribute `build` is the function)

MISSING = 0xFFFFFFFF  # MSM_FRCOL_MISSING
MAX_TABLE, MAX_ELEMENTS = 1 << 24, 1 << 26  # MSM_FRCOL_MAX_TABLE, MSM_FRCOL_MAX_ELEMENTS
ERR_INVALID_ARG = -2  # MSM_HIP_ERR_INVALID_ARG


def _abi():
    vp, sz, i, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    ip, u64p = C.POINTER(i), C.POINTER(C.c_uint64)
    return {
        "expand_device": [i, vp, vp, vp, vp, sz, u32, sz, u64p],
        "expand": [i, vp, vp, vp, sz, u32, sz, u64p],
        "pair_device": [i, vp, vp, vp, vp, vp, sz, u64p, u64p],
        "pair": [i, vp, vp, vp, vp, sz, u64p, u64p],
        "gather_device": [i, vp, vp, vp, sz, vp, sz],
        "gather": [i, vp, vp, sz, vp, sz],
        "release": [],
        "test_tile": [i],
        "test_last": [ip, ip],
    }


# function, by its name behind msm_frcol_ -> argument types (release returns nothing, the others an int)
FRCOL_ABI = _abi()
_lib = None


def frcol_lib():
    """Load libmsm_frcol.so (in-tree; include/msm_frcol.h), once.  Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        so = _build.AUX_LIBRARIES["frcol"].so
        if not os.path.exists(so):
            raise ImportError("libmsm_frcol.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % so)
        L = C.CDLL(so)
        L.msm_frcol_abi_version.restype = C.c_int
        for fn, argtypes in FRCOL_ABI.items():
            f = getattr(L, "msm_frcol_" + fn)
            f.argtypes = argtypes
            if fn == "release":
                f.restype = None
        _lib = L
    return _lib


def frcol_test_tile(entries=0):
    """test hook msm_frcol_test_tile: the calls from now on scan over tiles of `entries` entries (0: the design's 1024)"""
    _check(frcol_lib().msm_frcol_test_tile(int(entries)), "msm_frcol_test_tile")


def frcol_last():
    """(kernel launches, scan levels) of the last expand or pair of this process (test hook msm_frcol_test_last)"""
    v = [C.c_int(), C.c_int()]
    _check(frcol_lib().msm_frcol_test_last(*[C.byref(x) for x in v]), "msm_frcol_test_last")
    return tuple(x.value for x in v)


def frcol_release():
    """msm_frcol_release: free the library's scratch and staging buffers (they come back with the next call)"""
    frcol_lib().msm_frcol_release()


# ------------------------------------------------------------------------------------------------ operands
def _scalar_context(ctx, what):
    if ctx.scalar_width != 32:
        raise ValueError("%s takes 32-byte scalars; the context's scalar format is %d bytes wide" % (what, ctx.scalar_width))


def _scalars(ctx, v, name):
    t, n = _as_device_u8(v, 32, name)
    if t.device.index != ctx.device:
        raise ValueError("%s is on %s, the context on device %d" % (name, t.device, ctx.device))
    if n < 1:
        raise ValueError("%s holds no scalar" % name)
    return t, n


def _words(ctx, v, name):
    """a CUDA tensor of 32-bit words: torch.uint32, or int32 (counts are never negative; an index of -1 is MISSING)"""
    if not (isinstance(v, torch.Tensor) and v.is_cuda):
        raise TypeError("%s must be a CUDA(HIP) tensor of 32-bit words" % name)
    if v.dtype not in (torch.int32, torch.uint32) or not v.is_contiguous() or v.device.index != ctx.device:
        raise ValueError("%s must be a contiguous int32 or uint32 tensor on device %d" % (name, ctx.device))
    return v, v.numel()


def _out(like, out, n, name="out"):
    if out is None:
        return torch.empty((n, 32), dtype=torch.uint8, device=like.device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * n or not out.is_contiguous() or out.device != like.device:
        raise ValueError("%s must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes on %s" % (name, n, like.device))
    return out


def _apart(outputs, inputs):
    """every output (name, tensor) apart from every input and from the other outputs, as the library demands: ValueError naming the two
    operands otherwise -- before the C call, whose MSM_HIP_ERR_INVALID_ARG does not say which check failed"""
    span = lambda v: (v.data_ptr(), v.data_ptr() + v.numel() * v.element_size())
    for k, (name, o) in enumerate(outputs):
        for other, v in outputs[k + 1:] + list(inputs):
            (p, p_end), (q, q_end) = span(o), span(v)
            if p < q_end and q < p_end:
                raise ValueError("%s overlaps %s: every output lies apart from every input and from the other outputs" % (name, other))


_NO_TOTAL = (1 << 64) - 1  # what *total starts at: 2^24 words of 32 bits, each with a bias of 1, add up to less than 2^57


def _stream_behind(ctx, *tensors):
    """the context's stream, made to wait for torch's work on the operands"""
    ctx._order_after_torch(*tensors)
    return lib().msm_hip_stream(ctx._h)


# ------------------------------------------------------------------------------------------------ the three calls
def expand(ctx, t, counts, n_out, bias=0, out=None):
    """out = t[0] w[0] times, then t[1] w[1] times, ... with w[j] = counts[j] + bias (msm_frcol_expand_device): n_out scalars in a new tensor
    or `out`.  t: the table, n_t <= 2^24 scalars; counts: n_t 32-bit words on the device (scalars_multiplicities(counts=True)); bias: 0 -- over a
    column's counts halo2's A' -- or 1 -- with n_out = n + n_t plookup's s.  The w[j] must add up to n_out (<= 2^26): ValueError otherwise,
    naming the sum, and out is untouched.  out lies apart from t and counts: ValueError naming the two otherwise, and nothing is called."""
    _scalar_context(ctx, "expand")
    tt, n_t = _scalars(ctx, t, "t")
    cnt, m = _words(ctx, counts, "counts")
    n_out, bias = int(n_out), int(bias)
    if m != n_t or n_t > MAX_TABLE:
        raise ValueError("the table holds %d scalars (at most 2^24), counts %d words" % (n_t, m))
    if bias not in (0, 1) or not 1 <= n_out <= MAX_ELEMENTS:
        raise ValueError("bias is 0 or 1 and n_out lies in [1, 2^26]")
    out = _out(tt, out, n_out)
    _apart([("out", out)], [("t", tt), ("counts", cnt)])
    total = C.c_uint64(_NO_TOTAL)
    rc = frcol_lib().msm_frcol_expand_device(ctx.device, _stream_behind(ctx, tt, cnt), out.data_ptr(), tt.data_ptr(), cnt.data_ptr(), n_t, bias, n_out, C.byref(total))
    if rc == ERR_INVALID_ARG and total.value not in (_NO_TOTAL, n_out):  # (the library wrote the sum: it got as far as forming it)
        raise ValueError("the counts%s add up to %d, not to the %d outputs" % (" + 1" if bias else "", total.value, n_out))
    _check(rc, "msm_frcol_expand_device")
    return out


def permuted_pair(ctx, t, counts, out=None):
    """halo2's permuted columns (A', S') of a lookup of n values into the n table values t, from the counts (msm_frcol_pair_device): A' groups the
    looked-up values by table entry; S' holds t[j] where the run of t[j] begins and the table values never looked up elsewhere, ascending by
    index.  The counts must add up to n = len(t): ValueError otherwise.  out: None or a pair of tensors, apart from t, from counts and from
    one another (ValueError naming the two that share bytes).  -> (a_perm, s_perm)"""
    _scalar_context(ctx, "permuted_pair")
    tt, n = _scalars(ctx, t, "t")
    cnt, m = _words(ctx, counts, "counts")
    if m != n or n > MAX_TABLE:
        raise ValueError("the table holds %d scalars (at most 2^24), counts %d words" % (n, m))
    a_out, s_out = (None, None) if out is None else out
    a_out, s_out = _out(tt, a_out, n, "out[0]"), _out(tt, s_out, n, "out[1]")
    _apart([("out[0]", a_out), ("out[1]", s_out)], [("t", tt), ("counts", cnt)])
    total, used = C.c_uint64(_NO_TOTAL), C.c_uint64()
    rc = frcol_lib().msm_frcol_pair_device(ctx.device, _stream_behind(ctx, tt, cnt), a_out.data_ptr(), s_out.data_ptr(), tt.data_ptr(), cnt.data_ptr(), n, C.byref(total),
                                           C.byref(used))
    if rc == ERR_INVALID_ARG and total.value not in (_NO_TOTAL, n):
        raise ValueError("the counts add up to %d, not to the %d rows of the table" % (total.value, n))
    _check(rc, "msm_frcol_pair_device")
    return a_out, s_out


def gather(ctx, a, idx, out=None):
    """out[i] = a[idx[i]] (msm_frcol_gather_device): what a vector lookup does after the count -- it fetches the other columns of the matched
    rows.  idx: a CUDA int32 tensor with -1 for "missing" (scalars_multiplicities(indices=True)) or uint32 with 0xFFFFFFFF: those elements are
    32 zero bytes.  Any other index outside a raises ValueError (that element is then zero).  out lies apart from a and idx: ValueError
    naming the two otherwise, with nothing written."""
    _scalar_context(ctx, "gather")
    ta, n_a = _scalars(ctx, a, "a")
    ti, n = _words(ctx, idx.reshape(-1) if isinstance(idx, torch.Tensor) else idx, "idx")
    if n_a > MAX_ELEMENTS or not 1 <= n <= MAX_ELEMENTS:
        raise ValueError("a vector holds 1 .. 2^26 scalars")
    out = _out(ta, out, n)
    _apart([("out", out)], [("a", ta), ("idx", ti)])
    rc = frcol_lib().msm_frcol_gather_device(ctx.device, _stream_behind(ctx, ta, ti), out.data_ptr(), ta.data_ptr(), n_a, ti.data_ptr(), n)
    if rc == ERR_INVALID_ARG:  # (the operands lay apart and the ranges were checked above: what is left is an index)
        raise ValueError("an index is neither below the %d scalars of a nor -1" % n_a)
    _check(rc, "msm_frcol_gather_device")
    return out


# ------------------------------------------------------------------------------------------------ the arguments
def _counts(ctx, table_values, f, batch, n, lookup):
    """the counts of f's values among the table's, through the context's lookup: ValueError where a value is not in the table"""
    own = lookup is None
    if own:
        lookup = ctx.lookup_table(table_values)
    elif getattr(lookup, "n", None) != table_values.numel() // 32:
        raise ValueError("lookup must be the FrLookup of the %d table values" % (table_values.numel() // 32))
    try:
        _, cnt = ctx.scalars_multiplicities(lookup, f, batch=batch, n=n, counts=True)
    finally:
        if own:
            lookup.close()
    return cnt


def lookup_columns(ctx, table_values, a, lookup=None):
    """halo2's permuted columns of the lookup of the column a into the table: lookup_table (unless `lookup`, an FrLookup of table_values, is
    given), scalars_multiplicities(counts=True), permuted_pair -> (a_perm, s_perm).  len(a) == len(table_values): halo2 pads both to the
    usable rows.  A value of a that is not in the table raises ValueError, as scalars_multiplicities(strict=True) does.  Every curve's scalar
    field, Grumpkin's included."""
    tt, n_t = _scalars(ctx, table_values, "table_values")
    ta, n = _scalars(ctx, a, "a")
    if n != n_t:
        raise ValueError("a holds %d scalars, the table %d: halo2's columns have one length" % (n, n_t))
    return permuted_pair(ctx, tt, _counts(ctx, tt, ta, 1, None, lookup))


def sorted_by_table(ctx, table_values, f, batch=1, n=None, lookup=None):
    """plookup's s = (f, t) sorted by t, as batch * n + n_t scalars: every table value once more than it is looked up in the batch rows of f
    (f, batch, n: as scalars_multiplicities).  The caller slices the halves.  A value that is not in the table raises ValueError."""
    tt, n_t = _scalars(ctx, table_values, "table_values")
    tf, total = _scalars(ctx, f, "f")
    batch = int(batch)
    if batch < 1 or total % batch:
        raise ValueError("%d scalars are not %d rows" % (total, batch))
    n = total // batch if n is None else int(n)
    if not 1 <= n <= total // batch:
        raise ValueError("n must lie in [1, %d], the length of a row, not %d" % (total // batch, n))
    return expand(ctx, tt, _counts(ctx, tt, tf, batch, n, lookup), batch * n + n_t, bias=1)


def halo2_lookup(ctx, table_values, a, beta, gamma):
    """The columns of halo2's lookup argument: (a_perm, s_perm) = lookup_columns, and the grand product
    z[i] = prod_{k < i} (a[k] + beta)(t[k] + gamma) / ((a'[k] + beta)(s'[k] + gamma)) with its closing value `total` (32 host bytes), which is 1 in
    the data's form exactly when the two permutations hold.  beta, gamma: integers in [0, r) or their 32 bytes, always plain integers.  Chains
    scalars_add, scalars_mul, scalars_inverse (1 / 0 = 0) and scalars_scan(op="product", exclusive=True, totals=True) behind the columns; the
    inputs are left untouched.  Not on Grumpkin, whose scalar field the vector library has no unit for.  -> (a_perm, s_perm, z, total)"""
    a_perm, s_perm = lookup_columns(ctx, table_values, a)
    num = ctx.scalars_mul(ctx.scalars_add(a.reshape(-1, 32).clone(), beta), ctx.scalars_add(table_values.reshape(-1, 32).clone(), gamma))
    den = ctx.scalars_mul(ctx.scalars_add(a_perm.clone(), beta), ctx.scalars_add(s_perm.clone(), gamma))
    z, total = ctx.scalars_scan(ctx.scalars_mul(num, ctx.scalars_inverse(den)), op="product", exclusive=True, totals=True)
    return a_perm, s_perm, z, total
