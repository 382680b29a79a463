"""The columns of a memory argument on the device (libmsm_frmem.so, include/msm_frmem.h; msm-webgpu_amd/build.py's MEM_LIBRARIES): a stable argsort
of integer keys -- the address-sorted trace of halo2- and PLONK-style zkVMs -- and the access counters of offline memory checking (Spartan's
Spark, Lasso, Jolt): for every access its rank among the accesses to the same address and the one before it, for every address its count and
its last access.

Module-level functions that take a context (an MsmContext); neither api.py nor scalars.py imports this module.  Keys are contiguous CUDA tensors
of int32 / uint32 or int64 / uint64, read as unsigned words; what comes back are new int32 tensors (an index, a rank or a count is below 2^26;
MISSING reads -1) and, for the sorted keys, a tensor of the keys' type.  Every output is a new tensor, so none overlaps an operand.  A call runs
on the context's stream, ordered behind torch's work on its operands as columns._stream_behind orders the columns, and returns when it is
complete."""
import ctypes as C
import importlib
import os

import torch

from . import columns
from ._core import _check

_build = importlib.import_module(__package__ + ".build")  # (the module: the package's attribute `build` is the function)

MISSING = 0xFFFFFFFF  # MSM_FRMEM_MISSING
MAX_ELEMENTS = 1 << 26  # MSM_FRMEM_MAX_ELEMENTS
ERR_INVALID_ARG = -2  # MSM_HIP_ERR_INVALID_ARG


def _abi():
    vp, sz, i, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    ip, u64p = C.POINTER(i), C.POINTER(C.c_uint64)
    return {
        "sort_device": [i, vp, vp, vp, vp, sz, u32, sz],
        "sort": [i, vp, vp, vp, sz, u32, sz],
        "access_device": [i, vp, vp, vp, vp, vp, sz, vp, sz, u32, sz, u64p],
        "access": [i, vp, vp, vp, vp, sz, vp, sz, u32, sz, u64p],
        "release": [],
        "test_tile": [i],
        "test_last": [ip, ip],
    }


# function, by its name behind msm_frmem_ -> argument types (release returns nothing, the others an int)
FRMEM_ABI = _abi()
_lib = None


def frmem_lib():
    """Load libmsm_frmem.so (in-tree; include/msm_frmem.h), once.  Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        so = _build.MEM_LIBRARIES["frmem"].so
        if not os.path.exists(so):
            raise ImportError("libmsm_frmem.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % so)
        L = C.CDLL(so)
        L.msm_frmem_abi_version.restype = C.c_int
        for fn, argtypes in FRMEM_ABI.items():
            f = getattr(L, "msm_frmem_" + fn)
            f.argtypes = argtypes
            if fn == "release":
                f.restype = None
        _lib = L
    return _lib


def frmem_test_tile(entries=0):
    """test hook msm_frmem_test_tile: the calls from now on work over tiles of `entries` entries (0: the design's 1024)"""
    _check(frmem_lib().msm_frmem_test_tile(int(entries)), "msm_frmem_test_tile")


def frmem_last():
    """(kernel launches, levels) of the last sort or access of this process (test hook msm_frmem_test_last)"""
    v = [C.c_int(), C.c_int()]
    _check(frmem_lib().msm_frmem_test_last(*[C.byref(x) for x in v]), "msm_frmem_test_last")
    return tuple(x.value for x in v)


def frmem_release():
    """msm_frmem_release: free the library's scratch and staging buffers (they come back with the next call)"""
    frmem_lib().msm_frmem_release()


# ------------------------------------------------------------------------------------------------ operands
_KEY_BYTES = {torch.int32: 4, torch.uint32: 4, torch.int64: 8, torch.uint64: 8}


def _keys(ctx, v, name):
    """-> (the keys, bytes per key): a contiguous CUDA tensor of 32- or 64-bit integers on the context's device, 1 .. 2^26 of them"""
    if not (isinstance(v, torch.Tensor) and v.is_cuda):
        raise TypeError("%s must be a CUDA(HIP) tensor of 32- or 64-bit integers" % name)
    if v.dtype not in _KEY_BYTES:
        raise TypeError("%s must be int32, uint32, int64 or uint64, not %s" % (name, v.dtype))
    if v.dim() != 1 or not v.is_contiguous() or v.device.index != ctx.device:
        raise ValueError("%s must be a contiguous vector on device %d" % (name, ctx.device))
    if not 1 <= v.numel() <= MAX_ELEMENTS:
        raise ValueError("%s holds %d keys, not 1 .. 2^26" % (name, v.numel()))
    return v, _KEY_BYTES[v.dtype]


def _bits(bits, key_bytes, name):
    if bits is None:
        return 8 * key_bytes
    if isinstance(bits, bool) or not isinstance(bits, int):
        raise TypeError("bits must be an integer, not %r" % (bits,))
    if not 1 <= bits <= 8 * key_bytes:
        raise ValueError("bits must lie in [1, %d] for the %d-byte keys of %s, not %d" % (8 * key_bytes, key_bytes, name, bits))
    return bits


def _new(like, n, dtype=torch.int32):
    return torch.empty((n,), dtype=dtype, device=like.device)


# ------------------------------------------------------------------------------------------------ the two calls
def argsort(ctx, keys, bits=None, sorted_keys=False):
    """perm with keys[perm[0]] <= keys[perm[1]] <= .., equal keys in ascending index order (msm_frmem_sort_device): a stable ascending argsort of
    the keys read as unsigned words.  bits: the keys lie below 2^bits (default: their whole width); the sort runs ceil(bits / 8) passes, and a
    key that does not raises ValueError with nothing written.  -> perm (int32), or (perm, keys[perm]) with sorted_keys=True."""
    k, key_bytes = _keys(ctx, keys, "keys")
    bits = _bits(bits, key_bytes, "keys")
    n = k.numel()
    perm = _new(k, n)
    out = torch.empty_like(k) if sorted_keys else None
    rc = frmem_lib().msm_frmem_sort_device(ctx.device, columns._stream_behind(ctx, k), perm.data_ptr(), out.data_ptr() if sorted_keys else None, k.data_ptr(), key_bytes, bits, n)
    if rc == ERR_INVALID_ARG:  # (the operands and the ranges were checked above: what is left is a key)
        raise ValueError("a key is not below 2^%d" % bits)
    _check(rc, "msm_frmem_sort_device")
    return (perm, out) if sorted_keys else perm


def access_counters(ctx, addr, table_size=None, bits=None):
    """The counters of a memory argument over the accesses addr[0], addr[1], .. (msm_frmem_access_device):
        rank[i] = #{j < i : addr[j] = addr[i]},  prev[i] = the last j < i with addr[j] = addr[i] (-1: none),
        counts[a] = #{i : addr[i] = a},  last[a] = the last i with addr[i] = a (-1: none), for a < table_size,
    and the number of distinct addresses.  Without table_size counts and last are None.  With it every address must be below it; like an address
    that is not below 2^bits, one that is not raises ValueError with nothing written.  -> (rank, prev, counts, last, distinct), int32 tensors."""
    a, key_bytes = _keys(ctx, addr, "addr")
    bits = _bits(bits, key_bytes, "addr")
    n = a.numel()
    if table_size is not None:
        if isinstance(table_size, bool) or not isinstance(table_size, int):
            raise TypeError("table_size must be an integer, not %r" % (table_size,))
        if not 1 <= table_size <= MAX_ELEMENTS:
            raise ValueError("table_size must lie in [1, 2^26], not %d" % table_size)
    rank, prev = _new(a, n), _new(a, n)
    counts, last = (_new(a, table_size), _new(a, table_size)) if table_size is not None else (None, None)
    distinct = C.c_uint64()
    rc = frmem_lib().msm_frmem_access_device(ctx.device, columns._stream_behind(ctx, a), rank.data_ptr(), prev.data_ptr(), counts.data_ptr() if counts is not None else None,
                                             last.data_ptr() if last is not None else None, table_size or 0, a.data_ptr(), key_bytes, bits, n, C.byref(distinct))
    if rc == ERR_INVALID_ARG:
        raise ValueError("an address is not below 2^%d%s" % (bits, "" if table_size is None else " or not below the table's %d entries" % table_size))
    _check(rc, "msm_frmem_access_device")
    return rank, prev, counts, last, distinct.value


# ------------------------------------------------------------------------------------------------ the arguments
def sorted_trace(ctx, addr, *cols):
    """The access trace in (address, time) order: perm = argsort(addr), the sorted addresses, and every column -- n scalars of 32 bytes each, moved
    as stored by columns.gather -- under that one permutation.  -> (perm, addr_sorted, [col[perm] ..])"""
    a, _ = _keys(ctx, addr, "addr")
    checked = []
    for k, col in enumerate(cols):
        t, m = columns._scalars(ctx, col, "cols[%d]" % k)
        if m != a.numel():
            raise ValueError("cols[%d] holds %d scalars, addr %d addresses" % (k, m, a.numel()))
        checked.append(t)
    perm, addr_sorted = argsort(ctx, a, sorted_keys=True)
    return perm, addr_sorted, [columns.gather(ctx, t, perm) for t in checked]


def _as_scalars(words):
    """32-bit counters as 32-byte little-endian integers (torch byte ops): plain integers whatever the context's form"""
    n = words.numel()
    out = torch.zeros((n, 32), dtype=torch.uint8, device=words.device)
    out[:, :4] = words.contiguous().view(torch.uint8).view(n, 4)
    return out


def offline_products(ctx, table_values, addr, rank, counts, gamma, tau):
    """The grand products of the four multisets of read-only offline memory checking, from given counters.  With v[a] = table_values[a]:
        Init = (a, v[a], 0),  Final = (a, v[a], counts[a]),  RS = (addr_i, v[addr_i], rank_i),  WS = (addr_i, v[addr_i], rank_i + 1),
    each tuple (a, v, t) fingerprinted as (t * gamma + v) * gamma + a - tau.  Formed with scalars_mul_add and scalars_scan(op="product",
    totals=True) on the context, in its scalar form; gamma, tau: plain integers in [0, r).  Init * WS = RS * Final exactly when rank and counts
    are the counters of addr (up to the soundness error of the fingerprints).  -> (init, final, rs, ws), 32 host bytes each."""
    r = ctx._scalar_field("offline_check")  # (Grumpkin, whose field the vector library has no unit for, and narrow formats: refused here)
    tv, n_t = columns._scalars(ctx, table_values, "table_values")
    a, _ = _keys(ctx, addr, "addr")
    gamma, tau = int(gamma), int(tau)
    if not (0 <= gamma < r and 0 <= tau < r):
        raise ValueError("gamma and tau must lie in [0, r)")
    for name, v, want in (("rank", rank, a.numel()), ("counts", counts, n_t)):
        if not (isinstance(v, torch.Tensor) and v.is_cuda) or v.dtype not in (torch.int32, torch.uint32) or v.numel() != want or v.device != tv.device:
            raise ValueError("%s must be %d 32-bit words on %s" % (name, want, tv.device))
    one = (1 << 256) % r if ctx.scalar_mont256 else 1  # a counter's bytes are a plain integer: times this constant it is in the context's form
    signed = a.view(torch.int32 if a.element_size() == 4 else torch.int64)  # (an unsigned word with its top bit set reads negative: outside too)
    if bool(((signed < 0) | (signed >= n_t)).any()):
        raise ValueError("an address of addr is not below the table's %d entries" % n_t)
    idx = signed.to(torch.int32)
    where = torch.arange(n_t, dtype=torch.int32, device=tv.device)
    read = columns.gather(ctx, tv, idx)
    rank = rank.view(torch.int32)

    def product(address, value, time):
        shifted = ctx.scalars_mul_add(_as_scalars(address), one, (r - tau) % r)  # a - tau
        inner = ctx.scalars_mul_add(_as_scalars(time), gamma * one % r, value.reshape(-1, 32))  # t * gamma + v
        _, total = ctx.scalars_scan(ctx.scalars_mul_add(inner, gamma, shifted), op="product", totals=True)
        return total

    return (product(where, tv, torch.zeros_like(where)), product(where, tv, counts.view(torch.int32)), product(idx, read, rank), product(idx, read, rank + 1))


def offline_check(ctx, table_values, addr, gamma, tau):
    """Read-only offline memory checking of the accesses addr into the table (access_counters, then offline_products): the four grand products
    (init, final, rs, ws) with init * ws = rs * final.  Every address must be below len(table_values): ValueError otherwise.  The scalar fields and
    forms of scalars_mul_add and scalars_scan; on any other context (Grumpkin's, a narrow scalar format) it raises ValueError before any library
    is reached."""
    ctx._scalar_field("offline_check")
    tv, n_t = columns._scalars(ctx, table_values, "table_values")
    if n_t > MAX_ELEMENTS:
        raise ValueError("the table holds %d scalars, at most 2^26" % n_t)
    rank, _, counts, _, _ = access_counters(ctx, addr, table_size=n_t)
    return offline_products(ctx, tv, addr, rank, counts, gamma, tau)
