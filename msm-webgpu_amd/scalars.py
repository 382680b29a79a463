"""ctypes binding of the eight scalar-field libraries (libmsm_fr.so .. libmsm_frhash.so, msm-webgpu_amd/build.py's FR_LIBRARIES) and their Python
surface: one table of argument types, the test hooks, the handle classes and ScalarFieldOps, the scalars_* / prover / hashing methods that
MsmContext (api.py) inherits.  Every call into a library goes through ScalarFieldOps._fr_call."""
import ctypes as C
import functools
import os

import numpy as np
import torch

from . import build as _build
from ._core import FR_MAX_LOG_N, SCALAR_FIELDS, _as_device_u8, _check, lib, root_of_unity


class FrmleTerm(C.Structure):
    """msm_frmle_term (include/msm_frmle.h): coeff * prod_{f < degree} row[rows[f]]"""
    _fields_ = [("coeff", C.c_uint8 * 32), ("degree", C.c_uint32), ("rows", C.c_uint32 * 4)]


class FrgateTerm(C.Structure):
    """msm_frgate_term (include/msm_frgate.h): coeff * prod_{f < degree} row[rows[f]] at the rotation rots[f]"""
    _fields_ = [("coeff", C.c_uint8 * 32), ("degree", C.c_uint32), ("rows", C.c_uint32 * 8), ("rots", C.c_int32 * 8)]


def _abi():
    vp, u8p, sz, i, u32 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32
    ip, szp, u32p, u64p, vpp = C.POINTER(i), C.POINTER(sz), C.POINTER(u32), C.POINTER(C.c_uint64), C.POINTER(vp)
    mle, gate = C.POINTER(FrmleTerm), C.POINTER(FrgateTerm)
    return {
        "fr": {
            "ntt_device": [i, i, vp, vp, i, sz, u8p, u8p, u8p, u32],
            "ntt": [i, i, vp, i, sz, u8p, u8p, u8p, u32],
            "release": [],
            "test_pass_bits": [i],
            "test_last": [ip, ip],
        },
        "frvec": {
            "map_device": [i, i, vp, vp, vp, vp, vp, sz, i, u8p, u8p, u32],
            "inverse_device": [i, i, vp, vp, vp, sz, u32],
            "scan_device": [i, i, vp, vp, vp, sz, sz, i, u32, vp],
            "map": [i, i, vp, vp, vp, vp, sz, i, u8p, u8p, u32],
            "inverse": [i, i, vp, vp, sz, u32],
            "scan": [i, i, vp, vp, sz, sz, i, u32, vp],
            "release": [],
            "test_tile": [i],
            "test_last": [ip, ip],
        },
        "frpoly": {
            "eval_device": [i, i, vp, vp, sz, sz, u8p, u32, vp],
            "divide_device": [i, i, vp, vp, vp, sz, sz, u8p, u32, vp],
            "dot_device": [i, i, vp, vp, vp, sz, sz, u32, vp],
            "combine_device": [i, i, vp, vp, vp, sz, sz, u8p, u32],
            "powers_device": [i, i, vp, vp, sz, u8p, u8p, u32],
            "eval": [i, i, vp, sz, sz, u8p, u32, vp],
            "divide": [i, i, vp, vp, sz, sz, u8p, u32, vp],
            "dot": [i, i, vp, vp, sz, sz, u32, vp],
            "combine": [i, i, vp, vp, sz, sz, u8p, u32],
            "powers": [i, i, vp, sz, u8p, u8p, u32],
            "release": [],
            "test_tile": [i],
            "test_last": [ip, ip],
        },
        "frmle": {
            "fold_device": [i, i, vp, vp, vp, sz, sz, sz, u8p, u32],
            "eval_device": [i, i, vp, vp, sz, sz, sz, u8p, u32, vp],
            "eq_device": [i, i, vp, vp, sz, u8p, u8p, u32],
            "round_device": [i, i, vp, vp, sz, sz, sz, mle, sz, u8p, u32, vp],
            "fold": [i, i, vp, vp, sz, sz, sz, u8p, u32],
            "eval": [i, i, vp, sz, sz, sz, u8p, u32, vp],
            "eq": [i, i, vp, sz, u8p, u8p, u32],
            "round": [i, i, vp, sz, sz, sz, mle, sz, u8p, u32, vp],
            "release": [],
            "test_tile": [i],
            "test_last": [ip, ip],
        },
        "frmat": {
            "create": [i, i, sz, sz, sz, vp, vp, vp, u32, vpp],
            "info": [vp, szp, szp, szp, u32p],
            "destroy": [vp],
            "mul_device": [vp, vp, vp, sz, vp, sz, u32],
            "mul": [vp, vp, sz, vp, sz, u32],
            "release": [],
            "test_tile": [i],
            "test_last": [ip, ip],
        },
        "frgate": {
            "apply_device": [i, i, vp, vp, vp, sz, sz, sz, gate, sz, sz, vp, sz, u32],
            "apply": [i, i, vp, vp, sz, sz, sz, gate, sz, sz, vp, sz, u32],
            "release": [],
        },
        "frlook": {
            "create_device": [i, i, vp, vp, sz, u32, vpp],
            "create": [i, i, vp, sz, u32, vpp],
            "info": [vp, szp, szp, u32p],
            "destroy": [vp],
            "count_device": [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, u64p, u64p],
            "count": [vp, vp, vp, vp, vp, sz, sz, sz, u32, u64p, u64p],
            "release": [],
            "test_hash_bits": [i],
        },
        "frhash": {
            "create": [i, i, u32, u32, u32, u32, vp, vp, u32, vpp],
            "info": [vp, u32p, u32p, u32p],
            "destroy": [vp],
            "permute_device": [vp, vp, vp, vp, sz, u32],
            "permute": [vp, vp, vp, sz, u32],
            "hash_device": [vp, vp, vp, vp, sz, sz, sz, vp, u32, u32, u32],
            "hash": [vp, vp, vp, sz, sz, sz, vp, u32, u32, u32],
            "merkle_device": [vp, vp, vp, vp, sz, vp, u32, u32, u32],
            "merkle": [vp, vp, vp, sz, vp, u32, u32, u32],
            "release": [],
            "test_tile": [i],
        },
    }


# library -> function, by its name behind msm_<library>_ -> argument types (release and destroy return nothing, the others an int).  A
# <fn>_device takes what <fn> takes plus the stream: behind (curve, device), or behind the handle in frmat, frlook and frhash
FR_ABI = _abi()
_fr_libs = {}  # the scalar-field libraries loaded so far, by their name in msm-webgpu_amd/build.py's FR_LIBRARIES


def _load_fr(name):
    """Load libmsm_<name>.so (in-tree), once, with the argument types of FR_ABI[name].  Raises if the library has not been built -- there is no
    fallback path."""
    if name not in _fr_libs:
        so = _build.FR_LIBRARIES[name].so
        if not os.path.exists(so):
            raise ImportError("libmsm_%s.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % (name, so))
        L = C.CDLL(so)
        getattr(L, "msm_%s_abi_version" % name).restype = C.c_int
        for fn, argtypes in FR_ABI[name].items():
            f = getattr(L, "msm_%s_%s" % (name, fn))
            f.argtypes = argtypes
            if fn in ("release", "destroy"):
                f.restype = None
        _fr_libs[name] = L
    return _fr_libs[name]


def fr_lib():
    """Load libmsm_fr.so (in-tree; include/msm_fr.h): the scalar-field NTT.  Raises if it has not been built -- there is no fallback path."""
    return _load_fr("fr")


def frvec_lib():
    """Load libmsm_frvec.so (in-tree; include/msm_frvec.h): vector arithmetic over the scalar field.  Raises if it has not been built -- there is no
    fallback path."""
    return _load_fr("frvec")


def frpoly_lib():
    """Load libmsm_frpoly.so (in-tree; include/msm_frpoly.h): polynomial opening over the scalar field.  Raises if it has not been built -- there is
    no fallback path."""
    return _load_fr("frpoly")


def frmle_lib():
    """Load libmsm_frmle.so (in-tree; include/msm_frmle.h): the sumcheck over multilinear tables of the scalar field.  Raises if it has not been built
    -- there is no fallback path."""
    return _load_fr("frmle")


def frmat_lib():
    """Load libmsm_frmat.so (in-tree; include/msm_frmat.h): sparse matrix-vector products over the scalar field.  Raises if it has not been built
    (msm-webgpu_amd/build.py builds it beside the other five)."""
    return _load_fr("frmat")


def frgate_lib():
    """Load libmsm_frgate.so (in-tree; include/msm_frgate.h): constraint evaluation over rotated rows of the scalar field.  Raises if it has not been
    built (msm-webgpu_amd/build.py builds it beside the other six)."""
    return _load_fr("frgate")


def frlook_lib():
    """Load libmsm_frlook.so (in-tree; include/msm_frlook.h): lookup arguments over the scalar field -- multiplicities and table indices.  Raises
    if it has not been built (msm-webgpu_amd/build.py builds it beside the other seven)."""
    return _load_fr("frlook")


def frhash_lib():
    """Load libmsm_frhash.so (in-tree; include/msm_frhash.h): Poseidon and Poseidon2 over the scalar field -- batch permutations, sponges, Merkle trees.  Raises
    if it has not been built (msm-webgpu_amd/build.py builds it beside the other eight)."""
    return _load_fr("frhash")


lib_frlook, lib_frhash = frlook_lib, frhash_lib


def _fr(name, fn):
    """(msm_<name>_<fn> of libmsm_<name>.so, its name).  The library comes through its named loader above, looked up at the moment of the call:
    a test that replaces scalars.<name>_lib traps every call into that library."""
    where = "msm_%s_%s" % (name, fn)
    return getattr(globals()[name + "_lib"](), where), where


def _hook(name, fn, *args):
    """a test hook, release or destroy of a library, through _check (the two that return nothing count as 0)"""
    f, where = _fr(name, fn)
    _check(f(*args) or 0, where)


def _last(name):
    """the two ints of msm_<name>_test_last"""
    v = [C.c_int(), C.c_int()]
    _hook(name, "test_last", *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def fr_test_pass_bits(bits=0):
    """test hook msm_fr_test_pass_bits: cap the radix-2 levels of a pass of the scalar-field NTT at `bits` (0: the design's 10)"""
    _hook("fr", "test_pass_bits", int(bits))


def fr_last():
    """(passes, widest pass's levels) of the last scalar-field NTT of this process (test hook msm_fr_test_last)"""
    return _last("fr")


def fr_release():
    """msm_fr_release: free the scalar-field NTT's cached twiddles and scratch (they come back with the next call)"""
    _hook("fr", "release")


def frvec_test_tile(elements=0):
    """test hook msm_frvec_test_tile: shrink the tile of scalars_inverse and scalars_scan to `elements` (0: the design's 1024)"""
    _hook("frvec", "test_tile", int(elements))


def frvec_last():
    """(kernel launches, levels) of the last vector call of this process (test hook msm_frvec_test_last)"""
    return _last("frvec")


def frvec_release():
    """msm_frvec_release: free the vector library's scratch and staging buffers (they come back with the next call)"""
    _hook("frvec", "release")


def frpoly_test_tile(elements=0):
    """test hook msm_frpoly_test_tile: shrink the tile of scalars_eval, scalars_divide and scalars_dot to `elements` (0: the design's 1024)"""
    _hook("frpoly", "test_tile", int(elements))


def frpoly_last():
    """(kernel launches, levels) of the last opening call of this process (test hook msm_frpoly_test_last)"""
    return _last("frpoly")


def frpoly_release():
    """msm_frpoly_release: free the opening library's scratch, constants and staging buffers (they come back with the next call)"""
    _hook("frpoly", "release")


def frmle_test_tile(elements=0):
    """test hook msm_frmle_test_tile: shrink the tile of scalars_mle_eval and scalars_sumcheck_round to `elements` (0: the design's 1024)"""
    _hook("frmle", "test_tile", int(elements))


def frmle_last():
    """(kernel launches, levels) of the last sumcheck call of this process (test hook msm_frmle_test_last)"""
    return _last("frmle")


def frmle_release():
    """msm_frmle_release: free the sumcheck library's scratch, constants and staging buffers (they come back with the next call)"""
    _hook("frmle", "release")


def frmat_test_tile(entries=0):
    """test hook msm_frmat_test_tile: the matrices created from now on use tiles of `entries` entries (0: the design's 1024)"""
    _hook("frmat", "test_tile", int(entries))


def frmat_last():
    """(kernel launches, levels) of the last sparse product of this process (test hook msm_frmat_test_last)"""
    return _last("frmat")


def frmat_release():
    """msm_frmat_release: free the sparse-product library's staging buffers (they come back with the next call); the matrices stay"""
    _hook("frmat", "release")


def frgate_release():
    """msm_frgate_release: free the constraint-evaluation library's constants and staging buffers (they come back with the next call)"""
    _hook("frgate", "release")


def frlook_test_hash_bits(bits=0):
    """test hook msm_frlook_test_hash_bits: the tables created from now on keep only the low `bits` of the hash (0: the design's 32)"""
    _hook("frlook", "test_hash_bits", int(bits))


def frlook_release():
    """msm_frlook_release: free the lookup library's staging buffers (they come back with the next call); the tables stay"""
    _hook("frlook", "release")


def frhash_test_tile(lanes=0):
    """test hook msm_frhash_test_tile: only the first `lanes` lanes of a workgroup take a permutation (0: the design's 64)"""
    _hook("frhash", "test_tile", int(lanes))


def frhash_release():
    """msm_frhash_release: free the hashing library's staging buffers (they come back with the next call); the handles stay"""
    _hook("frhash", "release")


class _FrHandle:
    """What a library's create returned, resident on one device: _h, freed by close() -- msm_<_library>_destroy --, by collecting the object or
    by leaving a `with` block"""
    _library = None

    def close(self):
        if self._h:
            _hook(self._library, "destroy", self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrLookup(_FrHandle):
    """A lookup table over a scalar field, resident on one device (msm_frlook_create_device, include/msm_frlook.h): MsmContext.lookup_table makes
    it, MsmContext.scalars_multiplicities and MsmContext.logup count into it.  n: its entries; distinct: how many different values they hold;
    mont256: the form its keys were stored in.  close() frees it; so does collecting it or leaving a `with` block."""
    _library = "frlook"

    def __init__(self, handle, curve, device, n, distinct, mont256):
        self._h, self.curve, self.device = handle, curve, device
        self.n, self.distinct, self.mont256 = n, distinct, mont256


# the partial rounds of the alpha = 5, 128-bit column of the Poseidon paper's round-number table for R_F = 8, t = 2 .. 12 (circomlib's)
POSEIDON_PARTIAL_ROUNDS = {2: 56, 3: 57, 4: 56, 5: 60, 6: 60, 7: 63, 8: 64, 9: 63, 10: 60, 11: 66, 12: 60}


def poseidon_parameters(curve, t, full_rounds=8, partial_rounds=None):
    """(round_constants, mds) of a Poseidon permutation of width t over a curve's scalar field, as lists of integers: (full_rounds +
    partial_rounds) * t round constants and the t rows of the matrix, by the Poseidon paper's generator -- an 80-bit Grain LFSR seeded with
    the field's bit length, t and the round numbers; round constants rejected where they are not below r; the matrix 1 / (x_i + y_j) of
    2 t values reduced mod r.  partial_rounds=None: POSEIDON_PARTIAL_ROUNDS[t].  For BN254 these are circomlib's constants.  It does NOT
    run the paper's subspace-trail checks on the matrix (the reference script redraws a matrix that fails them): the caller vouches for
    parameters outside the published sets.  Pure Python, remembered."""
    t, full_rounds = int(t), int(full_rounds)
    if curve not in SCALAR_FIELDS:
        raise ValueError("no scalar field for %s" % (curve,))
    if not 2 <= t <= 12 or full_rounds % 2 or not 2 <= full_rounds <= 16:
        raise ValueError("a permutation has 2 <= t <= 12 and an even 2 <= full_rounds <= 16")
    partial_rounds = POSEIDON_PARTIAL_ROUNDS[t] if partial_rounds is None else int(partial_rounds)
    if not 0 <= partial_rounds <= 128:
        raise ValueError("a permutation has 0 .. 128 partial rounds")
    rc, mds = _poseidon_parameters(SCALAR_FIELDS[curve], t, full_rounds, partial_rounds)
    return list(rc), [list(row) for row in mds]


@functools.lru_cache(maxsize=None)
def _poseidon_parameters(r, t, full_rounds, partial_rounds):
    n = r.bit_length()
    state = 0  # bit 79 is b[0], the oldest
    for value, width in ((1, 2), (0, 4), (n, 12), (t, 12), (full_rounds, 10), (partial_rounds, 10), ((1 << 30) - 1, 30)):
        state = state << width | value

    def step():
        nonlocal state
        b = (state >> 17 ^ state >> 28 ^ state >> 41 ^ state >> 56 ^ state >> 66 ^ state >> 79) & 1  # b[62] ^ b[51] ^ b[38] ^ b[23] ^ b[13] ^ b[0]
        state = (state << 1 | b) & ((1 << 80) - 1)
        return b

    for _ in range(160):
        step()

    def draw():
        v = got = 0
        while got < n:
            if step():  # of every pair, the second bit where the first is 1
                v = v << 1 | step()
                got += 1
            else:
                step()
        return v

    rc = []
    while len(rc) < (full_rounds + partial_rounds) * t:
        v = draw()
        if v < r:
            rc.append(v)
    while True:
        xy = [draw() % r for _ in range(2 * t)]
        if len(set(xy)) == 2 * t:
            break
    return tuple(rc), tuple(tuple(pow(xy[i] + xy[t + j], r - 2, r) for j in range(t)) for i in range(t))


class FrHash(_FrHandle):
    """A Poseidon or Poseidon2 permutation over a scalar field (msm_frhash_create, include/msm_frhash.h): MsmContext.poseidon or
    MsmContext.poseidon2 makes it, MsmContext.scalars_permute, scalars_hash, merkle_tree and merkle_path use it.  kind: "poseidon" or
    "poseidon2"; t, full_rounds, partial_rounds: its shape; arity = t - 1; capacity, capacity_at, out_at: the sponge's convention, remembered
    for the calls.  close() frees it; so does collecting it or leaving a `with` block."""
    _library = "frhash"

    def __init__(self, handle, curve, device, t, full_rounds, partial_rounds, capacity, capacity_at, out_at, kind="poseidon"):
        self._h, self.curve, self.device, self.kind = handle, curve, device, kind
        self.t, self.full_rounds, self.partial_rounds, self.arity = t, full_rounds, partial_rounds, t - 1
        self.capacity, self.capacity_at, self.out_at = capacity, capacity_at, out_at


class FrMatrix(_FrHandle):
    """A sparse matrix over a scalar field, resident on one device (msm_frmat_create, include/msm_frmat.h): MsmContext.scalars_matrix makes it,
    MsmContext.scalars_matvec multiplies by it.  close() frees it; so does collecting it."""
    _library = "frmat"

    def __init__(self, handle, curve, device, rows, cols, nnz, has_transpose):
        self._h, self.curve, self.device = handle, curve, device
        self.rows, self.cols, self.nnz, self.has_transpose = rows, cols, nnz, has_transpose


# ------------------------------------------------------------------------------------------------ what the wrappers hand to C
def _in(b):
    """host bytes as the void* of an input; None stays None"""
    return C.cast(C.c_char_p(b), C.c_void_p) if b is not None else None


def _ptr(t, b=None):
    """an operand for C: the address of a device tensor, or host bytes (_in) where there is none"""
    return t.data_ptr() if t is not None else _in(b)


def _host_out(n, init=None):
    """a host output of n x 32 bytes -- init: the bytes it holds before the call, and its size -- -> (the buffer, its void*)"""
    buf = C.create_string_buffer(32 * n) if init is None else C.create_string_buffer(init, len(init))
    return buf, C.cast(buf, C.c_void_p)


def _dest(a, out, n, init=None):
    """Where a call writes -> (what the wrapper then returns through _result, its address for C): in place into the device tensor a unless
    `out` is given; for host bytes (a is None) a new buffer (_host_out)."""
    if a is None:
        return _host_out(n, init)
    dst = a if out is None else out
    return dst, dst.data_ptr()


def _result(res):
    """a device tensor as it is, a host buffer's bytes"""
    return res.raw if isinstance(res, C.Array) else res


def _const32(v, r, name):
    """an integer in [0, r) or its 32 little-endian bytes -> its 32 little-endian bytes"""
    k = int.from_bytes(v, "little") if isinstance(v, (bytes, bytearray)) else int(v)
    if isinstance(v, (bytes, bytearray)) and len(v) != 32:
        raise ValueError("%s must be an integer or its 32 little-endian bytes" % name)
    if not 0 <= k < r:
        raise ValueError("%s must lie in [0, r)" % name)
    return k.to_bytes(32, "little")


def _scalars32(values):
    return b"".join(c.to_bytes(32, "little") for c in values)


def _pack_terms(terms, batch, r, Term, what, max_terms, max_degree):
    """[(coeff, (factor, ..)), ..] -> (array of Term, the largest degree).  A factor is a row number or, where Term has rotations (FrgateTerm),
    (row, rotation)."""
    terms = list(terms)
    if not 1 <= len(terms) <= max_terms:
        raise ValueError("a %s takes 1 .. %d terms, not %d" % (what, max_terms, len(terms)))
    rotated = hasattr(Term, "rots")
    arr = (Term * len(terms))()
    top = 0
    for t, (coeff, factors) in zip(arr, terms):
        if rotated:
            factors = [(int(f), 0) if isinstance(f, (int, np.integer)) else (int(f[0]), int(f[1])) for f in factors]
        else:
            factors = [(int(f), 0) for f in factors]
        if not 1 <= len(factors) <= max_degree:
            raise ValueError("a term has 1 .. %d factors, not %d" % (max_degree, len(factors)))
        if any(not 0 <= row < batch for row, _ in factors):
            raise ValueError("a term names a row outside the %d rows" % batch)
        if any(not -2 ** 31 <= rot < 2 ** 31 for _, rot in factors):
            raise ValueError("a rotation is a signed 32-bit integer")
        t.coeff[:] = _const32(coeff, r, "a coefficient")
        t.degree = len(factors)
        t.rows[:len(factors)] = [row for row, _ in factors]
        if rotated:
            t.rots[:len(factors)] = [rot for _, rot in factors]
        top = max(top, len(factors))
    return arr, top


class ScalarFieldOps:
    """The scalar-field methods of a context: scalars_*, the provers built on them, hashing.  A mixin; the class it is mixed into provides
        curve, curve_id, device      the curve's name, its id in the C ABI, the device's index
        _h                           the handle of the libmsm_hip context whose stream the device calls run on
        scalar_width, scalar_mont256 the scalar format: 32 bytes wide is the only one taken here; canonical or s * 2^256 mod r
        _order_after_torch(*tensors) makes that stream wait for torch's work on the tensors
        msm(scalars)                 the commitment, for kzg_open
    and nothing else of it is used."""

    def _fr_call(self, name, fn, behind, handle, *rest):
        """The one way into a scalar-field library: msm_<name>_<fn>, through _check.  handle: None for a function that begins (curve, device),
        or the FrMatrix / FrLookup / FrHash it begins with.  behind: None for the host form; for operands on the device the tensor whose
        torch stream this context's stream is first ordered behind -- the call is then msm_<name>_<fn>_device, with this context's stream as
        the argument behind (curve, device) or behind the handle."""
        lead = (self.curve_id, self.device) if handle is None else (handle._h,)
        if behind is not None:
            self._order_after_torch(behind)
            lead += (lib().msm_hip_stream(self._h),)
            fn += "_device"
        f, where = _fr(name, fn)
        _check(f(*lead, *rest), where)

    def _scalar_field(self, what, grumpkin=False):
        """r of this context's curve (a G2 context takes its G1's) for a method that takes 32-byte scalars; grumpkin: whether the method's
        library has a unit for Grumpkin's scalar field"""
        if self.curve not in SCALAR_FIELDS or (self.curve == "grumpkin" and not grumpkin):
            raise ValueError("%s is not offered on the scalar field of %s" % (what, self.curve))
        if self.scalar_width != 32:
            raise ValueError("%s takes 32-byte scalars; the context's scalar format is %d bytes wide" % (what, self.scalar_width))
        return SCALAR_FIELDS[self.curve]

    def _mont256_flag(self):
        """MSM_FR_MONT256 = MSM_FRVEC_MONT256 = .. = MSM_FRHASH_MONT256 under the mont256 scalar format, else 0"""
        return self.FR_MONT256 if self.scalar_mont256 else 0

    def _new_out(self, out, n):
        """`out`, checked, or a new tensor of n x 32 bytes on this context's device, for a method that has no device input to take the device from"""
        if out is None:
            return torch.empty((n, 32), dtype=torch.uint8, device="cuda:%d" % self.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * n or not out.is_contiguous():
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes" % n)
        return out

    # -- scalar-field NTT (libmsm_fr.so): coefficients <-> evaluations of the vectors this context commits to
    FR_SCALE_INV_N, FR_MONT256 = 1, 2  # MSM_FR_SCALE_INV_N, MSM_FR_MONT256

    def scalars_fft(self, scalars, log_n=None, omega=None, inverse=False, shift=None, batch=1):
        """The transform of `batch` vectors of n = 2^log_n scalars (msm_fr_ntt_device, include/msm_fr.h), in natural order:
        out[i] = sum_j omega^(i j) (shift^j a[j]) -- the evaluations of the polynomial with coefficients a on the n-th roots of unity (on the coset
        shift * H with `shift`); inverse=True undoes it: omega^-1, 1 / n, and shift^-i afterwards.  scalars: a CUDA uint8 tensor of batch * n * 32
        bytes, transformed IN PLACE on this context's stream and returned -- it can go straight into msm() --, or host bytes (bytes come back).
        log_n: None takes it from the size.  omega: None takes root_of_unity(curve, log_n); an integer or 32 bytes otherwise, a primitive n-th root.
        The scalars are in this context's 32-byte scalar format (set_scalar_format: canonical, or mont256) and must be below r."""
        if self.curve not in SCALAR_FIELDS or self.curve == "grumpkin":
            raise ValueError("the scalar field of %s has no transform (2-adicity 1)" % self.curve)
        r = self._scalar_field("scalars_fft")
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be at least 1")
        t, buf, total = self._frvec_vector(scalars, "scalars")
        if log_n is None:
            n = total // batch
            if total % batch or n == 0 or n & (n - 1):
                raise ValueError("%d scalars are not %d vectors of a power-of-two length" % (total, batch))
            log_n = n.bit_length() - 1
        log_n = int(log_n)
        two_adicity = ((r - 1) & -(r - 1)).bit_length() - 1
        if not 0 <= log_n <= min(two_adicity, FR_MAX_LOG_N):
            raise ValueError("log_n must lie in [0, %d] on %s, not %d" % (min(two_adicity, FR_MAX_LOG_N), self.curve, log_n))
        if total != batch << log_n:
            raise ValueError("%d scalars are not %d vectors of 2^%d" % (total, batch, log_n))
        if omega is None:
            w = root_of_unity(self.curve, log_n)
        else:
            w = int.from_bytes(omega, "little") if isinstance(omega, (bytes, bytearray)) else int(omega)
            if isinstance(omega, (bytes, bytearray)) and len(omega) != 32:
                raise ValueError("omega must be an integer or 32 bytes")
            if not 0 < w < r or (w != 1 if log_n == 0 else pow(w, 1 << (log_n - 1), r) != r - 1):
                raise ValueError("omega is not a primitive 2^%d-th root of unity of the scalar field" % log_n)
        g = None
        if shift is not None:
            g = (int.from_bytes(shift, "little") if isinstance(shift, (bytes, bytearray)) else int(shift)) % r
            if g == 0:
                raise ValueError("shift must be invertible")
        flags = self._mont256_flag()
        pre = post = None
        if inverse:
            w = root_of_unity(self.curve, log_n, inverse=True) if omega is None else pow(w, r - 2, r)
            flags |= self.FR_SCALE_INV_N
            post = pow(g, r - 2, r).to_bytes(32, "little") if g is not None else None
        else:
            pre = g.to_bytes(32, "little") if g is not None else None
        res, dst = _dest(t, None, total, init=buf)  # (always in place: host bytes in a copy)
        self._fr_call("fr", "ntt", t, None, dst, log_n, batch, w.to_bytes(32, "little"), pre, post, flags)
        return _result(res)

    # -- vector arithmetic over the scalar field (libmsm_frvec.so): what lies between a transform and the next commitment
    FRVEC_EXCLUSIVE, FRVEC_MONT256 = 1, 2  # MSM_FRVEC_EXCLUSIVE, MSM_FRVEC_MONT256
    FRVEC_MAX_ELEMENTS = 1 << 26
    _FRVEC_MAPS = {"add": 0, "sub": 1, "mul": 2, "mul_add": 3, "mul_sub": 4}  # MSM_FRVEC_ADD ..
    _FRVEC_SCANS = {"sum": 0, "product": 1}  # MSM_FRVEC_SUM, MSM_FRVEC_PRODUCT

    def _frvec_vector(self, v, name):
        """-> (tensor or None, bytes or None, number of scalars)"""
        if isinstance(v, torch.Tensor) and v.is_cuda:
            t, n = _as_device_u8(v, 32, name)
            return t, None, n
        b = bytes(v)
        if len(b) % 32:
            raise ValueError("%s must be n x 32 bytes" % name)
        return None, b, len(b) // 32

    def _frvec_out(self, out, t, n, on_device):
        if out is None:
            return None
        if not on_device:
            raise TypeError("out is for device vectors; host bytes return bytes")
        if not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or out.numel() != 32 * n or not out.is_contiguous() or out.device != t.device:
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of %d x 32 bytes on %s" % (n, t.device))
        return out

    def _frvec_map(self, op, a, b, c, out):
        r = self._scalar_field("scalars_" + op)
        if op not in self._FRVEC_MAPS:
            raise ValueError("unknown op %r" % (op,))
        ta, ba, n = self._frvec_vector(a, "a")
        on_device = ta is not None
        if n < 1 or n > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("a vector holds 1 .. 2^26 scalars, not %d" % n)
        vecs, consts = [], []
        for name, v in (("b", b), ("c", c)):
            if v is None:  # (an op of two operands has no c)
                vecs.append(None), consts.append(None)
            elif isinstance(v, int) or (isinstance(v, (bytes, bytearray)) and len(v) == 32 and (on_device or n != 1)):
                k = int.from_bytes(v, "little") if isinstance(v, (bytes, bytearray)) else int(v)
                if not 0 <= k < r:
                    raise ValueError("the constant %s must lie in [0, r)" % name)
                vecs.append(None), consts.append(k.to_bytes(32, "little"))
            else:
                tv, bv, m = self._frvec_vector(v, name)
                if (tv is not None) != on_device:
                    raise TypeError("%s must be on the device exactly when a is" % name)
                if m != n:
                    raise ValueError("%s holds %d scalars, a holds %d" % (name, m, n))
                vecs.append(_ptr(tv, bv)), consts.append(None)
        res, dst = _dest(ta, self._frvec_out(out, ta, n, on_device), n)
        self._fr_call("frvec", "map", ta, None, dst, _ptr(ta, ba), vecs[0], vecs[1], n, self._FRVEC_MAPS[op], consts[0], consts[1], self._mont256_flag())
        return _result(res)

    def scalars_add(self, a, b, out=None):
        """a + b, element by element, over this context's scalar field (msm_frvec_map_device, include/msm_frvec.h).  a: a CUDA uint8 tensor of n x 32
        bytes -- the result is written over it (out=None) or into `out`, on this context's stream, and that tensor is returned -- or host bytes
        (bytes come back).  b: a vector like a, or an integer / its 32 little-endian bytes in [0, r), which is broadcast.  The vectors are in this
        context's 32-byte scalar format (canonical, or mont256) and must be below r; a constant is always a plain integer.  (Beside a host vector of ONE scalar, 32 bytes
        are a vector too.)"""
        return self._frvec_map("add", a, b, None, out)

    def scalars_sub(self, a, b, out=None):
        """a - b (as scalars_add)"""
        return self._frvec_map("sub", a, b, None, out)

    def scalars_mul(self, a, b, out=None):
        """a * b (as scalars_add)"""
        return self._frvec_map("mul", a, b, None, out)

    def scalars_mul_add(self, a, b, c, out=None):
        """a * b + c (as scalars_add; c: a vector or a constant, like b)"""
        if c is None:
            raise ValueError("scalars_mul_add needs c")
        return self._frvec_map("mul_add", a, b, c, out)

    def scalars_mul_sub(self, a, b, c, out=None):
        """a * b - c (as scalars_mul_add)"""
        if c is None:
            raise ValueError("scalars_mul_sub needs c")
        return self._frvec_map("mul_sub", a, b, c, out)

    def scalars_inverse(self, a, out=None):
        """1 / a element by element, 1 / 0 = 0 (msm_frvec_inverse_device): Montgomery's trick on the device, with one Fermat inversion per call.
        a, out: as scalars_add."""
        self._scalar_field("scalars_inverse")
        ta, ba, n = self._frvec_vector(a, "a")
        if n < 1 or n > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("a vector holds 1 .. 2^26 scalars, not %d" % n)
        res, dst = _dest(ta, self._frvec_out(out, ta, n, ta is not None), n)
        self._fr_call("frvec", "inverse", ta, None, dst, _ptr(ta, ba), n, self._mont256_flag())
        return _result(res)

    def scalars_scan(self, a, op="product", exclusive=False, batch=1, out=None, totals=False):
        """Running products (op="product") or sums (op="sum") along each of `batch` rows of a (msm_frvec_scan_device): out[i] = a[0] o .. o a[i];
        exclusive=True: a[0] o .. o a[i - 1], and out[0] is 1 (0 for sums).  a, out: as scalars_add.  totals=True: returns (result, totals) with
        every row's total -- what an exclusive scan does not store, e.g. the closing value of a grand product -- as batch x 32 host bytes."""
        self._scalar_field("scalars_scan")
        if op not in self._FRVEC_SCANS:
            raise ValueError("op must be \"sum\" or \"product\", not %r" % (op,))
        ta, ba, n = self._frpoly_rows(a, batch)
        batch = int(batch)
        res, dst = _dest(ta, self._frvec_out(out, ta, n * batch, ta is not None), n * batch)
        flags = self._mont256_flag() | (self.FRVEC_EXCLUSIVE if exclusive else 0)
        tot, tot_ptr = _host_out(batch) if totals else (None, None)
        self._fr_call("frvec", "scan", ta, None, dst, _ptr(ta, ba), n, batch, self._FRVEC_SCANS[op], flags, tot_ptr)
        return (_result(res), tot.raw) if totals else _result(res)

    # -- polynomial opening over the scalar field (libmsm_frpoly.so): what follows the last commitment
    FRPOLY_SHARED_B, FRPOLY_MONT256, FRPOLY_MAX_ROWS = 1, 2, 256  # MSM_FRPOLY_SHARED_B, MSM_FRPOLY_MONT256, MSM_FRPOLY_MAX_ROWS

    def _frpoly_rows(self, a, batch, name="a"):
        """-> (tensor or None, bytes or None, scalars per row)"""
        batch = int(batch)
        ta, ba, total = self._frvec_vector(a, name)
        if batch < 1 or total < 1 or total % batch or total > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        return ta, ba, total // batch

    def scalars_eval(self, a, z, batch=1):
        """The values a(z) = sum_j a[j] z^j of `batch` polynomials given by their coefficients, one row of a each (msm_frpoly_eval_device,
        include/msm_frpoly.h) -> batch x 32 host bytes in the data's form.  a: a CUDA uint8 tensor of batch x n x 32 bytes, or host bytes, in this
        context's 32-byte scalar format; z: an integer in [0, r) or its 32 little-endian bytes, always a plain integer."""
        r = self._scalar_field("scalars_eval")
        ta, ba, n = self._frpoly_rows(a, batch)
        zb = _const32(z, r, "z")
        values, values_ptr = _host_out(int(batch))
        self._fr_call("frpoly", "eval", ta, None, _ptr(ta, ba), n, int(batch), zb, self._mont256_flag(), values_ptr)
        return values.raw

    def scalars_divide(self, a, z, batch=1, out=None, values=False):
        """(a(X) - a(z)) / (X - z) for every row of a, by synthetic division (msm_frpoly_divide_device): out[i] = sum_{j > i} a[j] z^(j - i - 1), kept
        at the length of a (the last coefficient is 0).  a, out: as scalars_add -- in place on a device tensor unless `out` is given; z, batch: as
        scalars_eval.  values=True: returns (quotients, values) with every a(z) as batch x 32 host bytes."""
        r = self._scalar_field("scalars_divide")
        ta, ba, n = self._frpoly_rows(a, batch)
        batch = int(batch)
        zb = _const32(z, r, "z")
        res, dst = _dest(ta, self._frvec_out(out, ta, n * batch, ta is not None), n * batch)
        vals, vals_ptr = _host_out(batch) if values else (None, None)
        self._fr_call("frpoly", "divide", ta, None, dst, _ptr(ta, ba), n, batch, zb, self._mont256_flag(), vals_ptr)
        return (_result(res), vals.raw) if values else _result(res)

    def scalars_dot(self, a, b, batch=1):
        """sum_j a[row][j] b[row][j] for every row of a (msm_frpoly_dot_device) -> batch x 32 host bytes in the data's form.  b: as many scalars as
        a, or -- beside batch > 1 -- one row of n scalars that is used for every row of a.  a and b are both device tensors or both host bytes."""
        self._scalar_field("scalars_dot")
        ta, ba, n = self._frpoly_rows(a, batch)
        batch = int(batch)
        tb, bb, m = self._frvec_vector(b, "b")
        if (tb is not None) != (ta is not None):
            raise TypeError("b must be on the device exactly when a is")
        if m != n * batch and m != n:
            raise ValueError("b holds %d scalars; a holds %d rows of %d" % (m, batch, n))
        flags = self._mont256_flag() | (self.FRPOLY_SHARED_B if m == n and batch > 1 else 0)
        values, values_ptr = _host_out(batch)
        self._fr_call("frpoly", "dot", ta, None, _ptr(ta, ba), _ptr(tb, bb), n, batch, flags, values_ptr)
        return values.raw

    def scalars_combine(self, a, coeffs, out=None):
        """out[i] = sum_k coeffs[k] a[k][i]: the linear combination of the len(coeffs) rows of a (msm_frpoly_combine_device), e.g. the fold of the
        polynomials of a batched opening with powers of a challenge.  coeffs: 1 .. 256 integers in [0, r) (or their 32-byte encodings).  a: a CUDA
        uint8 tensor of len(coeffs) x n x 32 bytes -- the n scalars of the result go into `out` (a CUDA uint8 tensor, which may be row 0 of a) or
        a new tensor -- or host bytes (bytes come back)."""
        r = self._scalar_field("scalars_combine")
        coeffs = list(coeffs)
        if not 1 <= len(coeffs) <= self.FRPOLY_MAX_ROWS:
            raise ValueError("a combination takes 1 .. %d rows, not %d" % (self.FRPOLY_MAX_ROWS, len(coeffs)))
        ta, ba, n = self._frpoly_rows(a, len(coeffs))
        cb = b"".join(_const32(c, r, "a coefficient") for c in coeffs)
        out = self._frvec_out(out, ta, n, ta is not None)
        if ta is not None and out is None:
            out = torch.empty((n, 32), dtype=torch.uint8, device=ta.device)
        res, dst = _dest(out, None, n)
        self._fr_call("frpoly", "combine", ta, None, dst, _ptr(ta, ba), n, len(coeffs), cb, self._mont256_flag())
        return _result(res)

    def scalars_powers(self, g, n, scale=1, out=None):
        """scale * g^i for i < n as a CUDA uint8 tensor of n x 32 bytes in this context's scalar format (msm_frpoly_powers_device): the powers of a
        challenge, or the evaluation domain from a root of unity.  g, scale: integers in [0, r) or their 32 little-endian bytes."""
        r = self._scalar_field("scalars_powers")
        n = int(n)
        if n < 1 or n > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("a vector holds 1 .. 2^26 scalars, not %d" % n)
        gb, cb = _const32(g, r, "g"), _const32(scale, r, "scale")
        out = self._new_out(out, n)
        self._fr_call("frpoly", "powers", out, None, out.data_ptr(), n, gb, cb, self._mont256_flag())
        return out

    def kzg_open(self, coeffs, z):
        """A KZG opening of the polynomial with the coefficients `coeffs` (a CUDA uint8 tensor of n x 32 bytes, n <= the resident bases, or host
        bytes) at z over the resident monomial bases tau^j G: -> (y, W) with y = f(z) as 32 bytes in the data's form and W the commitment (G1) to
        (f - y) / (X - z).  scalars_divide into a fresh tensor, then msm."""
        if isinstance(coeffs, torch.Tensor) and coeffs.is_cuda:
            q, y = self.scalars_divide(coeffs, z, out=torch.empty_like(coeffs), values=True)
        else:
            q, y = self.scalars_divide(coeffs, z, values=True)
        return y, self.msm(q)

    # -- the sumcheck over multilinear tables of the scalar field (libmsm_frmle.so): the loop between the commitments of a Nova / Spartan /
    # HyperPlonk-style prover.  The FIRST variable of a table is the TOP bit of its index (include/msm_frmle.h).  Every curve's scalar field,
    # Grumpkin's included, from here on.
    FRMLE_MONT256, FRMLE_MAX_DEGREE, FRMLE_MAX_TERMS, FRMLE_MAX_ROWS = 2, 4, 8, 16  # MSM_FRMLE_MONT256, MSM_FRMLE_MAX_DEGREE, ..

    def _frmle_rows(self, a, batch, n, least):
        """-> (tensor or None, bytes or None, n, stride): `batch` rows, stride = scalars / batch apart, of which the first n (default: all) are the table"""
        ta, ba, stride = self._frpoly_rows(a, batch)
        n = stride if n is None else int(n)
        if n < least or n > stride or n & (n - 1):
            raise ValueError("a table holds a power of two of scalars, at least %d and at most the %d of a row, not %d" % (least, stride, n))
        return ta, ba, n, stride

    def scalars_mle_fold(self, a, c, batch=1, n=None, out=None):
        """Bind the top variable of `batch` multilinear tables to c (msm_frmle_fold_device, include/msm_frmle.h): row[i] = row[i] + c (row[i + n/2] -
        row[i]) for i < n / 2.  a: a CUDA uint8 tensor of batch x N x 32 bytes -- folded in place, or into `out` (same size; only the first n / 2
        scalars of every row are written) -- or host bytes (bytes of the same layout come back).  n: the table's length, a power of two <= N
        (default N): a sumcheck keeps halving n in one buffer.  c: an integer in [0, r) or its 32 little-endian bytes, always a plain integer."""
        r = self._scalar_field("scalars_mle_fold", grumpkin=True)
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 2)
        batch = int(batch)
        cb = _const32(c, r, "c")
        res, dst = _dest(ta, self._frvec_out(out, ta, stride * batch, ta is not None), stride * batch, init=ba)
        self._fr_call("frmle", "fold", ta, None, dst, _ptr(ta, ba), n, batch, stride, cb, self._mont256_flag())
        return _result(res)

    def scalars_mle_eval(self, a, point, batch=1, n=None):
        """The multilinear extensions of `batch` tables at `point` (msm_frmle_eval_device) -> batch x 32 host bytes in the data's form.  point:
        log2(n) integers in [0, r) (or their 32-byte encodings); point[0] is the variable at the TOP bit of the index -- a table indexed with x_0 at
        the lowest bit passes its point reversed.  a, batch, n: as scalars_mle_fold; nothing is written."""
        r = self._scalar_field("scalars_mle_eval", grumpkin=True)
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 1)
        batch = int(batch)
        point = list(point)
        if len(point) != n.bit_length() - 1:
            raise ValueError("a table of %d scalars has %d variables, the point %d" % (n, n.bit_length() - 1, len(point)))
        pb = b"".join(_const32(z, r, "a coordinate of the point") for z in point)
        values, values_ptr = _host_out(batch)
        self._fr_call("frmle", "eval", ta, None, _ptr(ta, ba), n, batch, stride, pb, self._mont256_flag(), values_ptr)
        return values.raw

    def scalars_eq(self, point, scale=1, out=None):
        """The table of scale * eq(point, .) over {0, 1}^k, k = len(point), as a CUDA uint8 tensor of 2^k x 32 bytes in this context's scalar format
        (msm_frmle_eq_device): out[i] = scale prod_j (bit_(k-1-j)(i) ? point[j] : 1 - point[j]).  point, scale: integers in [0, r) or their 32
        little-endian bytes."""
        r = self._scalar_field("scalars_eq", grumpkin=True)
        point = list(point)
        if len(point) > 26:
            raise ValueError("a table holds at most 2^26 scalars, not 2^%d" % len(point))
        n = 1 << len(point)
        pb = b"".join(_const32(z, r, "a coordinate of the point") for z in point)
        cb = _const32(scale, r, "scale")
        out = self._new_out(out, n)
        self._fr_call("frmle", "eq", out, None, out.data_ptr(), n, pb, cb, self._mont256_flag())
        return out

    def scalars_sumcheck_round(self, a, terms, batch=1, n=None, fold=None):
        """The values g(0) .. g(D) of a sumcheck round polynomial over `batch` multilinear tables (msm_frmle_round_device) -> (D + 1) x 32 host bytes
        in the data's form: g(t) = sum_{i < n/2} sum_terms coeff prod_f (row_f[i] + t (row_f[i + n/2] - row_f[i])), D the largest degree.  terms:
        1 .. 8 pairs (coeff, (row, ..)) of a plain integer coefficient and 1 .. 4 row numbers (a row may repeat); batch <= 16.  fold: None, or the
        previous round's challenge -- the call then first binds the top variable of ALL rows to it, in place (as scalars_mle_fold, n >= 4), and
        returns the round values of the folded tables, of n / 2 scalars: one pass over the data per round.  a, n: as scalars_mle_fold; host bytes
        with fold return (values, the folded bytes)."""
        r = self._scalar_field("scalars_sumcheck_round", grumpkin=True)
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 2 if fold is None else 4)
        batch = int(batch)
        if batch > self.FRMLE_MAX_ROWS:
            raise ValueError("a round takes at most %d rows, not %d" % (self.FRMLE_MAX_ROWS, batch))
        arr, top = _pack_terms(terms, batch, r, FrmleTerm, "round", self.FRMLE_MAX_TERMS, self.FRMLE_MAX_DEGREE)
        fb = None if fold is None else _const32(fold, r, "fold")
        values, values_ptr = _host_out(self.FRMLE_MAX_DEGREE + 1)
        res, dst = _dest(ta, None, stride * batch, init=ba)  # (the host form reads and, with fold, writes a copy of the bytes)
        self._fr_call("frmle", "round", ta, None, dst, n, batch, stride, arr, len(arr), fb, self._mont256_flag(), values_ptr)
        got = values.raw[:32 * (top + 1)]
        return got if ta is not None or fold is None else (got, res.raw)

    def sumcheck_prove(self, a, terms, batch, challenge):
        """The prover's side of a sumcheck of sum_x sum_terms coeff prod_f row_f[x] over `batch` tables of N = 2^k scalars (a: a CUDA uint8 tensor of
        batch x N x 32 bytes, DESTROYED: the rounds run in place), the counterpart of kzg_open: round j's values go to challenge(j, values) -- values:
        (D + 1) x 32 bytes in the data's form --, which returns the verifier's challenge, an integer in [0, r); every round after the first binds
        the previous challenge in the same pass (scalars_sumcheck_round with fold).  -> (the k rounds' values, the k challenges, every row's value
        at that point as batch x 32 bytes)."""
        r = self._scalar_field("sumcheck_prove", grumpkin=True)
        if not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise TypeError("sumcheck_prove runs in place on a CUDA(HIP) uint8 tensor")
        _, _, n, _ = self._frmle_rows(a, batch, None, 1)
        rounds, point = [], []
        while n >> len(point) > 1:
            j = len(point)
            values = self.scalars_sumcheck_round(a, terms, batch, n >> max(j - 1, 0), fold=point[-1] if j else None)
            c = int(challenge(j, values))
            if not 0 <= c < r:
                raise ValueError("challenge %d is not in [0, r)" % j)
            rounds.append(values)
            point.append(c)
        # the last challenge binds what is left of every row: two scalars, or -- N = 1 -- the row itself
        finals = self.scalars_mle_eval(a, point[-1:], batch, 2 if point else 1)
        return rounds, point, finals

    # -- sparse matrix-vector products over the scalar field (libmsm_frmat.so): the rows Az, Bz, Cz of an R1CS, between the commitment to the
    # witness (msm) and the sumcheck (sumcheck_prove)
    FRMAT_MONT256, FRMAT_WITH_TRANSPOSE, FRMAT_TRANSPOSE = 2, 4, 8  # MSM_FRMAT_MONT256, ..
    FRMAT_MAX_DIM, FRMAT_MAX_NNZ = 1 << 26, 1 << 28

    @staticmethod
    def _frmat_indices(v, name, bound):
        """any integer sequence, numpy array or CPU tensor -> a contiguous uint32 array; a negative or too large index raises"""
        if isinstance(v, torch.Tensor):
            if v.is_cuda:
                raise TypeError("%s comes from host memory" % name)
            v = v.numpy()
        a = np.asarray(v)
        if a.size == 0:
            return np.zeros(0, dtype=np.uint32)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError("%s must be a flat sequence of integers" % name)
        if int(a.min()) < 0 or int(a.max()) > bound:
            raise ValueError("%s holds an index outside [0, %d]" % (name, bound))
        return np.ascontiguousarray(a, dtype=np.uint32)

    def scalars_matrix(self, rows, cols, row_ptr, col_idx, values, transpose=False):
        """A rows x cols sparse matrix over this context's scalar field in CSR form -> FrMatrix (msm_frmat_create, include/msm_frmat.h), checked
        here on the host and resident on this context's device from its first product on.  row_ptr: rows + 1 integers from 0 to nnz, never
        decreasing; col_idx: nnz columns below cols, in any order within a row, repeats adding up; values: nnz integers in [0, r) or nnz x 32
        canonical little-endian bytes -- always plain integers, whatever the context's scalar format.  Indices: any integer sequence, a numpy array
        or a CPU tensor.  transpose=True also keeps the transposed structure, for scalars_matvec(..., transpose=True).  Every curve's scalar
        field, Grumpkin's included; a G2 context takes its G1's."""
        r = self._scalar_field("scalars_matrix", grumpkin=True)
        rows, cols = int(rows), int(cols)
        if not (1 <= rows <= self.FRMAT_MAX_DIM and 1 <= cols <= self.FRMAT_MAX_DIM):
            raise ValueError("a matrix has 1 .. 2^26 rows and columns, not %d x %d" % (rows, cols))
        ptr = self._frmat_indices(row_ptr, "row_ptr", self.FRMAT_MAX_NNZ)
        idx = self._frmat_indices(col_idx, "col_idx", cols - 1)
        nnz = int(idx.size)
        if ptr.size != rows + 1 or int(ptr[0]) != 0 or int(ptr[-1]) != nnz or (rows and bool((ptr[1:] < ptr[:-1]).any())):
            raise ValueError("row_ptr must hold rows + 1 integers from 0 to nnz = %d that never decrease" % nnz)
        if isinstance(values, (bytes, bytearray)):
            vb = bytes(values)
        elif isinstance(values, np.ndarray) and values.dtype == np.uint8:
            vb = values.tobytes()
        else:
            values = [int(v) for v in values]
            if any(not 0 <= v < r for v in values):
                raise ValueError("the values must lie in [0, r)")
            vb = _scalars32(values)
        if len(vb) != 32 * nnz:
            raise ValueError("%d values for %d columns" % (len(vb) // 32, nnz))
        h = C.c_void_p()
        self._fr_call("frmat", "create", None, None, rows, cols, nnz, ptr.ctypes.data, idx.ctypes.data if nnz else None, _in(vb) if nnz else None,
                      self.FRMAT_WITH_TRANSPOSE if transpose else 0, C.byref(h))
        return FrMatrix(h, self.curve, self.device, rows, cols, nnz, bool(transpose))

    def scalars_matvec(self, mat, x, out=None, transpose=False, pad_to=None):
        """y = M x -- transpose=True: M^T x, for a matrix made with transpose=True -- over the scalar field (msm_frmat_mul_device): y[i] = sum_j
        M[i][j] x[j].  x: a CUDA uint8 tensor of cols x 32 bytes (rows x 32 with transpose) in this context's 32-byte scalar format, or host bytes
        (bytes come back).  -> a CUDA uint8 tensor of pad_to x 32 bytes, or `out` (contiguous, that size; a row of a larger buffer will do):
        pad_to defaults to the exact length, and y[length .. pad_to) is zero whatever out held.  An element of x that is not below r raises
        MsmHipError (code -4) where an entry of the matrix references it; a column nobody references is not read."""
        self._scalar_field("scalars_matvec", grumpkin=True)
        if not isinstance(mat, FrMatrix) or not mat._h:
            raise TypeError("mat must be an open FrMatrix (scalars_matrix)")
        if mat.curve != self.curve or mat.device != self.device:
            raise ValueError("the matrix belongs to %s on device %d" % (mat.curve, mat.device))
        if transpose and not mat.has_transpose:
            raise ValueError("the matrix was made without transpose=True")
        in_len, out_len = (mat.rows, mat.cols) if transpose else (mat.cols, mat.rows)
        tx, bx, n = self._frvec_vector(x, "x")
        if n != in_len:
            raise ValueError("x holds %d scalars, the matrix takes %d" % (n, in_len))
        y_len = out_len if pad_to is None else int(pad_to)
        if not out_len <= y_len <= self.FRMAT_MAX_DIM:
            raise ValueError("pad_to must lie in [%d, 2^26], not %d" % (out_len, y_len))
        flags = self._mont256_flag() | (self.FRMAT_TRANSPOSE if transpose else 0)
        out = self._frvec_out(out, tx, y_len, tx is not None)
        if tx is not None and out is None:
            out = torch.empty((y_len, 32), dtype=torch.uint8, device=tx.device)
        res, dst = _dest(out, None, y_len)
        self._fr_call("frmat", "mul", tx, mat, dst, y_len, _ptr(tx, bx), n, flags)
        return _result(res)

    def r1cs_tables(self, a, b, c, z, n=None, out=None, first_row=0):
        """The tables Az, Bz, Cz of an R1CS as the rows first_row .. first_row + 2 of a batch x N x 32 byte CUDA buffer: three scalars_matvec calls
        over one z (a CUDA uint8 tensor of cols x 32 bytes).  N = n, or the next power of two >= the matrices' rows; the tail of every row is zero.
        out: None -- a new buffer of (first_row + 3) x N, whose other rows are NOT initialised -- or a contiguous buffer of batch x N x 32 bytes,
        whose other rows are left as they are: with scalars_eq(point, out=out[0]) and first_row=1 it is one sumcheck_prove input for eq A B - eq C."""
        mats = (a, b, c)
        if any(not isinstance(m, FrMatrix) for m in mats) or len({(m.rows, m.cols) for m in mats}) != 1:
            raise ValueError("a, b, c must be three FrMatrix of one shape")
        first_row = int(first_row)
        if n is None:
            n = 1
            while n < a.rows:
                n *= 2
        n = int(n)
        if n < a.rows or n & (n - 1) or first_row < 0:
            raise ValueError("n must be a power of two >= %d rows, first_row >= 0" % a.rows)
        if out is None:
            if not (isinstance(z, torch.Tensor) and z.is_cuda):
                raise TypeError("z must be a CUDA(HIP) uint8 tensor")
            out = torch.empty((first_row + 3, n, 32), dtype=torch.uint8, device=z.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda) or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() % (32 * n) or \
                out.numel() < 32 * n * (first_row + 3):
            raise ValueError("out must be a contiguous CUDA(HIP) uint8 tensor of batch x %d x 32 bytes with batch >= %d" % (n, first_row + 3))
        table = out.view(-1, n, 32)
        for k, m in enumerate(mats):
            self.scalars_matvec(m, z, out=table[first_row + k], pad_to=n)
        return out

    # -- constraint evaluation over the scalar field (libmsm_frgate.so): sums of products of rotated rows, the numerator of a PLONK / halo2-style
    # quotient over the extended coset domain, between two scalars_fft
    FRGATE_MONT256, FRGATE_ACCUMULATE = 2, 4  # MSM_FRGATE_MONT256, MSM_FRGATE_ACCUMULATE
    FRGATE_MAX_DEGREE, FRGATE_MAX_TERMS, FRGATE_MAX_ROWS = 8, 64, 32  # MSM_FRGATE_MAX_DEGREE, ..

    def scalars_gate(self, a, terms, batch=1, n=None, step=1, scale=None, out=None, accumulate=False):
        """out[i] = (out[i] if accumulate else 0) + scale[i mod len(scale)] * sum_terms coeff prod_f row_f[(i + rotation_f * step) mod n], i < n
        (msm_frgate_apply_device, include/msm_frgate.h): a constraint system evaluated element by element in one pass.  terms: 1 .. 64 pairs
        (coeff, factors) of a plain integer coefficient and 1 .. 8 factors, each a row number or (row, rotation) -- a rotation of any sign and
        size, in units of `step` elements, wrapping round the n elements.  a, batch, n: as scalars_mle_fold (batch <= 32 rows, n a power of two);
        a CUDA tensor runs on this context's stream, behind torch's; host bytes return bytes.  scale: None, or a vector like a of a power of two
        <= n of scalars.  out: a contiguous CUDA uint8 tensor of n x 32 bytes that overlaps neither a nor scale (a new one by default; with host
        bytes and accumulate, the n x 32 bytes to add onto).  The vectors are in this context's 32-byte scalar format and must be below r
        where they are read: the rows a term names, scale, and out with accumulate."""
        r = self._scalar_field("scalars_gate", grumpkin=True)
        ta, ba, n, stride = self._frmle_rows(a, batch, n, 1)
        batch, step = int(batch), int(step)
        if batch > self.FRGATE_MAX_ROWS:
            raise ValueError("a gate takes at most %d rows, not %d" % (self.FRGATE_MAX_ROWS, batch))
        if not 1 <= step <= n:
            raise ValueError("step must lie in [1, n = %d], not %d" % (n, step))
        arr, _ = _pack_terms(terms, batch, r, FrgateTerm, "gate", self.FRGATE_MAX_TERMS, self.FRGATE_MAX_DEGREE)
        on_device = ta is not None
        ts = bs = None
        scale_len = 0
        if scale is not None:
            ts, bs, scale_len = self._frvec_vector(scale, "scale")
            if (ts is not None) != on_device:
                raise TypeError("scale must be on the device exactly when a is")
            if scale_len < 1 or scale_len > n or scale_len & (scale_len - 1):
                raise ValueError("scale holds a power of two of scalars, at most n = %d, not %d" % (n, scale_len))
        flags = self._mont256_flag() | (self.FRGATE_ACCUMULATE if accumulate else 0)
        onto = None  # with host bytes and accumulate: what the host buffer holds before the call
        if on_device:
            if out is None:
                if accumulate:
                    raise ValueError("accumulate adds onto out")
                out = torch.empty((n, 32), dtype=torch.uint8, device=ta.device)
            else:
                self._frvec_out(out, ta, n, True)
            if ts is not None and ts.device != ta.device:
                raise ValueError("scale must be on %s" % (ta.device,))
            lo, hi = out.data_ptr(), out.data_ptr() + 32 * n
            for t, size in ((ta, 32 * batch * stride), (ts, 32 * scale_len)):
                if t is not None and lo < t.data_ptr() + size and t.data_ptr() < hi:
                    raise ValueError("out overlaps an input: a lane reads what its neighbours write to, the call is never in place")
        elif accumulate:
            onto, out = bytes(out) if out is not None else b"", None
            if len(onto) != 32 * n:
                raise ValueError("with host bytes, accumulate adds onto out: %d x 32 bytes" % n)
        else:
            self._frvec_out(out, None, n, False)
        res, dst = _dest(out, None, n, init=onto)
        self._fr_call("frgate", "apply", ta, None, dst, _ptr(ta, ba), n, batch, stride, arr, len(arr), step, _ptr(ts, bs), scale_len, flags)
        return _result(res)

    def vanishing_inverse(self, log_n, log_ext, shift):
        """The 2^log_ext values 1 / (shift^n w^(n i) - 1), i < 2^log_ext, w = root_of_unity(curve, log_n + log_ext), n = 2^log_n, as a CUDA uint8 tensor
        of 2^log_ext x 32 bytes in this context's scalar format: 1 / Z_H on the coset shift <w>, which has period 2^log_ext -- the `scale` of
        scalars_gate on the extended domain.  Computed with Python integers on the host.  Raises ValueError where shift^n = 1 (the coset meets H)."""
        r = self._scalar_field("vanishing_inverse")
        log_n, log_ext = int(log_n), int(log_ext)
        if log_n < 0 or log_ext < 0:
            raise ValueError("log_n and log_ext are not negative")
        w = root_of_unity(self.curve, log_n + log_ext)
        g = pow((int.from_bytes(shift, "little") if isinstance(shift, (bytes, bytearray)) else int(shift)) % r, 1 << log_n, r)
        wn = pow(w, 1 << log_n, r)  # a primitive 2^log_ext-th root
        vals, x = [], g
        for _ in range(1 << log_ext):
            if x in (0, 1):
                raise ValueError("Z_H vanishes on the coset: shift^n = %d" % x)
            vals.append(pow(x - 1, r - 2, r))
            x = x * wn % r
        if self.scalar_mont256:
            vals = [v * pow(2, 256, r) % r for v in vals]
        host = np.frombuffer(_scalars32(vals), dtype=np.uint8).reshape(-1, 32).copy()
        return torch.from_numpy(host).to("cuda:%d" % self.device)

    def quotient(self, coeffs, terms, batch, log_n, log_ext, shift):
        """The N = n 2^log_ext coefficients of t(X) = E(X) / Z_H(X), n = 2^log_n, as a CUDA uint8 tensor of N x 32 bytes:
        E(X) = sum_terms coeff prod_f column_f(omega^rotation_f X), omega = root_of_unity(curve, log_n) -- a rotation by +1 is the next row of H.
        coeffs: a CUDA uint8 tensor of batch x n x 32 bytes, the columns in coefficient form, left untouched.  Nothing leaves the device: a
        zero-padded copy of batch x N, scalars_fft onto the coset shift <root_of_unity(curve, log_n + log_ext)>, scalars_gate with step = 2^log_ext
        and scale = vanishing_inverse, scalars_fft back.  Needs 2^log_ext >= D - 1, D the largest degree among the terms: E / Z_H then has fewer
        than N coefficients, and where the constraints hold on H those from (D - 1) n upward are zero."""
        r = self._scalar_field("quotient")
        if not (isinstance(coeffs, torch.Tensor) and coeffs.is_cuda):
            raise TypeError("quotient takes a CUDA(HIP) uint8 tensor")
        batch, log_n, log_ext = int(batch), int(log_n), int(log_ext)
        t, total = _as_device_u8(coeffs, 32, "coeffs")
        if log_n < 0 or log_ext < 0 or batch < 1 or total != batch << log_n:
            raise ValueError("%d scalars are not %d columns of 2^%d" % (total, batch, log_n))
        if batch > self.FRGATE_MAX_ROWS or (batch << (log_n + log_ext)) > self.FRVEC_MAX_ELEMENTS:
            raise ValueError("the extended columns are at most %d rows and 2^26 scalars" % self.FRGATE_MAX_ROWS)
        _, top = _pack_terms(terms, batch, r, FrgateTerm, "gate", self.FRGATE_MAX_TERMS, self.FRGATE_MAX_DEGREE)
        if (1 << log_ext) < top - 1:
            raise ValueError("terms of degree %d need log_ext with 2^log_ext >= %d" % (top, top - 1))
        n, big = 1 << log_n, 1 << (log_n + log_ext)
        scale = self.vanishing_inverse(log_n, log_ext, shift)
        ext = torch.zeros((batch, big, 32), dtype=torch.uint8, device=t.device)
        ext[:, :n] = t.view(batch, n, 32)
        self.scalars_fft(ext, log_n + log_ext, shift=shift, batch=batch)
        out = self.scalars_gate(ext, terms, batch=batch, step=1 << log_ext, scale=scale)
        return self.scalars_fft(out, log_n + log_ext, inverse=True, shift=shift)

    # -- lookup arguments over the scalar field (libmsm_frlook.so): the multiplicity column of a logUp / plookup-style lookup and the table index
    # of every looked-up value, between the quotient and the commitments
    FRLOOK_MONT256, FRLOOK_MISSING = 2, 0xFFFFFFFF  # MSM_FRLOOK_MONT256, MSM_FRLOOK_MISSING
    FRLOOK_MAX_TABLE, FRLOOK_MAX_ELEMENTS = 1 << 24, 1 << 26  # MSM_FRLOOK_MAX_TABLE, MSM_FRLOOK_MAX_ELEMENTS

    def lookup_table(self, t, n=None):
        """A lookup table over this context's scalar field -> FrLookup (msm_frlook_create_device, include/msm_frlook.h).  t: a CUDA uint8 tensor of
        32-byte scalars in this context's scalar format (canonical, or mont256) -- e.g. the columns of a table folded with a challenge by
        scalars_combine --, of which the first n (default: all, at most 2^24) are the table; host bytes are taken too and go to the device with the
        first count.  The handle keeps a copy of its own: t is free afterwards.  A value may repeat: every match is credited to its lowest
        index.  A value that is not below r raises MsmHipError (code -4).  Every curve's scalar field, Grumpkin's included."""
        self._scalar_field("lookup_table", grumpkin=True)
        tt, bt, total = self._frvec_vector(t, "t")
        n = total if n is None else int(n)
        if not 1 <= n <= min(total, self.FRLOOK_MAX_TABLE):
            raise ValueError("a table holds 1 .. 2^24 scalars, at most the %d given, not %d" % (total, n))
        h, distinct = C.c_void_p(), C.c_size_t()
        self._fr_call("frlook", "create", tt, None, _ptr(tt, bt), n, self._mont256_flag(), C.byref(h))
        look = FrLookup(h, self.curve, self.device, n, 0, bool(self.scalar_mont256))
        self._fr_call("frlook", "info", None, look, None, C.byref(distinct), None)
        look.distinct = distinct.value
        return look

    def scalars_multiplicities(self, table, f, batch=1, n=None, out=None, indices=False, counts=False, strict=True):
        """m[j] = the number of elements of f equal to the table's value j (msm_frlook_count_device): the multiplicity column of a logUp, as
        table.n scalars in this context's scalar format (under mont256 the count k is k * 2^256 mod r).  table: an FrLookup of this context's
        curve, device and scalar format.  f: a CUDA uint8 tensor of batch rows, of which the first n scalars (default: the whole row; any n >= 1)
        are looked up, or host bytes of the same layout.  A table value that repeats gets all its matches at its lowest index and 0 at the others.
        -> m (a CUDA uint8 tensor of table.n x 32 bytes, or `out`; bytes for host bytes), or a tuple of m and what was asked for, in this
        order: indices=True, the table index of every element as a CUDA int32 tensor of batch x n, -1 where the value is not in the table (numpy
        uint32 with 0xFFFFFFFF for host bytes); counts=True, the counts as a CUDA tensor of table.n 32-bit words (torch.uint32; numpy uint32 for
        host bytes); strict=False, the pair (missing, first_missing): how many elements are not in the table and the lowest flat index
        row * n + i among them (None: none).  strict=True raises ValueError naming both instead.  m counts the elements that were found.  An
        element that is not below r raises MsmHipError (code -4)."""
        self._scalar_field("scalars_multiplicities", grumpkin=True)
        if not isinstance(table, FrLookup) or not table._h:
            raise TypeError("table must be an open FrLookup (lookup_table)")
        mont = bool(self.scalar_mont256)
        if table.curve != self.curve or table.device != self.device or table.mont256 != mont:
            raise ValueError("the table belongs to %s on device %d with mont256=%s" % (table.curve, table.device, table.mont256))
        batch = int(batch)
        tf, bf, total = self._frvec_vector(f, "f")
        if batch < 1 or total < 1 or total % batch or total > self.FRLOOK_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        stride = total // batch
        n = stride if n is None else int(n)
        if not 1 <= n <= stride:
            raise ValueError("n must lie in [1, %d], the length of a row, not %d" % (stride, n))
        miss, first = C.c_uint64(), C.c_uint64()
        out = self._frvec_out(out, tf, table.n, tf is not None)
        if tf is None:
            idx = np.empty(batch * n, dtype=np.uint32) if indices else None
            cnt = np.empty(table.n, dtype=np.uint32) if counts else None
            idx_ptr, cnt_ptr = idx.ctypes.data if indices else None, cnt.ctypes.data if counts else None
        else:
            if out is None:
                out = torch.empty((table.n, 32), dtype=torch.uint8, device=tf.device)
            idx = torch.empty((batch, n), dtype=torch.int32, device=tf.device) if indices else None
            cnt = torch.empty(table.n, dtype=torch.uint32, device=tf.device) if counts else None
            idx_ptr, cnt_ptr = idx.data_ptr() if indices else None, cnt.data_ptr() if counts else None
        res, dst = _dest(out, None, table.n)
        self._fr_call("frlook", "count", tf, table, dst, cnt_ptr, idx_ptr, _ptr(tf, bf), n, batch, stride, self._mont256_flag(), C.byref(miss), C.byref(first))
        if tf is None and indices:
            idx = idx.reshape(batch, n)
        if strict and miss.value:
            raise ValueError("%d looked-up values are not in the table; the first is element %d (row %d, position %d)" % (miss.value, first.value, first.value // n,
                                                                                                                        first.value % n))
        res = (_result(res),) + ((idx,) if indices else ()) + ((cnt,) if counts else ())
        if not strict:
            res += ((miss.value, first.value if miss.value else None),)
        return res[0] if len(res) == 1 else res

    def logup(self, table_values, f, beta, batch=1, n=None, lookup=None):
        """The columns of a logUp argument, prepared on the device: with m = scalars_multiplicities(lookup_table(table_values), f),
        h_f[i] = sum_rows 1 / (beta + f[row][i]), i < n, and h_t[j] = m[j] / (beta + t[j]) -> (m, h_f, h_t, sum h_f, sum h_t).  The lookup holds
        exactly when every value is in the table -- ValueError otherwise, as scalars_multiplicities(strict=True) -- and the two sums agree.
        table_values: a CUDA uint8 tensor of 32-byte scalars in this context's scalar format; f, batch, n: as scalars_multiplicities, on the
        device; beta: an integer in [0, r) or its 32 bytes, always a plain integer; lookup: an FrLookup already made of table_values (else one is
        made and closed here).  m, h_f, h_t: new CUDA uint8 tensors of table.n, n and table.n scalars; the sums: 32 host bytes each, in the
        data's form.  Chains scalars_add (beta broadcast), scalars_inverse, scalars_mul and scalars_scan(op="sum", totals=True) behind the
        lookup; the inputs are left untouched.  beta = -value is NOT detected: the vector library's 1 / 0 = 0 applies, and the term of that
        value is then missing from its sum -- draw beta after the columns are committed.  On Grumpkin, whose scalar field the vector library
        has no unit for, the same columns come from the libraries that have one (_logup_without_frvec): scalars_gate for beta + x, the
        products and the row sums, 1 / x as x^(r - 2) in 127 scalars_gate passes (again 1 / 0 = 0), scalars_mle_eval for the two sums --
        the same bytes, some hundred launches more; there batch * n and the table are at most 2^25 scalars."""
        r = self._scalar_field("logup", grumpkin=True)
        if not (isinstance(table_values, torch.Tensor) and table_values.is_cuda and isinstance(f, torch.Tensor) and f.is_cuda):
            raise TypeError("logup takes CUDA(HIP) uint8 tensors")
        tt, n_t = _as_device_u8(table_values, 32, "table_values")
        tf, total = _as_device_u8(f, 32, "f")
        batch = int(batch)
        if batch < 1 or total < 1 or total % batch:
            raise ValueError("%d scalars are not %d rows" % (total, batch))
        stride = total // batch
        n = stride if n is None else int(n)
        if not 1 <= n <= stride:
            raise ValueError("n must lie in [1, %d], the length of a row, not %d" % (stride, n))
        beta = int.from_bytes(_const32(beta, r, "beta"), "little")
        own = lookup is None
        if own:
            lookup = self.lookup_table(tt)
        elif not isinstance(lookup, FrLookup) or lookup.n != n_t:
            raise ValueError("lookup must be the FrLookup of the %d table values" % n_t)
        try:
            m = self.scalars_multiplicities(lookup, tf, batch=batch, n=n)
        finally:
            if own:
                lookup.close()
        den = torch.empty((batch * n, 32), dtype=torch.uint8, device=tf.device)  # a copy: 1 / (beta + f), row after row
        den.view(batch, n, 32).copy_(tf.view(batch, stride, 32)[:, :n])
        if self.curve == "grumpkin":
            return (m,) + self._logup_without_frvec(r, den, tt.view(-1, 32)[:n_t], m, beta, batch, n)
        self.scalars_inverse(self.scalars_add(den, beta))
        h_f = den if batch == 1 else den[:n].clone()
        for row in range(1, batch):
            self.scalars_add(h_f, den[row * n:(row + 1) * n])
        h_t = tt.view(-1, 32)[:n_t].clone()
        self.scalars_mul(self.scalars_inverse(self.scalars_add(h_t, beta)), m)
        _, sum_f = self.scalars_scan(h_f, op="sum", out=torch.empty_like(h_f), totals=True)
        _, sum_t = self.scalars_scan(h_t, op="sum", out=torch.empty_like(h_t), totals=True)
        return m, h_f, h_t, sum_f, sum_t

    def _gate_inverse(self, x, r):
        """1 / x element by element, 1 / 0 = 0, for a CUDA tensor of N = 2^k scalars, where the vector library has no unit: x^(r - 2), two bits
        of the exponent per scalars_gate pass (acc^4 x^d, d <= 3: degree <= 7), between two buffers of two rows (acc, x) because a gate is
        never in place -> a contiguous N x 32 tensor"""
        big = x.shape[0]
        bufs = [torch.empty((2, big, 32), dtype=torch.uint8, device=x.device) for _ in range(2)]
        for b in bufs:
            b[1].copy_(x)
        digits, e = [], r - 2
        while e:
            digits.append(e & 3)
            e >>= 2
        digits.reverse()
        self.scalars_gate(bufs[1], [(1, (1,) * digits[0])], batch=2, out=bufs[0][0])  # (the top digit is not 0)
        cur = 0
        for d in digits[1:]:
            self.scalars_gate(bufs[cur], [(1, (0,) * 4 + (1,) * d)], batch=2, out=bufs[1 - cur][0])
            cur = 1 - cur
        return bufs[cur][0]

    def _logup_without_frvec(self, r, den, table, m, beta, batch, n):
        """logup's columns behind the lookup from scalars_gate and scalars_mle_eval alone.  den: the batch * n looked-up scalars, row after row
        (overwritten); table, m: the table's values and multiplicities -> (h_f, h_t, sum h_f, sum h_t)"""
        def pow2(k):
            return max(2, 1 << (k - 1).bit_length())

        if max(pow2(batch * n), pow2(table.shape[0])) > 1 << 25:
            raise ValueError("on %s logup takes at most 2^25 looked-up scalars and table values" % self.curve)
        one = (pow(2, 256, r) if self.scalar_mont256 else 1).to_bytes(32, "little")
        dev = den.device

        def inverse_of_beta_plus(v):  # v: count x 32 -> 2^k x 32, the tail 1 / beta
            count, big = v.shape[0], pow2(v.shape[0])
            rows = torch.zeros((2, big, 32), dtype=torch.uint8, device=dev)
            rows[0, :count].copy_(v)
            rows[1].copy_(torch.frombuffer(bytearray(one), dtype=torch.uint8).to(dev))
            return self._gate_inverse(self.scalars_gate(rows, [(1, (0,)), (beta, (1,))], batch=2), r)

        def total(v):  # sum of 2^k scalars = 2^k times their multilinear extension at (1/2, .., 1/2)
            k = v.shape[0].bit_length() - 1
            at_half = int.from_bytes(self.scalars_mle_eval(v, [(r + 1) // 2] * k), "little")
            return (at_half << k) % r

        inv_f = inverse_of_beta_plus(den)
        wide = pow2(n)
        sum_rows = torch.zeros((wide, 32), dtype=torch.uint8, device=dev)
        for first in range(0, batch, self.FRGATE_MAX_ROWS):  # at most 32 rows to a gate, each padded with zeros to 2^k
            count = min(self.FRGATE_MAX_ROWS, batch - first)
            rows = torch.zeros((count, wide, 32), dtype=torch.uint8, device=dev)
            rows[:, :n].copy_(inv_f[first * n:(first + count) * n].view(count, n, 32))
            self.scalars_gate(rows, [(1, (c,)) for c in range(count)], batch=count, out=sum_rows, accumulate=True)
        n_t, big_t = table.shape[0], pow2(table.shape[0])
        pair = torch.zeros((2, big_t, 32), dtype=torch.uint8, device=dev)
        pair[0, :n_t].copy_(m)
        pair[1].copy_(inverse_of_beta_plus(table))
        prod = self.scalars_gate(pair, [(1, (0, 1))], batch=2)  # (zero behind the table: m is padded with zeros)
        sums = [total(v).to_bytes(32, "little") for v in (sum_rows, prod)]
        return sum_rows[:n].clone(), prod[:n_t].clone(), sums[0], sums[1]

    # -- algebraic hashing over the scalar field (libmsm_frhash.so): Poseidon permutations, sponges and Merkle trees on the stream of the
    # commitments
    FRHASH_MONT256, FRHASH_MAX_WIDTH, FRHASH_MAX_FULL_ROUNDS, FRHASH_MAX_PARTIAL_ROUNDS = 2, 12, 16, 128  # MSM_FRHASH_MONT256, MSM_FRHASH_MAX_WIDTH, ..
    FRHASH_MAX_ELEMENTS, FRHASH_MAX_LEVELS = 1 << 26, 64  # MSM_FRHASH_MAX_ELEMENTS, MSM_FRHASH_MAX_LEVELS
    FRHASH_POSEIDON2 = 16  # MSM_FRHASH_POSEIDON2
    POSEIDON2_WIDTHS = (2, 3, 4, 8, 12)

    def _frhash_create(self, r, t, full_rounds, partial_rounds, round_constants, matrix, flags, capacity, capacity_at, out_at, kind):
        """the tail that poseidon and poseidon2 share: the sponge's convention checked, the constants as bytes, msm_frhash_create -> FrHash"""
        capacity_at, out_at = int(capacity_at), int(out_at)
        if not 0 <= capacity_at < t or not 0 <= out_at < t:
            raise ValueError("capacity_at and out_at must lie in [0, t)")
        capacity = int.from_bytes(_const32(capacity, r, "capacity"), "little")
        h = C.c_void_p()
        self._fr_call("frhash", "create", None, None, t, full_rounds, partial_rounds, 5, _in(_scalars32(round_constants)), _in(_scalars32(matrix)), flags, C.byref(h))
        return FrHash(h, self.curve, self.device, t, full_rounds, partial_rounds, capacity, capacity_at, out_at, kind)

    def poseidon(self, t=3, full_rounds=8, partial_rounds=None, round_constants=None, mds=None, capacity=0, capacity_at=0, out_at=0):
        """A Poseidon permutation of width t over this context's scalar field (a G2 context takes its G1's) -> FrHash (msm_frhash_create,
        include/msm_frhash.h).  round_constants ((full_rounds + partial_rounds) * t integers) and mds (t rows of t integers) default to
        poseidon_parameters(curve, t, full_rounds, partial_rounds); give both or neither.  capacity, capacity_at, out_at: the sponge's
        convention, which the handle remembers for scalars_hash and merkle_tree -- (0, 0, 0) is circomlib's poseidon(inputs), (L * 2^64,
        t - 1, 0) halo2's ConstantLength<L>, (2^arity - 1, 0, 1) neptune's.  No device is touched: the tables go there with the first call."""
        r = self._scalar_field("poseidon", grumpkin=True)
        t, full_rounds = int(t), int(full_rounds)
        if (round_constants is None) != (mds is None):
            raise ValueError("give round_constants and mds, or neither")
        if not 2 <= t <= self.FRHASH_MAX_WIDTH or full_rounds % 2 or not 2 <= full_rounds <= self.FRHASH_MAX_FULL_ROUNDS:
            raise ValueError("a permutation has 2 <= t <= 12 and an even 2 <= full_rounds <= 16")
        if round_constants is None:
            partial_rounds = POSEIDON_PARTIAL_ROUNDS[t] if partial_rounds is None else int(partial_rounds)
            round_constants, mds = poseidon_parameters(self.curve, t, full_rounds, partial_rounds)
        elif partial_rounds is None:
            raise ValueError("parameters of the caller's come with their partial_rounds")
        partial_rounds = int(partial_rounds)
        if not 0 <= partial_rounds <= self.FRHASH_MAX_PARTIAL_ROUNDS:
            raise ValueError("a permutation has 0 .. 128 partial rounds")
        round_constants = [int(c) for c in round_constants]
        mds = [[int(c) for c in row] for row in mds]
        if len(round_constants) != (full_rounds + partial_rounds) * t or len(mds) != t or any(len(row) != t for row in mds):
            raise ValueError("round_constants holds (full_rounds + partial_rounds) * t integers and mds t rows of t")
        if any(not 0 <= c < r for c in round_constants) or any(not 0 <= c < r for row in mds for c in row):
            raise ValueError("round constants and matrix entries must lie in [0, r)")
        return self._frhash_create(r, t, full_rounds, partial_rounds, round_constants, [c for row in mds for c in row], 0, capacity, capacity_at, out_at, "poseidon")

    def poseidon2(self, t, full_rounds, partial_rounds, round_constants, diagonal, capacity=0, capacity_at=0, out_at=0):
        """A Poseidon2 permutation of width t in {2, 3, 4, 8, 12} over this context's scalar field -> FrHash with kind == "poseidon2"
        (msm_frhash_create under MSM_FRHASH_POSEIDON2; include/msm_frhash.h has the definition), which scalars_permute, scalars_hash,
        merkle_tree and merkle_path take like any other.  round_constants: full_rounds * t + partial_rounds integers in the order of their
        use (t per external round, one per internal round, t per external round).  diagonal: the t integers mu of the internal layer
        s[i] = mu[i] * s[i] + sum(s) -- the internal matrix's diagonal MINUS ONE, what the published parameter files call
        mat_internal_diag_m_1 or internal_matrix_diagonal.  The constants are the caller's: there is no default and no generator.
        capacity, capacity_at, out_at: as for poseidon; Barretenberg's sponge is (L * 2^64, t - 1, 0).  No device is touched."""
        r = self._scalar_field("poseidon2", grumpkin=True)
        t, full_rounds, partial_rounds = int(t), int(full_rounds), int(partial_rounds)
        if t not in self.POSEIDON2_WIDTHS or full_rounds % 2 or not 2 <= full_rounds <= self.FRHASH_MAX_FULL_ROUNDS:
            raise ValueError("a Poseidon2 permutation has t in {2, 3, 4, 8, 12} and an even 2 <= full_rounds <= 16")
        if not 0 <= partial_rounds <= self.FRHASH_MAX_PARTIAL_ROUNDS:
            raise ValueError("a permutation has 0 .. 128 partial rounds")
        round_constants, diagonal = [int(c) for c in round_constants], [int(c) for c in diagonal]
        if len(round_constants) != full_rounds * t + partial_rounds or len(diagonal) != t:
            raise ValueError("round_constants holds full_rounds * t + partial_rounds integers and diagonal t")
        if any(not 0 <= c < r for c in round_constants) or any(not 0 <= c < r for c in diagonal):
            raise ValueError("round constants and the diagonal must lie in [0, r)")
        return self._frhash_create(r, t, full_rounds, partial_rounds, round_constants, diagonal, self.FRHASH_POSEIDON2, capacity, capacity_at, out_at, "poseidon2")

    def _frhash_handle(self, h):
        if not isinstance(h, FrHash) or not h._h:
            raise TypeError("h must be an open FrHash (poseidon, poseidon2)")
        if SCALAR_FIELDS[h.curve] != SCALAR_FIELDS.get(self.curve) or h.device != self.device:
            raise ValueError("the permutation belongs to the scalar field of %s on device %d" % (h.curve, h.device))
        self._scalar_field("hashing", grumpkin=True)
        return self._mont256_flag()

    def _frhash_out(self, out, t, n, reads, overlap, in_place=False):
        """`out` for a hashing call whose input is t: checked -- n x 32 bytes on t's device that do not overlap the `reads` bytes the call reads
        of t (in_place: or begin where t begins), else ValueError(overlap) --, or a new tensor; for host bytes (t is None) no `out` at all"""
        out = self._frvec_out(out, t, n, t is not None)
        if t is not None and out is None:
            return torch.empty((n, 32), dtype=torch.uint8, device=t.device)
        if out is not None and not (in_place and out.data_ptr() == t.data_ptr()) and out.data_ptr() < t.data_ptr() + reads and t.data_ptr() < out.data_ptr() + 32 * n:
            raise ValueError(overlap)
        return out

    def scalars_permute(self, h, state, out=None):
        """out = the permutation of every state (msm_frhash_permute_device): state is a CUDA uint8 tensor of n x t x 32 bytes in this
        context's scalar format -- state i is scalars [i t, (i + 1) t) --, or host bytes of the same layout, which return bytes.  out: a
        contiguous CUDA uint8 tensor of the same size, `state` itself (in place) or one that does not overlap it (a new one by default).  An
        element that is not below r raises MsmHipError (code -4)."""
        flags = self._frhash_handle(h)
        ts, bs, total = self._frvec_vector(state, "state")
        if total < h.t or total % h.t or total > self.FRHASH_MAX_ELEMENTS:
            raise ValueError("%d scalars are not 1 .. 2^26 / t states of t = %d" % (total, h.t))
        n = total // h.t
        new = out is None and ts is not None
        out = self._frhash_out(out, ts, total, 32 * total, "out is state itself or does not overlap it", in_place=True)
        res, dst = _dest(out.view(n, h.t, 32) if new else out, None, total)
        self._fr_call("frhash", "permute", ts, h, dst, _ptr(ts, bs), n, flags)
        return _result(res)

    def scalars_hash(self, h, a, length, batch=1, stride=None, out=None):
        """out[row] = the sponge of the first `length` scalars of row `row` of a (msm_frhash_hash_device), rate t - 1, under the handle's
        capacity convention; nothing is padded.  a: a CUDA uint8 tensor of 32-byte scalars in this context's scalar format holding `batch`
        rows `stride` scalars apart (default: scalars / batch), of which the scalars behind `length` are not read; or host bytes of the same
        layout, which return bytes.  out: a contiguous CUDA uint8 tensor of batch x 32 bytes that does not overlap a."""
        flags = self._frhash_handle(h)
        ta, ba, total = self._frvec_vector(a, "a")
        batch, length = int(batch), int(length)
        if batch < 1 or total < 1 or total > self.FRHASH_MAX_ELEMENTS:
            raise ValueError("%d scalars are not %d rows of 1 .. 2^26 / batch scalars" % (total, batch))
        if stride is None:
            if total % batch:
                raise ValueError("%d scalars are not %d rows" % (total, batch))
            stride = total // batch
        stride = int(stride)
        if not 1 <= length <= stride or (batch - 1) * stride + length > total:
            raise ValueError("%d rows of %d scalars, %d apart, do not fit the %d scalars given" % (batch, length, stride, total))
        res, dst = _dest(self._frhash_out(out, ta, batch, 32 * total, "out overlaps a"), None, batch)
        self._fr_call("frhash", "hash", ta, h, dst, _ptr(ta, ba), batch, length, stride, _in(h.capacity.to_bytes(32, "little")), h.capacity_at, h.out_at, flags)
        return _result(res)

    def _merkle_levels(self, h, n_leaves):
        """the number of nodes of every level above the leaves, the lowest first"""
        a = h.arity
        if a == 1:
            if not 1 <= n_leaves <= self.FRHASH_MAX_LEVELS:
                raise ValueError("a tree of arity 1 is a chain of 1 .. %d levels over one leaf" % self.FRHASH_MAX_LEVELS)
            return [1] * n_leaves
        levels, n = [], n_leaves
        if n < a or n > self.FRHASH_MAX_ELEMENTS:
            raise ValueError("a tree of arity %d has %d^k leaves, k >= 1, at most 2^26, not %d" % (a, a, n_leaves))
        while n > 1:
            if n % a:
                raise ValueError("a tree of arity %d has %d^k leaves, k >= 1, not %d" % (a, a, n_leaves))
            n //= a
            levels.append(n)
        return levels

    def merkle_tree(self, h, leaves, out=None, levels=None):
        """The nodes above the leaves of the tree of arity t - 1 (msm_frhash_merkle_device): the level above the leaves first, the root
        last -- (n - 1) / (arity - 1) scalars for n = arity^k leaves, every node the sponge of the `arity` scalars below it under the handle's
        capacity convention.  leaves: a CUDA uint8 tensor of n x 32 bytes in this context's scalar format, or host bytes (which return
        bytes).  At arity 1 (t = 2) the tree is a chain over ONE leaf and `levels` (1 .. 64) says how long.  out: a contiguous CUDA uint8
        tensor of that many x 32 bytes that does not overlap the leaves.  One launch per level, on this context's stream."""
        flags = self._frhash_handle(h)
        tl, bl, n = self._frvec_vector(leaves, "leaves")
        if h.arity == 1:
            if n != 1 or levels is None:
                raise ValueError("at arity 1 the tree is a chain over one leaf: give levels")
            n = int(levels)
        elif levels is not None:
            raise ValueError("levels is for arity 1; the leaves say how deep a wider tree is")
        count = sum(self._merkle_levels(h, n))
        res, dst = _dest(self._frhash_out(out, tl, count, tl.numel() if tl is not None else 0, "out overlaps the leaves"), None, count)
        self._fr_call("frhash", "merkle", tl, h, dst, _ptr(tl, bl), n, _in(h.capacity.to_bytes(32, "little")), h.capacity_at, h.out_at, flags)
        return _result(res)

    def merkle_path(self, h, leaves, nodes, index):
        """The siblings of leaf `index` on its way to the root: a tensor of k x (arity - 1) x 32 bytes, level by level from the leaves up,
        each level's siblings in index order -- with plain torch indexing, nothing is hashed.  leaves and nodes: as merkle_tree took and
        returned them (CUDA tensors, or bytes, which return a list of k lists of 32-byte strings)."""
        if not isinstance(h, FrHash):
            raise TypeError("h must be an FrHash (poseidon)")
        a, index = h.arity, int(index)
        on_device = isinstance(leaves, torch.Tensor)
        lv = leaves.reshape(-1, 32) if on_device else [bytes(leaves)[i:i + 32] for i in range(0, len(bytes(leaves)), 32)]
        nd = nodes.reshape(-1, 32) if on_device else [bytes(nodes)[i:i + 32] for i in range(0, len(bytes(nodes)), 32)]
        n = len(lv)
        counts = self._merkle_levels(h, len(nd) if a == 1 else n)
        if sum(counts) != len(nd) or not 0 <= index < n:
            raise ValueError("nodes is not the tree over these leaves, or index is not a leaf")
        rows, below, first_node = [], lv, 0
        for count in counts:
            first = index - index % a
            rows.append([below[first + p] for p in range(a) if first + p != index])
            index //= a
            below, first_node = nd[first_node:first_node + count], first_node + count
        if on_device:
            return torch.stack([torch.stack(row) if row else lv.new_empty((0, 32)) for row in rows]) if rows else lv.new_empty((0, a - 1, 32))
        return rows
