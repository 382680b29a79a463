"""What the scalar-field wrappers hand to C, pinned: every host-bytes wrapper runs once on a bare context against eight recording stand-ins for
the libraries, and the calls -- function name and normalised arguments, in order -- must be those of tests/golden/scalars_calls.json, which is
what `python tests/test_scalars_calls.py` printed before the wrappers left api.py.  No library is loaded and no device is touched."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scalars_calls.json")
LIBRARIES = ("fr", "frvec", "frpoly", "frmle", "frmat", "frgate", "frlook", "frhash")
# host forms that no wrapper reaches without a device: scalars_powers and scalars_eq only have a device form, and nothing asks a matrix or a
# permutation for its info
UNREACHABLE = {"msm_frpoly_powers", "msm_frmle_eq", "msm_frmat_info", "msm_frhash_info"}
# arguments that arrive as a bare address (numpy's .ctypes.data): position -> bytes behind it, from the other arguments; None: an output
ADDRESSES = {"msm_frmat_create": {5: lambda a: 4 * (a[2] + 1), 6: lambda a: 4 * a[4]}, "msm_frlook_count": {2: None, 3: None}}


def _norm(v):
    if v is None or isinstance(v, int):
        return v
    if isinstance(v, (bytes, bytearray)):
        return {"bytes": bytes(v).hex()}
    if isinstance(v, C.Array):  # a string buffer, or an array of structures
        return {"buffer": C.sizeof(v), "hex": bytes(v).hex()}
    if isinstance(v, (C.c_void_p, C.c_char_p)):
        held = [o for o in (v._objects or {}).values() if isinstance(o, (bytes, C.Array))] if isinstance(v._objects, dict) else [v._objects]
        held = [o for o in held if isinstance(o, (bytes, C.Array))]
        if held:  # a cast pointer to a buffer or to bytes
            return {"buffer": len(bytes(held[0])), "hex": bytes(held[0]).hex()}
        return {"pointer": v.value}
    if hasattr(v, "_obj"):  # byref
        return {"byref": type(v._obj).__name__, "value": v._obj.value}
    raise TypeError("an argument of %s" % type(v))


class Recorder:
    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, fn):
        def call(*args):
            at = ADDRESSES.get(fn, {})
            self._calls.append([fn, [("out" if at[k] is None else C.string_at(a, at[k](args)).hex()) if k in at and a is not None else _norm(a)
                                     for k, a in enumerate(args)]])
            return 0
        return call


def _bare_context(api, curve="bn254", mont=False):
    """An MsmContext that never touched the library (no device needed)"""
    ctx = api.MsmContext.__new__(api.MsmContext)
    ctx._h = C.c_void_p()
    ctx.curve, ctx.scalar_width, ctx.scalar_signed, ctx.scalar_mont256, ctx.n_bases, ctx._keepalive = curve, 32, False, mont, 0, {}
    ctx.curve_id, ctx.modulus = api.CURVES[curve]
    ctx.device = 0
    return ctx


def _scalars(first, n):
    return b"".join((first + 7 * k).to_bytes(32, "little") for k in range(n))


def _drive(api):
    ctx, mont = _bare_context(api), _bare_context(api, mont=True)
    v8, w8, v4 = _scalars(3, 8), _scalars(1000, 8), _scalars(50, 4)
    # the transform
    ctx.scalars_fft(v8)
    ctx.scalars_fft(v8, log_n=2, batch=2, shift=5, inverse=True)
    ctx.scalars_fft(v4, omega=api.root_of_unity("bn254", 2), shift=(9).to_bytes(32, "little"))
    mont.scalars_fft(v4)
    # vectors
    ctx.scalars_add(v8, w8)
    ctx.scalars_sub(v8, 11)
    ctx.scalars_mul(v8, (12).to_bytes(32, "little"))
    ctx.scalars_mul_add(v8, w8, 13)
    ctx.scalars_mul_sub(v8, 14, w8)
    ctx.scalars_inverse(v8)
    ctx.scalars_scan(v8)
    ctx.scalars_scan(v8, op="sum", exclusive=True, batch=2, totals=True)
    mont.scalars_inverse(v4)
    mont.scalars_scan(v4, exclusive=True)
    # openings
    ctx.scalars_eval(v8, 21, batch=2)
    ctx.scalars_divide(v8, 22)
    ctx.scalars_divide(v8, (23).to_bytes(32, "little"), batch=2, values=True)
    ctx.scalars_dot(v8, w8)
    ctx.scalars_dot(v8, v4, batch=2)
    ctx.scalars_combine(v8, [1, 2])
    mont.scalars_eval(v4, 3)
    # the sumcheck
    ctx.scalars_mle_fold(v8, 31)
    ctx.scalars_mle_fold(v8, 32, batch=2, n=2)
    ctx.scalars_mle_eval(v8, [1, 2, 3])
    ctx.scalars_mle_eval(v8, [4], batch=2, n=2)
    ctx.scalars_sumcheck_round(v8, [(1, (0, 1)), (5, (1, 1, 0))], batch=2)
    ctx.scalars_sumcheck_round(v8, [(2, (0,))], batch=2, fold=33)
    mont.scalars_mle_fold(v4, 1)
    # sparse matrices
    m = ctx.scalars_matrix(2, 3, [0, 2, 3], [0, 2, 1], [5, 6, 7], transpose=True)
    assert (m.rows, m.cols, m.nnz, m.has_transpose) == (2, 3, 3, True) and not m._h
    ctx.scalars_matrix(1, 1, [0, 0], [], b"")
    for c, flag in ((ctx, False), (mont, True)):
        mat = api.FrMatrix(C.c_void_p(0x1000), "bn254", 0, 2, 3, 3, True)
        try:
            c.scalars_matvec(mat, _scalars(1, 3))
            if not flag:
                c.scalars_matvec(mat, _scalars(1, 2), transpose=True, pad_to=4)
        finally:
            mat.close()
    # gates
    ctx.scalars_gate(v8, [(1, (0, (1, -1))), (3, ((0, 2),))], batch=2)
    ctx.scalars_gate(v8, [(1, (0,))], batch=2, n=4, step=2, scale=_scalars(9, 2), out=v4, accumulate=True)
    mont.scalars_gate(v4, [(1, (0, 0))])
    # lookups
    for c, flag in ((ctx, False), (mont, True)):
        t = c.lookup_table(v8, n=4)
        assert (t.n, t.distinct, t.mont256) == (4, 0, flag) and not t._h
        table = api.FrLookup(C.c_void_p(0x2000), "bn254", 0, 4, 4, flag)
        try:
            c.scalars_multiplicities(table, v8, strict=False)
            if not flag:
                c.scalars_multiplicities(table, v8, batch=2, n=3, indices=True, counts=True)
        finally:
            table.close()
    # hashing
    h = ctx.poseidon(t=2, full_rounds=2, partial_rounds=1, round_constants=[1, 2, 3, 4, 5, 6], mds=[[1, 2], [3, 4]], capacity=7)
    assert (h.t, h.arity, h.capacity, h.kind) == (2, 1, 7, "poseidon") and not h._h
    h = ctx.poseidon2(3, 2, 1, [1, 2, 3, 4, 5, 6, 7], [8, 9, 10], capacity_at=2)
    assert (h.t, h.kind, h.capacity_at) == (3, "poseidon2", 2) and not h._h
    for c, flag in ((ctx, False), (mont, True)):
        h = api.FrHash(C.c_void_p(0x3000), "bn254", 0, 3, 8, 57, 77, 1, 2)
        try:
            c.scalars_permute(h, _scalars(1, 6))
            if not flag:
                c.scalars_hash(h, v8, 3, batch=2)
                c.scalars_hash(h, v8, 2, batch=3, stride=3)
                c.merkle_tree(h, v4)
        finally:
            h.close()
    chain = api.FrHash(C.c_void_p(0x4000), "bn254", 0, 2, 8, 56, 0, 0, 0)
    try:
        ctx.merkle_tree(chain, _scalars(1, 1), levels=3)
    finally:
        chain.close()
    # the hooks
    api.fr_test_pass_bits(4)
    api.frlook_test_hash_bits(5)
    for k, lib in enumerate(("frvec", "frpoly", "frmle", "frmat", "frhash")):
        getattr(api, lib + "_test_tile")(2 + k)
    assert [getattr(api, lib + "_last")() for lib in ("fr", "frvec", "frpoly", "frmle", "frmat")] == [(0, 0)] * 5
    for lib in LIBRARIES:
        getattr(api, lib + "_release")()


def record():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from msm_webgpu_amd import api

    calls, before = [], dict(api._fr_libs)
    api._fr_libs.update({name: Recorder(calls) for name in LIBRARIES})
    try:
        _drive(api)
    finally:
        api._fr_libs.clear()
        api._fr_libs.update(before)
    return calls


def test_the_wrappers_make_the_recorded_calls():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record()))
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d: %s" % (k, w[0])


def test_every_host_form_is_driven():
    from msm_webgpu_amd import scalars

    host = {"msm_%s_%s" % (lib, fn) for lib, table in scalars.FR_ABI.items() for fn in table if not fn.endswith("_device")}
    assert set(scalars.FR_ABI) == set(LIBRARIES)
    with open(GOLDEN) as f:
        driven = {fn for fn, _ in json.load(f)}
    assert driven <= host and host - driven == UNREACHABLE
    assert 4 * len(UNREACHABLE) <= len(host)


if __name__ == "__main__":
    print(json.dumps(record(), indent=1))
