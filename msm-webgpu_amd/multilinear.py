"""Multilinear tables with the variable x_j at bit j of the index -- arkworks' order (DenseMultilinearExtension::fix_variables, ml_sumcheck),
HyperPlonk's and Jolt's, and the order of the multilinear-to-univariate folds of Gemini, HyperKZG and Zeromorph -- over libmsm_frmle.so with
MSM_FRMLE_LOW_FIRST (include/msm_frmle.h): the first challenge binds the LOWEST bit, pairing element 2 i with element 2 i + 1, where the
scalars_mle_* methods of a context pair i with i + n / 2.

Module-level functions that take a context (an MsmContext), as columns.py has them; api.py, scalars.py, _core.py and the package's __init__ do
not import this module.  order="low" (the default) sets the flag; order="top" leaves it out and returns what the context's method of the
same call returns, byte for byte.  Every curve's scalar field, Grumpkin's included -- gemini_open excepted, which needs scalars_eval.

In place, a low-first bind leaves the first n / 2 scalars of every row as its result and the scalars [n / 2, n) of the row UNSPECIFIED (the
top-first bind leaves them as they were); the scalars [n, stride) are not touched."""
import torch

from ._core import _as_device_u8
from .scalars import FrmleTerm, _const32, _dest, _host_out, _pack_terms, _ptr, _result

LOW_FIRST = 8  # MSM_FRMLE_LOW_FIRST


def _flags(ctx, order):
    return ctx._mont256_flag() | (LOW_FIRST if order == "low" else 0)


def _order_checked(order):
    if order not in ("low", "top"):
        raise ValueError("order is 'low' (x_j at bit j of the index) or 'top' (x_j at bit k - 1 - j), not %r" % (order,))


def fold(ctx, a, c, batch=1, n=None, out=None, order="low"):
    """Bind the first variable of `batch` tables to c (msm_frmle_fold_device): low first row[i] = row[2 i] + c (row[2 i + 1] - row[2 i]), i < n / 2.
    a, c, batch, n, out: as MsmContext.scalars_mle_fold -- in place on a device tensor (the scalars [n / 2, n) of every row are then unspecified
    under order="low") or into `out` (only the first n / 2 scalars of every row are written, a is only read); host bytes return bytes."""
    _order_checked(order)
    r = ctx._scalar_field("multilinear.fold", grumpkin=True)
    ta, ba, n, stride = ctx._frmle_rows(a, batch, n, 2)
    batch = int(batch)
    cb = _const32(c, r, "c")
    res, dst = _dest(ta, ctx._frvec_out(out, ta, stride * batch, ta is not None), stride * batch, init=ba)
    ctx._fr_call("frmle", "fold", ta, None, dst, _ptr(ta, ba), n, batch, stride, cb, _flags(ctx, order))
    return _result(res)


def evaluate(ctx, a, point, batch=1, n=None, order="low"):
    """The multilinear extensions of `batch` tables at `point` (msm_frmle_eval_device) -> batch x 32 host bytes in the data's form; low first
    point[j] is the variable at bit j of the index.  Arguments as MsmContext.scalars_mle_eval; nothing is written."""
    _order_checked(order)
    r = ctx._scalar_field("multilinear.evaluate", grumpkin=True)
    ta, ba, n, stride = ctx._frmle_rows(a, batch, n, 1)
    batch = int(batch)
    point = list(point)
    if len(point) != n.bit_length() - 1:
        raise ValueError("a table of %d scalars has %d variables, the point %d" % (n, n.bit_length() - 1, len(point)))
    pb = b"".join(_const32(z, r, "a coordinate of the point") for z in point)
    values, values_ptr = _host_out(batch)
    ctx._fr_call("frmle", "eval", ta, None, _ptr(ta, ba), n, batch, stride, pb, _flags(ctx, order), values_ptr)
    return values.raw


def eq(ctx, point, scale=1, out=None, order="low"):
    """The table of scale * eq(point, .) as a CUDA uint8 tensor of 2^k x 32 bytes (msm_frmle_eq_device): low first
    out[i] = scale prod_j (bit_j(i) ? point[j] : 1 - point[j]).  Arguments as MsmContext.scalars_eq."""
    _order_checked(order)
    r = ctx._scalar_field("multilinear.eq", grumpkin=True)
    point = list(point)
    if len(point) > 26:
        raise ValueError("a table holds at most 2^26 scalars, not 2^%d" % len(point))
    n = 1 << len(point)
    pb = b"".join(_const32(z, r, "a coordinate of the point") for z in point)
    cb = _const32(scale, r, "scale")
    out = ctx._new_out(out, n)
    ctx._fr_call("frmle", "eq", out, None, out.data_ptr(), n, pb, cb, _flags(ctx, order))
    return out


def sumcheck_round(ctx, a, terms, batch=1, n=None, fold=None, order="low"):
    """The values g(0) .. g(D) of a round polynomial (msm_frmle_round_device) -> (D + 1) x 32 host bytes in the data's form: low first
    g(t) = sum_{i < n/2} sum_terms coeff prod_f (row_f[2 i] + t (row_f[2 i + 1] - row_f[2 i])).  fold: None, or the previous round's challenge: the
    call first binds the lowest variable of ALL rows to it in place (as fold(); n >= 4) and returns the round values of the folded tables.
    Arguments and the host form as MsmContext.scalars_sumcheck_round."""
    _order_checked(order)
    r = ctx._scalar_field("multilinear.sumcheck_round", grumpkin=True)
    ta, ba, n, stride = ctx._frmle_rows(a, batch, n, 2 if fold is None else 4)
    batch = int(batch)
    if batch > ctx.FRMLE_MAX_ROWS:
        raise ValueError("a round takes at most %d rows, not %d" % (ctx.FRMLE_MAX_ROWS, batch))
    arr, top = _pack_terms(terms, batch, r, FrmleTerm, "round", ctx.FRMLE_MAX_TERMS, ctx.FRMLE_MAX_DEGREE)
    fb = None if fold is None else _const32(fold, r, "fold")
    values, values_ptr = _host_out(ctx.FRMLE_MAX_DEGREE + 1)
    res, dst = _dest(ta, None, stride * batch, init=ba)  # (the host form reads and, with fold, writes a copy of the bytes)
    ctx._fr_call("frmle", "round", ta, None, dst, n, batch, stride, arr, len(arr), fb, _flags(ctx, order), values_ptr)
    got = values.raw[:32 * (top + 1)]
    return got if ta is not None or fold is None else (got, res.raw)


def sumcheck_prove(ctx, a, terms, batch, challenge, order="low"):
    """The prover's side of a sumcheck over `batch` tables of N = 2^k scalars, as MsmContext.sumcheck_prove (a: a CUDA uint8 tensor, DESTROYED)
    -- round j binds x_j, low first the variable at bit j of the index, so the transcript is the one an arkworks-order verifier checks.
    -> (the k rounds' values, the k challenges, every row's value at that point as batch x 32 bytes)."""
    _order_checked(order)
    r = ctx._scalar_field("multilinear.sumcheck_prove", grumpkin=True)
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        raise TypeError("sumcheck_prove runs in place on a CUDA(HIP) uint8 tensor")
    _, _, n, _ = ctx._frmle_rows(a, batch, None, 1)
    rounds, point = [], []
    while n >> len(point) > 1:
        j = len(point)
        values = sumcheck_round(ctx, a, terms, batch, n >> max(j - 1, 0), fold=point[-1] if j else None, order=order)
        c = int(challenge(j, values))
        if not 0 <= c < r:
            raise ValueError("challenge %d is not in [0, r)" % j)
        rounds.append(values)
        point.append(c)
    # the last challenge binds what is left of every row: two scalars (one variable: the orders agree), or -- N = 1 -- the row itself
    finals = evaluate(ctx, a, point[-1:], batch, 2 if point else 1, order=order)
    return rounds, point, finals


def _one_row(ctx, a, what):
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        raise TypeError("%s takes a CUDA(HIP) uint8 tensor" % what)
    t, n = _as_device_u8(a, 32, "a")
    if n < 2 or n & (n - 1) or n > 1 << 26:
        raise ValueError("%s takes 2^k scalars, 1 <= k <= 26, not %d" % (what, n))
    return t, n


def gemini_folds(ctx, a, point):
    """The folds of Gemini's (HyperKZG's, Zeromorph's) multilinear-to-univariate reduction of one table of N = 2^k scalars, k >= 1, on the
    device (a: a CUDA uint8 tensor, left as it is): f_0 = a, f_(j+1)[i] = f_j[2 i] + point[j] (f_j[2 i + 1] - f_j[2 i]) -> ONE new tensor of N - 1
    scalars, f_1 | f_2 | .. | f_k of N/2, N/4, .., 1 scalars; its last scalar, f_k[0], is the multilinear value of a at `point`.  k low-first
    folds, each out of the previous slice into the next: k launches and no copy."""
    r = ctx._scalar_field("multilinear.gemini_folds", grumpkin=True)
    t, n = _one_row(ctx, a, "gemini_folds")
    point = list(point)
    if len(point) != n.bit_length() - 1:
        raise ValueError("a table of %d scalars has %d variables, the point %d" % (n, n.bit_length() - 1, len(point)))
    cs = [_const32(z, r, "a coordinate of the point") for z in point]
    out = torch.empty((n - 1, 32), dtype=torch.uint8, device=t.device)
    flags = ctx._mont256_flag() | LOW_FIRST
    src, at, m = t.data_ptr(), 0, n  # f_j: m scalars at src; f_(j+1) goes to scalar `at` of out
    for j, cb in enumerate(cs):
        dst = out.data_ptr() + 32 * at
        ctx._fr_call("frmle", "fold", t if j == 0 else out, None, dst, src, m, 1, m, cb, flags)
        src, at, m = dst, at + m // 2, m // 2
    return out


def gemini_slices(n):
    """[(first scalar, scalars)] of f_1 .. f_k in the tensor gemini_folds returns for a table of n = 2^k scalars"""
    out, at, m = [], 0, n // 2
    while m >= 1:
        out.append((at, m))
        at, m = at + m, m // 2
    return out


def gemini_open(ctx, coeffs, point, challenge):
    """The prover's first two moves of a Gemini / HyperKZG opening of the multilinear polynomial with the table `coeffs` (a CUDA uint8 tensor of
    N = 2^k scalars, N <= the resident bases, which are a monomial SRS tau^j G as for kzg_open) at `point`: the folds f_1 .. f_k (gemini_folds),
    the commitments C_j = msm(f_j), j = 1 .. k - 1, to them as univariate polynomials, r = int(challenge(commitments)) in [1, r), and
    f_j(r), f_j(-r), f_j(r^2) for j = 0 .. k - 1 (scalars_eval).  -> (value, commitments, r, evals): value = f_k[0], the multilinear value, as 32
    bytes in the data's form; evals: k x 3 x 32 host bytes in the data's form.  The verifier's check, for every j < k with u_j = point[j]:
    f_(j+1)(r^2) = (1 - u_j) (f_j(r) + f_j(-r)) / 2 + u_j (f_j(r) - f_j(-r)) / (2 r), f_k(r^2) being `value`.  The batched KZG witnesses of the
    three evaluation points are kzg_open over a combination the caller forms."""
    order_r = ctx._scalar_field("multilinear.gemini_open")
    t, n = _one_row(ctx, coeffs, "gemini_open")
    if n > ctx.n_bases:
        raise ValueError("%d coefficients, but %d resident bases" % (n, ctx.n_bases))
    folds = gemini_folds(ctx, t, point)
    slices = gemini_slices(n)
    polys = [t] + [folds[at:at + m] for at, m in slices[:-1]]  # f_0 .. f_(k-1)
    commitments = [ctx.msm(f) for f in polys[1:]]
    r = int(challenge(commitments))
    if not 1 <= r < order_r:
        raise ValueError("the challenge is not in [1, r)")
    zs = (r, order_r - r, r * r % order_r)
    evals = b"".join(ctx.scalars_eval(f, z) for f in polys for z in zs)
    value = bytes(folds[-1].cpu().numpy().tobytes())
    return value, commitments, r, evals
