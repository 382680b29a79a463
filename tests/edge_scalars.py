"""Scalars that sit on the edges of C-bit signed window recoding (test infrastructure; no GPU, no oracle).

The engine cuts a scalar of `bits` bits into nwin windows of C bits, lowest first, and makes each a signed digit: chunk + carry, minus 2^C with a
carry into the next window when that reaches 2^(C-1) (recode.h, bias_scalar).  nwin is (254 + C) / C for 32-byte scalars and (8 w + C) / C for
narrow scalars of w bytes, so the top window holds a partial chunk (or nothing) plus the carry from below.  edge_values plants, for one value
width and one C:
  - every chunk 2^(C-1): a digit of -2^(C-1) and a carry through every window, into the top one;
  - every chunk 2^C - 1: digits of 0 and the same carry chain;
  - 2^(C-1) - 1 (the largest digit without a carry) and 2^(C-1) alone, at each window position;
  - a full top chunk, with and without a carry into it;
  - the largest value, 0 and 1; for 32-byte values (which must stay below the scalar field's r) also r - 1 and r - 2^(C-1).
Each value says which edges it claims: "min_digit" (some window's digit is -2^(C-1)) and "top_carry" (a carry enters the top window).
tests/test_edge_scalars.py checks those claims against an independent model of the recode.
Byte windows (U8 / U16) are unsigned digits of 8 bits: their edges are the 8-bit ones (C = 8), which plant 0x80, 0x7F and 0xFF in every byte."""
import numpy as np


def windows(bits, c, narrow):
    """windows of a C-bit recode of values of `bits` bits: the engine's nwin_of / narrow_nwin_of"""
    return (bits + c) // c if narrow else (254 + c) // c


def edge_values(bits, c, r=None):
    """[(name, value, claims)] for values of `bits` bits (narrow: 8 w; 32-byte: r's bit length, and then every value is < r) and C-bit windows"""
    narrow = r is None
    nwin = windows(bits, c, narrow)
    top = (1 << bits) - 1 if narrow else r - 1  # the format's largest value
    h = 1 << (c - 1)
    positions = [k * c for k in range(nwin) if k * c < bits]  # windows that hold value bits
    every = lambda chunk: sum(chunk << p for p in positions) & ((1 << bits) - 1)
    # the highest window with value bits, and a value whose bits there are all set
    t = positions[-1]
    top_chunk = ((1 << bits) - 1) ^ ((1 << t) - 1)
    chain = every(h) & ((1 << t) - 1)  # carries from window 0 up to window t
    full_t = t + c <= bits  # the window at t is a whole chunk, and the top window above it holds only the carry
    out = [("every_chunk_half", every(h), ("min_digit", "top_carry")),
           ("every_chunk_full", every((1 << c) - 1), ("top_carry",)),
           ("top_chunk_full", top_chunk, ("top_carry",) if full_t else ()),
           ("top_chunk_full_with_carry", top_chunk | chain, (("min_digit",) if t else ()) + ("top_carry",)),
           ("max", top, ()), ("zero", 0, ()), ("one", 1, ())]
    for p in positions:
        k = p // c
        out.append(("half_minus_one_at_%d" % k, ((h - 1) << p) & ((1 << bits) - 1), ()))
        if p + c <= bits:  # (2^(C-1) fits the window)
            out.append(("half_at_%d" % k, h << p, ("min_digit",) + (("top_carry",) if k + 2 == nwin else ())))
    if not narrow:
        out += [("r_minus_1", r - 1, ()), ("r_minus_half", r - h, ())]
        out = [(name, fit_below(v, r, t), claims) for name, v, claims in out]
    return out


def fit_below(v, r, t):
    """a 32-byte value below r that keeps v's bits under bit t (the top window's chunk): if v >= r, its chunk at t becomes one less than r's"""
    if v < r:
        return v
    return (v & ((1 << t) - 1)) | (((r >> t) - 1) << t)


def edge_vector(bits, c, n, seed, r=None):
    """n values: the edges of edge_values first (in its order; n = 1 takes the longest carry chain), then uniform values of `bits` bits (below r)"""
    edges = [v for _, v, _ in edge_values(bits, c, r)]
    rng = np.random.default_rng(seed)
    out = edges[:n]
    while len(out) < n:
        v = int.from_bytes(rng.bytes((bits + 7) // 8), "little") & ((1 << bits) - 1)
        out.append(v if r is None else v % r)
    return out
