"""Points of small prime order on the three curves with a cofactor (BLS12-381 G1, BN254 G2, BLS12-381 G2), from the big-integer models of
oracle/*_ref.py alone (test infrastructure).  On these curves the library multiplies ANY point of the curve by the scalar as an integer, so a
base of order 3 or 11 is a legal input -- and the one that drives a ladder's accumulator through acc = +-T and the identity again and again,
and that fills a fixed-base table with identity records.

Nothing is taken from memory but the three group orders, and each of them is checked where it is used: it must annihilate the curve point the
torsion point is derived from.  The small prime factors of a cofactor come from trial division below 2^20."""
import functools
import importlib

# #E(Fp) = h1 r on BLS12-381 G1; #E'(Fp2) = r (2p - r) on BN254's twist; #E'(Fp2) = r h2 on BLS12-381's
BLS12_381_H1 = 0x396C8C005555E1568C00AAAB0000AAAB
BLS12_381_H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5
COFACTOR_CURVES = ("bls12_381", "bn254_g2", "bls12_381_g2")
# the orders the tests use (each is found again by trial division before a point of that order is built)
ORDERS = {"bls12_381": (3, 11, 10177), "bn254_g2": (10069,), "bls12_381_g2": (13, 23)}
TRIAL_BOUND = 1 << 20


def ref_module(curve):
    return importlib.import_module("oracle.%s_ref" % curve)


def is_g2(ref):
    return hasattr(ref, "f2_mul")


def cofactor(curve):
    ref = ref_module(curve)
    return {"bls12_381": BLS12_381_H1, "bn254_g2": 2 * ref.P - ref.R, "bls12_381_g2": BLS12_381_H2}[curve]


@functools.lru_cache(maxsize=None)
def small_prime_factors(h):
    """{prime: multiplicity} for the prime factors of h below 2^20, by trial division"""
    out = {}
    for q in range(2, TRIAL_BOUND):
        while h % q == 0:
            out[q] = out.get(q, 0) + 1
            h //= q
    return out


def imul(ref, k, pt):
    """k pt for the INTEGER k >= 0, by double-and-add over ref.add (ref.mul reduces k modulo r first: wrong outside the subgroup of order r)"""
    assert k >= 0
    acc = None
    while k:
        if k & 1:
            acc = ref.add(acc, pt)
        pt = ref.add(pt, pt)
        k >>= 1
    return acc


def enc(ref, pt):
    """the wire record of a point, all-zero for the identity"""
    return ref.affine_to_bytes(pt) if is_g2(ref) else ref.affine_to_bytes64(pt)


def fp_sqrt(p, a):
    """a square root of a modulo p = 3 mod 4, or None"""
    assert p % 4 == 3
    a %= p
    y = pow(a, (p + 1) // 4, p)
    return y if y * y % p == a else None


def f2_sqrt(ref, a):
    """a square root of a = a0 + a1 u in Fp[u] / (u^2 + 1), p = 3 mod 4, or None.  With x = x0 + x1 u: x0^2 - x1^2 = a0 and 2 x0 x1 = a1, so
    x0^2 = (a0 +- s) / 2 for s^2 = a0^2 + a1^2 (the norm, which is a square of Fp exactly when a is one of Fp2) and x1 = a1 / (2 x0)."""
    p = ref.P
    a0, a1 = a[0] % p, a[1] % p
    if a1 == 0:
        y = fp_sqrt(p, a0)
        if y is not None:
            return (y, 0)
        return (0, fp_sqrt(p, -a0))  # (c u)^2 = -c^2, and -a0 is a square when a0 is not (p = 3 mod 4)
    s = fp_sqrt(p, a0 * a0 + a1 * a1)
    if s is None:
        return None
    half = pow(2, -1, p)
    for cand in ((a0 + s) * half % p, (a0 - s) * half % p):
        x0 = fp_sqrt(p, cand)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, p) % p)
            if ref.f2_sqr(x) == (a0, a1):
                return x
    return None


def curve_points(ref, count, seed=4242):
    """`count` points of the curve, with no regard to the subgroup.  G1: the model's sampler (try-and-increment on a seeded x).  G2: the twist
    y^2 = x^3 + b' solved for x = (1, 1), (2, 1), ..., with b' = y_G^2 - x_G^3 read off the model's generator."""
    if not is_g2(ref):
        pts = ref.sample_points(seed, count)
    else:
        b2 = ref.f2_sub(ref.f2_sqr(ref.G[1]), ref.f2_mul(ref.f2_sqr(ref.G[0]), ref.G[0]))
        pts, i = [], 0
        while len(pts) < count:
            i += 1
            x = (i, 1)
            y = f2_sqrt(ref, ref.f2_add(ref.f2_mul(ref.f2_sqr(x), x), b2))
            if y is not None:
                pts.append((x, y))
    assert all(pt is not None and ref.is_on_curve(pt) for pt in pts)
    return pts


@functools.lru_cache(maxsize=None)
def torsion_point(curve, f):
    """a point T of the curve of prime order f: f T = O and T != O.  A curve point S is pushed into the f-part of the group, Q = (N / f^e) S with
    N the group order and f^e the power of f in it, and multiplied by f for as long as that does not reach the identity.  (Dividing N by f
    alone would not do: the 11-torsion of BLS12-381 G1 is all rational, h1 = 3 * 11^2 * 10177^2 * ..., and N / 11 kills every point.)"""
    ref = ref_module(curve)
    h = cofactor(curve)
    e = small_prime_factors(h).get(f, 0)
    assert e > 0, "%d does not divide the cofactor of %s" % (f, curve)
    order = h * ref.R
    assert ref.R % f != 0
    for seed in curve_points(ref, 8):
        q = imul(ref, order // f ** e, seed)
        assert imul(ref, f ** e, q) is None, "the group order does not annihilate a point of the curve"
        if q is None:
            continue
        while True:
            nxt = imul(ref, f, q)
            if nxt is None:
                break
            q = nxt
        assert q is not None and ref.is_on_curve(q) and imul(ref, f, q) is None
        return q
    raise AssertionError("no point of order %d among the seeds" % f)


def multiples(ref, f, t):
    """[0 T, 1 T, ..., (f - 1) T] by repeated addition: the expected value of k T is entry k mod f"""
    out, acc = [], None
    for _ in range(f):
        out.append(acc)
        acc = ref.add(acc, t)
    assert acc is None and all(pt is not None for pt in out[1:])
    return out
