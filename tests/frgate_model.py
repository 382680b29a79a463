"""Pure-Python model of libmsm_frgate.so (include/msm_frgate.h) and of MsmContext.quotient over Python integers: the definitions, nothing of how
the device goes about them.  Values are PLAIN integers below r; data in the mont256 form are taken out of it and put back with mont()."""


def factors_of(term):
    """(coeff, factors) -> (coeff, [(row, rotation), ..]): a factor is a row number or a pair (row, rotation)"""
    coeff, factors = term
    return coeff, [(f, 0) if isinstance(f, int) else (int(f[0]), int(f[1])) for f in factors]


def degree(terms):
    return max(len(factors) for _, factors in terms)


def apply(rows, terms, n, step, scale, acc, r):
    """out[i] = (acc[i] if acc else 0) + scale[i mod len(scale)] sum_t coeff_t prod_f rows[row_f][(i + rot_f step) mod n], i < n; scale, acc: None
    or lists"""
    terms = [factors_of(t) for t in terms]
    out = []
    for i in range(n):
        e = 0
        for coeff, factors in terms:
            p = coeff
            for row, rot in factors:
                p = p * rows[row][(i + rot * step) % n] % r
            e += p
        if scale is not None:
            e = e * scale[i % len(scale)]
        out.append(((acc[i] if acc is not None else 0) + e) % r)
    return out


def mont(vals, r, back=False):
    """plain values -> a * 2^256 mod r (back=True: the other way)"""
    f = pow(2, 256, r)
    if back:
        f = pow(f, r - 2, r)
    return [v * f % r for v in vals]


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def term_bytes(terms):
    """msm_frgate_term records: coeff[32], degree, rows[8], rots[8]"""
    import struct

    out = b""
    for coeff, factors in (factors_of(t) for t in terms):
        pad = (0,) * (8 - len(factors))
        out += int(coeff).to_bytes(32, "little") + struct.pack("<I8I8i", len(factors), *(tuple(f[0] for f in factors) + pad + tuple(f[1] for f in factors) + pad))
    return out


# ---- the quotient, by schoolbook arithmetic ---------------------------------------------------------------------------------------------------------
def evaluate(coeffs, x, r):
    s = 0
    for c in reversed(coeffs):
        s = (s * x + c) % r
    return s


def vanishing_inverse(log_n, log_ext, shift, omega_big, r):
    """1 / (shift^n omega_N^(n i) - 1), i < 2^log_ext: 1 / Z_H on the coset shift <omega_N>, N = n 2^log_ext, which has period 2^log_ext"""
    n = 1 << log_n
    g = pow(shift, n, r)
    return [pow((g * pow(omega_big, n * i, r) - 1) % r, r - 2, r) for i in range(1 << log_ext)]


def interpolate(values, omega, r, shift=1):
    """the coefficients of the polynomial of degree < len(values) with p(shift omega^i) = values[i], by the schoolbook inverse transform"""
    m = len(values)
    wi, inv, gi = pow(omega, r - 2, r), pow(m, r - 2, r), pow(shift, r - 2, r)
    powers = [pow(wi, k, r) for k in range(m)]
    return [sum(values[j] * powers[i * j % m] for j in range(m)) * inv % r * pow(gi, i, r) % r for i in range(m)]


def quotient(columns, terms, log_n, log_ext, shift, omega_big, r):
    """columns: lists of n coefficients.  The N = n 2^log_ext coefficients of t(X) = E(X) / Z_H(X), E = sum_t coeff_t prod_f column_f(omega^rot_f X),
    omega = omega_big^(2^log_ext): E and 1 / Z_H on the coset shift <omega_big>, then the interpolation"""
    n, ext = 1 << log_n, 1 << log_ext
    big = n * ext
    domain = [shift * pow(omega_big, i, r) % r for i in range(big)]
    tables = [[evaluate(col, x, r) for x in domain] for col in columns]
    e = apply(tables, terms, big, ext, vanishing_inverse(log_n, log_ext, shift, omega_big, r), None, r)
    return interpolate(e, omega_big, r, shift)
