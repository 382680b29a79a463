"""Pure-Python model of libmsm_frpoly.so (include/msm_frpoly.h) over Python integers: plain Horner, not the tiled algorithm.  Values are PLAIN
integers below r; a vector in the mont256 form is taken out of it and put back with mont()."""


def evaluate(a, z, r):
    """sum a[j] z^j"""
    h = 0
    for x in reversed(a):
        h = (x + z * h) % r
    return h


def divide(a, z, r):
    """-> (q, a(z)): q[i] = sum_{j > i} a[j] z^(j - i - 1), q[n - 1] = 0 -- the coefficients of (a(X) - a(z)) / (X - z) at length n"""
    n = len(a)
    q, h = [0] * n, 0
    for i in range(n - 1, -1, -1):
        q[i] = h
        h = (a[i] + z * h) % r
    return q, h


def dot(a, b, r):
    return sum(x * y for x, y in zip(a, b)) % r


def combine(rows, coeffs, r):
    """rows: len(coeffs) lists of the same length"""
    return [sum(c * row[i] for c, row in zip(coeffs, rows)) % r for i in range(len(rows[0]))]


def powers(g, n, r, scale=1):
    out, x = [], scale % r
    for _ in range(n):
        out.append(x)
        x = x * g % r
    return out


def rows_of(a, batch):
    n = len(a) // batch
    assert n * batch == len(a)
    return [a[v * n:(v + 1) * n] for v in range(batch)]


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
