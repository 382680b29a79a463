"""Pure-Python model of libmsm_frmle.so under MSM_FRMLE_LOW_FIRST (include/msm_frmle.h) over Python integers, written from the definitions by
the bits of the index: the variable x_j of a table of 2^k values is bit j of the index, and the first challenge binds bit 0 -- element 2 i with
element 2 i + 1.  Values are PLAIN integers below r.  Nothing here comes from tests/frmle_model.py (the top-first model); tests/
test_frmle_low_abi.py holds the two against each other through the bit reversal of the index."""


def bit(i, j):
    return (i >> j) & 1


def fold(a, c, r):
    """x_0 (bit 0 of the index) bound to c: out[i] = a[2 i] + c (a[2 i + 1] - a[2 i]); the other variables move down one bit"""
    return [(a[2 * i] + c * (a[2 * i + 1] - a[2 * i])) % r for i in range(len(a) // 2)]


def eq(point, r, scale=1):
    """out[i] = scale prod_j (bit_j(i) ? point[j] : 1 - point[j])"""
    out = []
    for i in range(1 << len(point)):
        v = scale % r
        for j, z in enumerate(point):
            v = v * (z if bit(i, j) else 1 - z) % r
        out.append(v)
    return out


def evaluate(a, point, r):
    """sum_i a[i] prod_j (bit_j(i) ? point[j] : 1 - point[j])"""
    assert len(a) == 1 << len(point)
    return sum(x * w for x, w in zip(a, eq(point, r))) % r


def degree(terms):
    return max(len(rows) for _, rows in terms)


def round_values(rows, terms, r):
    """g(t), t = 0 .. D: sum_{i < n/2} sum_terms coeff prod_f (row_f[2 i] + t (row_f[2 i + 1] - row_f[2 i]))"""
    out = []
    for t in range(degree(terms) + 1):
        g = 0
        for i in range(len(rows[0]) // 2):
            for coeff, which in terms:
                p = coeff
                for f in which:
                    p = p * (rows[f][2 * i] + t * (rows[f][2 * i + 1] - rows[f][2 * i])) % r
                g += p
        out.append(g % r)
    return out


def prove(rows, terms, challenge, r):
    """-> (round values, point, every row's final value): round j binds x_j -- bit 0 of what is left -- to challenge(j, values)"""
    rows = [list(row) for row in rows]
    transcript, point = [], []
    while len(rows[0]) > 1:
        values = round_values(rows, terms, r)
        c = challenge(len(point), values) % r
        transcript.append(values)
        point.append(c)
        rows = [fold(row, c, r) for row in rows]
    return transcript, point, [row[0] for row in rows]


def gemini_folds(a, point, r):
    """[f_1, .., f_k]: f_0 = a, f_(j+1) = f_j with its lowest variable bound to point[j]"""
    out = []
    for u in point:
        a = fold(a, u, r)
        out.append(a)
    return out


def horner(coeffs, z, r):
    """sum_j coeffs[j] z^j"""
    v = 0
    for c in reversed(coeffs):
        v = (v * z + c) % r
    return v


def bit_reversed(a):
    """out[rev(i)] = a[i], rev over log2(len(a)) bits"""
    k = len(a).bit_length() - 1
    out = [0] * len(a)
    for i, x in enumerate(a):
        out[int(format(i, "0%db" % k)[::-1], 2) if k else 0] = x
    return out


def mont(vals, r, back=False):
    """plain values -> a * 2^256 mod r (back=True: the other way)"""
    f = pow(2, 256, r)
    if back:
        f = pow(f, -1, r)
    return [v * f % r for v in vals]


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
