"""Pure-Python model of libmsm_frmle.so (include/msm_frmle.h) over Python integers: the definitions, not the tiled algorithm.  Values are PLAIN
integers below r; a table in the mont256 form is taken out of it and put back with mont().  The FIRST variable is the TOP bit of the index:
binding pairs element i with element i + n / 2."""


def fold(a, c, r):
    """the top variable bound to c: n / 2 values"""
    h = len(a) // 2
    return [(a[i] + c * (a[i + h] - a[i])) % r for i in range(h)]


def evaluate(a, point, r):
    """the multilinear extension of a (2^len(point) values) at point"""
    assert len(a) == 1 << len(point)
    for z in point:
        a = fold(a, z, r)
    return a[0] % r


def eq(point, r, scale=1):
    """out[i] = scale prod_j (bit_(k-1-j)(i) ? point[j] : 1 - point[j])"""
    out = [scale % r]
    for z in point:  # (the next variable is the next LOWER bit)
        out = [v for x in out for v in (x * (1 - z) % r, x * z % r)]
    return out


def eq1(w, t, r):
    return (w * t + (1 - w) * (1 - t)) % r


def eq_value(w, z, r):
    """eq(w, z) = prod_j (w_j z_j + (1 - w_j)(1 - z_j))"""
    v = 1
    for x, y in zip(w, z):
        v = v * eq1(x, y, r) % r
    return v


def degree(terms):
    return max(len(rows) for _, rows in terms)


def round_values(rows, terms, r):
    """g(t), t = 0 .. D, of g(t) = sum_{i < n/2} sum_terms coeff prod_f (lo_f + t (hi_f - lo_f)); rows: lists of n values; terms: [(coeff, (row, ..)), ..]"""
    h = len(rows[0]) // 2
    out = []
    for t in range(degree(terms) + 1):
        g = 0
        for i in range(h):
            for coeff, which in terms:
                p = coeff
                for f in which:
                    p = p * (rows[f][i] + t * (rows[f][i + h] - rows[f][i])) % r
                g += p
        out.append(g % r)
    return out


def claimed_sum(rows, terms, r):
    """sum_x sum_terms coeff prod_f row_f[x]"""
    s = 0
    for i in range(len(rows[0])):
        for coeff, which in terms:
            p = coeff
            for f in which:
                p = p * rows[f][i] % r
            s += p
    return s % r


def interpolate(values, x, r):
    """the polynomial of degree < len(values) through (t, values[t]), t = 0 .., at x"""
    total = 0
    for t, v in enumerate(values):
        num = den = 1
        for u in range(len(values)):
            if u != t:
                num = num * (x - u) % r
                den = den * (t - u) % r
        total += v * num * pow(den, r - 2, r)
    return total % r


def prove(rows, terms, challenge, r):
    """-> (round values, point, every row's final value): the k rounds, each followed by challenge(round, values) -> int"""
    rows = [list(row) for row in rows]
    transcript, point = [], []
    while len(rows[0]) > 1:
        values = round_values(rows, terms, r)
        c = challenge(len(point), values) % r
        transcript.append(values)
        point.append(c)
        rows = [fold(row, c, r) for row in rows]
    return transcript, point, [row[0] for row in rows]


def verify(claim, transcript, point, finals, terms, r):
    """the verifier: g_j(0) + g_j(1) is the running claim, which becomes g_j(c_j); the last one is the terms over the rows' final values"""
    for values, c in zip(transcript, point):
        if (values[0] + values[1]) % r != claim % r:
            return False
        claim = interpolate(values, c, r)
    return claim == claimed_sum([[v] for v in finals], terms, r)


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
