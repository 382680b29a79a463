"""The definitions of include/msm_frcol.h in pure Python, on lists of integers (a scalar is the integer of its 32 little-endian bytes AS STORED):
run expansion, halo2's permuted pair, gather, the levels of the scan, the count sets the tests share, and the properties the two lookup
arguments ask of their columns."""
MISSING = 0xFFFFFFFF
TILE = 1024


def to_bytes(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def from_bytes(b):
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


def total(counts, bias=0):
    """the sum of counts[j] + bias, never wrapped"""
    return sum(c + bias for c in counts)


def expand(t, counts, bias=0):
    """t[0] w[0] times, then t[1] w[1] times .. with w[j] = counts[j] + bias"""
    out = []
    for v, c in zip(t, counts):
        out += [v] * (c + bias)
    return out


def pair(t, counts):
    """-> (a_out, s_out, used) by the definition: off, r and z"""
    assert len(t) == len(counts) == sum(counts)
    z = [j for j, c in enumerate(counts) if c == 0]
    a_out, s_out, off, r = [], [], 0, 0
    for j, c in enumerate(counts):
        for d in range(c):
            k = off + d
            a_out.append(t[j])
            s_out.append(t[j] if d == 0 else t[z[k - r - 1]])
        off += c
        r += c > 0
    return a_out, s_out, r


def gather(a, idx):
    """-> (out, ok): zero for MISSING; zero and ok = False for any other index that is not below len(a)"""
    out = [a[i] if i < len(a) else 0 for i in idx]
    return out, all(i < len(a) or i == MISSING for i in idx)


def levels(n_t, tile=TILE):
    """the lengths of the scan's levels: the table, then one node per tile, until a level fits one tile -- always at least two"""
    out = [n_t]
    while True:
        out.append(-(-out[-1] // tile))
        if out[-1] <= tile:
            return out


def launches(n_t, tile=TILE):
    return 2 * len(levels(n_t, tile))


# ---- count sets: name -> counts of n_t entries that add up to `n` -------------------------------------------------------------------------------------------
COUNT_SETS = ("all ones", "all in the first", "all in the middle", "all in the last", "alternating 0 and 2", "zeros then one count", "random")


def counts(name, n_t, n, rnd):
    """n_t counts whose sum is n (for "all ones" and "alternating 0 and 2" as far as n allows: the rest goes to the last entry that has a count)"""
    c = [0] * n_t
    if name == "all ones":
        for j in range(min(n_t, n)):
            c[j] = 1
        c[min(n_t, n) - 1] += n - min(n_t, n)
    elif name.startswith("all in the"):
        c[{"first": 0, "middle": n_t // 2, "last": n_t - 1}[name.split()[-1]]] = n
    elif name == "alternating 0 and 2":
        left, last = n, 0
        for j in range(1, n_t, 2):
            if left >= 2:
                c[j], left, last = 2, left - 2, j
        c[last] += left
    elif name == "zeros then one count":  # a stretch of zeros (longer than two tiles where the table is) and then everything in one entry
        c[n_t - 1 if n_t < 4 else n_t - 2] = n
    elif name == "random":
        for _ in range(n):
            c[rnd.randrange(n_t) if rnd.random() < 0.7 else rnd.randrange(max(1, n_t // 8))] += 1
    else:
        raise KeyError(name)
    assert sum(c) == n and len(c) == n_t
    return c


# ---- what the arguments ask ---------------------------------------------------------------------------------------------------------------------------------
def halo2_holds(a, t, a_perm, s_perm):
    """A' a permutation of a, S' of t (multisets), A'[0] = S'[0], and every later A'[i] is S'[i] or A'[i - 1]"""
    return (sorted(a_perm) == sorted(a) and sorted(s_perm) == sorted(t) and a_perm[0] == s_perm[0]
            and all(a_perm[i] in (s_perm[i], a_perm[i - 1]) for i in range(1, len(a_perm))))


def plookup_holds(f, t, s):
    """s is f and t together (multisets), and every adjacent pair of s is an equal pair or a pair of neighbours of t"""
    steps = set(zip(t, t[1:]))
    return sorted(s) == sorted(list(f) + list(t)) and all(x == y or (x, y) in steps for x, y in zip(s, s[1:]))


def lookup_counts(t, f):
    """the counts libmsm_frlook.so writes: every match at the LOWEST index of its value"""
    first = {}
    for j, v in enumerate(t):
        first.setdefault(v, j)
    c = [0] * len(t)
    for v in f:
        c[first[v]] += 1
    return c


def grand_product(a, t, a_perm, s_perm, beta, gamma, r):
    """halo2's z: z[i] = prod_{k < i} (a[k] + beta)(t[k] + gamma) / ((a'[k] + beta)(s'[k] + gamma)), and the closing value; 1 / 0 = 0"""
    z, acc = [], 1
    for k in range(len(a)):
        z.append(acc)
        den = (a_perm[k] + beta) * (s_perm[k] + gamma) % r
        acc = acc * (a[k] + beta) * (t[k] + gamma) * pow(den, r - 2, r) % r
    return z, acc
