"""The definitions of include/msm_frmem.h in pure Python, on lists of integers: the stable argsort, the access counters of a memory argument, the
levels and launches the library plans, the key sets the tests share, and the four multisets of read-only offline memory checking."""
MISSING = 0xFFFFFFFF
TILE = 1024
DIGITS = 256


def argsort(keys):
    """the index of the k-th smallest key; equal keys in ascending index order"""
    return sorted(range(len(keys)), key=lambda i: (keys[i], i))


def access(keys, n_t=None):
    """-> (rank, prev, counts, last, distinct) by the definitions; counts and last are None without a table"""
    seen, before = {}, {}
    rank, prev = [], []
    for i, a in enumerate(keys):
        rank.append(seen.get(a, 0))
        prev.append(before.get(a, MISSING))
        seen[a] = seen.get(a, 0) + 1
        before[a] = i
    if n_t is None:
        return rank, prev, None, None, len(seen)
    assert all(a < n_t for a in keys)
    return rank, prev, [seen.get(a, 0) for a in range(n_t)], [before.get(a, MISSING) for a in range(n_t)], len(seen)


def scan_levels(length, tile=TILE):
    """the lengths of a scan's levels: `length` entries, then one node per tile, until a level fits one tile"""
    out = [length]
    while out[-1] > tile:
        out.append(-(-out[-1] // tile))
    return out


def levels(n, tile=TILE):
    """the keys, their digit counts (256 per tile of keys), and the levels of nodes above those"""
    return [n] + scan_levels(DIGITS * -(-n // tile), tile)


def passes(bits):
    return -(-bits // 8)


def launches(n, bits, tile=TILE, access=False, table=False):
    """a pass: the digit counts, the sums upwards, the scans downwards, the scatter; access adds the fill (where counts or last are asked for), the
    scan of the heads over the sorted keys and the writes"""
    per_pass = 2 + 2 * (len(levels(n, tile)) - 2) + 1
    total = passes(bits) * per_pass
    if access:
        total += (1 if table else 0) + 2 * (len(scan_levels(n, tile)) - 1) + 1 + 1
    return total


# ---- key sets: name -> n keys below 2^bits ------------------------------------------------------------------------------------------------------------------
KEY_SETS = ("uniform", "all equal", "ascending", "descending", "top byte varies", "lowest byte varies", "i mod 3", "two alternating", "all zero", "all ones")


def keys(name, n, bits, rnd):
    top = (1 << bits) - 1
    if name == "uniform":
        out = [rnd.getrandbits(bits) for _ in range(n)]
    elif name == "all equal":
        out = [rnd.getrandbits(bits)] * n
    elif name == "ascending":  # (never decreasing; strictly ascending where 2^bits >= n)
        out = [(i << bits) // n for i in range(n)]
    elif name == "descending":
        out = [(i << bits) // n for i in reversed(range(n))]
    elif name == "top byte varies":
        low = rnd.getrandbits(bits) & ((1 << max(bits - 8, 0)) - 1)
        out = [rnd.getrandbits(min(bits, 8)) << max(bits - 8, 0) | low for _ in range(n)]
    elif name == "lowest byte varies":
        high = rnd.getrandbits(bits) & ~0xFF & top
        out = [high | rnd.getrandbits(min(bits, 8)) for _ in range(n)]
    elif name == "i mod 3":
        out = [min(i % 3, top) for i in range(n)]
    elif name == "two alternating":
        a, b = rnd.getrandbits(bits), rnd.getrandbits(bits)
        out = [a if i & 1 else b for i in range(n)]
    elif name == "all zero":
        out = [0] * n
    elif name == "all ones":
        out = [top] * n
    else:
        raise KeyError(name)
    assert len(out) == n and all(0 <= k <= top for k in out)
    return out


# ---- read-only offline memory checking ------------------------------------------------------------------------------------------------------------------------
def fingerprint(a, v, t, gamma, tau, r):
    return ((t * gamma + v) * gamma + a - tau) % r


def offline_products(table, addr, rank, counts, gamma, tau, r):
    """-> (init, final, rs, ws): the grand products of the four multisets' fingerprints"""
    out = [1, 1, 1, 1]
    for a, v in enumerate(table):
        out[0] = out[0] * fingerprint(a, v, 0, gamma, tau, r) % r
        out[1] = out[1] * fingerprint(a, v, counts[a], gamma, tau, r) % r
    for a, t in zip(addr, rank):
        out[2] = out[2] * fingerprint(a, table[a], t, gamma, tau, r) % r
        out[3] = out[3] * fingerprint(a, table[a], t + 1, gamma, tau, r) % r
    return tuple(out)
