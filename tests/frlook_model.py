"""Lookup arguments in Python integers: what libmsm_frlook.so (include/msm_frlook.h) computes -- the multiplicity column m[j] = #{(row, i) :
f[row][i] = t[j]} credited to the LOWEST index of a repeated table value, the table index of every looked-up value, the missing elements --
and how it gets there: the hash of a key, the slot array and the probe sequence of csrc/frlook_kernels.h, so that the slots of the host program
can be compared word by word."""

EMPTY = MISSING = 0xFFFFFFFF
NO_MISSING = (1 << 64) - 1
M32 = 0xFFFFFFFF


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


# ---- the semantics -------------------------------------------------------------------------------------------------------------------------------------
def lookup(table, rows, n=None):
    """table: the keys AS STORED; rows: lists of looked-up values as stored, of which the first n (default: all) of each are looked up
    -> (counts[n_t], idx[batch * n], missing, first_missing, distinct)"""
    first = {}
    for j, v in enumerate(table):
        first.setdefault(v, j)
    counts, idx, missing, first_missing = [0] * len(table), [], 0, NO_MISSING
    for row in rows:
        for v in (row if n is None else row[:n]):
            j = first.get(v, MISSING)
            if j == MISSING:
                missing += 1
                first_missing = min(first_missing, len(idx))
            else:
                counts[j] += 1
            idx.append(j)
    return counts, idx, missing, first_missing, len(first)


def multiplicities(counts, r, mont256=False):
    """the counts as scalars of the data's form: k, or k * 2^256 mod r"""
    return mont(counts, r) if mont256 else list(counts)


def logup(table, rows, beta, r):
    """plain integers -> (m, h_f, h_t, sum h_f, sum h_t): h_f[i] = sum_rows 1 / (beta + f[i]), h_t[j] = m[j] / (beta + t[j]), with 1 / 0 = 0"""
    def inv(v):
        return pow(v % r, r - 2, r)

    m = lookup(table, rows)[0]
    h_f = [sum(inv(beta + row[i]) for row in rows) % r for i in range(len(rows[0]))]
    h_t = [k * inv(beta + t) % r for k, t in zip(m, table)]
    return m, h_f, h_t, sum(h_f) % r, sum(h_t) % r


# ---- the hash table -------------------------------------------------------------------------------------------------------------------------------------
def _rotl(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


def key_hash(v, bits=0):
    """MurmurHash3_x86_32 of the 32 little-endian bytes of v, seed 0x9e3779b9 (frl_hash); bits: the low bits kept (0 or 32: all)"""
    h = 0x9E3779B9
    for i in range(8):
        k = ((v >> (32 * i)) & M32) * 0xCC9E2D51 & M32
        k = _rotl(k, 15) * 0x1B873593 & M32
        h = (_rotl(h ^ k, 13) * 5 + 0xE6546B64) & M32
    h ^= 32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return h if bits in (0, 32) else h & ((1 << bits) - 1)


def slot_count(n_t):
    p = 1
    while p < n_t:
        p <<= 1
    return 2 * p


def build_slots(table, bits=0):
    """the slot array after the entries were inserted in index order (the host program's order) -> (slots, distinct)"""
    size = slot_count(len(table))
    slots, distinct = [EMPTY] * size, 0
    for j, v in enumerate(table):
        s = key_hash(v, bits) & (size - 1)
        while True:
            if slots[s] == EMPTY:
                slots[s] = j
                distinct += 1
                break
            if table[slots[s]] == v:
                slots[s] = min(slots[s], j)
                break
            s = (s + 1) & (size - 1)
    return slots, distinct


def probes(table, slots, v, bits=0):
    """how many slots a lookup of v reads"""
    size = len(slots)
    s, count = key_hash(v, bits) & (size - 1), 1
    while slots[s] != EMPTY and table[slots[s]] != v:
        s, count = (s + 1) & (size - 1), count + 1
    return count


def keys_hashing_to(slot, size, how_many, r, start=1):
    """the first `how_many` integers from `start` on whose full hash lands in `slot` of `size` slots: a chain that begins there"""
    out, v = [], start
    while len(out) < how_many:
        if key_hash(v) & (size - 1) == slot:
            out.append(v)
        v += 1
    assert v < r
    return out


# ---- the tables both the host test and the GPU test run ---------------------------------------------------------------------------------------------------
def table(name, r, rnd):
    """a named table of plain integers below r"""
    if name.startswith("random "):
        return [rnd.randrange(r) for _ in range(int(name.split()[1]))]
    if name.startswith("range "):  # keys that differ in word 0 only
        return list(range(int(name.split()[1])))
    if name == "word 7 only":  # keys that differ in the top word only
        return [k << 224 for k in range(64)]
    if name == "tripled":  # every value three times, interleaved
        base = [rnd.randrange(r) for _ in range(22)]
        return base + base + base
    if name == "identical":
        return [rnd.randrange(r)] * 65
    if name == "zero and r - 1":
        return [r - 1, 0, 1, r - 2, 0, r - 1]
    if name == "wrapping chain":  # five keys that start at the last slot of the 16 of an 8-entry table, three that start at slot 0
        return keys_hashing_to(15, 16, 5, r) + keys_hashing_to(0, 16, 3, r)
    raise KeyError(name)


TABLES = ("random 1", "random 2", "random 63", "random 64", "random 65", "random 1025", "range 64", "range 1025", "word 7 only", "tripled", "identical", "zero and r - 1",
          "wrapping chain")
