"""The Poseidon permutation, the sponge over it, the Merkle tree and its paths over Python integers: what libmsm_frhash.so (include/msm_frhash.h)
must compute, byte for byte.  Also the Poseidon paper's parameter generator (Grain LFSR), written here on its own so that
msm_webgpu_amd.api.poseidon_parameters has something to be compared with.  Pure Python."""
import functools

DEFAULT_PARTIAL = {2: 56, 3: 57, 4: 56, 5: 60, 6: 60, 7: 63, 8: 64, 9: 63, 10: 60, 11: 66, 12: 60}  # alpha = 5, 128 bits, R_F = 8


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------------
def _grain_bits(r, t, full_rounds, partial_rounds):
    """the generator's output bits: an 80-bit LFSR, 160 outputs discarded, then of every pair the second bit where the first is 1"""
    state = []
    for value, width in ((1, 2), (0, 4), (r.bit_length(), 12), (t, 12), (full_rounds, 10), (partial_rounds, 10), ((1 << 30) - 1, 30)):
        state += [(value >> (width - 1 - i)) & 1 for i in range(width)]
    assert len(state) == 80

    def step():
        b = state[62] ^ state[51] ^ state[38] ^ state[23] ^ state[13] ^ state[0]
        state.pop(0)
        state.append(b)
        return b

    for _ in range(160):
        step()
    while True:
        first, second = step(), step()
        if first:
            yield second


@functools.lru_cache(maxsize=None)
def parameters(r, t, full_rounds=8, partial_rounds=None):
    """-> (round constants [(R_F + R_P) t], M as t rows): round constants rejected where >= r, then 2 t values reduced mod r (all redrawn
    while two coincide), M[i][j] = 1 / (x_i + y_j)"""
    partial_rounds = DEFAULT_PARTIAL[t] if partial_rounds is None else partial_rounds
    bits, n = _grain_bits(r, t, full_rounds, partial_rounds), r.bit_length()

    def draw():
        v = 0
        for _ in range(n):
            v = v << 1 | next(bits)
        return v

    rc = []
    while len(rc) < (full_rounds + partial_rounds) * t:
        v = draw()
        if v < r:
            rc.append(v)
    while True:
        xy = [draw() % r for _ in range(2 * t)]
        if len(set(xy)) == 2 * t:
            break
    mds = [[pow(xy[i] + xy[t + j], r - 2, r) for j in range(t)] for i in range(t)]
    return tuple(rc), tuple(tuple(row) for row in mds)


# ---- the permutation ---------------------------------------------------------------------------------------------------------------------------------
class Poseidon:
    def __init__(self, r, t, full_rounds, partial_rounds, rc, mds, capacity=0, capacity_at=0, out_at=0):
        assert len(rc) == (full_rounds + partial_rounds) * t and len(mds) == t and all(len(row) == t for row in mds) and full_rounds % 2 == 0
        self.r, self.t, self.full_rounds, self.partial_rounds = r, t, full_rounds, partial_rounds
        self.rc, self.mds = list(rc), [list(row) for row in mds]
        self.capacity, self.capacity_at, self.out_at = capacity, capacity_at, out_at

    def permute(self, state):
        r, t, half = self.r, self.t, self.full_rounds // 2
        s = list(state)
        assert len(s) == t
        for k in range(self.full_rounds + self.partial_rounds):
            s = [(s[i] + self.rc[k * t + i]) % r for i in range(t)]
            if k < half or k >= half + self.partial_rounds:
                s = [pow(x, 5, r) for x in s]
            else:
                s[0] = pow(s[0], 5, r)
            s = [sum(self.mds[i][j] * s[j] for j in range(t)) % r for i in range(t)]
        return s

    def hash(self, row, capacity=None, capacity_at=None, out_at=None):
        """the sponge of rate t - 1 over the elements of `row` (at least one); nothing is padded"""
        t = self.t
        capacity = self.capacity if capacity is None else capacity
        capacity_at = self.capacity_at if capacity_at is None else capacity_at
        out_at = self.out_at if out_at is None else out_at
        assert len(row) >= 1 and 0 <= capacity_at < t and 0 <= out_at < t
        others = [p for p in range(t) if p != capacity_at]
        s = [0] * t
        s[capacity_at] = capacity % self.r
        for b in range(0, len(row), t - 1):
            for p, x in zip(others, row[b:b + t - 1]):
                s[p] = (s[p] + x) % self.r
            s = self.permute(s)
        return s[out_at]

    def merkle(self, leaves):
        """-> the levels above the leaves, the first above them first, the root's last; arity t - 1 (1: each level hashes the single element below)"""
        a = self.t - 1
        levels, level = [], list(leaves)
        if a == 1:
            raise ValueError("arity 1 needs the number of levels: merkle_chain")
        assert len(level) >= a
        while len(level) > 1:
            assert len(level) % a == 0
            level = [self.hash(level[a * j:a * j + a]) for j in range(len(level) // a)]
            levels.append(level)
        return levels

    def merkle_chain(self, leaf, k):
        out = []
        for _ in range(k):
            leaf = self.hash([leaf])
            out.append(leaf)
        return out

    def path(self, leaves, levels, index):
        """the siblings of leaf `index`, level by level: k rows of arity - 1"""
        a = self.t - 1
        rows, below = [], list(leaves)
        for level in levels:
            first = index - index % a
            rows.append([below[first + p] for p in range(a) if first + p != index])
            index //= a
            below = level
        return rows

    def verify(self, leaf, index, siblings, root):
        a = self.t - 1
        for row in siblings:
            at = index % a
            leaf = self.hash(list(row[:at]) + [leaf] + list(row[at:]))
            index //= a
        return leaf == root


def standard(r, t, full_rounds=8, partial_rounds=None, **convention):
    partial_rounds = DEFAULT_PARTIAL[t] if partial_rounds is None else partial_rounds
    rc, mds = parameters(r, t, full_rounds, partial_rounds)
    return Poseidon(r, t, full_rounds, partial_rounds, rc, mds, **convention)


def to_bytes(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def mont(values, r):
    return [v * pow(2, 256, r) % r for v in values]


def unmont(values, r):
    inv = pow(pow(2, 256, r), r - 2, r)
    return [v * inv % r for v in values]
