"""The Poseidon2 permutation (Grassi, Khovratovich, Schofnegger 2023) over Python integers, written twice: `Poseidon2` in the structured form of
include/msm_frhash.h -- the M4 chain of additions and doublings, position sums across the blocks of four, the internal layer as one sum and t
products -- and `Poseidon2Dense` with the two linear layers as explicit t x t matrices, M_E and M_I = J + diag(mu).  tests/test_frhash2_host.py
asserts that the two agree; libmsm_frhash.so under MSM_FRHASH_POSEIDON2 must give either, byte for byte.  The sponge, the tree and its paths are
those of tests/frhash_model.py with the permutation swapped.  Pure Python."""
import random

from tests import frhash_model as M

WIDTHS = (2, 3, 4, 8, 12)
M4 = ((5, 7, 1, 3), (4, 6, 1, 1), (1, 3, 5, 7), (1, 1, 4, 6))


def m4_chain(x, r):
    """M4 x by the paper's eight additions and doublings"""
    t0, t1 = x[0] + x[1], x[2] + x[3]
    t2, t3 = 2 * x[1] + t1, 2 * x[3] + t0
    t4, t5 = 4 * t1 + t3, 4 * t0 + t2
    return [(t3 + t5) % r, t5 % r, (t2 + t4) % r, t4 % r]


def external_matrix(t):
    """M_E as t rows: circ(2, 1), circ(2, 1, 1), M4, or circ(2 M4, M4, ..)"""
    if t in (2, 3):
        return [[2 if i == j else 1 for j in range(t)] for i in range(t)]
    assert t in (4, 8, 12)
    if t == 4:
        return [list(row) for row in M4]
    return [[(2 if i // 4 == j // 4 else 1) * M4[i % 4][j % 4] for j in range(t)] for i in range(t)]


class Poseidon2(M.Poseidon):
    """rc: R_F t + R_P constants in the order of their use -- t per external round, one per internal round, t per external round; mu: what the
    published parameter files call mat_internal_diag_m_1 (the internal matrix's diagonal is mu[i] + 1)"""

    def __init__(self, r, t, full_rounds, partial_rounds, rc, mu, capacity=0, capacity_at=0, out_at=0):
        assert t in WIDTHS and len(rc) == full_rounds * t + partial_rounds and len(mu) == t and full_rounds % 2 == 0
        self.r, self.t, self.full_rounds, self.partial_rounds = r, t, full_rounds, partial_rounds
        self.rc, self.mu = list(rc), list(mu)
        self.capacity, self.capacity_at, self.out_at = capacity, capacity_at, out_at

    def external(self, s):
        r, t = self.r, self.t
        if t < 4:
            total = sum(s)
            return [(x + total) % r for x in s]
        blocks = [m4_chain(s[b:b + 4], r) for b in range(0, t, 4)]
        if t == 4:
            return blocks[0]
        position = [sum(block[p] for block in blocks) for p in range(4)]
        return [(block[p] + position[p]) % r for block in blocks for p in range(4)]

    def internal(self, s):
        total = sum(s)  # (taken before any element changes)
        return [(m * x + total) % self.r for m, x in zip(self.mu, s)]

    def permute(self, state):
        r, t, half = self.r, self.t, self.full_rounds // 2
        s, rc = list(state), iter(self.rc)
        assert len(s) == t
        s = self.external(s)
        for _ in range(half):
            s = self.external([pow(x + next(rc), 5, r) for x in s])
        for _ in range(self.partial_rounds):
            s[0] = pow(s[0] + next(rc), 5, r)
            s = self.internal(s)
        for _ in range(half):
            s = self.external([pow(x + next(rc), 5, r) for x in s])
        return s


class Poseidon2Dense(Poseidon2):
    """the same permutation with both linear layers as matrix-vector products"""

    def external(self, s):
        return [sum(m * x for m, x in zip(row, s)) % self.r for row in external_matrix(self.t)]

    def internal(self, s):
        t = self.t
        m_i = [[1 + (self.mu[i] if i == j else 0) for j in range(t)] for i in range(t)]
        return [sum(m * x for m, x in zip(row, s)) % self.r for row in m_i]


def random_parameters(r, t, full_rounds, partial_rounds, seed=0):
    """(rc, mu) drawn from a seeded generator: the tests' own parameters -- no published constant set is claimed"""
    rnd = random.Random("poseidon2 %d %d %d %d %d" % (r, t, full_rounds, partial_rounds, seed))
    return [rnd.randrange(r) for _ in range(full_rounds * t + partial_rounds)], [rnd.randrange(r) for _ in range(t)]


def sample(r, t, full_rounds=8, partial_rounds=56, seed=0, dense=False, **convention):
    rc, mu = random_parameters(r, t, full_rounds, partial_rounds, seed)
    return (Poseidon2Dense if dense else Poseidon2)(r, t, full_rounds, partial_rounds, rc, mu, **convention)
