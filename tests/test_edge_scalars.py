"""The edge generator of the launch matrix (tests/edge_scalars.py) against an independent model of C-bit signed recoding: every value claims
only edges it reaches, every claimed edge is reached by some value, and every value fits its format.  No GPU."""
import pytest

from tests.edge_scalars import edge_values, edge_vector, windows

BN254_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BLS12_381_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PALLAS_R = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001  # Pallas' scalar field = Vesta's base field


def recode(v, c, nwin):
    """signed C-bit digits of v, low to high (a chunk plus the carry from below; from 2^(C-1) on it becomes negative and carries one), and the
    carry INTO each window"""
    digits, carries_in, carry = [], [], 0
    for k in range(nwin):
        carries_in.append(carry)
        d = ((v >> (k * c)) & ((1 << c) - 1)) + carry
        carry = 1 if d >= 1 << (c - 1) else 0
        digits.append(d - (carry << c))
    assert carry == 0, "the recode does not fit %d windows" % nwin
    assert sum(d << (k * c) for k, d in enumerate(digits)) == v
    return digits, carries_in


# (value bits, window bits, r): the narrow formats at every width they run at (byte windows: the 8-bit edges), the 32-byte ones on three fields
CASES = [(8, 8, None), (16, 8, None)] + [(8 * w, c, None) for w in (4, 8) for c in (12, 14, 16)] + \
        [(r.bit_length(), c, r) for r in (BN254_R, BLS12_381_R, PALLAS_R) for c in (12, 14, 16)]


@pytest.mark.parametrize("bits,c,r", CASES, ids=["%d-%d-%s" % (b, c, "narrow" if r is None else hex(r)[:6]) for b, c, r in CASES])
def test_claimed_edges_are_reached(bits, c, r):
    nwin = windows(bits, c, r is None)
    edges = edge_values(bits, c, r)
    reached = set()
    for name, v, claims in edges:
        assert v >= 0, name
        if r is None:
            assert v < 1 << bits, (name, hex(v))
        else:
            assert v < r, (name, hex(v))
        digits, carries_in = recode(v, c, nwin)
        got = set()
        if -(1 << (c - 1)) in digits:
            got.add("min_digit")
        if carries_in[-1]:
            got.add("top_carry")
        for claim in claims:
            assert claim in got, (name, hex(v), claim, digits)
        reached |= got
        if r is None:
            assert all(abs(d) <= 1 << (c - 1) for d in digits)
    assert reached == {"min_digit", "top_carry"}
    names = [name for name, _, _ in edges]
    assert len(names) == len(set(names))
    # every window position gets 2^(C-1) - 1 (the largest digit without a carry)
    assert sum(name.startswith("half_minus_one_at_") for name in names) == len([k for k in range(nwin) if k * c < bits])
    values = [v for _, v, _ in edges]
    assert 0 in values and 1 in values and ((1 << bits) - 1 if r is None else r - 1) in values
    if r is not None:
        assert r - (1 << (c - 1)) in values


@pytest.mark.parametrize("bits,c,r", [(32, 14, None), (64, 12, None), (254, 16, BN254_R)])
def test_edge_vector(bits, c, r):
    edges = [v for _, v, _ in edge_values(bits, c, r)]
    v = edge_vector(bits, c, 4097, seed=1, r=r)
    assert len(v) == 4097 and v[:len(edges)] == edges
    assert all(0 <= x < (r if r else 1 << bits) for x in v)
    assert edge_vector(bits, c, 1, seed=1, r=r) == [edges[0]]
    recode(edges[0], c, windows(bits, c, r is None))
    assert v == edge_vector(bits, c, 4097, seed=1, r=r)  # deterministic
