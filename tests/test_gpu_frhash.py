"""Poseidon on the device (include/msm_frhash.h; MsmContext.poseidon, scalars_permute, scalars_hash, merkle_tree) against the pure-Python model
(tests/frhash_model.py), byte for byte: batches of 1, 63, 64, 65 and 257 permutations at t = 2, 3, 5, 9 and 12 on BN254 and BLS12-381, at
t = 3 on the other three fields and at one width of their tidy boundary each, both data forms, in place and out of place, and again with four
lanes to a workgroup; every field's two widths on either side of the width from which the S-box input is tidied, at either alignment; sponges
of every length at which the last block is empty, short or full, with a stride whose padding is not below r and must not be read, under the
three capacity conventions; trees of arity 2, 4, 8, 11 and 1, every node compared, with and without the short tile; the known answer; the
rejection of a value >= r at the first, a middle and the last position with a correct call right behind it; the same bytes on a second run."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frhash_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
ERR_NONCANONICAL = -4
WIDTHS = (2, 3, 5, 9, 12)
COUNTS = (1, 63, 64, 65, 257)
CASES = [(c, t) for c in ("bn254", "bls12_381") for t in WIDTHS] + [(c, 3) for c in ("grumpkin", "pallas", "vesta")] + [("grumpkin", 9), ("pallas", 7), ("vesta", 8)]


@pytest.fixture(scope="module")
def contexts(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(curve="bn254", mont=False):
        if curve not in made:
            made[curve] = m.MsmContext(0, curve)
        made[curve].set_scalar_format(mont256=mont)
        return made[curve]

    yield get
    api.frhash_test_tile(0)
    for c in made.values():
        c.close()
    api.frhash_release()


_reference = {}


def reference(curve, t):
    """the model's permutation of 257 states, computed once: (the model, the states, their images)"""
    if (curve, t) not in _reference:
        r, rnd = api.SCALAR_FIELDS[curve], rng(1000 + t)
        p = M.standard(r, t)
        states = [[r - 1] * t, [0] * t] + [[rnd.randrange(r) for _ in range(t)] for _ in range(max(COUNTS) - 2)]
        _reference[(curve, t)] = (p, states, [p.permute(s) for s in states])
    return _reference[(curve, t)]


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


def host(t):
    return M.from_bytes(raw(t))


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def flat(rows):
    return [x for row in rows for x in row]


def handle(ctx, p):
    return ctx.poseidon(p.t, p.full_rounds, p.partial_rounds, capacity=p.capacity, capacity_at=p.capacity_at, out_at=p.out_at)


# ---- permutations ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,t", CASES, ids=["%s-t%d" % c for c in CASES])
def test_permutations_of_every_count_and_form(contexts, curve, t):
    r = api.SCALAR_FIELDS[curve]
    p, states, images = reference(curve, t)
    for mont in (False, True):
        ctx = contexts(curve, mont)
        with handle(ctx, p) as h:
            for tile in (0, 4):  # 64 lanes to a workgroup; four, so that 65 states span 17 workgroups
                api.frhash_test_tile(tile)
                for n in COUNTS:
                    src = dev(form(flat(states[:n]), r, mont))
                    before = raw(src)
                    want = M.to_bytes(form(flat(images[:n]), r, mont))
                    big = torch.full((3, n * t, 32), 0xFF, dtype=torch.uint8, device="cuda")  # out of place, into the middle of a buffer of 0xFF
                    got = ctx.scalars_permute(h, src, out=big[1])
                    assert got.data_ptr() == big[1].data_ptr() and raw(big[1]) == want, (curve, t, mont, tile, n)
                    assert raw(big[0]) == b"\xff" * (32 * n * t) and raw(big[2]) == b"\xff" * (32 * n * t) and raw(src) == before
                    assert raw(ctx.scalars_permute(h, src, out=src)) == want, (curve, t, mont, tile, n, "in place")
            api.frhash_test_tile(0)
            assert tuple(ctx.scalars_permute(h, dev(form(flat(states[:3]), r, mont))).shape) == (3, t, 32)
            assert ctx.scalars_permute(h, M.to_bytes(form(flat(states[:5]), r, mont))) == M.to_bytes(form(flat(images[:5]), r, mont))  # the host form


# ---- each field's tidy boundary -------------------------------------------------------------------------------------------------------------------
# frh_permute tidies the S-box input iff (t + 4)^2 > FQ_HEADROOM (70, 127, 127, 169, 169): the last width that is not tidied, the first that is
EDGE = {"bls12_381": (4, 5), "pallas": (7, 8), "vesta": (7, 8), "bn254": (9, 10), "grumpkin": (9, 10)}
EDGES = [(c, t) for c, widths in EDGE.items() for t in widths]


def shifted(data, shift, around=0):
    """the bytes on the device, `shift` (0 or 16) bytes into a 32-byte-aligned tensor, with `around` bytes of 0xFF on either side: (the whole, the view)"""
    whole = torch.full((shift + 2 * around + len(data),), 0xFF, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 32 == 0
    view = whole[shift + around:shift + around + len(data)]
    view.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return whole, view


@pytest.mark.parametrize("curve,t", EDGES, ids=["%s-t%d" % c for c in EDGES])
def test_the_widths_on_either_side_of_the_tidy_boundary(contexts, curve, t):
    """The device multiplies through csrc/fq29_asm.h, which the host program's FQ_CHECK run does not: the widest state whose S-box input is squared
    as it is, (t + 4)^2 of FQ_HEADROOM (for BN254 and Grumpkin at t = 9 all of it), and the next one, on the device.  State 0 is all r - 1, state
    1 all 0; the standard parameters, and constants and matrix all r - 1 with rounds (2, 1); 1 and 65 states; both forms; in place, and out of
    place into 0xFF with the 32 bytes on either side compared; operands at 0 and at 16 mod 32; 64 and four lanes to a workgroup.  The sponges
    take 2 (t - 1) + 1 elements, under halo2's convention on canonical data and neptune's on a * 2^256.  The model's time is the test's: 65
    permutations and twice 17 sponges of three blocks with the standard rounds, 65 of each with three rounds, and the standard parameters
    themselves -- 1.3 s at t = 10 on a CPU without a GPU, 0.4 s of it the parameters."""
    r, rnd = api.SCALAR_FIELDS[curve], rng(1400 + t)
    length = 2 * (t - 1) + 1
    states = [[r - 1] * t, [0] * t] + [[rnd.randrange(r) for _ in range(t)] for _ in range(63)]
    rows = [[r - 1] * length, [0] * length] + [[rnd.randrange(r) for _ in range(length)] for _ in range(63)]
    rc, mds = M.parameters(r, t)
    shapes = ((8, M.DEFAULT_PARTIAL[t], rc, mds, 17), (2, 1, [r - 1] * (3 * t), [[r - 1] * t] * t, 65))
    for rf, rp, rc, mds, n_rows in shapes:
        images = None
        for mont in (False, True):
            convention = dict(capacity=(1 << (t - 1)) - 1, capacity_at=0, out_at=1) if mont else dict(capacity=(length << 64) % r, capacity_at=t - 1, out_at=0)
            p = M.Poseidon(r, t, rf, rp, rc, mds, **convention)
            images = images or [p.permute(s) for s in states]
            hashes = [p.hash(row) for row in rows[:n_rows]]
            ctx = contexts(curve, mont)
            with ctx.poseidon(t, rf, rp, round_constants=list(rc), mds=[list(row) for row in mds], **convention) as h:
                for tile in (0, 4):
                    api.frhash_test_tile(tile)
                    for n in (1, 65):
                        for shift in (0, 16):
                            where = (curve, t, rf, rp, mont, tile, n, shift)
                            want = M.to_bytes(form(flat(images[:n]), r, mont))
                            _, src = shifted(M.to_bytes(form(flat(states[:n]), r, mont)), shift)
                            whole, out = shifted(bytes(len(want)), shift, around=32)
                            assert ctx.scalars_permute(h, src, out=out).data_ptr() == out.data_ptr() and src.data_ptr() % 32 == shift
                            assert raw(whole) == b"\xff" * (shift + 32) + want + b"\xff" * 32, where
                            assert raw(src) == M.to_bytes(form(flat(states[:n]), r, mont)), where
                            ctx.scalars_permute(h, src, out=src)
                            assert raw(src) == want, where + ("in place",)
                            k = min(n, n_rows)
                            _, a = shifted(M.to_bytes(form(flat(rows[:k]), r, mont)), shift)
                            whole, out = shifted(bytes(32 * k), shift, around=32)
                            ctx.scalars_hash(h, a, length, batch=k, out=out)
                            assert raw(whole) == b"\xff" * (shift + 32) + M.to_bytes(form(hashes[:k], r, mont)) + b"\xff" * 32, where + ("sponge",)
                api.frhash_test_tile(0)


def test_the_hash_is_of_the_values(contexts):
    """a canonical vector and its a * 2^256 image hash to each other's images; a G2 context takes its G1's field; two runs give the same bytes"""
    r = api.SCALAR_FIELDS["bn254"]
    p, states, images = reference("bn254", 3)
    plain = dev(flat(states[:65]))
    ctx = contexts("bn254", False)
    with ctx.poseidon() as h:
        one, two = ctx.scalars_permute(h, plain), ctx.scalars_permute(h, plain)
        assert raw(one) == raw(two) == M.to_bytes(flat(images[:65]))
        ctx = contexts("bn254", True)
        assert host(ctx.scalars_permute(h, dev(M.mont(flat(states[:65]), r)))) == M.mont(host(one), r)
    g2 = m.MsmContext(0, "bn254_g2")
    with g2.poseidon() as h:
        assert raw(g2.scalars_permute(h, plain)) == raw(one)
    g2.close()


def test_no_partial_rounds_and_parameters_of_the_callers(contexts):
    ctx = contexts("bls12_381", False)
    r, rnd = api.SCALAR_FIELDS["bls12_381"], rng(1100)
    for t, rf, rp in ((3, 8, 0), (12, 2, 0), (5, 16, 128), (4, 2, 1)):
        rc = [rnd.randrange(r) for _ in range((rf + rp) * t)]
        mds = [[rnd.randrange(r) for _ in range(t)] for _ in range(t)]
        rc[0], mds[0][0] = r - 1, r - 1
        p = M.Poseidon(r, t, rf, rp, rc, mds)
        states = [[rnd.randrange(r) for _ in range(t)] for _ in range(3)]
        with ctx.poseidon(t, rf, rp, round_constants=rc, mds=mds) as h:
            assert host(ctx.scalars_permute(h, dev(flat(states)))) == flat(p.permute(s) for s in states), (t, rf, rp)


# ---- sponges ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("t", WIDTHS)
def test_sponges_of_every_length_and_convention(contexts, curve, t):
    r, rnd = api.SCALAR_FIELDS[curve], rng(1200 + t)
    lengths = sorted({1, max(1, t - 2), t - 1, t, 2 * (t - 1), 2 * (t - 1) + 1})
    conventions = ((0, 0, 0), ((lengths[-1] << 64) % r, t - 1, 0), ((1 << (t - 1)) - 1, 0, 1))  # circomlib's, halo2's, neptune's
    rows = 5
    for k, (capacity, capacity_at, out_at) in enumerate(conventions):
        p = M.standard(r, t, capacity=capacity, capacity_at=capacity_at, out_at=out_at)
        mont = k == 1
        ctx = contexts(curve, mont)
        with handle(ctx, p) as h:
            for length in lengths:
                data = [[rnd.randrange(r) for _ in range(length)] for _ in range(rows)]
                data[0] = [r - 1] * length
                want = form([p.hash(row) for row in data], r, mont)
                stride = length + 3
                padded = dev(flat(form(row, r, mont) + [r, (1 << 256) - 1, r + 1] for row in data))  # (the padding is not below r: it is not read)
                api.frhash_test_tile(2 if length == t else 0)
                assert host(ctx.scalars_hash(h, padded, length, batch=rows)) == want, (curve, t, k, length)
                tight = dev(flat(form(row, r, mont) for row in data))
                out = torch.full((rows + 2, 32), 0xFF, dtype=torch.uint8, device="cuda")
                ctx.scalars_hash(h, tight, length, batch=rows, out=out[1:rows + 1])
                assert host(out[1:rows + 1]) == want and raw(out[0]) == raw(out[rows + 1]) == b"\xff" * 32
                assert stride * rows == padded.shape[0]
            api.frhash_test_tile(0)
            assert ctx.scalars_hash(h, M.to_bytes(form(data[1], r, mont)), lengths[-1]) == M.to_bytes(form([p.hash(data[1])], r, mont))  # the host form


def test_the_known_answers_come_out_of_the_device(contexts):
    ctx = contexts("bn254", False)
    with ctx.poseidon(3, 8, 57) as h:
        assert host(ctx.scalars_hash(h, dev([1, 2]), 2)) == [7853200120776062878684798364095072458815029376092732009249414926327459813530]
    with ctx.poseidon(2, 8, 56) as h:
        assert host(ctx.scalars_hash(h, dev([1]), 1)) == [18586133768512220936620570745912940619677854269274689475585506675881198879027]


# ---- trees -----------------------------------------------------------------------------------------------------------------------------------------
TREES = [(3, 2), (3, 32), (3, 2048), (5, 1024), (9, 512), (12, 121)]


@pytest.mark.parametrize("t,n", TREES, ids=["arity%d-%d" % (t - 1, n) for t, n in TREES])
def test_trees_node_by_node(contexts, t, n):
    curve = "bn254"
    r, rnd = api.SCALAR_FIELDS[curve], rng(1300 + t)
    p = M.standard(r, t, capacity=(1 << (t - 1)) - 1, capacity_at=0, out_at=1)
    leaves = [rnd.randrange(r) for _ in range(n)]
    want = flat(p.merkle(leaves))
    for mont in (False, True):
        ctx = contexts(curve, mont)
        src = dev(form(leaves, r, mont))
        before = raw(src)
        with handle(ctx, p) as h:
            for tile in (0, 3):
                api.frhash_test_tile(tile)
                nodes = ctx.merkle_tree(h, src)
                assert tuple(nodes.shape) == ((n - 1) // (t - 2), 32) and host(nodes) == form(want, r, mont), (t, n, mont, tile)
            api.frhash_test_tile(0)
            assert raw(src) == before
            if n <= 32:
                assert ctx.merkle_tree(h, M.to_bytes(form(leaves, r, mont))) == M.to_bytes(form(want, r, mont))  # the host form


def test_a_chain_of_arity_one(contexts):
    ctx = contexts("bls12_381", False)
    r = api.SCALAR_FIELDS["bls12_381"]
    p = M.standard(r, 2)
    with handle(ctx, p) as h:
        for tile in (0, 1):
            api.frhash_test_tile(tile)
            assert host(ctx.merkle_tree(h, dev([r - 2]), levels=3)) == p.merkle_chain(r - 2, 3)
        api.frhash_test_tile(0)


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_value_not_below_r_is_refused_and_the_next_call_is_correct(contexts):
    r = api.SCALAR_FIELDS["bn254"]
    p, states, images = reference("bn254", 3)
    ctx = contexts("bn254", False)
    good = flat(states[:65])
    with ctx.poseidon() as h:
        for bad in (r, (1 << 256) - 1):
            for at in (0, 100, len(good) - 1):
                with pytest.raises(api.MsmHipError) as e:
                    ctx.scalars_permute(h, dev(good[:at] + [bad] + good[at + 1:]))
                assert e.value.code == ERR_NONCANONICAL, (hex(bad), at)
                assert host(ctx.scalars_permute(h, dev(good))) == flat(images[:65])
        row = good[:10]
        for at in (0, 4, 9):
            with pytest.raises(api.MsmHipError) as e:
                ctx.scalars_hash(h, dev(row[:at] + [r] + row[at + 1:]), 5, batch=2)
            assert e.value.code == ERR_NONCANONICAL, at
            with pytest.raises(api.MsmHipError) as e:
                ctx.merkle_tree(h, dev((row[:at] + [r] + row[at + 1:])[:8]) if at < 8 else dev(row[:7] + [r]))
            assert e.value.code == ERR_NONCANONICAL, at
        assert host(ctx.scalars_hash(h, dev(row), 5, batch=2)) == [p.hash(row[:5]), p.hash(row[5:])]
        assert host(ctx.merkle_tree(h, dev(row[:8]))) == flat(p.merkle(row[:8]))
