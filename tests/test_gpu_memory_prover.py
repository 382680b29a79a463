"""msm_webgpu_amd.memory on the device, as a prover uses it, on BN254 and BLS12-381 in both scalar forms: read-only offline memory checking, whose
four grand products equal the host model's (Python integers) and satisfy Init * WS = RS * Final exactly while the counters are the right ones;
the address-sorted trace of three columns against the host's stable sort of the rows; and the counters chained behind the lookup library's
table indices."""
import pytest
import torch

from tests import frmem_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
CURVES = ("bn254", "bls12_381")
SHAPES = [(1027, 300, "skewed"), (1027, 300, "uniform"), (1 << 12, 1 << 12, "skewed"), (1 << 12, 1 << 12, "uniform")]  # (accesses, table entries, addresses)


def _dev(values):
    return torch.frombuffer(bytearray(b"".join(int(v).to_bytes(32, "little") for v in values)), dtype=torch.uint8).cuda().view(-1, 32)


def _ints(t):
    b = t.cpu().numpy().tobytes()
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


@pytest.fixture(scope="module", params=[(c, m) for c in CURVES for m in (False, True)], ids=lambda p: "%s-%s" % (p[0], "mont256" if p[1] else "canonical"))
def field(request, built):
    """(context, memory, r, stored(v): the integers as the context's form stores them, plain(bytes): a stored value as an integer)"""
    import msm_webgpu_amd as m
    from msm_webgpu_amd import api, memory

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    curve, mont = request.param
    r = api.SCALAR_FIELDS[curve]
    c = m.MsmContext(0, curve)
    c.set_scalar_format(mont256=mont)
    inv = pow(1 << 256, r - 2, r)
    yield (c, memory, r, (lambda v: [x * (1 << 256) % r for x in v]) if mont else (lambda v: list(v)),
           (lambda b: int.from_bytes(b, "little") * inv % r) if mont else (lambda b: int.from_bytes(b, "little")))
    c.close()


def _addresses(kind, n, n_t, rnd):
    if kind == "uniform":
        return [rnd.randrange(n_t) for _ in range(n)]
    return [rnd.randrange(n_t) if rnd.random() < 0.3 else rnd.randrange(1 + n_t // 50) for _ in range(n)]  # most accesses into a fiftieth of the table


@pytest.mark.parametrize("n,n_t,kind", SHAPES, ids=lambda v: str(v))
def test_offline_check_closes_and_equals_the_host_model(field, n, n_t, kind):
    ctx, mem, r, stored, plain = field
    rnd = rng(131 + n + len(kind))
    table = [rnd.randrange(r) for _ in range(n_t)]
    addr = _addresses(kind, n, n_t, rnd)
    gamma, tau = rnd.randrange(r), rnd.randrange(r)
    dt = _dev(stored(table))
    da = torch.tensor(addr, dtype=torch.int32, device="cuda")
    got = [plain(p) for p in mem.offline_check(ctx, dt, da, gamma, tau)]
    rank, _, counts, _, _ = M.access(addr, n_t)
    want = M.offline_products(table, addr, rank, counts, gamma, tau, r)
    assert tuple(got) == want
    assert got[0] * got[3] % r == got[2] * got[1] % r  # Init * WS = RS * Final
    assert _ints(dt) == stored(table) and da.tolist() == addr  # the inputs are untouched
    # the same through 64-bit addresses
    assert [plain(p) for p in mem.offline_check(ctx, dt, da.to(torch.int64), gamma, tau)] == got
    # two entries of rank swapped, one count raised: the products are still the model's for THOSE counters, and the equality breaks
    d_rank, _, d_counts, _, _ = mem.access_counters(ctx, da, table_size=n_t)
    assert d_rank.tolist() == rank and d_counts.tolist() == counts
    i, j = next((i, j) for i in range(n) for j in range(i + 1, n) if addr[i] != addr[j] and rank[i] != rank[j])
    swapped = list(rank)
    swapped[i], swapped[j] = rank[j], rank[i]
    bad = [plain(p) for p in mem.offline_products(ctx, dt, da, torch.tensor(swapped, dtype=torch.int32, device="cuda"), d_counts, gamma, tau)]
    assert tuple(bad) == M.offline_products(table, addr, swapped, counts, gamma, tau, r) and bad[0] * bad[3] % r != bad[2] * bad[1] % r
    raised = list(counts)
    raised[addr[0]] += 1
    bad = [plain(p) for p in mem.offline_products(ctx, dt, da, d_rank, torch.tensor(raised, dtype=torch.int32, device="cuda"), gamma, tau)]
    assert tuple(bad) == M.offline_products(table, addr, rank, raised, gamma, tau, r) and bad[0] * bad[3] % r != bad[2] * bad[1] % r
    with pytest.raises(ValueError, match="table"):  # a 64-bit address that would wrap into the table in 32 bits is outside it
        mem.offline_products(ctx, dt, da.to(torch.int64) + (1 << 32), d_rank, d_counts, gamma, tau)
    with pytest.raises(ValueError, match="table"):
        mem.offline_check(ctx, dt[:-1], torch.tensor([n_t - 1], dtype=torch.int32, device="cuda"), gamma, tau)  # an address outside the table


@pytest.mark.parametrize("n,n_t,kind", SHAPES, ids=lambda v: str(v))
def test_sorted_trace_is_the_hosts_stable_sort_of_the_rows(field, n, n_t, kind):
    ctx, mem, r, stored, plain = field
    rnd = rng(141 + n)
    addr = _addresses(kind, n, n_t, rnd)
    cols = [[rnd.randrange(r) for _ in range(n)] for _ in range(3)]
    da = torch.tensor(addr, dtype=torch.int64, device="cuda")
    perm, addr_sorted, moved = mem.sorted_trace(ctx, da, *[_dev(c) for c in cols])
    rows = sorted(zip(addr, range(n), *cols), key=lambda row: row[0])  # (Python's sort is stable)
    assert addr_sorted.tolist() == [row[0] for row in rows] and perm.tolist() == [row[1] for row in rows] == M.argsort(addr)
    assert [_ints(m) for m in moved] == [[row[2 + k] for row in rows] for k in range(3)]
    p, a = perm.tolist(), addr_sorted.tolist()
    assert all(a[k] < a[k + 1] or (a[k] == a[k + 1] and p[k] < p[k + 1]) for k in range(n - 1))  # equal addresses: ascending original indices
    with pytest.raises(ValueError, match=r"cols\[1\]"):
        mem.sorted_trace(ctx, da, _dev(cols[0]), _dev(cols[1][:-1]))


def test_counters_behind_the_lookup_librarys_indices(field):
    """scalars_multiplicities(indices=True) -> access_counters(table_size=n_t): the counts are the lookup's own counts=True"""
    ctx, mem, r, stored, plain = field
    rnd = rng(151)
    n_t, n = 300, 1027
    table = rnd.sample(range(1, 1 << 40), n_t)
    addr = _addresses("skewed", n, n_t, rnd)
    dt, df = _dev(stored(table)), _dev(stored([table[a] for a in addr]))
    with ctx.lookup_table(dt) as look:
        _, idx, cnt = ctx.scalars_multiplicities(look, df, indices=True, counts=True)
    assert idx.reshape(-1).tolist() == addr
    rank, prev, counts, last, distinct = mem.access_counters(ctx, idx.reshape(-1), table_size=n_t)
    assert torch.equal(counts.view(torch.int32), cnt.view(torch.int32)) and counts.tolist() == M.access(addr, n_t)[2]
    assert (rank.tolist(), prev.view(torch.int32).tolist()) == tuple([v if v != M.MISSING else -1 for v in col] for col in M.access(addr, n_t)[:2]) and distinct == len(set(addr))


def test_grumpkin_is_refused_before_any_library(built):
    import msm_webgpu_amd as m
    from msm_webgpu_amd import memory

    c = m.MsmContext(0, "grumpkin")
    try:
        with pytest.raises(ValueError, match="grumpkin"):
            memory.offline_check(c, _dev([1, 2, 3]), torch.tensor([0, 2], dtype=torch.int32, device="cuda"), 5, 7)
        assert memory.argsort(c, torch.tensor([3, 1, 3, 0], dtype=torch.int32, device="cuda")).tolist() == [3, 1, 0, 2]  # (the sort knows no field)
    finally:
        c.close()
