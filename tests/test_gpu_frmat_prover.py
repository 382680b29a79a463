"""The line libmsm_frmat.so exists for, on the device from the witness to the transcript: Az, Bz, Cz of a satisfied R1CS (MsmContext.r1cs_tables)
beside eq(tau, .) (scalars_eq) are one sumcheck_prove input for eq A B - eq C, whose transcript the model's verifier (tests/frmle_model.py)
accepts against a claimed sum of 0; and every final value M~(r_x) z equals <M^T eq(r_x, .), z>, the identity the inner sumcheck of a Spartan
prover rests on, which ties the two directions of the product together.  BN254 and Grumpkin; 2^6 rows under the tile hook and 2^11 at the
design tile.  The inner product is scalars_dot where the field has it; Grumpkin's scalar field, which libmsm_frpoly.so does not offer, takes
g(0) + g(1) of the round polynomial of the same two tables (scalars_sumcheck_round), which is the same sum."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frmat_model as F
from tests import frmle_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(curve, mont):
        if curve not in made:
            made[curve] = m.MsmContext(0, curve)
        made[curve].set_scalar_format(mont256=mont)
        return made[curve]

    yield get
    api.frmat_test_tile(0)
    api.frmle_test_tile(0)
    for c in made.values():
        c.close()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def r1cs(n, r, rnd):
    """a satisfied R1CS of n rows and n columns: A and B random -- one to three entries a row, and column 0, the constant one, in a quarter of the
    rows --, z random with z[0] = 1, and C one entry a row, chosen so that (Az)_i (Bz)_i = (Cz)_i"""
    z = [1] + [rnd.randrange(1, r) for _ in range(n - 1)]

    def random_matrix():
        ptr, idx, val = [0], [], []
        for i in range(n):
            cols = [rnd.randrange(n) for _ in range(rnd.randrange(1, 4))] + ([0] if i % 4 == 0 else [])
            idx += cols
            val += [rnd.randrange(r) for _ in cols]
            ptr.append(len(idx))
        return ptr, idx, val

    a, b = random_matrix(), random_matrix()
    az, bz = F.matvec(n, n, *a, z, r), F.matvec(n, n, *b, z, r)
    c_idx = [rnd.randrange(n) for _ in range(n)]
    c_val = [x * y * pow(z[j], r - 2, r) % r for x, y, j in zip(az, bz, c_idx)]
    c = (list(range(n + 1)), c_idx, c_val)
    assert F.matvec(n, n, *c, z, r) == [x * y % r for x, y in zip(az, bz)]
    return a, b, c, z


@pytest.mark.parametrize("k,tile,mont", [(6, 8, False), (6, 8, True), (11, 0, False)], ids=["2^6 tile 8", "2^6 tile 8 mont256", "2^11 design tile"])
@pytest.mark.parametrize("curve", ["bn254", "grumpkin"])
def test_r1cs_sumcheck_from_the_witness_to_the_transcript(contexts, curve, k, tile, mont):
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    rnd = rng(700 + k)
    n = 1 << k
    a, b, c, z = r1cs(n, r, rnd)
    form = (lambda v: M.mont(v, r)) if mont else list
    back = (lambda v: M.mont(v, r, back=True)) if mont else list
    api.frmat_test_tile(tile)
    api.frmle_test_tile(tile)
    mats = [ctx.scalars_matrix(n, n, *x, transpose=True) for x in (a, b, c)]
    api.frmat_test_tile(0)
    zd = dev(form(z))
    tau = [rnd.randrange(r) for _ in range(k)]
    buf = torch.empty(4, n, 32, dtype=torch.uint8, device="cuda")
    ctx.scalars_eq(tau, out=buf[0])
    assert ctx.r1cs_tables(*mats, zd, out=buf, first_row=1) is buf
    tables = [back(M.from_bytes(buf[j].cpu().numpy().tobytes())) for j in range(4)]
    assert tables[1:] == [F.matvec(n, n, *x, z, r) for x in (a, b, c)] and tables[0] == M.eq(tau, r)
    terms = [(1, (0, 1, 2)), (r - 1, (0, 3))]  # eq A B - eq C
    stream = rng(800 + k)
    rounds, point, finals = ctx.sumcheck_prove(buf, terms, 4, lambda j, values: stream.randrange(r))
    transcript = [back(M.from_bytes(v)) for v in rounds]
    finals = back(M.from_bytes(finals))
    assert len(point) == k and M.verify(0, transcript, point, finals, terms, r)
    assert not M.verify(1, transcript, point, finals, terms, r)
    assert finals[0] == M.eq_value(tau, point, r)
    # the inner sumcheck's claim: M~(r_x, .) summed against z
    eq_rx = ctx.scalars_eq(point)
    pair = torch.empty(2, n, 32, dtype=torch.uint8, device="cuda")
    pair[1].copy_(zd)
    for j, mat in enumerate(mats):
        col = ctx.scalars_matvec(mat, eq_rx, out=pair[0], transpose=True)
        if curve == "grumpkin":
            g = back(M.from_bytes(ctx.scalars_sumcheck_round(pair, [(1, (0, 1))], batch=2)))
            dot = (g[0] + g[1]) % r
        else:
            dot = back(M.from_bytes(ctx.scalars_dot(col, zd)))[0]
        assert dot == finals[1 + j], (curve, k, "ABC"[j])
    api.frmle_test_tile(0)
    for mat in mats:
        mat.close()
