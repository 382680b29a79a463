"""MsmContext.quotient and MsmContext.vanishing_inverse on the device: the quotient of a small circuit -- columns a, b, c with a b - c = 0 and
c - a(omega X) = 0 on all of H, weighted by two challenges -- has no coefficient from (D - 1) n upward, satisfies t(z) Z_H(z) = E(z) at a random z
with the columns' values taken by scalars_eval, and stops doing the former as soon as one witness element is changed; 1 / Z_H on the coset against
Python integers."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import frgate_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
LOG_N, LOG_EXT, SHIFT = 10, 2, 7
CASES = [("bn254", False), ("bn254", True), ("bls12_381", False)]


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
    for c in made.values():
        c.close()
    api.frgate_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


def form(vals, r, mont):
    return M.mont(vals, r) if mont else list(vals)


def plain(vals, r, mont):
    return M.mont(vals, r, back=True) if mont else list(vals)


def witness(r, n, seed):
    """a[i] b[i] = c[i] and c[i] = a[i + 1], cyclically: the last b is chosen so that the wrap closes"""
    rnd = rng(seed)
    a, b, c = [0] * n, [rnd.randrange(1, r) for _ in range(n)], [0] * n
    a[0] = rnd.randrange(1, r)
    for i in range(n):
        if i == n - 1:
            b[i] = a[0] * pow(a[i], r - 2, r) % r
        c[i] = a[i] * b[i] % r
        if i < n - 1:
            a[i + 1] = c[i]
    assert c[n - 1] == a[0]
    return a, b, c


@pytest.mark.parametrize("curve,mont", CASES, ids=["%s-%s" % (c, "mont256" if f else "canonical") for c, f in CASES])
def test_vanishing_inverse_against_python_integers(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r = api.SCALAR_FIELDS[curve]
    for log_n, log_ext, shift in ((LOG_N, LOG_EXT, SHIFT), (3, 0, 5), (0, 3, r - 2), (4, 4, 3)):
        got = ctx.vanishing_inverse(log_n, log_ext, shift)
        assert got.is_cuda and tuple(got.shape) == (1 << log_ext, 32)
        want = M.vanishing_inverse(log_n, log_ext, shift, api.root_of_unity(curve, log_n + log_ext), r)
        assert host(got) == form(want, r, mont), (curve, log_n, log_ext)
        g = pow(shift, 1 << log_n, r)  # (what the values are: the inverses of Z_H at the first 2^log_ext points of the coset)
        w = api.root_of_unity(curve, log_n + log_ext)
        assert all(v * (g * pow(w, i << log_n, r) - 1) % r == 1 for i, v in enumerate(want))
    with pytest.raises(ValueError):
        ctx.vanishing_inverse(3, 2, 1)  # the coset is H itself
    with pytest.raises(ValueError):
        ctx.vanishing_inverse(3, 2, api.root_of_unity(curve, 3))


@pytest.mark.parametrize("curve,mont", CASES, ids=["%s-%s" % (c, "mont256" if f else "canonical") for c, f in CASES])
def test_quotient_of_a_satisfied_and_of_a_broken_circuit(contexts, curve, mont):
    ctx = contexts(curve, mont)
    r, rnd = api.SCALAR_FIELDS[curve], rng(900)
    n, big = 1 << LOG_N, 1 << (LOG_N + LOG_EXT)
    omega = api.root_of_unity(curve, LOG_N)
    a, b, c = witness(r, n, 901)
    al0, al1 = rnd.randrange(1, r), rnd.randrange(1, r)
    # al0 (a b - c) + al1 (c - a(omega X)): D = 2
    terms = [(al0, (0, 1)), ((r - al0) % r, (2,)), (al1, (2,)), ((r - al1) % r, ((0, 1),))]

    def coefficients(a, b, c):
        return ctx.scalars_fft(dev(form(a + b + c, r, mont)), LOG_N, inverse=True, batch=3)

    cols = coefficients(a, b, c)
    kept = cols.clone()
    t = ctx.quotient(cols, terms, 3, LOG_N, LOG_EXT, SHIFT)
    assert t.is_cuda and tuple(t.shape) == (big, 32) and torch.equal(cols, kept)  # the columns are left untouched
    coeffs = plain(host(t), r, mont)
    assert not any(coeffs[n:]) and any(coeffs[:n])  # from (D - 1) n upward: all zero
    z = rnd.randrange(2, r)
    va, vb, vc = plain(M.from_bytes(ctx.scalars_eval(cols, z, batch=3)), r, mont)
    vaw, = plain(M.from_bytes(ctx.scalars_eval(cols[:n], z * omega % r)), r, mont)
    tz, = plain(M.from_bytes(ctx.scalars_eval(t, z)), r, mont)
    assert tz * (pow(z, n, r) - 1) % r == (al0 * (va * vb - vc) + al1 * (vc - vaw)) % r
    # one witness element changed: the division leaves a remainder, which shows in the top coefficients
    c[3] = (c[3] + 1) % r
    broken = ctx.quotient(coefficients(a, b, c), terms, 3, LOG_N, LOG_EXT, SHIFT)
    assert any(plain(host(broken), r, mont)[n:])
    with pytest.raises(ValueError):  # 2^log_ext >= D - 1
        ctx.quotient(cols, [(1, (0, 1, 2, 0))], 3, LOG_N, 1, SHIFT)
    with pytest.raises(ValueError):  # three columns of 2^LOG_N, not of 2^(LOG_N + 1)
        ctx.quotient(cols, terms, 3, LOG_N + 1, LOG_EXT, SHIFT)


def test_quotient_against_the_schoolbook_model(contexts):
    """a small domain, every coefficient against the model: degree 3 terms on a domain extended by 4, a rotation by -1 and one by 2"""
    ctx = contexts("bn254", False)
    r, rnd = api.SCALAR_FIELDS["bn254"], rng(910)
    log_n, log_ext = 3, 2
    n = 1 << log_n
    omega, omega_big = api.root_of_unity("bn254", log_n), api.root_of_unity("bn254", log_n + log_ext)
    # any columns: E need not vanish on H for E / Z_H on the coset, interpolated, to be what the model computes
    vals = [[rnd.randrange(r) for _ in range(n)] for _ in range(3)]
    cols = [M.interpolate(v, omega, r) for v in vals]
    terms = [(rnd.randrange(r), (0, (1, -1), 2)), (r - 1, ((2, 2), 0)), (5, (1,))]
    got = ctx.quotient(dev(cols[0] + cols[1] + cols[2]), terms, 3, log_n, log_ext, SHIFT)
    assert host(got) == M.quotient(cols, terms, log_n, log_ext, SHIFT, omega_big, r)
