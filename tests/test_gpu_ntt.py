"""The scalar-field NTT on the device (include/msm_fr.h, MsmContext.scalars_fft) against the pure-Python model (tests/ntt_model.py), bit for bit:
sizes below and around one wave, the tile seams of the design's B = 10 levels per pass, one to four passes under the pass-width hook, batches,
both scalar representations, extreme inputs, inverse and coset round trips, a custom omega, the rejection of a value >= r, the four fields and a
G2 context, and the host form."""
import pytest
import torch

import msm_webgpu_amd as m
from msm_webgpu_amd import api
from tests import ntt_model as M
from tests.util import rng

pytestmark = pytest.mark.gpu
B = 10  # csrc/ntt_kernels.h: NTT_PASS_BITS
ERR_NONCANONICAL = -4
R = api.SCALAR_FIELDS["bn254"]


@pytest.fixture(scope="module")
def contexts(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(curve="bn254"):
        if curve not in made:
            made[curve] = m.MsmContext(0, curve)
        return made[curve]

    yield get
    api.fr_test_pass_bits(0)
    for c in made.values():
        c.close()
    api.fr_release()


def dev(vals):
    return torch.frombuffer(bytearray(M.to_bytes(vals)), dtype=torch.uint8).reshape(-1, 32).cuda()


def host(t):
    return M.from_bytes(t.cpu().numpy().tobytes())


def passes_for(log_n, cap):
    return 1 if log_n == 0 else -(-log_n // cap)


# below and around one wave; the tile seams B - 1, B, B + 1 (2B and 2B + 1 are beyond 2^17 elements: the pass structures of two and three passes
# are covered at small sizes by the pass-width hook below, and on the CPU by tests/test_ntt_host.py); 14: the first size with two-level twiddle tables
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 6, 7, B - 1, B, B + 1, 14])
def test_forward_at_the_design_pass_width(contexts, log_n):
    ctx = contexts()
    api.fr_test_pass_bits(0)
    n = 1 << log_n
    a = [rng(200 + log_n).randrange(R) for _ in range(n)]
    w = api.root_of_unity("bn254", log_n)
    t = dev(a)
    assert ctx.scalars_fft(t) is t
    assert host(t) == M.ntt(a, w, R), log_n
    assert api.fr_last() == (passes_for(log_n, B), log_n if log_n <= B else -(-log_n // passes_for(log_n, B)))


@pytest.mark.parametrize("log_n,passes", [(4, 1), (5, 2), (8, 2), (9, 3), (12, 3), (13, 4)])
def test_one_to_four_passes_under_the_pass_width_hook(contexts, log_n, passes):
    ctx = contexts()
    n = 1 << log_n
    rnd = rng(300 + log_n)
    a = [rnd.randrange(R) for _ in range(n)]
    w = api.root_of_unity("bn254", log_n)
    g = rnd.randrange(2, R)
    api.fr_test_pass_bits(4)
    try:
        t = dev(a)
        ctx.scalars_fft(t, log_n)
        assert api.fr_last()[0] == passes and api.fr_last()[1] <= 4
        assert host(t) == M.ntt(a, w, R), log_n
        ctx.scalars_fft(t, inverse=True)
        assert api.fr_last()[0] == passes
        assert host(t) == a, (log_n, "inverse")
        ctx.scalars_fft(t, shift=g)
        assert host(t) == M.ntt(a, w, R, pre=g), (log_n, "coset")
    finally:
        api.fr_test_pass_bits(0)


@pytest.mark.parametrize("log_n,batch", [(9, 3), (0, 1), (0, 5), (B + 1, 2)])
def test_batches(contexts, log_n, batch):
    ctx = contexts()
    n = 1 << log_n
    a = [rng(400 + log_n).randrange(R) for _ in range(batch * n)]
    w = api.root_of_unity("bn254", log_n)
    t = dev(a)
    ctx.scalars_fft(t, batch=batch)
    assert host(t) == sum((M.ntt(a[v * n:(v + 1) * n], w, R) for v in range(batch)), [])
    with pytest.raises(ValueError):
        ctx.scalars_fft(t, log_n=log_n, batch=batch + 1)


@pytest.mark.parametrize("log_n", [6, B, B + 1])
def test_both_representations_and_extreme_inputs(contexts, log_n):
    n = 1 << log_n
    w = api.root_of_unity("bn254", log_n)
    mont = pow(2, 256, R)
    inputs = {"random": [rng(500).randrange(R) for _ in range(n)], "all r - 1": [R - 1] * n, "all 0": [0] * n, "delta": [0] * (n - 1) + [1],
              "constant": [0x1234567] * n}
    ctx = m.MsmContext(0)
    try:
        for name, a in inputs.items():
            want = M.ntt(a, w, R)
            ctx.set_scalar_format(mont256=False)
            assert host(ctx.scalars_fft(dev(a))) == want, (log_n, name)
            ctx.set_scalar_format(mont256=True)
            assert host(ctx.scalars_fft(dev([v * mont % R for v in a]))) == [v * mont % R for v in want], (log_n, name, "mont256")
        for width in (8, 16):
            ctx.set_scalar_format(width=width)
            with pytest.raises(ValueError):
                ctx.scalars_fft(dev(inputs["random"]))
    finally:
        ctx.close()


def test_forward_then_inverse_is_the_identity(contexts):
    ctx = contexts()
    a = [rng(600).randrange(R) for _ in range(1 << 10)]
    t = dev(a)
    ctx.scalars_fft(t)
    assert host(t) != a
    ctx.scalars_fft(t, inverse=True)
    assert host(t) == a


@pytest.mark.parametrize("log_n", [3, 10, B + 2])
def test_coset_forward_and_round_trip(contexts, log_n):
    ctx = contexts()
    n = 1 << log_n
    rnd = rng(700 + log_n)
    a = [rnd.randrange(R) for _ in range(n)]
    g = rnd.randrange(2, R)
    w = api.root_of_unity("bn254", log_n)
    t = dev(a)
    ctx.scalars_fft(t, shift=g)
    assert host(t) == M.ntt(a, w, R, pre=g), log_n  # a(g omega^i)
    ctx.scalars_fft(t, inverse=True, shift=g.to_bytes(32, "little"))
    assert host(t) == a, log_n


def test_custom_omega(contexts):
    ctx = contexts()
    w11 = api.root_of_unity("bn254", 11)
    w = pow(w11, 3, R)  # another primitive 2^11-th root ...
    w = w * w % R       # ... whose square is a primitive 2^10-th root that root_of_unity does not give
    assert w != api.root_of_unity("bn254", 10) and pow(w, 512, R) == R - 1
    a = [rng(800).randrange(R) for _ in range(1 << 10)]
    for omega in (w, w.to_bytes(32, "little")):
        t = dev(a)
        ctx.scalars_fft(t, omega=omega)
        assert host(t) == M.ntt(a, w, R)
    ctx.scalars_fft(t, omega=w, inverse=True)
    assert host(t) == a
    with pytest.raises(ValueError):
        ctx.scalars_fft(t, omega=w11)


@pytest.mark.parametrize("log_n", [4, B + 1])
def test_a_value_not_below_r_is_refused_and_the_next_call_succeeds(contexts, log_n):
    ctx = contexts()
    n = 1 << log_n
    a = [rng(900).randrange(R) for _ in range(n)]
    w = api.root_of_unity("bn254", log_n)
    for bad in (R, (1 << 256) - 1):
        b = list(a)
        b[n - 3] = bad
        with pytest.raises(m.MsmHipError) as e:
            ctx.scalars_fft(dev(b))
        assert e.value.code == ERR_NONCANONICAL
        with pytest.raises(m.MsmHipError) as e:
            ctx.scalars_fft(M.to_bytes(b))
        assert e.value.code == ERR_NONCANONICAL
        assert host(ctx.scalars_fft(dev(a))) == M.ntt(a, w, R)


@pytest.mark.parametrize("curve", ["bn254", "pallas", "vesta", "bls12_381", "bn254_g2"])
def test_every_field(contexts, curve):
    ctx = contexts(curve)
    r = api.SCALAR_FIELDS[curve]
    rnd = rng(1000)
    a = [rnd.randrange(r) for _ in range(1 << 9)]
    a[5], a[6] = r - 1, 0
    w = api.root_of_unity(curve, 9)
    g = rnd.randrange(2, r)
    t = dev(a)
    ctx.scalars_fft(t, shift=g)
    assert host(t) == M.ntt(a, w, r, pre=g), curve
    ctx.scalars_fft(t, inverse=True, shift=g)
    assert host(t) == a, curve
    b = list(a)
    b[100] = r
    with pytest.raises(m.MsmHipError) as e:
        ctx.scalars_fft(dev(b))
    assert e.value.code == ERR_NONCANONICAL


def test_grumpkin_is_refused(contexts):
    with pytest.raises(ValueError):
        contexts("grumpkin").scalars_fft(dev([1, 2]))
    one = (1).to_bytes(32, "little")
    t = dev([1])
    assert api.fr_lib().msm_fr_ntt_device(1, 0, None, t.data_ptr(), 0, 1, one, None, None, 0) == -2


@pytest.mark.parametrize("log_n,batch", [(0, 1), (7, 2), (B + 1, 1)])
def test_host_form_equals_device_form(contexts, log_n, batch):
    ctx = contexts()
    n = 1 << log_n
    rnd = rng(1100 + log_n)
    a = [rnd.randrange(R) for _ in range(batch * n)]
    g = rnd.randrange(2, R)
    for kw in (dict(), dict(shift=g), dict(inverse=True), dict(inverse=True, shift=g)):
        got = ctx.scalars_fft(M.to_bytes(a), batch=batch, **kw)
        assert isinstance(got, bytes) and got == M.to_bytes(host(ctx.scalars_fft(dev(a), batch=batch, **kw))), (log_n, kw)
    w = api.root_of_unity("bn254", log_n)
    assert M.from_bytes(ctx.scalars_fft(M.to_bytes(a), batch=batch)) == sum((M.ntt(a[v * n:(v + 1) * n], w, R) for v in range(batch)), [])


def test_release_and_reuse(contexts):
    ctx = contexts()
    a = [rng(1200).randrange(R) for _ in range(1 << (B + 1))]
    want = M.ntt(a, api.root_of_unity("bn254", B + 1), R)
    assert host(ctx.scalars_fft(dev(a))) == want
    api.fr_release()  # twiddles and scratch gone ...
    assert host(ctx.scalars_fft(dev(a))) == want  # ... and back


def test_the_caller_device_is_left_alone(contexts):
    ctx = contexts()
    before = torch.cuda.current_device()
    ctx.scalars_fft(dev([1, 2, 3, 4]))
    assert torch.cuda.current_device() == before
