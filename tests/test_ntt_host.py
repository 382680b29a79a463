"""The scalar-field NTT of libmsm_fr.so on the CPU: a stand-alone program (tests/host_harness/ntt_harness.cpp) runs the plan and tables of
csrc/ntt_plan.h and, element by element, the functions a lane of the kernel runs (csrc/ntt_kernels.h), compiled with g++ -DFQ_CHECK so that every
limb and value bound of csrc/fq29.h is asserted -- the test that catches a lazy-bound overflow -- against the pure-Python model
(tests/ntt_model.py), which is itself checked against the O(n^2) definition.  Host logic only."""
import os
import subprocess
import sys

import pytest

from tests import ntt_model as M
from tests.util import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254", "pallas", "vesta", "bls12_381")
B = 10  # the design's levels per pass (csrc/ntt_kernels.h: NTT_PASS_BITS)


def _api():
    from msm_webgpu_amd import api

    return api


@pytest.mark.parametrize("field", FIELDS)
def test_the_model_is_the_definition(field):
    api = _api()
    r = api.SCALAR_FIELDS[field]
    rnd = rng(7)
    for log_n in (0, 1, 2, 3, 6):
        n = 1 << log_n
        w = api.root_of_unity(field, log_n)
        a = [rnd.randrange(r) for _ in range(n)]
        assert M.ntt(a, w, r) == M.ntt_definition(a, w, r), log_n
        s, t, c = rnd.randrange(1, r), rnd.randrange(1, r), rnd.randrange(1, r)
        assert M.ntt(a, w, r, s, t, c) == M.ntt_definition(a, w, r, s, t, c), log_n
        assert M.intt(M.ntt(a, w, r), w, r) == a and M.intt(M.ntt(a, w, r, pre=s), w, r, shift=s) == a


def test_generated_field_constants_are_in_sync():
    for field in FIELDS:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_constants.py"), "fr", field], capture_output=True, text=True, check=True).stdout
        assert out == open(os.path.join(ROOT, "msm-webgpu_amd", "csrc", "fr_%s_constants.h" % field)).read(), field
        assert "CURVE_B" not in out and "GLV" not in out and "FQ_GEN" not in out  # a field, no curve


def _build(tmp, field, sanitize=False):
    exe = str(tmp / ("ntt_harness_%s%s" % (field, "_san" if sanitize else "")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFQ_CHECK", "-DMSM_FIELD_NS=fr_" + field, '-DMSM_CURVE_CONSTANTS="fr_%s_constants.h"' % field, "-I",
                           os.path.join(ROOT, "msm-webgpu_amd", "csrc")] + san + [os.path.join(ROOT, "tests", "host_harness", "ntt_harness.cpp"), "-o", exe])
    return exe


def _run(exe, tmp, log_n, cap, batch, a, omega, pre=None, post=None, scale=False):
    head = omega.to_bytes(32, "little") + b"".join(b"\1" + v.to_bytes(32, "little") if v is not None else bytes(33) for v in (pre, post))
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(head + M.to_bytes(a))
    p = subprocess.run([exe, str(log_n), str(cap), str(batch), "1" if scale else "0", str(fin), str(fout)], capture_output=True, text=True)
    assert p.returncode in (0, 3), (p.returncode, p.stderr[-500:])
    return p.returncode, M.from_bytes(fout.read_bytes())


@pytest.fixture(scope="module", params=FIELDS)
def harness(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ntt_" + request.param)
    return request.param, _build(tmp, request.param), tmp


def _inputs(r, n, rnd):
    return {"random": [rnd.randrange(r) for _ in range(n)], "all r - 1": [r - 1] * n, "all 0": [0] * n, "delta": [0] * (n - 1) + [1] if n > 1 else [1],
            "delta at 0": [r - 1] + [0] * (n - 1)}


@pytest.mark.parametrize("bits", [B, B - 1])
def test_a_full_tile_keeps_its_bounds(harness, bits):
    """one tile of 2^bits elements through all its levels, bounds asserted: random inputs, all r - 1 (the largest values the lazy sums see), all 0, a
    delta; both data representations (the Montgomery form a 2^256 mod r runs through the same code: the transform is linear)"""
    field, exe, tmp = harness
    api = _api()
    r = api.SCALAR_FIELDS[field]
    n = 1 << bits
    w = api.root_of_unity(field, bits)
    mont = pow(2, 256, r)
    for name, a in _inputs(r, n, rng(11)).items():
        want = M.ntt(a, w, r)
        rc, got = _run(exe, tmp, bits, bits, 1, a, w)
        assert rc == 0 and got == want, (field, bits, name)
        rc, got = _run(exe, tmp, bits, bits, 1, [v * mont % r for v in a], w)
        assert rc == 0 and got == [v * mont % r for v in want], (field, bits, name, "mont256")
    a = _inputs(r, n, rng(12))["random"]
    s, t = 5, r - 3  # ... and with every factor in play: both shifts and 1 / n
    rc, got = _run(exe, tmp, bits, bits, 1, a, w, pre=s, post=t, scale=True)
    assert rc == 0 and got == M.ntt(a, w, r, s, t, pow(n, r - 2, r)), (field, bits)


@pytest.mark.parametrize("log_n,cap,batch", [(0, B, 2), (1, B, 1), (5, 4, 1), (8, 4, 3), (9, 4, 1), (12, 4, 1), (13, 4, 1), (B + 1, B, 2), (2 * B - 6, B - 3, 1), (14, B, 1)])
def test_every_pass_structure_against_the_model(harness, log_n, cap, batch):
    """one to four passes, columns and digit reversal, a batch, the two-level tables (n > 2^13); forward, coset, inverse with 1 / n"""
    field, exe, tmp = harness
    api = _api()
    r = api.SCALAR_FIELDS[field]
    n = 1 << log_n
    w = api.root_of_unity(field, log_n)
    rnd = rng(100 + log_n)
    a = [rnd.randrange(r) for _ in range(batch * n)]
    a[0] = r - 1
    g = rnd.randrange(2, r)
    for pre, post, scale, omega in ((None, None, False, w), (g, None, False, w), (None, pow(g, r - 2, r), True, pow(w, r - 2, r))):
        rc, got = _run(exe, tmp, log_n, cap, batch, a, omega, pre, post, scale)
        want = sum((M.ntt(a[v * n:(v + 1) * n], omega, r, pre or 1, post or 1, pow(n, r - 2, r) if scale else 1) for v in range(batch)), [])
        assert rc == 0 and got == want, (field, log_n, cap, pre is not None, scale)


def test_a_value_not_below_r_is_reported(harness):
    field, exe, tmp = harness
    api = _api()
    r = api.SCALAR_FIELDS[field]
    w = api.root_of_unity(field, 6)
    a = [1] * 64
    assert _run(exe, tmp, 6, 4, 1, a, w)[0] == 0
    for bad in (r, r + 1, (1 << 256) - 1):
        a[37] = bad
        assert _run(exe, tmp, 6, 4, 1, a, w)[0] == 3, hex(bad)


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code: indices into the tile, the tables and the data; shifts)"""
    api = _api()
    field = "bls12_381"
    exe = _build(tmp_path, field, sanitize=True)
    r = api.SCALAR_FIELDS[field]
    for log_n, cap, batch in ((B, B, 1), (B + 1, B, 2), (13, 4, 1), (0, B, 1)):
        n = 1 << log_n
        w = api.root_of_unity(field, log_n)
        a = [r - 1 - i for i in range(batch * n)]
        rc, got = _run(exe, tmp_path, log_n, cap, batch, a, w, pre=7, post=9, scale=True)
        assert rc == 0 and got == sum((M.ntt(a[v * n:(v + 1) * n], w, r, 7, 9, pow(n, r - 2, r)) for v in range(batch)), []), (log_n, cap)
