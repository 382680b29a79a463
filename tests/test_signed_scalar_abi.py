"""The signed and 128-bit narrow scalar formats of the C ABI (include/msm_hip.h: MSM_HIP_SCALAR_SIGNED, MSM_HIP_SCALAR_U128) and their mirrors,
without a GPU: the two new values are pinned beside the six MSM_HIP_SCALARS_* names (whose set stays what it was), the Python binding maps
(width, signed) onto the format values, the C++ wrapper offers both width setters, and the pure-Python model of the recode
(tests/signed_scalar_model.py, which the GPU stage test compares the engine's digit planes with) reassembles every value from its digits."""
import os
import random
import re

import pytest

from tests import signed_scalar_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "msm_hip.h")) as f:
        return f.read()


def _define(name):
    m = re.search(r"^#define %s\s+(\d+)u\b" % name, _header(), re.M)
    assert m, "%s is not defined in include/msm_hip.h" % name
    return int(m.group(1))


def test_new_format_values_are_pinned():
    assert _define("MSM_HIP_SCALAR_SIGNED") == 16
    assert _define("MSM_HIP_SCALAR_U128") == 8


def test_the_six_scalars_names_are_still_the_whole_set():
    d = {k: int(v) for k, v in re.findall(r"#define (MSM_HIP_SCALARS_\w+) (\d+)u", _header())}
    assert d == {"MSM_HIP_SCALARS_CANONICAL": 0, "MSM_HIP_SCALARS_MONT256": 1, "MSM_HIP_SCALARS_U8": 2, "MSM_HIP_SCALARS_U16": 3,
                 "MSM_HIP_SCALARS_U32": 4, "MSM_HIP_SCALARS_U64": 5}


def test_abi_version_is_unchanged(built):
    import msm_webgpu_amd as m

    assert m.lib().msm_hip_abi_version() == 7  # the new formats arrived within version 7
    # host-only: the setter refuses a missing context whatever the format, the new values included
    for fmt in (8, 18, 24):
        assert m.lib().msm_hip_set_scalar_format(None, fmt) == -2


def test_python_binding_maps_width_and_signedness_onto_the_formats():
    from msm_webgpu_amd import api

    signed, u128 = _define("MSM_HIP_SCALAR_SIGNED"), _define("MSM_HIP_SCALAR_U128")
    assert api.SCALAR_SIGNED == signed and api.SCALAR_U128 == u128
    assert api.SCALAR_WIDTHS == {1: 2, 2: 3, 4: 4, 8: 5}  # (pinned: the 128-bit format lives beside it)
    want = {(w, False): f for w, f in api.SCALAR_WIDTHS.items()}
    want[(16, False)] = u128
    want.update({(w, True): f | signed for (w, _), f in list(want.items())})
    assert api.SCALAR_FORMATS == want
    assert {api.SCALAR_FORMATS[(w, True)] for w in (1, 2, 4, 8, 16)} == {18, 19, 20, 21, 24}
    # the values that must stay invalid are none of them
    assert not set(api.SCALAR_FORMATS.values()) & {6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 22, 23, 25}


def test_cpp_wrapper_has_both_width_setters():
    with open(os.path.join(ROOT, "include", "msm_hip.hpp")) as f:
        src = f.read()
    assert "void set_scalar_width(int bytes)" in src
    assert "void set_scalar_width(int bytes, bool is_signed)" in src
    assert "MSM_HIP_SCALAR_U128" in src and "MSM_HIP_SCALAR_SIGNED" in src


# ---------------------------------------------------------------------------------------------------------------- the recode model
def _values(width, signed, seed, count=200):
    lo, hi = model.value_range(width, signed)
    rnd = random.Random(seed)
    vals = model.edge_values(width, signed)
    vals += [rnd.randint(lo, hi) for _ in range(count)]
    vals += [s * (1 << k) for k in range(0, 8 * width - 1, 5) for s in ((1, -1) if signed else (1,))]  # single bits, both signs
    return [v for v in vals if lo <= v <= hi]


@pytest.mark.parametrize("c", model.WINDOW_BITS)
@pytest.mark.parametrize("fmt", sorted(model.FORMATS))
def test_digits_reassemble_the_value(fmt, c):
    width, signed = model.FORMATS[fmt]
    wts = model.weights(width, c)
    nwin = model.windows(width, c)
    assert len(wts) == nwin
    half = 1 << (c - 1)
    for v in _values(width, signed, seed=width * 100 + c):
        d = model.digits(v, width, signed, c)
        assert len(d) == nwin
        assert sum(x * w for x, w in zip(d, wts)) == v, (fmt, c, v)
        if model.byte_windows(width):
            assert all(abs(x) <= 255 for x in d)  # the 255 slots of a byte window
            if signed:
                assert abs(d[-1]) <= 128  # I8's byte and I16's high byte
        else:
            assert all(abs(x) <= half for x in d)
            assert all((x <= 0) if v < 0 else (x >= 0) for x in d[-1:])  # the top window holds only what the carry leaves
            assert abs(d[-1]) <= (1 if 8 * width % c == 0 else half)


def test_window_counts():
    # (8 w + C) / C: the table of DESIGN.md
    assert [model.windows(16, c) for c in (16, 14, 12)] == [9, 10, 11]
    assert [model.windows(8, c) for c in (16, 14, 12)] == [5, 5, 6]
    assert [model.windows(4, c) for c in (16, 14, 12)] == [3, 3, 3]
    assert [model.windows(w, 12) for w in (1, 2)] == [1, 2]


@pytest.mark.parametrize("fmt", sorted(model.FORMATS))
def test_edges_are_covered_and_encode_round_trips(fmt):
    width, signed = model.FORMATS[fmt]
    lo, hi = model.value_range(width, signed)
    edges = model.edge_values(width, signed)
    assert {0, 1, hi, lo} <= set(edges)
    if signed:
        assert -1 in edges
        assert abs(lo) == hi + 1  # the minimum's magnitude does not fit the signed type
    if width == 16:
        assert (1 << 127) in {abs(v) for v in edges}
    raw = model.encode(edges, width, signed)
    assert len(raw) == width * len(edges)
    back = [int.from_bytes(raw[width * i:width * (i + 1)], "little", signed=signed) for i in range(len(edges))]
    assert back == edges
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254's scalar field
    s32 = model.scalars32(edges, r)
    assert [int.from_bytes(s32[32 * i:32 * (i + 1)], "little") for i in range(len(edges))] == [v % r for v in edges]


def test_plane_codes_decode_to_the_digits():
    for c in model.WINDOW_BITS:
        half = 1 << (c - 1)
        for d in (0, 1, -1, half - 1, -(half - 1), -half):
            code = 0 if d == 0 else d if d > 0 else 0x8000 | (-d & (half - 1))
            assert model.decode_plane(code, c) == d
            assert model.plane_digit(d, c) == d
        assert model.plane_digit(half, c) == 0
