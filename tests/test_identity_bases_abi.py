"""MSM_HIP_BASES_ZERO_IS_IDENTITY without a GPU: the flag's value in the C header and its Python mirror, and the opt-in encoding of the point at
infinity as (0, 0) by points_to_bytes in Python and C++ (include/msm_hip.hpp).  The GPU side: tests/test_gpu_identity_bases.py."""
import os
import re
import subprocess

import pytest

import msm_webgpu_amd as m
from oracle import bn254_ref, cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_flags():
    text = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (MSM_HIP_(?:BASES_\w+|CHECK_ON_CURVE)) (\d+)u", text)}


def test_header_defines_the_flag_as_128():
    flags = header_flags()
    assert flags["MSM_HIP_BASES_ZERO_IS_IDENTITY"] == 128
    assert m.BASES_ZERO_IS_IDENTITY == 128
    others = [v for k, v in flags.items() if k != "MSM_HIP_BASES_ZERO_IS_IDENTITY"]
    assert 128 not in others and 64 not in flags.values()  # (64 stays an invalid flag)


def test_points_to_bytes_default_still_raises():
    pts = [(1, 2), None]
    with pytest.raises(ValueError):
        m.points_to_bytes(pts)
    with pytest.raises(ValueError):
        m.points_to_bytes(pts, zero_is_identity=False)


def test_points_to_bytes_opt_in_writes_zero_records():
    pts = bn254_ref.bytes_to_points(cpu.sample_points(5, 3))
    b = m.points_to_bytes([pts[0], None, pts[1], None, pts[2]], zero_is_identity=True)
    assert len(b) == 5 * 64
    assert b[64:128] == bytes(64) and b[192:256] == bytes(64)
    assert b[:64] + b[128:192] + b[256:] == m.points_to_bytes(pts)
    assert m.points_to_bytes([None], zero_is_identity=True) == bytes(64)


def test_cpp_mirror_encodes_the_identity(built, tmp_path):
    exe = str(tmp_path / "test_identity_encoding")
    libdir = os.path.join(ROOT, "msm-webgpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_identity_encoding.cpp"),
                           "-L", libdir, "-lmsm_hip", "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "identity encoding ok" in r.stdout
