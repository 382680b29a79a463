"""The narrow scalar formats of the C ABI (include/msm_hip.h) and their mirrors, without a GPU: the format values are pinned, the Python
binding maps widths onto them, and the C++ wrapper offers the width setter."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines():
    with open(os.path.join(ROOT, "include", "msm_hip.h")) as f:
        return {k: int(v) for k, v in re.findall(r"#define (MSM_HIP_SCALARS_\w+) (\d+)u", f.read())}


def test_format_values_are_pinned():
    d = _defines()
    assert d == {"MSM_HIP_SCALARS_CANONICAL": 0, "MSM_HIP_SCALARS_MONT256": 1, "MSM_HIP_SCALARS_U8": 2, "MSM_HIP_SCALARS_U16": 3,
                 "MSM_HIP_SCALARS_U32": 4, "MSM_HIP_SCALARS_U64": 5}


def test_python_binding_maps_widths_onto_the_formats():
    from msm_webgpu_amd import api

    d = _defines()
    assert api.SCALAR_WIDTHS == {1: d["MSM_HIP_SCALARS_U8"], 2: d["MSM_HIP_SCALARS_U16"], 4: d["MSM_HIP_SCALARS_U32"], 8: d["MSM_HIP_SCALARS_U64"]}


def test_cpp_wrapper_has_the_width_setter():
    with open(os.path.join(ROOT, "include", "msm_hip.hpp")) as f:
        src = f.read()
    assert "void set_scalar_width(int bytes)" in src
    for name in ("MSM_HIP_SCALARS_U8", "MSM_HIP_SCALARS_U16", "MSM_HIP_SCALARS_U32", "MSM_HIP_SCALARS_U64"):
        assert name in src
