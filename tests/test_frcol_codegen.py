"""The code-generation gates (tools/check_long_branch_hazard.py, tools/check_machine_verifier.py) over the one unit of libmsm_frcol.so; its seven
kernels sit in the library's namespace, use no scratch memory and spill nothing, and their LDS and registers are what DESIGN.md section 4.26
states.  Resource metadata only."""
import importlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402

# the name in DESIGN.md's table -> what the kernel's symbol holds
KERNELS = {"k_frcol_sums<true>": "12k_frcol_sumsILb1E", "k_frcol_sums<false>": "12k_frcol_sumsILb0E", "k_frcol_scan<true>": "12k_frcol_scanILb1E",
           "k_frcol_scan<false>": "12k_frcol_scanILb0E", "k_frcol_expand": "14k_frcol_expand", "k_frcol_pair": "12k_frcol_pair", "k_frcol_gather": "14k_frcol_gather"}


def _lib():
    return importlib.import_module("msm_webgpu_amd.build").AUX_LIBRARIES["frcol"]


def _stated():
    """kernel -> (VGPRs, SGPRs, LDS bytes) from the table of DESIGN.md section 4.26"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("### 4.26"):]
    section = section[:section.index("\n## ")]
    rows = dict((k, (int(v), int(s), int(lds))) for k, v, s, lds in re.findall(r"^\| `(k_frcol_[\w<>]+)` \| (\d+) \| (\d+) \| (\d+) B \| 0 B \| 0 \|$", section, flags=re.M))
    assert sorted(rows) == sorted(KERNELS), rows
    return rows


def _asm():
    paths = chk.compile_to_asm([], units=list(_lib().units))
    assert len(paths) == 1 and os.path.basename(paths[0]).startswith("frcol")
    return paths[0]


def test_the_unit_has_no_long_branch_hazard(built):
    long_branches, found, live = chk.check_file(_asm())
    assert found == [] and live == [], (found, live)


def test_the_unit_passes_the_machine_verifier():
    import check_machine_verifier as mv

    reports = mv.check(units=list(_lib().units))
    assert reports == {"frcol.hip": []}, reports


def test_the_kernels_use_no_scratch_and_the_resources_the_design_states(built):
    stated = _stated()
    with open(_asm()) as f:
        text = f.read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == len(KERNELS) and all(n.startswith("_ZN5frcol") for n in names), names
    for k, part in KERNELS.items():
        assert len([n for n in names if part in n]) == 1, (k, names)
    # the kernel descriptors and the metadata: no private segment, nothing spilled, no dynamic stack
    assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text) == ["0"] * len(KERNELS)
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * len(KERNELS)
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS) and re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS)
    assert not re.search(r"\.uses_dynamic_stack:\s+true", text)
    # LDS and registers, kernel by kernel, as DESIGN.md section 4.26 states them
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.symbol:\s+(\S+?)\.kd.*?\.vgpr_count:\s+(\d+)", text, flags=re.S)
    assert len(meta) == len(KERNELS)
    for lds, sgprs, symbol, vgprs in meta:
        k = [k for k, part in KERNELS.items() if part in symbol]
        assert len(k) == 1 and (int(vgprs), int(sgprs), int(lds)) == stated[k[0]], (symbol, vgprs, sgprs, lds, stated)


def test_library_on_disk_was_built_from_the_current_sources(built):
    b = importlib.import_module("msm_webgpu_amd.build")
    assert os.path.exists(_lib().so) and not b.needs_build(_lib()) and b.device_asm_is_current(_lib())
