"""The code-generation gates (tools/check_long_branch_hazard.py, tools/check_machine_verifier.py) over the one unit of libmsm_frmem.so; its fifteen
kernels sit in the library's namespace, use no scratch memory and spill nothing, and their LDS and registers are what DESIGN.md section 4.27
states.  Resource metadata only."""
import importlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402

# the name in DESIGN.md's table -> what the kernel's symbol holds (j: 32-bit keys, m: 64-bit; Li0 nodes, Li1 digit counts, Li2 heads of runs)
KERNELS = {"k_frmem_hist<u32>": "12k_frmem_histIjE", "k_frmem_hist<u64>": "12k_frmem_histImE", "k_frmem_scatter<u32>": "15k_frmem_scatterIjE",
           "k_frmem_scatter<u64>": "15k_frmem_scatterImE", "k_frmem_sums<nodes>": "12k_frmem_sumsILi0EjE", "k_frmem_sums<counts>": "12k_frmem_sumsILi1EjE",
           "k_frmem_sums<heads,u32>": "12k_frmem_sumsILi2EjE", "k_frmem_sums<heads,u64>": "12k_frmem_sumsILi2EmE", "k_frmem_scan<nodes>": "12k_frmem_scanILi0EjE",
           "k_frmem_scan<counts>": "12k_frmem_scanILi1EjE", "k_frmem_scan<heads,u32>": "12k_frmem_scanILi2EjE", "k_frmem_scan<heads,u64>": "12k_frmem_scanILi2EmE",
           "k_frmem_fill": "12k_frmem_fill", "k_frmem_access<u32>": "14k_frmem_accessIjE", "k_frmem_access<u64>": "14k_frmem_accessImE"}


def _lib():
    return importlib.import_module("msm_webgpu_amd.build").MEM_LIBRARIES["frmem"]


def _stated():
    """kernel -> (VGPRs, SGPRs, LDS bytes) from the table of DESIGN.md section 4.27"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("### 4.27"):]
    section = section[:section.index("\n## ")]
    rows = dict((k, (int(v), int(s), int(lds))) for k, v, s, lds in re.findall(r"^\| `(k_frmem_[\w<>,]+)` \| (\d+) \| (\d+) \| (\d+) B \| 0 B \| 0 \|$", section, flags=re.M))
    assert sorted(rows) == sorted(KERNELS), rows
    return rows


def _asm():
    paths = chk.compile_to_asm([], units=list(_lib().units))
    assert len(paths) == 1 and os.path.basename(paths[0]).startswith("frmem")
    return paths[0]


def test_the_unit_has_no_long_branch_hazard(built):
    long_branches, found, live = chk.check_file(_asm())
    assert found == [] and live == [], (found, live)


def test_the_unit_passes_the_machine_verifier():
    import check_machine_verifier as mv

    reports = mv.check(units=list(_lib().units))
    assert reports == {"frmem.hip": []}, reports


def test_the_kernels_use_no_scratch_and_the_resources_the_design_states(built):
    stated = _stated()
    with open(_asm()) as f:
        text = f.read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == len(KERNELS) and all(n.startswith("_ZN5frmem") for n in names), names
    for k, part in KERNELS.items():
        assert len([n for n in names if part in n]) == 1, (k, names)
    # the kernel descriptors and the metadata: no private segment, nothing spilled, no dynamic stack
    assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text) == ["0"] * len(KERNELS)
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * len(KERNELS)
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS) and re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS)
    assert not re.search(r"\.uses_dynamic_stack:\s+true", text)
    # no atomic of any kind, in LDS or in memory: the ranks come from ballots and from counts with one writer each
    assert not re.search(r"^\s*(ds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*|global_atomic\w*|flat_atomic\w*)\s", text, flags=re.M)
    # LDS and registers, kernel by kernel, as DESIGN.md section 4.27 states them
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.symbol:\s+(\S+?)\.kd.*?\.vgpr_count:\s+(\d+)", text, flags=re.S)
    assert len(meta) == len(KERNELS)
    for lds, sgprs, symbol, vgprs in meta:
        k = [k for k, part in KERNELS.items() if part in symbol]
        assert len(k) == 1 and (int(vgprs), int(sgprs), int(lds)) == stated[k[0]], (symbol, vgprs, sgprs, lds, stated)


def test_library_on_disk_was_built_from_the_current_sources(built):
    b = importlib.import_module("msm_webgpu_amd.build")
    assert os.path.exists(_lib().so) and not b.needs_build(_lib()) and b.device_asm_is_current(_lib())
