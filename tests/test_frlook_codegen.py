"""The code-generation gates (tools/check_long_branch_hazard.py, tools/check_machine_verifier.py) over the five units of libmsm_frlook.so, which
are not among the other seven libraries' units; every unit's kernels sit in the unit's own namespace, they use no scratch memory and spill
nothing, their LDS and vector registers are what DESIGN.md section 4.23 states, and the libraries on disk are the current sources'.  Resource
metadata only."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402

KERNELS = ("k_frlook_build", "k_frlook_count", "k_frlook_finish")


def _units():
    import importlib

    return list(importlib.import_module("msm_webgpu_amd.build").FR_LIBRARIES["frlook"].units)


def _stated():
    """kernel -> (VGPRs, LDS bytes) from the table of DESIGN.md section 4.23"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("### 4.23"):]
    section = section[:section.index("\n## ")]
    rows = dict((k, (int(v), int(lds))) for k, v, lds in re.findall(r"^\| `(k_frlook_\w+)` \| (\d+) \| \d+ \| (\d+) B \| 0 B \| 0 \|$", section, flags=re.M))
    assert sorted(rows) == sorted(KERNELS), rows
    return rows


def test_frlook_units_have_no_long_branch_hazard(built):
    paths = chk.compile_to_asm([], units=_units())
    assert len(paths) == 5 and all("frlook_" in os.path.basename(p) for p in paths)
    for path in paths:
        long_branches, found, live = chk.check_file(path)
        assert found == [] and live == [], (path, found, live)


def test_frlook_units_pass_the_machine_verifier():
    import check_machine_verifier as mv

    reports = mv.check(units=_units())
    assert sorted(reports) == sorted(_units())
    for unit, found in reports.items():
        assert found == [], (unit, found)


def test_each_unit_holds_its_kernels_in_its_own_namespace_without_scratch(built):
    stated = _stated()
    for path in chk.compile_to_asm([], units=_units()):
        with open(path) as f:
            text = f.read()
        names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
        field = "frl_" + os.path.basename(path).split("-hip-")[0][len("frlook_"):]
        assert len(names) == len(KERNELS), (path, names)
        for k in KERNELS:
            mine = [n for n in names if ("%d%s" % (len(field), field)) in n and ("%d%s" % (len(k), k)) in n]
            assert len(mine) == 1, (path, k, names)
        # the kernel descriptors and the metadata: no private segment, nothing spilled, no dynamic stack, no LDS
        assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS) and re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert not re.search(r"\.uses_dynamic_stack:\s+true", text), path
        # LDS and vector registers, kernel by kernel, as DESIGN.md section 4.23 states them
        meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.symbol:\s+(\S+?)\.kd.*?\.vgpr_count:\s+(\d+)", text, flags=re.S)
        assert len(meta) == len(KERNELS), path
        for lds, symbol, vgprs in meta:
            k = [k for k in KERNELS if ("%d%s" % (len(k), k)) in symbol]
            assert len(k) == 1 and (int(vgprs), int(lds)) == stated[k[0]], (path, symbol, vgprs, lds, stated)


def test_the_aggregated_count_has_no_compare_and_swap_loop(built):
    """k_frlook_count adds with one atomic add per group of equal indices -- the deferred group's flush inside the chunk loop and behind it, and
    the groups' leaders --, and nothing in it spins: the only compare-and-swap of a unit is the build's claim of a slot"""
    for path in chk.compile_to_asm([], units=_units()):
        with open(path) as f:
            text = f.read()
        assert len(re.findall(r"^\s*global_atomic_cmpswap\b", text, flags=re.M)) == 1, path
        assert len(re.findall(r"^\s*global_atomic_add\b", text, flags=re.M)) == 4, path  # counts[j] three times, and distinct
        assert len(re.findall(r"^\s*global_atomic_add_x2\b", text, flags=re.M)) == 1 and len(re.findall(r"^\s*global_atomic_umin_x2\b", text, flags=re.M)) == 1, path


def test_library_on_disk_was_built_from_the_current_sources(built):
    import importlib

    b = importlib.import_module("msm_webgpu_amd.build")
    assert os.path.exists(b.FR_LIBRARIES["frlook"].so) and not b.needs_build(b.FR_LIBRARIES["frlook"])
    assert b.device_asm_is_current(b.FR_LIBRARIES["frlook"])
