"""The code-generation gates (tools/check_long_branch_hazard.py, tools/check_machine_verifier.py) over the five units of libmsm_frmat.so, which
are not among the other five libraries' units; every unit's kernels sit in the unit's own namespace, none of them uses scratch memory or spills,
their LDS is what DESIGN.md section 4.21 states, and the library on disk is the current sources'.  Resource metadata only."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402

KERNELS = ("k_frmat_lift", "k_frmat_tile", "k_frmat_stitch")


def _units():
    import importlib

    return list(importlib.import_module("msm_webgpu_amd.build").FR_LIBRARIES["frmat"].units)


def test_frmat_units_have_no_long_branch_hazard(built):
    paths = chk.compile_to_asm([], units=_units())
    assert len(paths) == 5 and all("frmat_" in os.path.basename(p) for p in paths)
    for path in paths:
        long_branches, found, live = chk.check_file(path)
        assert found == [] and live == [], (path, found, live)


def test_frmat_units_pass_the_machine_verifier():
    import check_machine_verifier as mv

    reports = mv.check(units=_units())
    assert sorted(reports) == sorted(_units())
    for unit, found in reports.items():
        assert found == [], (unit, found)


def test_each_unit_holds_its_kernels_in_its_own_namespace_without_scratch(built):
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("### 4.21"):]
    section = section[:section.index("\n## ")]
    assert "LDS 10,240 B" in section  # (the LDS size asserted below is the one the document states)
    for path in chk.compile_to_asm([], units=_units()):
        with open(path) as f:
            text = f.read()
        names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
        field = "frt_" + os.path.basename(path).split("-hip-")[0][len("frmat_"):]
        assert len(names) == len(KERNELS), (path, names)
        for k in KERNELS:
            mine = [n for n in names if ("%d%s" % (len(field), field)) in n and ("%d%s" % (len(k), k)) in n]
            assert len(mine) == 1, (path, k, names)
        # the kernel descriptors and the metadata: no private segment, nothing spilled, no dynamic stack
        assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS) and re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert not re.search(r"\.uses_dynamic_stack:\s+true", text), path
        # LDS: 256 slots of nine limbs and 256 flags in tile and stitch; none in lift
        assert sorted(int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", text)) == [0, 10240, 10240], path


def test_library_on_disk_was_built_from_the_current_sources(built):
    import importlib

    b = importlib.import_module("msm_webgpu_amd.build")
    assert os.path.exists(b.FR_LIBRARIES["frmat"].so) and not b.needs_build(b.FR_LIBRARIES["frmat"])
    assert b.device_asm_is_current(b.FR_LIBRARIES["frmat"])
