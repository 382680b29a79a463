"""The code-generation gates (tools/check_long_branch_hazard.py, tools/check_machine_verifier.py) over the five units of libmsm_frmle.so, which
are not among the other four libraries' units; every unit's kernels sit in the unit's own namespace, none of them uses scratch memory or spills,
and the library on disk is the current sources'."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402

# k_frmle_round is instantiated per number of points, 2 .. 5
KERNELS = ("k_frmle_fold", "k_frmle_eval", "k_frmle_eq", "k_frmle_sum") + ("k_frmle_round",) * 4


def _units():
    import importlib

    return list(importlib.import_module("msm_webgpu_amd.build").FR_LIBRARIES["frmle"].units)


def test_frmle_units_have_no_long_branch_hazard(built):
    paths = chk.compile_to_asm([], units=_units())
    assert len(paths) == 5 and all("frmle_" in os.path.basename(p) for p in paths)
    for path in paths:
        long_branches, found, live = chk.check_file(path)
        assert found == [] and live == [], (path, found, live)


def test_frmle_units_pass_the_machine_verifier():
    import check_machine_verifier as mv

    reports = mv.check(units=_units())
    assert sorted(reports) == sorted(_units())
    for unit, found in reports.items():
        assert found == [], (unit, found)


def test_each_unit_holds_its_kernels_in_its_own_namespace_without_scratch(built):
    for path in chk.compile_to_asm([], units=_units()):
        with open(path) as f:
            text = f.read()
        names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
        field = "frm_" + os.path.basename(path).split("-hip-")[0][len("frmle_"):]
        assert len(names) == len(KERNELS), (path, names)
        for k in set(KERNELS):
            mine = [n for n in names if ("%d%s" % (len(field), field)) in n and ("%d%s" % (len(k), k)) in n]
            assert len(mine) == KERNELS.count(k), (path, k, names)
        # the kernel descriptors and the metadata: no private segment, nothing spilled, no dynamic stack
        assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS) and re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * len(KERNELS), path
        assert not re.search(r"\.uses_dynamic_stack:\s+true", text), path
        # LDS: 256 slots of nine limbs in eval, round and sum; none in fold and eq
        assert sorted(int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", text)) == [0, 0] + [9216] * 6, path


def test_library_on_disk_was_built_from_the_current_sources(built):
    import importlib

    b = importlib.import_module("msm_webgpu_amd.build")
    assert os.path.exists(b.FR_LIBRARIES["frmle"].so) and not b.needs_build(b.FR_LIBRARIES["frmle"])
    assert b.device_asm_is_current(b.FR_LIBRARIES["frmle"])
