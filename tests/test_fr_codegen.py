"""The code-generation gates (tools/check_long_branch_hazard.py, tools/check_machine_verifier.py; tests/test_codegen_hazards.py) over the four
scalar-field units of libmsm_fr.so, which are not among libmsm_hip.so's translation units and so are not seen by the gates' default run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402


def _units():
    import importlib

    return list(importlib.import_module("msm_webgpu_amd.build").FR_LIBRARIES["fr"].units)


def test_fr_units_have_no_long_branch_hazard(built):
    paths = chk.compile_to_asm([], units=_units())
    assert len(paths) == 4 and all("fr_" in os.path.basename(p) for p in paths)
    for path in paths:
        long_branches, found, live = chk.check_file(path)
        assert found == [] and live == [], (path, found, live)
        with open(path) as f:
            assert "k_ntt_pass" in f.read(), path


def test_fr_units_pass_the_machine_verifier():
    import check_machine_verifier as mv

    reports = mv.check(units=_units())
    assert sorted(reports) == sorted(_units())
    for unit, found in reports.items():
        assert found == [], (unit, found)


def test_library_on_disk_was_built_from_the_current_sources(built):
    import importlib

    b = importlib.import_module("msm_webgpu_amd.build")
    assert os.path.exists(b.FR_LIBRARIES["fr"].so) and not b.needs_build(b.FR_LIBRARIES["fr"])
    assert b.device_asm_is_current(b.FR_LIBRARIES["fr"])
