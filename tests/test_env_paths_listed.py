"""No untested settings: every MSM_HIP_* variable the library reads (getenv in msm-webgpu_amd/csrc) has a row in the oracle-checked GPU test
tests/test_gpu_env_paths.py, or an explicit exclusion with its reason, and is documented in INTEGRATION.md.  (Build-time variables read by
build.py are not the library's settings.)  Also: the decision after which that module starts no further child process."""
import os
import re

import pytest

from tests import test_gpu_env_paths as gpu_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msm-webgpu_amd", "csrc")
GETENV = re.compile(r'getenv\(\s*"(MSM_HIP_[A-Z0-9_]+)"\s*\)')


def library_settings(csrc=CSRC):
    names = set()
    for f in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, f), errors="replace") as fh:
            names.update(GETENV.findall(fh.read()))
    return names


def unlisted(names):
    """names with neither a row nor an exclusion"""
    return sorted(n for n in names if n not in gpu_rows.row_variables() and n not in gpu_rows.EXCLUDED)


def undocumented(names):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    return sorted(n for n in names if not re.search(r"`%s(=[^`]*)?`" % n, doc) and not re.search(r"`[^`]*\b%s\b[^`]*`" % n, doc))


def test_settings_are_found():
    names = library_settings()
    assert len(names) >= 20 and "MSM_HIP_WINDOW_BITS" in names and "MSM_HIP_COMBINE_THREADS" in names, names


def test_every_setting_has_a_row_or_an_exclusion():
    assert unlisted(library_settings()) == []
    assert all(reason for reason in gpu_rows.EXCLUDED.values())
    # an exclusion or a row names a variable the library still reads
    assert set(gpu_rows.EXCLUDED) <= library_settings()
    assert gpu_rows.row_variables() <= library_settings()


def test_every_setting_is_documented():
    assert undocumented(library_settings()) == []


def test_guard_catches_a_new_setting(tmp_path):
    """a getenv of a name no row and no document knows makes both checks fail"""
    for f in os.listdir(CSRC):
        with open(os.path.join(CSRC, f), "rb") as src, open(tmp_path / f, "wb") as dst:
            dst.write(src.read())
    with open(tmp_path / "msm_hip.hip", "a") as f:
        f.write('\nstatic const char* probe_ = getenv("MSM_HIP_FOO");\n')
    names = library_settings(str(tmp_path))
    assert unlisted(names) == ["MSM_HIP_FOO"]
    assert undocumented(names) == ["MSM_HIP_FOO"]


@pytest.mark.parametrize("rc,abnormal", [(0, False), (1, False), (2, False), (None, True), (-6, True), (-9, True), (-11, True),
                                         (124, True), (134, True), (137, True), (139, True)])
def test_abnormal_exit_decision(rc, abnormal):
    assert gpu_rows.is_abnormal(rc) is abnormal


def test_rows_are_well_formed():
    ids = [r[0] for r in gpu_rows.ROWS]
    assert len(ids) == len(set(ids))
    for rid, env, workload, limit, check in gpu_rows.ROWS:
        assert env and all(k.startswith("MSM_HIP_") for k in env), rid
        assert "GPU_MAX_HW_QUEUES" not in env and not any(k.startswith(("HIP_", "HSA_", "AMD_")) for k in env), rid
        assert 0 < limit <= 240 and callable(check), rid
