"""The recode and the sort see no field, so the library holds them once: csrc/sort_kernels.h is compiled by msm_hip.hip alone, and a curve unit
(curve_<name>.hip) emits nothing but its own curve's kernels.  Read off the device assembly the build leaves behind, like the code-generation
gates (tests/test_codegen_hazards.py)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msm-webgpu_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402

# kernels of the library before the sort left the curve units: 183 in the unit of the host code, 51 in each of four G1 units, 45 in each G2 unit
KERNELS_BEFORE = 183 + 4 * 51 + 2 * 45
# the nine sort kernels that each of the six curve units of that time emitted and nothing could launch
DEAD_BEFORE = 6 * 9


def _kernels_by_unit():
    """unit name -> demangled names of the kernels its device assembly defines"""
    out = {}
    for path in chk.compile_to_asm([]):
        with open(path) as f:
            mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), flags=re.M)
        names = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
        out[os.path.basename(path).split("-hip-")[0]] = [n for n in names if n]
    return out


def _globals_of(header):
    with open(os.path.join(CSRC, header)) as f:
        text = f.read()
    names = re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", text)
    assert len(names) == text.count("__global__"), header  # every kernel of the header was recognised
    return sorted(set(names))


def test_every_sort_kernel_is_compiled_by_one_unit():
    units = _kernels_by_unit()
    assert len(units) == 8
    sort_kernels = _globals_of("sort_kernels.h")
    assert "k_sort_fine" in sort_kernels and "k_scatter_coarse" in sort_kernels and "k_copy_runs" in sort_kernels
    for k in sort_kernels:
        emitters = [u for u, names in units.items() if any(re.search(r"\bmsm_sort::%s\b" % k, n) for n in names)]
        assert emitters == ["msm_hip"], (k, emitters)
        assert not any(re.search(r"(?<!msm_sort)::%s\b" % k, n) for names in units.values() for n in names), k  # ... and in no other namespace
    # k_count (recode.h) is shared with the curve units, which build it over their own endomorphism split and over nothing else
    assert _globals_of("recode.h") == ["k_count"]
    for u, names in units.items():
        for n in names:
            if re.search(r"\bk_count<", n):
                assert ("glv_split_fn" in n) == (u != "msm_hip"), (u, n)


def test_a_curve_unit_holds_only_its_own_kernels():
    units = _kernels_by_unit()
    curve_units = sorted(u for u in units if u.startswith("curve_"))
    assert len(curve_units) == 7
    for u in curve_units:
        ns = "msmk" if u == "curve_bn254" else "msmk_" + u[len("curve_"):]
        assert units[u], u
        for n in units[u]:
            # in the unit's namespace, or the shared k_count over the unit's split functor
            assert re.search(r"\b%s::" % ns, n), (u, n)
            assert set(re.findall(r"\b(msmk\w*)::", n)) == {ns}, (u, n)
            if not re.search(r"^(void )?%s::k_\w+" % ns, n):
                assert re.search(r"^void msm_recode::k_count<\d+, 4, %s::glv_split_fn" % ns, n), (u, n)
    assert all(re.search(r"^(void )?msm_(sort|recode)::", n) for n in units["msm_hip"]), "the host code's unit holds the curve-neutral kernels only"


def test_the_dead_sort_kernels_are_gone():
    total = sum(len(names) for names in _kernels_by_unit().values())
    assert total <= KERNELS_BEFORE - DEAD_BEFORE, total
