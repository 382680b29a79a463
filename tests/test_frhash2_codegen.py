"""How the Poseidon2 path of libmsm_frhash.so is built, beside tests/test_frhash_codegen.py (registers, LDS, scratch, spills: the whole kernels):
each kernel holds an instance of the lane's function for either kind of handle, and in neither is a table of constants read with a vector
load -- the only global loads are the two halves of an element of the lane's own data.  Resource metadata and assembly text only."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_long_branch_hazard as chk  # noqa: E402


def _units():
    import importlib

    return list(importlib.import_module("msm_webgpu_amd.build").FR_LIBRARIES["frhash"].units)


def _kernels(text):
    """the assembly of each kernel: from its label to its .amdhsa_kernel descriptor"""
    bodies = re.findall(r"^(_Z\w*k_frhash_\w+):[^\n]*\n(.*?)^\s*\.amdhsa_kernel \1$", text, flags=re.M | re.S)
    assert len(bodies) == 2, [name for name, _ in bodies]
    return bodies


def test_no_table_is_read_with_a_vector_load_and_both_instances_are_there(built):
    for path in chk.compile_to_asm([], units=_units()):
        with open(path) as f:
            text = f.read()
        for name, body in _kernels(text):
            loads = re.findall(r"^\s*(global_load\w*\s.*)$", body, flags=re.M)
            # a lane's element is two 16-byte loads at the lane's own address; an instance of the lane's function has one such site, a kernel
            # one instance for either kind.  A constant read through a pointer carried round a loop shows as a load with a scalar base.
            assert len(loads) == 4, (path, name, loads)
            for load in loads:
                assert re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\[\d+:\d+\], off(?: offset:16)?$", load.strip()), (path, name, load)
            assert not re.search(r"^\s*(?:flat|scratch|buffer)_load", body, flags=re.M), (path, name)
            # the tables come through s_load_dwordx8: the Poseidon instance has 7 sites (in, out, the constants, the matrix's single product and
            # its pair), the Poseidon2 instance at least its three tables (external constants, internal constants, mu) beside in and out
            assert len(re.findall(r"^\s*s_load_dwordx8\b", body, flags=re.M)) >= 7 + 3, (path, name)
