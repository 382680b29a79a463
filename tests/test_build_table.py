"""msm-webgpu_amd/build.py's table of libraries, checked for every pair of them: libmsm_hip.so and the eight scalar-field libraries of
FR_LIBRARIES share no unit, no file but the field arithmetic and the host scaffold, no exported symbol with storage; and each still exports
the C functions it did before the table (tests/golden/fr_exports.json: names only, from this project's own libraries)."""
import importlib
import itertools
import json
import os
import subprocess

import pytest

FOUR = ["bls12_381", "bn254", "pallas", "vesta"]
FIVE = ["bls12_381", "bn254", "grumpkin", "pallas", "vesta"]
FIELDS = {"fr": FOUR, "frvec": FOUR, "frpoly": FOUR, "frmle": FIVE, "frmat": FIVE, "frgate": FIVE, "frlook": FIVE, "frhash": FIVE}
# what two libraries may both list: the field arithmetic, the host field, the fields' constants, the host scaffold
SHARED = {"fq29.h", "fq29_asm.h", "host_fr.h", "fr_host_common.h"} | {"fr_%s_constants.h" % f for f in FIVE}
# std::piecewise_construct, an empty tag of the C++ library that every user of std::map defines weakly: a constant, not state
NOT_STATE = {"_ZSt19piecewise_construct"}


def _build():
    return importlib.import_module("msm_webgpu_amd.build")


def _libraries():
    """name -> (library file, units, sources), libmsm_hip.so included"""
    b = _build()
    libs = {"hip": (b.SO, b.TRANSLATION_UNITS, b.SOURCES)}
    libs.update((name, (lib.so, lib.units, lib.sources)) for name, lib in b.FR_LIBRARIES.items())
    return libs


def _symbols(so):
    """(type, name) of every symbol the library defines"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], universal_newlines=True)
    return [tuple(ln.split()[1:]) for ln in out.splitlines() if len(ln.split()) == 3]


def test_the_table_holds_the_eight_libraries_in_order():
    b = _build()
    assert list(b.FR_LIBRARIES) == ["fr", "frvec", "frpoly", "frmle", "frmat", "frgate", "frlook", "frhash"]
    for name, lib in b.FR_LIBRARIES.items():
        assert lib.name == name and os.path.basename(lib.so) == "libmsm_%s.so" % name
        assert [os.path.basename(h) for h in lib.headers] == ["msm_%s.h" % name, "msm_hip.h"] and all(os.path.exists(h) for h in lib.headers)
    assert os.path.basename(os.path.join(b.HERE, "libmsm_hip.so")) == "libmsm_hip.so" and len(b.TRANSLATION_UNITS) == 8


def test_units_are_the_expected_lists():
    b = _build()
    for name, lib in b.FR_LIBRARIES.items():
        assert sorted(lib.units) == ["%s_%s.hip" % (name, f) for f in FIELDS[name]], name
        assert lib.units[0] == name + "_bn254.hip", name  # (the unit that carries the host code is compiled first)
        assert b.library_of(lib.units) is lib and b.library_of(lib.units[1:2]) is lib
    assert sorted(b.TRANSLATION_UNITS) == sorted(["msm_hip.hip"] + ["curve_%s.hip" % c for c in FIVE + ["bn254_g2", "bls12_381_g2"]])
    assert b.library_of(b.TRANSLATION_UNITS) is None and b.library_of([]) is None and b.library_of(None) is None


def test_sources_are_todays_lists():
    b = _build()
    for name, lib in b.FR_LIBRARIES.items():
        stem = "ntt" if name == "fr" else name
        want = set(lib.units) | {name + "_unit.h", stem + "_kernels.h", stem + "_host.h", stem + "_plan.h", "fr_host_common.h", "host_fr.h"}
        want |= {"fr_%s_constants.h" % f for f in FIELDS[name]} | (set() if name == "frlook" else {"fq29.h", "fq29_asm.h"})
        assert set(lib.sources) == want and len(lib.sources) == len(want), name


def test_every_listed_source_exists_and_every_unit_is_a_source():
    b = _build()
    for name, (_, units, sources) in _libraries().items():
        assert set(units) <= set(sources), name
        for f in sources:
            assert os.path.exists(os.path.join(b.CSRC, f)), (name, f)


def test_every_pair_of_libraries_is_apart():
    libs = _libraries()
    for (a, (_, a_units, a_sources)), (c, (_, c_units, c_sources)) in itertools.combinations(libs.items(), 2):
        assert not set(a_units) & set(c_units), (a, c)
        assert set(a_sources) & set(c_sources) <= SHARED, (a, c)


def test_no_library_lists_a_file_of_another():
    libs = _libraries()
    for name, (_, _, sources) in libs.items():
        own = [f for f in sources if f not in SHARED]
        for other in libs:
            if other not in (name, "hip"):
                assert not any(f.startswith(other + "_") for f in own), (name, other)
        if name != "hip":
            assert not any(f.startswith(("curve_", "msm_")) or (f.startswith("fq2") and not f.startswith("fq29")) for f in sources), name
        assert any(f.startswith("ntt_") for f in sources) == (name == "fr"), name


def test_every_library_is_built_from_the_current_sources(built):
    b = _build()
    assert os.path.exists(b.SO) and not b.needs_build() and b.device_asm_is_current()
    for name, lib in b.FR_LIBRARIES.items():
        assert os.path.exists(lib.so) and not b.needs_build(lib), name
        assert b.device_asm_is_current(lib), name
        assert [os.path.basename(f) for f in b.device_asm_files(lib)] == [os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s" for u in lib.units]


def test_every_library_exports_the_c_functions_it_did(built):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fr_exports.json")) as f:
        want = json.load(f)
    libs = _libraries()
    assert sorted(want) == sorted(libs)
    for name, (so, _, _) in libs.items():
        got = sorted(s for t, s in _symbols(so) if t in "TW" and s.startswith("msm_"))
        assert got == want[name], name


def test_no_two_libraries_define_the_same_static_storage(built):
    """the rule for the state of csrc/fr_host_common.h: a lock, a map of per-device state or a test hook that two libraries both defined
    would be one object in a process that loads both"""
    owners = {}
    for name, (so, _, _) in _libraries().items():
        for s in {s for t, s in _symbols(so) if t in "BbDdVvu"} - NOT_STATE:
            owners.setdefault(s, []).append(name)
    assert {s: names for s, names in owners.items() if len(names) > 1} == {}
    assert sum("lock_of" in s for s in owners) == 8 and sum("states_of" in s and not s.startswith("_ZGV") for s in owners) == 8  # (one of each per library)
