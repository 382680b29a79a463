"""libmsm_frmem.so in the C ABI (include/msm_frmem.h) and in the build (msm-webgpu_amd/build.py's MEM_LIBRARIES), without a GPU: the header's
declarations are the library's exports at ABI version 1, it shares no symbol with static storage with libmsm_hip.so, the eight scalar-field
libraries or libmsm_frcol.so, those ten are still current after build() and export what they did, the build's helpers answer for the new row as
they do for the old, and a call without a device says so and leaves its buffers alone."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# std::piecewise_construct, an empty tag of the C++ library that every user of std::map defines weakly: a constant, not state
NOT_STATE = {"_ZSt19piecewise_construct"}
DECLARED = {
    "msm_frmem_abi_version": r"int msm_frmem_abi_version\s*\(void\)",
    "msm_frmem_sort_device": r"int msm_frmem_sort_device\s*\(int device, void\* stream, uint32_t\* perm_out, void\* keys_out, const void\* keys, size_t key_bytes, uint32_t key_bits, size_t n\)",
    "msm_frmem_sort": r"int msm_frmem_sort\s*\(int device, uint32_t\* perm_out, void\* keys_out, const void\* keys, size_t key_bytes, uint32_t key_bits, size_t n\)",
    "msm_frmem_access_device": r"int msm_frmem_access_device\s*\(int device, void\* stream, uint32_t\* rank_out, uint32_t\* prev_out, uint32_t\* counts_out, uint32_t\* last_out, size_t n_t, const void\* keys,\s*size_t key_bytes, uint32_t key_bits, size_t n, uint64_t\* distinct\)",
    "msm_frmem_access": r"int msm_frmem_access\s*\(int device, uint32_t\* rank_out, uint32_t\* prev_out, uint32_t\* counts_out, uint32_t\* last_out, size_t n_t, const void\* keys, size_t key_bytes,\s*uint32_t key_bits, size_t n, uint64_t\* distinct\)",
    "msm_frmem_release": r"void msm_frmem_release\s*\(void\)",
    "msm_frmem_test_tile": r"int msm_frmem_test_tile\s*\(int entries\)",
    "msm_frmem_test_last": r"int msm_frmem_test_last\s*\(int\* launches, int\* levels\)",
}


def _build():
    return importlib.import_module("msm_webgpu_amd.build")


def _symbols(so):
    """(type, name) of every symbol the library defines"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], universal_newlines=True)
    return [tuple(ln.split()[1:]) for ln in out.splitlines() if len(ln.split()) == 3]


def _others(b):
    """the ten libraries that were there before: name -> file"""
    others = {"hip": b.SO}
    others.update((name, row.so) for name, row in list(b.FR_LIBRARIES.items()) + list(b.AUX_LIBRARIES.items()))
    assert len(others) == 10
    return others


def test_the_headers_declarations_are_the_librarys_exports(built):
    from msm_webgpu_amd import memory

    b = _build()
    with open(os.path.join(ROOT, "include", "msm_frmem.h")) as f:
        full = f.read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name, pattern in DECLARED.items():
        assert re.search(r"\b" + pattern, text), name
    assert sorted(set(re.findall(r"\b(msm_frmem_\w+)\s*\(", text))) == sorted(DECLARED)
    exported = sorted(s for t, s in _symbols(b.MEM_LIBRARIES["frmem"].so) if t in "TW" and s.startswith("msm_"))
    assert exported == sorted(DECLARED)
    for name, value in (("MISSING", "0xFFFFFFFFu"), ("MAX_ELEMENTS", r"\(1u << 26\)")):
        assert re.search(r"#define MSM_FRMEM_%s %s\s" % (name, value), text), name
    for word in ("MSM_HIP_ERR_INVALID_ARG", "NO output is written", "ONE device-to-host copy", "stable ascending argsort", "no atomics", "serialised"):  # (the conventions are stated)
        assert word in full, word
    L = memory.frmem_lib()
    assert L.msm_frmem_abi_version() == 1
    assert sorted("msm_frmem_" + fn for fn in memory.FRMEM_ABI) == sorted(set(DECLARED) - {"msm_frmem_abi_version"})
    assert (memory.MISSING, memory.MAX_ELEMENTS) == (0xFFFFFFFF, 1 << 26)
    # the binding has one argument type per parameter of the declaration
    for fn, argtypes in memory.FRMEM_ABI.items():
        params = re.search(r"\bmsm_frmem_%s\s*\(([^)]*)\)" % fn, text).group(1)
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), fn


def test_the_python_module_stands_beside_the_pinned_ones(built):
    """memory.py is nobody's import: neither api.py nor scalars.py nor columns.py nor the package names it or anything of it"""
    import msm_webgpu_amd
    from msm_webgpu_amd import api, columns, memory, scalars

    names = ("argsort", "access_counters", "sorted_trace", "offline_check", "offline_products", "frmem_lib", "frmem_test_tile", "frmem_last", "frmem_release")
    for mod in (msm_webgpu_amd, api, scalars, columns):
        for name in names:
            assert not hasattr(mod, name), (mod.__name__, name)
    assert "frmem" not in scalars.FR_ABI and "frmem" not in _build().FR_LIBRARIES and "frmem" not in _build().AUX_LIBRARIES
    for name in names:
        assert callable(getattr(memory, name)), name
    for src in ("api.py", "scalars.py", "__init__.py", "_core.py", "columns.py"):
        with open(os.path.join(ROOT, "msm-webgpu_amd", src)) as f:
            assert not re.search(r"^\s*(from|import)\b.*\bmemory\b", f.read(), flags=re.M), src
    with open(os.path.join(ROOT, "msm-webgpu_amd", "memory.py")) as f:
        assert not re.search(r"^\s*(from|import)\b.*\b(api|scalars)\b", f.read(), flags=re.M)


def test_the_table_row_and_what_the_build_answers_for_it(built):
    b = _build()
    assert list(b.MEM_LIBRARIES) == ["frmem"]
    lib = b.MEM_LIBRARIES["frmem"]
    assert isinstance(lib, b.FrLibrary) and lib.name == "frmem" and os.path.basename(lib.so) == "libmsm_frmem.so" and lib.units == ["frmem.hip"]
    assert sorted(lib.sources) == ["fr_host_common.h", "frmem.hip", "frmem_host.h", "frmem_kernels.h", "frmem_plan.h"]
    assert [os.path.basename(h) for h in lib.headers] == ["msm_frmem.h", "msm_hip.h"] and all(os.path.exists(h) for h in lib.headers)
    assert all(os.path.exists(os.path.join(b.CSRC, f)) for f in lib.sources)
    assert b.library_of(["frmem.hip"]) is lib and b.library_of(lib.units) is lib
    # one helper yields the rows of all three tables, in order, and the others are answered for as before
    rows = b.library_rows()
    assert rows == list(b.FR_LIBRARIES.values()) + list(b.AUX_LIBRARIES.values()) + [lib] and len(rows) == 10
    for row in rows[:-1]:
        assert b.library_of(row.units) is row and b.library_of(row.units[:1]) is row, row.name
        assert not set(row.units) & set(lib.units) and set(row.sources) & set(lib.sources) == {"fr_host_common.h"}, row.name
    assert b.library_of(b.TRANSLATION_UNITS) is None and b.library_of([]) is None and b.library_of(None) is None
    assert b.library_of(["frmem.hip", "frcol.hip"]) is None
    assert not set(b.SOURCES) & set(lib.sources)
    with open(os.path.join(ROOT, "msm-webgpu_amd", "build.py")) as f:
        src = f.read()
    assert src.count("list(AUX_LIBRARIES.values())") == 0 and src.count("library_rows()") >= 4  # (no concatenation of the tables but the helper's)
    # built, stamped and its device assembly kept, by the same rules
    assert os.path.exists(lib.so) and not b.needs_build(lib) and b.device_asm_is_current(lib)
    assert [os.path.basename(f) for f in b.device_asm_files(lib)] == ["frmem-hip-amdgcn-amd-amdhsa-gfx950.s"]
    assert os.path.dirname(b.device_asm_files(lib)[0]) == b.TEMPS
    with open(lib.so + ".stamp") as f:
        assert f.read().strip() == b.build_stamp(lib)
    assert b.build_stamp(lib) not in {b.build_stamp()} | {b.build_stamp(row) for row in rows[:-1]}


def test_the_ten_other_libraries_are_still_current_and_export_what_they_did(built):
    b = _build()
    assert os.path.exists(b.SO) and b.stamp_is_current() and not b.needs_build()
    for row in b.library_rows()[:-1]:
        assert os.path.exists(row.so) and not b.needs_build(row), row.name
        with open(row.so + ".stamp") as f:
            assert f.read().strip() == b.build_stamp(row), row.name
    with open(os.path.join(ROOT, "tests", "golden", "fr_exports.json")) as f:
        want = json.load(f)
    for name, so in _others(b).items():
        got = sorted(s for t, s in _symbols(so) if t in "TW" and s.startswith("msm_"))
        if name in want:
            assert got == want[name], name
        assert not set(got) & set(DECLARED), name  # and no exported function of one is an exported function of the other


def test_no_static_storage_is_shared_with_the_other_ten(built):
    """the rule for the state of csrc/fr_host_common.h: a lock, a map of per-device state or a test hook that this library and another both
    defined would be one object in a process that loads both"""
    b = _build()
    mine = {s for t, s in _symbols(b.MEM_LIBRARIES["frmem"].so) if t in "BbDdVvu"} - NOT_STATE
    assert sum("lock_of" in s for s in mine) == 1 and sum("states_of" in s and not s.startswith("_ZGV") for s in mine) == 1  # its own lock and its own map
    # ... named after its namespace, the hooks too (__hip_cuid_<hash>: the compiler's own mark of a translation unit)
    assert all("frmem" in s for s in mine if not s.startswith("__hip_cuid_")), sorted(mine)
    for name, so in _others(b).items():
        theirs = {s for t, s in _symbols(so) if t in "BbDdVvu"} - NOT_STATE
        assert not mine & theirs, (name, sorted(mine & theirs))


def test_a_call_without_a_device_says_so_and_leaves_its_buffers_alone(built):
    from msm_webgpu_amd import memory

    L = memory.frmem_lib()
    buf = C.create_string_buffer(b"\xa5" * 4096, 4096)
    base = C.addressof(buf)
    distinct = C.c_uint64(77)
    if torch.cuda.is_available():
        assert L.msm_frmem_sort(99, base, base + 1024, base + 2048, 4, 32, 100) == -1  # (a device that is not there)
        assert L.msm_frmem_access(99, base, base + 400, base + 800, base + 1000, 50, base + 2048, 4, 32, 100, C.byref(distinct)) == -1
    else:
        assert L.msm_frmem_sort(0, base, base + 1024, base + 2048, 4, 32, 100) == -1
        assert L.msm_frmem_sort_device(0, None, base, None, base + 2048, 8, 64, 100) == -1
        assert L.msm_frmem_access(0, base, base + 400, base + 800, base + 1000, 50, base + 2048, 4, 32, 100, C.byref(distinct)) == -1
        assert L.msm_frmem_access_device(0, None, None, None, None, base, 1, base + 2048, 4, 8, 100, C.byref(distinct)) == -1
    assert buf.raw == b"\xa5" * 4096 and distinct.value == 77
    launches, levels = memory.frmem_last()
    assert (launches, levels) == (0, 0) or torch.cuda.is_available()
