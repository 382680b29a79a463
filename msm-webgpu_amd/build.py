"""Build libmsm_hip.so, the scalar-field libraries (FR_LIBRARIES: libmsm_fr.so ... libmsm_frhash.so) and the field-neutral ones (AUX_LIBRARIES:
libmsm_frcol.so; MEM_LIBRARIES: libmsm_frmem.so) in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import collections
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# MSM_HIP_SO: load (and build into) another file, e.g. a diagnostic variant next to the product library
SO = os.environ.get("MSM_HIP_SO") or os.path.join(HERE, "libmsm_hip.so")
SOURCES = ["msm_hip.hip", "msm_plan.h", "msm_ctx.h", "msm_enqueue.h", "msm_bases.h", "msm_oneshot.h", "msm_hooks.h", "msm_mul.h", "msm_fft.h", "curve_bn254.hip", "curve_grumpkin.hip", "curve_pallas.hip", "curve_vesta.hip", "curve_bls12_381.hip", "curve_bn254_g2.hip", "curve_bls12_381_g2.hip", "fq2.h", "bn254_g2_constants.h", "bls12_381_g2_constants.h", "fq28x14_asm.h", "bls12_381_constants.h", "curve_ops.h", "msm_layout.h", "recode.h", "sort_kernels.h", "msm_kernels.h", "g1.h", "fq29.h", "fq29_asm.h", "host_g1.h", "host_fr.h", "host_pool.h", "host_worker.h", "glv.h", "scalar_mul.h", "msm_mgpu.h", "curve_select.h", "curve_unit.h", "grumpkin_constants.h", "bn254_constants.h", "pallas_constants.h", "vesta_constants.h"]
HEADER = os.path.join(HERE, "..", "include", "msm_hip.h")
# The scalar-field libraries (include/msm_<name>.h), each a library of its own beside libmsm_hip.so: one translation unit per scalar field, its
# own sources and stamp.  None of them is part of libmsm_hip.so (SO, SOURCES, TRANSLATION_UNITS and the no-argument forms of the functions
# below are that library's alone).  A new library is one more row of FR_LIBRARIES.
FrLibrary = collections.namedtuple("FrLibrary", "name so units sources headers")
FIELDS = ["bn254", "grumpkin", "pallas", "vesta", "bls12_381"]
NO_GRUMPKIN = [f for f in FIELDS if f != "grumpkin"]  # (no transform needs Grumpkin's scalar field: r - 1 = 2 * odd)


def _fr_library(name, fields=FIELDS, stem=None, field_math=True):
    """stem: what the kernels, host and plan headers are called (the library's name, but for the NTT); field_math: csrc/fq29.h, the multipliers"""
    units = ["%s_%s.hip" % (name, f) for f in fields]
    own = [name + "_unit.h"] + ["%s_%s.h" % (stem or name, part) for part in ("kernels", "host", "plan")]
    math = ["fq29.h", "fq29_asm.h"] if field_math else []
    sources = units + own + ["fr_host_common.h", "host_fr.h"] + math + ["fr_%s_constants.h" % f for f in fields]
    return FrLibrary(name, os.path.join(HERE, "libmsm_%s.so" % name), units, sources, [os.path.join(HERE, "..", "include", "msm_%s.h" % name), HEADER])


FR_LIBRARIES = collections.OrderedDict((lib.name, lib) for lib in [
    _fr_library("fr", NO_GRUMPKIN, stem="ntt"),  # the NTT
    _fr_library("frvec", NO_GRUMPKIN),  # vector arithmetic: map, batch inverse, scan
    _fr_library("frpoly", NO_GRUMPKIN),  # polynomial opening: eval, divide, dot, combine, powers
    _fr_library("frmle"),  # the sumcheck over multilinear tables: fold, eval, eq, round
    _fr_library("frmat"),  # sparse matrix-vector products: the rows Az, Bz, Cz of an R1CS
    _fr_library("frgate"),  # constraint evaluation: sums of products of rotated rows, the numerator of a PLONK quotient
    _fr_library("frlook", field_math=False),  # lookup arguments: it matches keys and computes nothing, so of the field's files the constants alone
    _fr_library("frhash"),  # Poseidon: batch permutations, sponges and Merkle trees
])
# Libraries that move scalars as stored and so are ONE translation unit for all fields, without a field's constants or arithmetic: rows of the same
# shape in a table of their own (DESIGN.md sections 4.25, 4.26), built, stamped and gated exactly like the rows of FR_LIBRARIES.
AUX_LIBRARIES = collections.OrderedDict((lib.name, lib) for lib in [
    FrLibrary("frcol", os.path.join(HERE, "libmsm_frcol.so"), ["frcol.hip"], ["frcol.hip", "frcol_kernels.h", "frcol_host.h", "frcol_plan.h", "fr_host_common.h"],
              [os.path.join(HERE, "..", "include", "msm_frcol.h"), HEADER]),  # lookup columns from counts: run expansion, halo2's permuted pair, gather
])
# Libraries over integer keys, without scalars at all: a third table of the same rows.
MEM_LIBRARIES = collections.OrderedDict((lib.name, lib) for lib in [
    FrLibrary("frmem", os.path.join(HERE, "libmsm_frmem.so"), ["frmem.hip"], ["frmem.hip", "frmem_kernels.h", "frmem_host.h", "frmem_plan.h", "fr_host_common.h"],
              [os.path.join(HERE, "..", "include", "msm_frmem.h"), HEADER]),  # memory arguments: stable argsort of integer keys, access counters
])
TEMPS = os.path.join(HERE, "..", "build", "temps" if not os.environ.get("MSM_HIP_SO") else "temps_" + os.path.basename(SO))


def library_rows():
    """Every row of every table, in build order: what build(), library_of(), device_asm_files() and needs_build() know of libraries beside libmsm_hip.so"""
    return [lib for table in (FR_LIBRARIES, AUX_LIBRARIES, MEM_LIBRARIES) for lib in table.values()]


def library_of(units):
    """The row (library_rows()) whose units contain `units`; None for libmsm_hip.so's units (and for none at all)."""
    return next((lib for lib in library_rows() if units and set(units) <= set(lib.units)), None)


def device_asm_files(lib=None):
    """The device assembly of every translation unit of a library (lib: one of library_rows(); None: libmsm_hip.so), as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in (lib.units if lib else TRANSLATION_UNITS)]


def device_asm_is_current(lib=None):
    """True if build() left the device assembly of the library's CURRENT sources behind (same staleness rule as the library itself)."""
    if needs_build(lib) or not all(os.path.exists(f) for f in device_asm_files(lib)):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in (lib.sources if lib else SOURCES) if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in device_asm_files(lib))


def build_stamp(lib=None):
    """what the library on disk must have been built FROM to be the product: a hash over the compile flags (the environment switches of the
    diagnostic builds included -- MSM_HIP_SLP, MSM_HIP_NO_ASM, MSM_HIP_EXTRA_FLAGS ...) and the contents of every source and public header.
    Written next to the library by build(); a library whose stamp differs (built once with variant flags, or from other sources) is rebuilt
    instead of being silently reused, and the code-generation gates (tools/check_machine_verifier.py, tools/check_long_branch_hazard.py) check
    the stamp of the library they vouch for."""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(lib.sources if lib else SOURCES)] + (lib.headers if lib else [HEADER]):
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def stamp_path():
    return SO + ".stamp"


def stamp_is_current():
    """True if the library on disk was built from the current sources with the current flags"""
    try:
        with open(stamp_path()) as f:
            return f.read().strip() == build_stamp()
    except OSError:
        return False


def variant_flags():
    """the environment switches that change the generated code (the diagnostic builds)"""
    return [k for k in ("MSM_HIP_SLP", "MSM_HIP_NO_ASM", "MSM_HIP_ASM_SMVP_ONLY", "MSM_HIP_EXTRA_FLAGS") if os.environ.get(k)]


def needs_build(lib=None):
    if lib:
        # a scalar-field library is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)
        if os.environ.get("MSM_HIP_SO"):
            return False
        try:
            with open(lib.so + ".stamp") as f:
                return not os.path.exists(lib.so) or f.read().strip() != build_stamp(lib)
        except OSError:
            return True
    if not os.path.exists(SO):
        return True
    if os.environ.get("MSM_HIP_SO"):
        # a diagnostic library named explicitly (built here with variant flags, run on the GPU box without them in the environment): its own
        # modification time decides -- the stamp rule below is the PRODUCT's
        t = os.path.getmtime(SO)
        return any(os.path.getmtime(d) > t for d in [os.path.join(CSRC, s) for s in SOURCES] + [HEADER] if os.path.exists(d))
    if os.path.exists(stamp_path()):
        return not stamp_is_current()
    # a library without a stamp (built by an older checkout): the modification times decide, as they used to
    t = os.path.getmtime(SO)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [HEADER]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


TRANSLATION_UNITS = ["msm_hip.hip", "curve_bls12_381_g2.hip", "curve_bn254_g2.hip", "curve_bls12_381.hip", "curve_bn254.hip", "curve_grumpkin.hip", "curve_pallas.hip", "curve_vesta.hip"]  # host + the curve-neutral sort; one per curve


def compile_flags():
    """hipcc flags of every translation unit (the environment switches of the diagnostic builds included)"""
    # -fno-slp-vectorize: the SLP vectoriser packs the limb arrays into <2 x i32> values, which the backend keeps in 64 / 128-bit register
    # tuples -- the shape on which this LLVM's register coalescer miscompiled the all-assembly diagnostic build (profiles/
    # r04_asm_everywhere_rootcause.txt; gate: tools/check_machine_verifier.py).  Without it: same registers, 1 - 2 % shorter single-MSM
    # latency, throughput unchanged (profiles/r04_ab_noslp.txt).  MSM_HIP_SLP=1 restores the compiler's default.
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC"]
    if os.environ.get("MSM_HIP_SLP") != "1":
        flags.append("-fno-slp-vectorize")
    if os.environ.get("MSM_HIP_NO_ASM") == "1":  # the C++ multipliers everywhere
        flags.append("-DFQ29_NO_ASM")
    if os.environ.get("MSM_HIP_ASM_SMVP_ONLY") == "1":  # rounds 1 - 3: the inline-assembly multipliers only in the SMVP's mixed addition, C++ elsewhere
        flags.append("-DFQ29_ASM_SMVP_ONLY")
    return flags + os.environ.get("MSM_HIP_EXTRA_FLAGS", "").split()


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950: every translation unit of csrc/ to an object (in parallel), then -shared -> msm-webgpu_amd/libmsm_hip.so and,
    from the scalar-field units, every library of FR_LIBRARIES (msm-webgpu_amd/libmsm_fr.so ... msm-webgpu_amd/libmsm_frhash.so) and of
    AUX_LIBRARIES and MEM_LIBRARIES (msm-webgpu_amd/libmsm_frcol.so, msm-webgpu_amd/libmsm_frmem.so).  Each library is rebuilt only when its own sources or the flags changed."""
    do_hip = force or needs_build()
    todo = [lib for lib in library_rows() if (force and not os.environ.get("MSM_HIP_SO")) or needs_build(lib)]
    if not do_hip and not todo:
        return SO
    if variant_flags() and not os.environ.get("MSM_HIP_SO"):
        # the product library is only ever built with the gated flags: a variant build must name its own file
        raise RuntimeError("variant build flags (%s) need MSM_HIP_SO=<another file>: libmsm_hip.so is the product" % ", ".join(variant_flags()))
    from concurrent.futures import ThreadPoolExecutor

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the compiler's intermediate files are kept (build/temps/, git-ignored): the device assembly among them is what the code-generation
    # gate reads (tools/check_long_branch_hazard.py, tests/test_codegen_hazards.py) instead of compiling everything a second time
    os.makedirs(TEMPS, exist_ok=True)
    flags = compile_flags()

    def compile_unit(name):
        obj = os.path.join(TEMPS, os.path.splitext(name)[0] + ".o")
        cmd = [hipcc] + flags + ["-save-temps=cwd", "-c", os.path.join(CSRC, name), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, cwd=TEMPS)
        return obj

    def link(objs, so):
        cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "--hip-link"] + objs + ["-o", so + ".tmp"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, cwd=TEMPS)
        os.replace(so + ".tmp", so)

    # one pool for the units of all the libraries (the long curve units first), never more than 16 compilers at once
    units = (TRANSLATION_UNITS if do_hip else []) + [u for lib in todo for u in lib.units]
    with ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 1, 16)) as pool:
        objs = dict(zip(units, pool.map(compile_unit, units)))
    if do_hip:
        link([objs[u] for u in TRANSLATION_UNITS], SO)
        with open(stamp_path(), "w") as f:
            f.write(build_stamp() + "\n")
    for lib in todo:
        link([objs[u] for u in lib.units], lib.so)
        with open(lib.so + ".stamp", "w") as f:
            f.write(build_stamp(lib) + "\n")
    return SO


if __name__ == "__main__":
    print(build(force=True, verbose=True))
