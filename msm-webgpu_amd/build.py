"""Build libmsm_hip.so, libmsm_fr.so, libmsm_frvec.so, libmsm_frpoly.so, libmsm_frmle.so, libmsm_frmat.so, libmsm_frgate.so, libmsm_frlook.so and libmsm_frhash.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# MSM_HIP_SO: load (and build into) another file, e.g. a diagnostic variant next to the product library
SO = os.environ.get("MSM_HIP_SO") or os.path.join(HERE, "libmsm_hip.so")
SOURCES = ["msm_hip.hip", "curve_bn254.hip", "curve_grumpkin.hip", "curve_pallas.hip", "curve_vesta.hip", "curve_bls12_381.hip", "curve_bn254_g2.hip", "curve_bls12_381_g2.hip", "fq2.h", "bn254_g2_constants.h", "bls12_381_g2_constants.h", "fq28x14_asm.h", "bls12_381_constants.h", "curve_ops.h", "msm_layout.h", "recode.h", "sort_kernels.h", "msm_kernels.h", "g1.h", "fq29.h", "fq29_asm.h", "host_g1.h", "host_fr.h", "host_pool.h", "host_worker.h", "glv.h", "scalar_mul.h", "msm_mgpu.h", "curve_select.h", "curve_unit.h", "grumpkin_constants.h", "bn254_constants.h", "pallas_constants.h", "vesta_constants.h"]
HEADER = os.path.join(HERE, "..", "include", "msm_hip.h")
# libmsm_fr.so (include/msm_fr.h): the scalar-field NTT, a library of its own -- one translation unit per field, its own sources and stamp.  None
# of it is part of libmsm_hip.so (TRANSLATION_UNITS, SOURCES and device_asm_files() below are that library's alone).
FR_SO = os.path.join(HERE, "libmsm_fr.so")
FR_UNITS = ["fr_bn254.hip", "fr_pallas.hip", "fr_vesta.hip", "fr_bls12_381.hip"]
FR_SOURCES = FR_UNITS + ["fr_unit.h", "ntt_kernels.h", "ntt_host.h", "ntt_plan.h", "host_fr.h", "fq29.h", "fq29_asm.h", "fr_bn254_constants.h", "fr_pallas_constants.h",
                         "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FR_HEADERS = [os.path.join(HERE, "..", "include", "msm_fr.h"), HEADER]
# libmsm_frvec.so (include/msm_frvec.h): vector arithmetic over the scalar field -- map, batch inverse, scan --, the third library, built the same way
FRVEC_SO = os.path.join(HERE, "libmsm_frvec.so")
FRVEC_UNITS = ["frvec_bn254.hip", "frvec_pallas.hip", "frvec_vesta.hip", "frvec_bls12_381.hip"]
FRVEC_SOURCES = FRVEC_UNITS + ["frvec_unit.h", "frvec_kernels.h", "frvec_host.h", "frvec_plan.h", "host_fr.h", "fq29.h", "fq29_asm.h", "fr_bn254_constants.h",
                               "fr_pallas_constants.h", "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FRVEC_HEADERS = [os.path.join(HERE, "..", "include", "msm_frvec.h"), HEADER]
# libmsm_frpoly.so (include/msm_frpoly.h): polynomial opening over the scalar field -- eval, divide, dot, combine, powers --, the fourth library
FRPOLY_SO = os.path.join(HERE, "libmsm_frpoly.so")
FRPOLY_UNITS = ["frpoly_bn254.hip", "frpoly_pallas.hip", "frpoly_vesta.hip", "frpoly_bls12_381.hip"]
FRPOLY_SOURCES = FRPOLY_UNITS + ["frpoly_unit.h", "frpoly_kernels.h", "frpoly_host.h", "frpoly_plan.h", "host_fr.h", "fq29.h", "fq29_asm.h", "fr_bn254_constants.h",
                                 "fr_pallas_constants.h", "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FRPOLY_HEADERS = [os.path.join(HERE, "..", "include", "msm_frpoly.h"), HEADER]
# libmsm_frmle.so (include/msm_frmle.h): the sumcheck over multilinear tables -- fold, eval, eq, round --, the fifth library; the only one with a
# unit for Grumpkin's scalar field (no transform needs it here)
FRMLE_SO = os.path.join(HERE, "libmsm_frmle.so")
FRMLE_UNITS = ["frmle_bn254.hip", "frmle_grumpkin.hip", "frmle_pallas.hip", "frmle_vesta.hip", "frmle_bls12_381.hip"]
FRMLE_SOURCES = FRMLE_UNITS + ["frmle_unit.h", "frmle_kernels.h", "frmle_host.h", "frmle_plan.h", "host_fr.h", "fq29.h", "fq29_asm.h", "fr_bn254_constants.h",
                               "fr_grumpkin_constants.h", "fr_pallas_constants.h", "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FRMLE_HEADERS = [os.path.join(HERE, "..", "include", "msm_frmle.h"), HEADER]
# libmsm_frmat.so (include/msm_frmat.h): sparse matrix-vector products over the scalar field -- the rows Az, Bz, Cz of an R1CS --, the sixth library;
# like the fifth it has a unit for Grumpkin's scalar field
FRMAT_SO = os.path.join(HERE, "libmsm_frmat.so")
FRMAT_UNITS = ["frmat_bn254.hip", "frmat_grumpkin.hip", "frmat_pallas.hip", "frmat_vesta.hip", "frmat_bls12_381.hip"]
FRMAT_SOURCES = FRMAT_UNITS + ["frmat_unit.h", "frmat_kernels.h", "frmat_host.h", "frmat_plan.h", "host_fr.h", "fq29.h", "fq29_asm.h", "fr_bn254_constants.h",
                               "fr_grumpkin_constants.h", "fr_pallas_constants.h", "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FRMAT_HEADERS = [os.path.join(HERE, "..", "include", "msm_frmat.h"), HEADER]
# libmsm_frgate.so (include/msm_frgate.h): constraint evaluation over the scalar field -- sums of products of rotated rows, the numerator of a
# PLONK quotient --, the seventh library; like the fifth and sixth it has a unit for Grumpkin's scalar field
FRGATE_SO = os.path.join(HERE, "libmsm_frgate.so")
FRGATE_UNITS = ["frgate_bn254.hip", "frgate_grumpkin.hip", "frgate_pallas.hip", "frgate_vesta.hip", "frgate_bls12_381.hip"]
FRGATE_SOURCES = FRGATE_UNITS + ["frgate_unit.h", "frgate_kernels.h", "frgate_host.h", "frgate_plan.h", "host_fr.h", "fq29.h", "fq29_asm.h", "fr_bn254_constants.h",
                                 "fr_grumpkin_constants.h", "fr_pallas_constants.h", "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FRGATE_HEADERS = [os.path.join(HERE, "..", "include", "msm_frgate.h"), HEADER]
# libmsm_frlook.so (include/msm_frlook.h): lookup arguments over the scalar field -- the multiplicity column and the table indices of a logUp --,
# the eighth library; it matches keys and computes nothing, so of the field's files it needs the constants alone (no fq29.h)
FRLOOK_SO = os.path.join(HERE, "libmsm_frlook.so")
FRLOOK_UNITS = ["frlook_bn254.hip", "frlook_grumpkin.hip", "frlook_pallas.hip", "frlook_vesta.hip", "frlook_bls12_381.hip"]
FRLOOK_SOURCES = FRLOOK_UNITS + ["frlook_unit.h", "frlook_kernels.h", "frlook_host.h", "frlook_plan.h", "host_fr.h", "fr_bn254_constants.h",
                                 "fr_grumpkin_constants.h", "fr_pallas_constants.h", "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FRLOOK_HEADERS = [os.path.join(HERE, "..", "include", "msm_frlook.h"), HEADER]
# libmsm_frhash.so (include/msm_frhash.h): Poseidon over the scalar field -- batch permutations, sponges and Merkle trees --, the ninth library;
# a unit for every scalar field, Grumpkin's included
FRHASH_SO = os.path.join(HERE, "libmsm_frhash.so")
FRHASH_UNITS = ["frhash_bn254.hip", "frhash_grumpkin.hip", "frhash_pallas.hip", "frhash_vesta.hip", "frhash_bls12_381.hip"]
FRHASH_SOURCES = FRHASH_UNITS + ["frhash_unit.h", "frhash_kernels.h", "frhash_host.h", "frhash_plan.h", "host_fr.h", "fq29.h", "fq29_asm.h", "fr_bn254_constants.h",
                                 "fr_grumpkin_constants.h", "fr_pallas_constants.h", "fr_vesta_constants.h", "fr_bls12_381_constants.h"]
FRHASH_HEADERS = [os.path.join(HERE, "..", "include", "msm_frhash.h"), HEADER]
TEMPS = os.path.join(HERE, "..", "build", "temps" if not os.environ.get("MSM_HIP_SO") else "temps_" + os.path.basename(SO))


def device_asm_files():
    """The device assembly of every translation unit, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in TRANSLATION_UNITS]


def device_asm_is_current():
    """True if build() left the device assembly of the CURRENT sources behind (same staleness rule as the library itself)."""
    if needs_build() or not all(os.path.exists(f) for f in device_asm_files()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in device_asm_files())


def fr_device_asm_files():
    """The device assembly of libmsm_fr.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FR_UNITS]


def fr_build_stamp():
    """build_stamp() for libmsm_fr.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FR_SOURCES)] + FR_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def fr_needs_build():
    """libmsm_fr.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FR_SO + ".stamp") as f:
            return not os.path.exists(FR_SO) or f.read().strip() != fr_build_stamp()
    except OSError:
        return True


def fr_device_asm_is_current():
    """device_asm_is_current() for libmsm_fr.so's units"""
    if fr_needs_build() or not all(os.path.exists(f) for f in fr_device_asm_files()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FR_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in fr_device_asm_files())


def frvec_device_asm_files():
    """The device assembly of libmsm_frvec.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FRVEC_UNITS]


def frvec_build_stamp():
    """build_stamp() for libmsm_frvec.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FRVEC_SOURCES)] + FRVEC_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def frvec_needs_build():
    """libmsm_frvec.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FRVEC_SO + ".stamp") as f:
            return not os.path.exists(FRVEC_SO) or f.read().strip() != frvec_build_stamp()
    except OSError:
        return True


def frvec_device_asm_is_current():
    """device_asm_is_current() for libmsm_frvec.so's units"""
    if frvec_needs_build() or not all(os.path.exists(f) for f in frvec_device_asm_files()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FRVEC_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in frvec_device_asm_files())


def frpoly_device_asm_paths():
    """The device assembly of libmsm_frpoly.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FRPOLY_UNITS]


def frpoly_build_stamp():
    """build_stamp() for libmsm_frpoly.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FRPOLY_SOURCES)] + FRPOLY_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def frpoly_needs_build():
    """libmsm_frpoly.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FRPOLY_SO + ".stamp") as f:
            return not os.path.exists(FRPOLY_SO) or f.read().strip() != frpoly_build_stamp()
    except OSError:
        return True


def frpoly_device_asm_is_current():
    """device_asm_is_current() for libmsm_frpoly.so's units"""
    if frpoly_needs_build() or not all(os.path.exists(f) for f in frpoly_device_asm_paths()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FRPOLY_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in frpoly_device_asm_paths())


def frmle_device_asm_paths():
    """The device assembly of libmsm_frmle.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FRMLE_UNITS]


def frmle_build_stamp():
    """build_stamp() for libmsm_frmle.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FRMLE_SOURCES)] + FRMLE_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def frmle_needs_build():
    """libmsm_frmle.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FRMLE_SO + ".stamp") as f:
            return not os.path.exists(FRMLE_SO) or f.read().strip() != frmle_build_stamp()
    except OSError:
        return True


def frmle_device_asm_is_current():
    """device_asm_is_current() for libmsm_frmle.so's units"""
    if frmle_needs_build() or not all(os.path.exists(f) for f in frmle_device_asm_paths()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FRMLE_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in frmle_device_asm_paths())


def frmat_device_asm_paths():
    """The device assembly of libmsm_frmat.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FRMAT_UNITS]


def frmat_build_stamp():
    """build_stamp() for libmsm_frmat.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FRMAT_SOURCES)] + FRMAT_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def frmat_needs_build():
    """libmsm_frmat.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FRMAT_SO + ".stamp") as f:
            return not os.path.exists(FRMAT_SO) or f.read().strip() != frmat_build_stamp()
    except OSError:
        return True


def frmat_device_asm_is_current():
    """device_asm_is_current() for libmsm_frmat.so's units"""
    if frmat_needs_build() or not all(os.path.exists(f) for f in frmat_device_asm_paths()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FRMAT_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in frmat_device_asm_paths())


def frgate_device_asm_paths():
    """The device assembly of libmsm_frgate.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FRGATE_UNITS]


def frgate_build_stamp():
    """build_stamp() for libmsm_frgate.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FRGATE_SOURCES)] + FRGATE_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def frgate_needs_build():
    """libmsm_frgate.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FRGATE_SO + ".stamp") as f:
            return not os.path.exists(FRGATE_SO) or f.read().strip() != frgate_build_stamp()
    except OSError:
        return True


def frgate_device_asm_is_current():
    """device_asm_is_current() for libmsm_frgate.so's units"""
    if frgate_needs_build() or not all(os.path.exists(f) for f in frgate_device_asm_paths()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FRGATE_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in frgate_device_asm_paths())


def frlook_device_asm_paths():
    """The device assembly of libmsm_frlook.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FRLOOK_UNITS]


def frlook_build_stamp():
    """build_stamp() for libmsm_frlook.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FRLOOK_SOURCES)] + FRLOOK_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def frlook_needs_build():
    """libmsm_frlook.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FRLOOK_SO + ".stamp") as f:
            return not os.path.exists(FRLOOK_SO) or f.read().strip() != frlook_build_stamp()
    except OSError:
        return True


def frlook_device_asm_is_current():
    """device_asm_is_current() for libmsm_frlook.so's units"""
    if frlook_needs_build() or not all(os.path.exists(f) for f in frlook_device_asm_paths()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FRLOOK_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in frlook_device_asm_paths())


def frhash_device_asm_paths():
    """The device assembly of libmsm_frhash.so's units, as build() leaves it behind."""
    return [os.path.join(TEMPS, os.path.splitext(u)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s") for u in FRHASH_UNITS]


def frhash_build_stamp():
    """build_stamp() for libmsm_frhash.so: the compile flags and the contents of its own sources"""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for path in [os.path.join(CSRC, f) for f in sorted(FRHASH_SOURCES)] + FRHASH_HEADERS:
        if os.path.exists(path):
            h.update(b"\0" + os.path.basename(path).encode() + b"\0")
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def frhash_needs_build():
    """libmsm_frhash.so is missing, or was built from other sources or flags (a diagnostic MSM_HIP_SO build leaves it alone)"""
    if os.environ.get("MSM_HIP_SO"):
        return False
    try:
        with open(FRHASH_SO + ".stamp") as f:
            return not os.path.exists(FRHASH_SO) or f.read().strip() != frhash_build_stamp()
    except OSError:
        return True


def frhash_device_asm_is_current():
    """device_asm_is_current() for libmsm_frhash.so's units"""
    if frhash_needs_build() or not all(os.path.exists(f) for f in frhash_device_asm_paths()):
        return False
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in FRHASH_SOURCES if os.path.exists(os.path.join(CSRC, f)))
    return all(os.path.getmtime(f) >= newest for f in frhash_device_asm_paths())


def build_stamp():
    """what the library on disk must have been built FROM to be the product: a hash over the compile flags (the environment switches of the
    diagnostic builds included -- MSM_HIP_SLP, MSM_HIP_NO_ASM, MSM_HIP_EXTRA_FLAGS ...) and the contents of every source.  Written next to the
    library by build(); a library whose stamp differs (built once with variant flags, or from other sources) is rebuilt instead of being
    silently reused, and the code-generation gates (tools/check_machine_verifier.py, tools/check_long_branch_hazard.py) check the stamp of the
    library they vouch for."""
    import hashlib

    h = hashlib.sha256()
    h.update("\0".join(compile_flags()).encode())
    for f in sorted(SOURCES) + [HEADER]:
        path = f if os.path.isabs(f) else os.path.join(CSRC, f)
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


def needs_build():
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
    from the scalar-field units, msm-webgpu_amd/libmsm_fr.so, msm-webgpu_amd/libmsm_frvec.so, msm-webgpu_amd/libmsm_frpoly.so,
    msm-webgpu_amd/libmsm_frmle.so, msm-webgpu_amd/libmsm_frmat.so, msm-webgpu_amd/libmsm_frgate.so, msm-webgpu_amd/libmsm_frlook.so and msm-webgpu_amd/libmsm_frhash.so.  Each library is rebuilt only when its own sources or the flags changed."""
    do_hip, do_fr = force or needs_build(), (force and not os.environ.get("MSM_HIP_SO")) or fr_needs_build()
    do_frvec = (force and not os.environ.get("MSM_HIP_SO")) or frvec_needs_build()
    do_frpoly = (force and not os.environ.get("MSM_HIP_SO")) or frpoly_needs_build()
    do_frmle = (force and not os.environ.get("MSM_HIP_SO")) or frmle_needs_build()
    do_frmat = (force and not os.environ.get("MSM_HIP_SO")) or frmat_needs_build()
    do_frgate = (force and not os.environ.get("MSM_HIP_SO")) or frgate_needs_build()
    do_frlook = (force and not os.environ.get("MSM_HIP_SO")) or frlook_needs_build()
    do_frhash = (force and not os.environ.get("MSM_HIP_SO")) or frhash_needs_build()
    if not do_hip and not do_fr and not do_frvec and not do_frpoly and not do_frmle and not do_frmat and not do_frgate and not do_frlook and not do_frhash:
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

    # one pool for the units of all nine libraries (the long curve units first), never more than 16 compilers at once
    units = (TRANSLATION_UNITS if do_hip else []) + (FR_UNITS if do_fr else []) + (FRVEC_UNITS if do_frvec else []) + (FRPOLY_UNITS if do_frpoly else []) + (FRMLE_UNITS if do_frmle else []) + (FRMAT_UNITS if do_frmat else []) + (FRGATE_UNITS if do_frgate else []) + (FRLOOK_UNITS if do_frlook else []) + (FRHASH_UNITS if do_frhash else [])
    with ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 1, 16)) as pool:
        objs = dict(zip(units, pool.map(compile_unit, units)))
    if do_hip:
        link([objs[u] for u in TRANSLATION_UNITS], SO)
        with open(stamp_path(), "w") as f:
            f.write(build_stamp() + "\n")
    if do_fr:
        link([objs[u] for u in FR_UNITS], FR_SO)
        with open(FR_SO + ".stamp", "w") as f:
            f.write(fr_build_stamp() + "\n")
    if do_frvec:
        link([objs[u] for u in FRVEC_UNITS], FRVEC_SO)
        with open(FRVEC_SO + ".stamp", "w") as f:
            f.write(frvec_build_stamp() + "\n")
    if do_frpoly:
        link([objs[u] for u in FRPOLY_UNITS], FRPOLY_SO)
        with open(FRPOLY_SO + ".stamp", "w") as f:
            f.write(frpoly_build_stamp() + "\n")
    if do_frmle:
        link([objs[u] for u in FRMLE_UNITS], FRMLE_SO)
        with open(FRMLE_SO + ".stamp", "w") as f:
            f.write(frmle_build_stamp() + "\n")
    if do_frmat:
        link([objs[u] for u in FRMAT_UNITS], FRMAT_SO)
        with open(FRMAT_SO + ".stamp", "w") as f:
            f.write(frmat_build_stamp() + "\n")
    if do_frgate:
        link([objs[u] for u in FRGATE_UNITS], FRGATE_SO)
        with open(FRGATE_SO + ".stamp", "w") as f:
            f.write(frgate_build_stamp() + "\n")
    if do_frlook:
        link([objs[u] for u in FRLOOK_UNITS], FRLOOK_SO)
        with open(FRLOOK_SO + ".stamp", "w") as f:
            f.write(frlook_build_stamp() + "\n")
    if do_frhash:
        link([objs[u] for u in FRHASH_UNITS], FRHASH_SO)
        with open(FRHASH_SO + ".stamp", "w") as f:
            f.write(frhash_build_stamp() + "\n")
    return SO


if __name__ == "__main__":
    print(build(force=True, verbose=True))
