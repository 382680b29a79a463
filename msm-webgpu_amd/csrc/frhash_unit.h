// One scalar field's worth of libmsm_frhash.so: define MSM_FIELD_NS and MSM_CURVE_CONSTANTS (a field-only constants header, tools/gen_constants.py
// fr <name>) and include this file.  A translation unit holds one field (frhash_<name>.hip); the unit that defines MSM_FRHASH_HOST_UNIT also holds
// the library's host code (csrc/frhash_host.h).
#include <hip/hip_runtime.h>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frhash_kernels.h"
#undef MSM_CURVE_UNIT
#ifdef MSM_FRHASH_HOST_UNIT
#include "frhash_host.h"
#endif
