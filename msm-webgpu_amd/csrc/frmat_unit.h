// One scalar field's worth of libmsm_frmat.so: define MSM_FIELD_NS and MSM_CURVE_CONSTANTS (a field-only constants header, tools/gen_constants.py
// fr <name>) and include this file.  A translation unit holds one field (frmat_<name>.hip); the unit that defines MSM_FRMAT_HOST_UNIT also holds
// the library's host code (csrc/frmat_host.h).
#include <hip/hip_runtime.h>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frmat_kernels.h"
#undef MSM_CURVE_UNIT
#ifdef MSM_FRMAT_HOST_UNIT
#include "frmat_host.h"
#endif
