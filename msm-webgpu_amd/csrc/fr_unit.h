// One scalar field's worth of the NTT (libmsm_fr.so): define MSM_FIELD_NS and MSM_CURVE_CONSTANTS (a field-only constants header, tools/
// gen_constants.py fr <name>) and include this file.  A translation unit holds one field (fr_<name>.hip); the unit that defines MSM_FR_HOST_UNIT
// also holds the library's host code (csrc/ntt_host.h).
#include <hip/hip_runtime.h>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "ntt_kernels.h"
#undef MSM_CURVE_UNIT
#ifdef MSM_FR_HOST_UNIT
#include "ntt_host.h"
#endif
