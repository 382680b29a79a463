// One scalar field's worth of libmsm_frlook.so: define MSM_FIELD_NS and MSM_CURVE_CONSTANTS (a field-only constants header, tools/gen_constants.py
// fr <name>) and include this file.  A translation unit holds one field (frlook_<name>.hip); the unit that defines MSM_FRLOOK_HOST_UNIT also holds
// the library's host code (csrc/frlook_host.h).  Of the constants only r (FQ_P32) is used: keys are matched, not computed with.
#include <hip/hip_runtime.h>

#include MSM_CURVE_CONSTANTS
#include "frlook_kernels.h"
#ifdef MSM_FRLOOK_HOST_UNIT
#include "frlook_host.h"
#endif
