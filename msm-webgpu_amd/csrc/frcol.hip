// libmsm_frcol.so (include/msm_frcol.h), whole: the kernels of csrc/frcol_kernels.h and the host code of csrc/frcol_host.h.  One translation unit for
// all curves -- scalars are moved as stored, so no field's constants are included.
#include <hip/hip_runtime.h>

#include "frcol_host.h"
