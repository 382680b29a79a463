// libmsm_frmem.so (include/msm_frmem.h), whole: the kernels of csrc/frmem_kernels.h and the host code of csrc/frmem_host.h.  One translation unit:
// integer keys, so no field's constants or arithmetic are included.
#include <hip/hip_runtime.h>

#include "frmem_host.h"
