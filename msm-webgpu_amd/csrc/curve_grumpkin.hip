// Grumpkin as its own translation unit of libmsm_hip.so: the arithmetic headers and the kernels instantiated with this curve's constants
// (csrc/curve_unit.h, csrc/curve_select.h) and the table through which msm_hip.hip reaches them (csrc/curve_ops.h; filled by msm_kernels.h, curve_ops_table).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/msm_hip.h"
#define MSM_FIELD_NS grumpkin
#define MSM_KERNEL_NS msmk_grumpkin
#define MSM_CURVE_CONSTANTS "grumpkin_constants.h"
#include "curve_unit.h"

extern "C" const CurveOps* msm_hip_curve_ops_grumpkin(void) {
  static const CurveOps ops = msmk_grumpkin::curve_ops_table();
  return &ops;
}
