// The scalar field of Grumpkin as a translation unit of libmsm_frgate.so: fq29.h over the field's constants and the constraint-evaluation kernel
// (csrc/frgate_unit.h, csrc/frgate_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frg_grumpkin
#define MSM_CURVE_CONSTANTS "fr_grumpkin_constants.h"
#include "frgate_unit.h"

extern "C" const FrgateOps* msm_frgate_ops_grumpkin(void) {
  static const FrgateOps ops = {frg_grumpkin::FQ_P32, frg_grumpkin::frgate_launch_apply};
  return &ops;
}
