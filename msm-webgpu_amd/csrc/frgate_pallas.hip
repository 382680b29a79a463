// The scalar field of Pallas as a translation unit of libmsm_frgate.so: fq29.h over the field's constants and the constraint-evaluation kernel
// (csrc/frgate_unit.h, csrc/frgate_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frg_pallas
#define MSM_CURVE_CONSTANTS "fr_pallas_constants.h"
#include "frgate_unit.h"

extern "C" const FrgateOps* msm_frgate_ops_pallas(void) {
  static const FrgateOps ops = {frg_pallas::FQ_P32, frg_pallas::frgate_launch_apply};
  return &ops;
}
