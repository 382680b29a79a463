// The scalar field of Vesta as a translation unit of libmsm_frgate.so: fq29.h over the field's constants and the constraint-evaluation kernel
// (csrc/frgate_unit.h, csrc/frgate_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frg_vesta
#define MSM_CURVE_CONSTANTS "fr_vesta_constants.h"
#include "frgate_unit.h"

extern "C" const FrgateOps* msm_frgate_ops_vesta(void) {
  static const FrgateOps ops = {frg_vesta::FQ_P32, frg_vesta::frgate_launch_apply};
  return &ops;
}
