// The scalar field of Pallas as a translation unit of libmsm_frpoly.so: fq29.h over the field's constants and the opening kernels (csrc/frpoly_unit.h,
// csrc/frpoly_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frp_pallas
#define MSM_CURVE_CONSTANTS "fr_pallas_constants.h"
#include "frpoly_unit.h"

extern "C" const FrpolyOps* msm_frpoly_ops_pallas(void) {
  static const FrpolyOps ops = {frp_pallas::FQ_P32, frp_pallas::frpoly_launch_fold, frp_pallas::frpoly_launch_suffix, frp_pallas::frpoly_launch_combine, frp_pallas::frpoly_launch_powers};
  return &ops;
}
