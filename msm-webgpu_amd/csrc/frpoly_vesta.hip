// The scalar field of Vesta as a translation unit of libmsm_frpoly.so: fq29.h over the field's constants and the opening kernels (csrc/frpoly_unit.h,
// csrc/frpoly_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frp_vesta
#define MSM_CURVE_CONSTANTS "fr_vesta_constants.h"
#include "frpoly_unit.h"

extern "C" const FrpolyOps* msm_frpoly_ops_vesta(void) {
  static const FrpolyOps ops = {frp_vesta::FQ_P32, frp_vesta::frpoly_launch_fold, frp_vesta::frpoly_launch_suffix, frp_vesta::frpoly_launch_combine, frp_vesta::frpoly_launch_powers};
  return &ops;
}
