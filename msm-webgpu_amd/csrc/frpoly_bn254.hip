// The scalar field of BN254 as a translation unit of libmsm_frpoly.so: fq29.h over the field's constants and the opening kernels (csrc/frpoly_unit.h,
// csrc/frpoly_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frp_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FRPOLY_HOST_UNIT 1  // this unit also carries the library's host code
#include "frpoly_unit.h"

extern "C" const FrpolyOps* msm_frpoly_ops_bn254(void) {
  static const FrpolyOps ops = {frp_bn254::FQ_P32, frp_bn254::frpoly_launch_fold, frp_bn254::frpoly_launch_suffix, frp_bn254::frpoly_launch_combine, frp_bn254::frpoly_launch_powers};
  return &ops;
}
