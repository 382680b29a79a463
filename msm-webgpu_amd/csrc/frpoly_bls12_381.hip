// The scalar field of BLS12-381 as a translation unit of libmsm_frpoly.so: fq29.h over the field's constants and the opening kernels (csrc/frpoly_unit.h,
// csrc/frpoly_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frp_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "frpoly_unit.h"

extern "C" const FrpolyOps* msm_frpoly_ops_bls12_381(void) {
  static const FrpolyOps ops = {frp_bls12_381::FQ_P32, frp_bls12_381::frpoly_launch_fold, frp_bls12_381::frpoly_launch_suffix, frp_bls12_381::frpoly_launch_combine, frp_bls12_381::frpoly_launch_powers};
  return &ops;
}
