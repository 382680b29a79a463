// The scalar field of BLS12-381 as a translation unit of libmsm_frvec.so: fq29.h over the field's constants and the vector kernels (csrc/frvec_unit.h,
// csrc/frvec_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frv_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "frvec_unit.h"

extern "C" const FrvecOps* msm_frvec_ops_bls12_381(void) {
  static const FrvecOps ops = {frv_bls12_381::FQ_P32, frv_bls12_381::frvec_launch_map, frv_bls12_381::frvec_launch_inverse, frv_bls12_381::frvec_launch_fold, frv_bls12_381::frvec_launch_scan};
  return &ops;
}
