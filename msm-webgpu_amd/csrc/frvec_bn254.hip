// The scalar field of BN254 as a translation unit of libmsm_frvec.so: fq29.h over the field's constants and the vector kernels (csrc/frvec_unit.h,
// csrc/frvec_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frv_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FRVEC_HOST_UNIT 1  // this unit also carries the library's host code
#include "frvec_unit.h"

extern "C" const FrvecOps* msm_frvec_ops_bn254(void) {
  static const FrvecOps ops = {frv_bn254::FQ_P32, frv_bn254::frvec_launch_map, frv_bn254::frvec_launch_inverse, frv_bn254::frvec_launch_fold, frv_bn254::frvec_launch_scan};
  return &ops;
}
