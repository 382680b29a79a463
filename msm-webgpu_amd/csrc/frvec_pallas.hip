// The scalar field of Pallas as a translation unit of libmsm_frvec.so: fq29.h over the field's constants and the vector kernels (csrc/frvec_unit.h,
// csrc/frvec_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frv_pallas
#define MSM_CURVE_CONSTANTS "fr_pallas_constants.h"
#include "frvec_unit.h"

extern "C" const FrvecOps* msm_frvec_ops_pallas(void) {
  static const FrvecOps ops = {frv_pallas::FQ_P32, frv_pallas::frvec_launch_map, frv_pallas::frvec_launch_inverse, frv_pallas::frvec_launch_fold, frv_pallas::frvec_launch_scan};
  return &ops;
}
