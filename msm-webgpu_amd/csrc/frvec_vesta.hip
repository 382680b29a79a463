// The scalar field of Vesta as a translation unit of libmsm_frvec.so: fq29.h over the field's constants and the vector kernels (csrc/frvec_unit.h,
// csrc/frvec_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frv_vesta
#define MSM_CURVE_CONSTANTS "fr_vesta_constants.h"
#include "frvec_unit.h"

extern "C" const FrvecOps* msm_frvec_ops_vesta(void) {
  static const FrvecOps ops = {frv_vesta::FQ_P32, frv_vesta::frvec_launch_map, frv_vesta::frvec_launch_inverse, frv_vesta::frvec_launch_fold, frv_vesta::frvec_launch_scan};
  return &ops;
}
