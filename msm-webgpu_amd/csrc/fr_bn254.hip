// The scalar field of BN254 as a translation unit of libmsm_fr.so: fq29.h over the field's constants and the NTT kernels (csrc/fr_unit.h,
// csrc/ntt_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS fr_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FR_HOST_UNIT 1  // this unit also carries the library's host code
#include "fr_unit.h"

extern "C" const FrOps* msm_fr_ops_bn254(void) {
  static const FrOps ops = {fr_bn254::FQ_P32, fr_bn254::FR_TWO_ADICITY, fr_bn254::ntt_launch_pass};
  return &ops;
}
