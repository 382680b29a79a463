// The scalar field of BLS12-381 as a translation unit of libmsm_fr.so: fq29.h over the field's constants and the NTT kernels (csrc/fr_unit.h,
// csrc/ntt_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS fr_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "fr_unit.h"

extern "C" const FrOps* msm_fr_ops_bls12_381(void) {
  static const FrOps ops = {fr_bls12_381::FQ_P32, fr_bls12_381::FR_TWO_ADICITY, fr_bls12_381::ntt_launch_pass};
  return &ops;
}
