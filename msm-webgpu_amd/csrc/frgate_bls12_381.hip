// The scalar field of BLS12-381 as a translation unit of libmsm_frgate.so: fq29.h over the field's constants and the constraint-evaluation kernel
// (csrc/frgate_unit.h, csrc/frgate_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frg_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "frgate_unit.h"

extern "C" const FrgateOps* msm_frgate_ops_bls12_381(void) {
  static const FrgateOps ops = {frg_bls12_381::FQ_P32, frg_bls12_381::frgate_launch_apply};
  return &ops;
}
