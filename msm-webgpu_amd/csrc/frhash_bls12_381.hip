// The scalar field of BLS12-381 as a translation unit of libmsm_frhash.so: fq29.h over the field's constants and the Poseidon kernels
// (csrc/frhash_unit.h, csrc/frhash_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frh_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "frhash_unit.h"

extern "C" const FrhashOps* msm_frhash_ops_bls12_381(void) {
  static const FrhashOps ops = {frh_bls12_381::FQ_P32, frh_bls12_381::frhash_launch_permute, frh_bls12_381::frhash_launch_hash};
  return &ops;
}
