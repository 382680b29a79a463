// The scalar field of BN254 as a translation unit of libmsm_frhash.so: fq29.h over the field's constants and the Poseidon kernels
// (csrc/frhash_unit.h, csrc/frhash_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frh_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FRHASH_HOST_UNIT 1  // this unit also carries the library's host code
#include "frhash_unit.h"

extern "C" const FrhashOps* msm_frhash_ops_bn254(void) {
  static const FrhashOps ops = {frh_bn254::FQ_P32, frh_bn254::frhash_launch_permute, frh_bn254::frhash_launch_hash};
  return &ops;
}
