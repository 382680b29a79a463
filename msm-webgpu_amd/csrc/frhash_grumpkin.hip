// The scalar field of Grumpkin as a translation unit of libmsm_frhash.so: fq29.h over the field's constants and the Poseidon kernels
// (csrc/frhash_unit.h, csrc/frhash_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frh_grumpkin
#define MSM_CURVE_CONSTANTS "fr_grumpkin_constants.h"
#include "frhash_unit.h"

extern "C" const FrhashOps* msm_frhash_ops_grumpkin(void) {
  static const FrhashOps ops = {frh_grumpkin::FQ_P32, frh_grumpkin::frhash_launch_permute, frh_grumpkin::frhash_launch_hash};
  return &ops;
}
