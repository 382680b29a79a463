// The scalar field of Vesta as a translation unit of libmsm_frhash.so: fq29.h over the field's constants and the Poseidon kernels
// (csrc/frhash_unit.h, csrc/frhash_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frh_vesta
#define MSM_CURVE_CONSTANTS "fr_vesta_constants.h"
#include "frhash_unit.h"

extern "C" const FrhashOps* msm_frhash_ops_vesta(void) {
  static const FrhashOps ops = {frh_vesta::FQ_P32, frh_vesta::frhash_launch_permute, frh_vesta::frhash_launch_hash};
  return &ops;
}
