// The scalar field of BLS12-381 as a translation unit of libmsm_frlook.so: the field's r and the lookup kernels (csrc/frlook_unit.h,
// csrc/frlook_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frl_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "frlook_unit.h"

extern "C" const FrlookOps* msm_frlook_ops_bls12_381(void) {
  static const FrlookOps ops = {frl_bls12_381::FQ_P32, frl_bls12_381::frlook_launch_build, frl_bls12_381::frlook_launch_count, frl_bls12_381::frlook_launch_finish};
  return &ops;
}
