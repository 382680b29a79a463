// The scalar field of BN254 as a translation unit of libmsm_frlook.so: the field's r and the lookup kernels (csrc/frlook_unit.h,
// csrc/frlook_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frl_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FRLOOK_HOST_UNIT 1  // this unit also carries the library's host code
#include "frlook_unit.h"

extern "C" const FrlookOps* msm_frlook_ops_bn254(void) {
  static const FrlookOps ops = {frl_bn254::FQ_P32, frl_bn254::frlook_launch_build, frl_bn254::frlook_launch_count, frl_bn254::frlook_launch_finish};
  return &ops;
}
