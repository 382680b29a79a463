// The scalar field of Grumpkin as a translation unit of libmsm_frlook.so: the field's r and the lookup kernels (csrc/frlook_unit.h,
// csrc/frlook_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frl_grumpkin
#define MSM_CURVE_CONSTANTS "fr_grumpkin_constants.h"
#include "frlook_unit.h"

extern "C" const FrlookOps* msm_frlook_ops_grumpkin(void) {
  static const FrlookOps ops = {frl_grumpkin::FQ_P32, frl_grumpkin::frlook_launch_build, frl_grumpkin::frlook_launch_count, frl_grumpkin::frlook_launch_finish};
  return &ops;
}
