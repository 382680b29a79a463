// The scalar field of Grumpkin as a translation unit of libmsm_frmat.so: fq29.h over the field's constants and the sparse-product kernels
// (csrc/frmat_unit.h, csrc/frmat_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frt_grumpkin
#define MSM_CURVE_CONSTANTS "fr_grumpkin_constants.h"
#include "frmat_unit.h"

extern "C" const FrmatOps* msm_frmat_ops_grumpkin(void) {
  static const FrmatOps ops = {frt_grumpkin::FQ_P32, frt_grumpkin::frmat_launch_lift, frt_grumpkin::frmat_launch_tile, frt_grumpkin::frmat_launch_stitch};
  return &ops;
}
