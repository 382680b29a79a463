// The scalar field of Grumpkin as a translation unit of libmsm_frmle.so: fq29.h over the field's constants and the sumcheck kernels (csrc/frmle_unit.h,
// csrc/frmle_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frm_grumpkin
#define MSM_CURVE_CONSTANTS "fr_grumpkin_constants.h"
#include "frmle_unit.h"

extern "C" const FrmleOps* msm_frmle_ops_grumpkin(void) {
  static const FrmleOps ops = {frm_grumpkin::FQ_P32, frm_grumpkin::frmle_launch_fold, frm_grumpkin::frmle_launch_eval, frm_grumpkin::frmle_launch_eq, frm_grumpkin::frmle_launch_round, frm_grumpkin::frmle_launch_sum};
  return &ops;
}
