// The scalar field of Pallas as a translation unit of libmsm_frmle.so: fq29.h over the field's constants and the sumcheck kernels (csrc/frmle_unit.h,
// csrc/frmle_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frm_pallas
#define MSM_CURVE_CONSTANTS "fr_pallas_constants.h"
#include "frmle_unit.h"

extern "C" const FrmleOps* msm_frmle_ops_pallas(void) {
  static const FrmleOps ops = {frm_pallas::FQ_P32, frm_pallas::frmle_launch_fold, frm_pallas::frmle_launch_eval, frm_pallas::frmle_launch_eq, frm_pallas::frmle_launch_round, frm_pallas::frmle_launch_sum};
  return &ops;
}
