// The scalar field of BN254 as a translation unit of libmsm_frmle.so: fq29.h over the field's constants and the sumcheck kernels (csrc/frmle_unit.h,
// csrc/frmle_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frm_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FRMLE_HOST_UNIT 1  // this unit also carries the library's host code
#include "frmle_unit.h"

extern "C" const FrmleOps* msm_frmle_ops_bn254(void) {
  static const FrmleOps ops = {frm_bn254::FQ_P32, frm_bn254::frmle_launch_fold, frm_bn254::frmle_launch_eval, frm_bn254::frmle_launch_eq, frm_bn254::frmle_launch_round, frm_bn254::frmle_launch_sum};
  return &ops;
}
