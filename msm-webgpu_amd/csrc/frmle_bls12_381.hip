// The scalar field of BLS12-381 as a translation unit of libmsm_frmle.so: fq29.h over the field's constants and the sumcheck kernels (csrc/frmle_unit.h,
// csrc/frmle_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frm_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "frmle_unit.h"

extern "C" const FrmleOps* msm_frmle_ops_bls12_381(void) {
  static const FrmleOps ops = {frm_bls12_381::FQ_P32, frm_bls12_381::frmle_launch_fold, frm_bls12_381::frmle_launch_eval, frm_bls12_381::frmle_launch_eq, frm_bls12_381::frmle_launch_round, frm_bls12_381::frmle_launch_sum};
  return &ops;
}
