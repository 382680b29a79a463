// The scalar field of BLS12-381 as a translation unit of libmsm_frmat.so: fq29.h over the field's constants and the sparse-product kernels
// (csrc/frmat_unit.h, csrc/frmat_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frt_bls12_381
#define MSM_CURVE_CONSTANTS "fr_bls12_381_constants.h"
#include "frmat_unit.h"

extern "C" const FrmatOps* msm_frmat_ops_bls12_381(void) {
  static const FrmatOps ops = {frt_bls12_381::FQ_P32, frt_bls12_381::frmat_launch_lift, frt_bls12_381::frmat_launch_tile, frt_bls12_381::frmat_launch_stitch};
  return &ops;
}
