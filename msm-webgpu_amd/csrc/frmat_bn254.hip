// The scalar field of BN254 as a translation unit of libmsm_frmat.so: fq29.h over the field's constants and the sparse-product kernels
// (csrc/frmat_unit.h, csrc/frmat_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frt_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FRMAT_HOST_UNIT 1  // this unit also carries the library's host code
#include "frmat_unit.h"

extern "C" const FrmatOps* msm_frmat_ops_bn254(void) {
  static const FrmatOps ops = {frt_bn254::FQ_P32, frt_bn254::frmat_launch_lift, frt_bn254::frmat_launch_tile, frt_bn254::frmat_launch_stitch};
  return &ops;
}
