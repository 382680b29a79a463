// The scalar field of BN254 as a translation unit of libmsm_frgate.so: fq29.h over the field's constants and the constraint-evaluation kernel
// (csrc/frgate_unit.h, csrc/frgate_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frg_bn254
#define MSM_CURVE_CONSTANTS "fr_bn254_constants.h"
#define MSM_FRGATE_HOST_UNIT 1  // this unit also carries the library's host code
#include "frgate_unit.h"

extern "C" const FrgateOps* msm_frgate_ops_bn254(void) {
  static const FrgateOps ops = {frg_bn254::FQ_P32, frg_bn254::frgate_launch_apply};
  return &ops;
}
