// The scalar field of Pallas as a translation unit of libmsm_frmat.so: fq29.h over the field's constants and the sparse-product kernels
// (csrc/frmat_unit.h, csrc/frmat_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frt_pallas
#define MSM_CURVE_CONSTANTS "fr_pallas_constants.h"
#include "frmat_unit.h"

extern "C" const FrmatOps* msm_frmat_ops_pallas(void) {
  static const FrmatOps ops = {frt_pallas::FQ_P32, frt_pallas::frmat_launch_lift, frt_pallas::frmat_launch_tile, frt_pallas::frmat_launch_stitch};
  return &ops;
}
