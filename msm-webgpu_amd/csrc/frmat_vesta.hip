// The scalar field of Vesta as a translation unit of libmsm_frmat.so: fq29.h over the field's constants and the sparse-product kernels
// (csrc/frmat_unit.h, csrc/frmat_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS frt_vesta
#define MSM_CURVE_CONSTANTS "fr_vesta_constants.h"
#include "frmat_unit.h"

extern "C" const FrmatOps* msm_frmat_ops_vesta(void) {
  static const FrmatOps ops = {frt_vesta::FQ_P32, frt_vesta::frmat_launch_lift, frt_vesta::frmat_launch_tile, frt_vesta::frmat_launch_stitch};
  return &ops;
}
