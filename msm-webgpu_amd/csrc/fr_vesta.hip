// The scalar field of Vesta as a translation unit of libmsm_fr.so: fq29.h over the field's constants and the NTT kernels (csrc/fr_unit.h,
// csrc/ntt_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS fr_vesta
#define MSM_CURVE_CONSTANTS "fr_vesta_constants.h"
#include "fr_unit.h"

extern "C" const FrOps* msm_fr_ops_vesta(void) {
  static const FrOps ops = {fr_vesta::FQ_P32, fr_vesta::FR_TWO_ADICITY, fr_vesta::ntt_launch_pass};
  return &ops;
}
