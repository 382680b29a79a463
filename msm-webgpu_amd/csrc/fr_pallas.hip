// The scalar field of Pallas as a translation unit of libmsm_fr.so: fq29.h over the field's constants and the NTT kernels (csrc/fr_unit.h,
// csrc/ntt_kernels.h), reached by the host code through the table below.
#define MSM_FIELD_NS fr_pallas
#define MSM_CURVE_CONSTANTS "fr_pallas_constants.h"
#include "fr_unit.h"

extern "C" const FrOps* msm_fr_ops_pallas(void) {
  static const FrOps ops = {fr_pallas::FQ_P32, fr_pallas::FR_TWO_ADICITY, fr_pallas::ntt_launch_pass};
  return &ops;
}
