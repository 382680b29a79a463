// One curve's worth of device + host arithmetic and kernels: define MSM_FIELD_NS, MSM_KERNEL_NS and MSM_CURVE_CONSTANTS, include
// this file (csrc/curve_select.h).  A translation unit holds one curve (curve_<name>.hip); a G2 unit lists the same headers itself, with
// fq2.h over a prime field of its own in place of fq29.h.
#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "g1.h"
#include "host_g1.h"
#include "glv.h"
#include "msm_kernels.h"
#undef MSM_CURVE_UNIT
