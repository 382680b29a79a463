// Host build (g++ -DFQ_CHECK) of csrc/scalar_mul.h -- the ladders and the shared-inversion normalisation behind msm_hip_mul_each /
// msm_hip_mul_base -- for CPU-side tests of the exact code the HIP kernels inline, every limb bound asserted.  Test-only: not part of
// libmsm_hip.so.  A G1 curve is chosen as for fq29_harness.cpp (-DMSM_FIELD_NS=... -DMSM_CURVE_CONSTANTS=... -DHARNESS_FIELD_NS=...);
// -DHARNESS_G2 sets a G2 unit up as fq2_harness.cpp does (-DHARNESS_G2_BLS12_381: BLS12-381's).
#include <cstring>
#include <vector>

#ifdef HARNESS_G2
#define MSM_CURVE_UNIT 1
#ifdef HARNESS_G2_BLS12_381
#define MSM_FIELD_NS bls12_381_g2_fp
#include "bls12_381_constants.h"
#else
#define MSM_FIELD_NS bn254_g2_fp
#include "bn254_constants.h"
#endif
#include "fq29.h"
#undef MSM_FIELD_NS
#define MSM_FQ2 1
#ifdef HARNESS_G2_BLS12_381
#define MSM_BASE_NS bls12_381_g2_fp
#define MSM_FIELD_NS bls12_381_g2
#include "bls12_381_g2_constants.h"
#else
#define MSM_BASE_NS bn254_g2_fp
#define MSM_FIELD_NS bn254_g2
#include "bn254_g2_constants.h"
#endif
#include "fq2.h"
#include "g1.h"
#include "glv.h"
#include "scalar_mul.h"
#define HARNESS_FIELD_NS MSM_FIELD_NS
#else
#include "scalar_mul.h"
#endif

#ifndef HARNESS_FIELD_NS
#define HARNESS_FIELD_NS bn254
#endif
using namespace HARNESS_FIELD_NS;
constexpr int HB = 4 * FQ_WORDS;  // bytes of a coordinate on the wire

// the inversion the kernels take from msm_kernels.h (Fermat; Fq2: through the norm), restated for the host
#ifndef MSM_FQ2
static fq host_fq_inv(const fq& a) {
  fq acc = fq_one();
  for (int bit = 32 * FQ_WORDS - 1; bit >= 0; bit--) {
    acc = fq_sqr(acc);
    if ((FQ_PM2_32[bit >> 5] >> (bit & 31)) & 1u) acc = fq_mul(acc, a);
  }
  return acc;
}
#else
static fq host_fq_inv(const fq& a) {
  const fp a0 = f2_c0(a), a1 = f2_c1(a);
  const fp nrm = fpn::fq_mul2(a0, a0, a1, a1);
  fp acc = fpn::fq_one();
  for (int bit = 32 * FP_WORDS - 1; bit >= 0; bit--) {
    acc = fpn::fq_sqr(acc);
    if ((FQ_PM2_32[bit >> 5] >> (bit & 31)) & 1u) acc = fpn::fq_mul(acc, nrm);
  }
  return f2_make(fpn::fq_mul(a0, acc), fpn::fq_mul(fpn::fq_sub<3>(fpn::fq_zero(), a1), acc));
}
#endif

static fq load_fq(const uint8_t* b) {  // canonical LE bytes -> Montgomery, canonical
  uint32_t w[FQ_WORDS];
  memcpy(w, b, HB);
  return fq_to_mont(fq_unpack(w));
}

// k_mul_normalize's walk over n results: workgroups of `lanes` lanes, lane l of a group takes elements l, l + lanes, ... of the group's
// lanes * SMUL_CHUNK elements
static void normalize_all(uint32_t* xy, const uint32_t* z, size_t n, size_t lanes) {
  std::vector<uint32_t> prefix(n * FQ_WORDS + 1);
  const size_t group = lanes * SMUL_CHUNK;
  for (size_t g0 = 0; g0 < n; g0 += group) {
    const size_t end = g0 + group < n ? g0 + group : n;
    for (size_t l = 0; l < lanes && g0 + l < end; l++) {
      const fq prod = smul_norm_forward(z, prefix.data(), g0 + l, lanes, end);
      smul_norm_backward(xy, z, prefix.data(), g0 + l, lanes, end, host_fq_inv(prod));
    }
  }
}

extern "C" {
int h_smul_chunk(void) { return SMUL_CHUNK; }

// out[i] = scalars[i] * points[i] as k_mul_each + k_mul_normalize compute it.  mode 0: the plain ladder, 1: the endomorphism's.
// points: n x 2 HB canonical affine; scalars: n x 32 B; out: n x 2 HB.  Returns the number of scalars >= r (their outputs are zero records).
size_t h_smul(int mode, const uint8_t* points, const uint8_t* scalars, size_t n, size_t lanes, uint8_t* out) {
  std::vector<uint32_t> xy(n * 2 * FQ_WORDS + 1), z(n * FQ_WORDS + 1);
  size_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t k[8];
    memcpy(k, scalars + 32 * i, 32);
    g1_xyzz r = g1_identity();
    if (smul_geq_r(k)) {
      bad++;
    } else {
      const fq px = load_fq(points + 2 * HB * i), py = load_fq(points + 2 * HB * i + HB);
      r = mode ? smul_endo(px, py, k) : smul_plain(px, py, k);
    }
    smul_store_jacobian(xy.data(), z.data(), i, r);
  }
  normalize_all(xy.data(), z.data(), n, lanes);
  memcpy(out, xy.data(), n * 2 * HB);
  return bad;
}

// out[i] = scalars[i] * P through the fixed-base table of digit width c, built as the device builds it: the ladder (mode as h_smul) over the
// entries' scalars, the shared-inversion normalisation, then packed Montgomery records.  Returns the number of scalars >= r.
size_t h_smul_fixed(int mode, int c, const uint8_t* point, const uint8_t* scalars, size_t n, uint8_t* out) {
  const size_t entries = (size_t)smul_fixed_windows(c) << (c - 1);
  std::vector<uint32_t> table(entries * 2 * FQ_WORDS + 1), tz(entries * FQ_WORDS + 1);
  const fq px = load_fq(point), py = load_fq(point + HB);
  for (size_t e = 0; e < entries; e++) {
    uint32_t k[8];
    smul_table_scalar(c, (int)(e >> (c - 1)), (uint32_t)(e & ((1u << (c - 1)) - 1u)) + 1u, k);
    smul_store_jacobian(table.data(), tz.data(), e, mode ? smul_endo(px, py, k) : smul_plain(px, py, k));
  }
  normalize_all(table.data(), tz.data(), entries, 256);
  for (size_t e = 0; e < 2 * entries; e++) smul_st(table.data() + e * FQ_WORDS, fq_to_mont(smul_ld(table.data() + e * FQ_WORDS)));
  std::vector<uint32_t> xy(n * 2 * FQ_WORDS + 1), z(n * FQ_WORDS + 1);
  size_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t k[8];
    memcpy(k, scalars + 32 * i, 32);
    g1_xyzz r = g1_identity();
    if (smul_geq_r(k)) bad++;
    else r = smul_fixed(table.data(), c, k);
    smul_store_jacobian(xy.data(), z.data(), i, r);
  }
  normalize_all(xy.data(), z.data(), n, 5);
  memcpy(out, xy.data(), n * 2 * HB);
  return bad;
}

// the normalisation alone: n Jacobian records (X, Y, Z canonical integers, Z = 0 the identity) -> n affine records
void h_smul_normalize(const uint8_t* jac, size_t n, size_t lanes, uint8_t* out) {
  std::vector<uint32_t> xy(n * 2 * FQ_WORDS + 1), z(n * FQ_WORDS + 1);
  for (size_t i = 0; i < n; i++) {
    smul_st(xy.data() + i * 2 * FQ_WORDS, load_fq(jac + 3 * HB * i));
    smul_st(xy.data() + i * 2 * FQ_WORDS + FQ_WORDS, load_fq(jac + 3 * HB * i + HB));
    smul_st(z.data() + i * FQ_WORDS, load_fq(jac + 3 * HB * i + 2 * HB));
  }
  normalize_all(xy.data(), z.data(), n, lanes);
  memcpy(out, xy.data(), n * 2 * HB);
}
}
