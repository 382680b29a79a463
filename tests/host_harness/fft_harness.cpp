// Host build (g++ -DFQ_CHECK) of what msm_hip_bases_fft adds to csrc/scalar_mul.h -- the butterfly (smul_butterfly) and the normalisation that
// keeps Montgomery records (smul_norm_backward<true>) -- with every limb bound asserted, and of csrc/host_fr.h, the host's twiddle arithmetic.
// Test-only: not part of libmsm_hip.so.  A G1 curve is chosen as for scalar_mul_harness.cpp
// (-DMSM_FIELD_NS=... -DMSM_CURVE_CONSTANTS=... -DHARNESS_FIELD_NS=...).
#include <cstring>
#include <vector>

#include "host_fr.h"
#include "scalar_mul.h"

#ifndef HARNESS_FIELD_NS
#define HARNESS_FIELD_NS bn254
#endif
using namespace HARNESS_FIELD_NS;
constexpr int HB = 4 * FQ_WORDS;  // bytes of a coordinate on the wire

// the inversion the kernels take from msm_kernels.h (Fermat), restated for the host
static fq host_fq_inv(const fq& a) {
  fq acc = fq_one();
  for (int bit = 32 * FQ_WORDS - 1; bit >= 0; bit--) {
    acc = fq_sqr(acc);
    if ((FQ_PM2_32[bit >> 5] >> (bit & 31)) & 1u) acc = fq_mul(acc, a);
  }
  return acc;
}

static fq load_fq(const uint8_t* b) {  // canonical LE bytes -> Montgomery, canonical (0 stays 0: the all-zero record stays the identity)
  uint32_t w[FQ_WORDS];
  memcpy(w, b, HB);
  return fq_to_mont(fq_unpack(w));
}

// k_mul_normalize's / k_fft_normalize's walk over n results in workgroups of `lanes` lanes
template <bool MONT>
static void normalize_all(uint32_t* xy, const uint32_t* z, size_t n, size_t lanes) {
  std::vector<uint32_t> prefix(n * FQ_WORDS + 1);
  const size_t group = lanes * SMUL_CHUNK;
  for (size_t g0 = 0; g0 < n; g0 += group) {
    const size_t end = g0 + group < n ? g0 + group : n;
    for (size_t l = 0; l < lanes && g0 + l < end; l++) {
      const fq prod = smul_norm_forward(z, prefix.data(), g0 + l, lanes, end);
      smul_norm_backward<MONT>(xy, z, prefix.data(), g0 + l, lanes, end, host_fq_inv(prod));
    }
  }
}

template <int LADDER>
static void butterflies(const uint32_t* a, const uint32_t* b, const uint8_t* w, size_t n, uint32_t* xy, uint32_t* z) {
  for (size_t i = 0; i < n; i++) {
    uint32_t k[8];
    memcpy(k, w + 32 * i, 32);
    g1_xyzz sum, diff;
    smul_butterfly<LADDER>(a + i * 2 * FQ_WORDS, false, b + i * 2 * FQ_WORDS, false, k, sum, diff);
    smul_store_jacobian(xy, z, 2 * i, sum);
    smul_store_jacobian(xy, z, 2 * i + 1, diff);
  }
}

extern "C" {
// n butterflies as k_fft_stage runs them: out records 2 i and 2 i + 1 = a_i + w_i b_i and a_i - w_i b_i, through the Montgomery-keeping
// normalisation (then out of Montgomery form: canonical integers, the identity as the all-zero record).
// ladder: 0 none (every w_i must be 1), 1 smul_plain, 2 smul_endo.  a, b: n x 2 HB canonical affine, all-zero = the identity; w: n x 32 B below r.
void h_fft_butterfly(int ladder, const uint8_t* a, const uint8_t* b, const uint8_t* w, size_t n, size_t lanes, uint8_t* out) {
  std::vector<uint32_t> ra(n * 2 * FQ_WORDS + 1), rb(n * 2 * FQ_WORDS + 1), xy(2 * n * 2 * FQ_WORDS + 1), z(2 * n * FQ_WORDS + 1);
  for (size_t i = 0; i < 2 * n; i++) {
    smul_st(ra.data() + i * FQ_WORDS, load_fq(a + HB * i));
    smul_st(rb.data() + i * FQ_WORDS, load_fq(b + HB * i));
  }
  if (ladder == 2) butterflies<SMUL_LADDER_ENDO>(ra.data(), rb.data(), w, n, xy.data(), z.data());
  else if (ladder == 1) butterflies<SMUL_LADDER_PLAIN>(ra.data(), rb.data(), w, n, xy.data(), z.data());
  else butterflies<SMUL_LADDER_NONE>(ra.data(), rb.data(), w, n, xy.data(), z.data());
  normalize_all<true>(xy.data(), z.data(), 2 * n, lanes);
  for (size_t e = 0; e < 4 * n; e++) smul_st(xy.data() + e * FQ_WORDS, fq_from_mont(smul_ld(xy.data() + e * FQ_WORDS)));
  memcpy(out, xy.data(), 2 * n * 2 * HB);
}

// the normalisation alone: n Jacobian records (X, Y, Z canonical integers, Z = 0 the identity) -> n affine records.  mont = 0: the form
// k_mul_normalize runs (wire records); 1: the Montgomery-keeping form, its records handed back as they are (x R mod p, y R mod p)
void h_fft_normalize(int mont, const uint8_t* jac, size_t n, size_t lanes, uint8_t* out) {
  std::vector<uint32_t> xy(n * 2 * FQ_WORDS + 1), z(n * FQ_WORDS + 1);
  for (size_t i = 0; i < n; i++) {
    smul_st(xy.data() + i * 2 * FQ_WORDS, load_fq(jac + 3 * HB * i));
    smul_st(xy.data() + i * 2 * FQ_WORDS + FQ_WORDS, load_fq(jac + 3 * HB * i + HB));
    smul_st(z.data() + i * FQ_WORDS, load_fq(jac + 3 * HB * i + 2 * HB));
  }
  if (mont) normalize_all<true>(xy.data(), z.data(), n, lanes);
  else normalize_all<false>(xy.data(), z.data(), n, lanes);
  memcpy(out, xy.data(), n * 2 * HB);
}

// csrc/host_fr.h over this curve's r
int h_fr_is_primitive_root(const uint8_t* omega, int log_n) { return host_fr::is_primitive_root(host_fr::Field(FR_R32), omega, log_n) ? 1 : 0; }
void h_fr_twiddles(const uint8_t* omega, int log_n, uint8_t* out) {  // out: 2^(log_n - 1) x 32 B
  std::vector<uint32_t> tw;
  host_fr::twiddle_table(host_fr::Field(FR_R32), omega, log_n, tw);
  memcpy(out, tw.data(), tw.size() * 4);
}
void h_fr_inverse_of_n(int log_n, uint8_t* out) {
  uint32_t k[8];
  host_fr::inverse_of_n(host_fr::Field(FR_R32), log_n, k);
  memcpy(out, k, 32);
}
}
