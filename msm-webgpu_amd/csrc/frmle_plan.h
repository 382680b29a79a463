// The constants and the level structure of libmsm_frmle.so's calls: pure host code, no HIP (csrc/frmle_host.h launches what this plans; the host
// program of tests/test_frmle_host.py runs the same plan through the same per-lane code on the CPU).  Needs the Frmle*Args of csrc/frmle_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "host_fr.h"

namespace msm_frmle {

using host_fr::Field;
using host_fr::Fr;

inline Fr pow2(const Field& f, int k) {  // 2^k mod r
  Fr x = {{1, 0, 0, 0}};
  for (int i = 0; i < k; i++) x = f.add(x, x);
  return x;
}
inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }
inline bool power_of_two(size_t n) { return n && !(n & (n - 1)); }
inline int log2_of(size_t n) {  // n a power of two
  int k = 0;
  while (((size_t)1 << k) < n) k++;
  return k;
}

// the device's Montgomery radix is R = 2^261 (csrc/fq29.h); F = 2^256 for mont256 data, 1 otherwise.  Below, values with an m are in the HOST's
// Montgomery form (csrc/host_fr.h: 2^256), whatever the data's form is.
inline Fr form(const Field& f, bool mont) { return mont ? pow2(f, 256) : Fr{{1, 0, 0, 0}}; }
// xm times the plain value k, as a plain value: what the device reads
inline void store_scaled(const Field& f, const Fr& xm, const Fr& k, uint32_t w[8]) { host_fr::store_words(f.mul(xm, k), w); }
inline Fr one_minus_m(const Field& f, const Fr& xm) {  // (1 - x) in the host's form, from x in it
  const Fr neg = Field::sub_raw(f.modulus(), xm);      // r - x in (0, r]: add() reduces the sum
  return f.add(neg, f.one());
}

// rows of n values: level l has len[l] values per row in ceil(len[l] / tile) tiles; the last level has one tile per row (as csrc/frpoly_plan.h)
inline std::vector<size_t> plan_levels(size_t n, uint32_t tile) {
  std::vector<size_t> len(1, n);
  while ((len.back() + tile - 1) / tile > 1) len.push_back((len.back() + tile - 1) / tile);
  return len;
}

inline FrmleFoldArgs plan_fold(const Field& f, const uint8_t c[32]) {
  FrmleFoldArgs g;
  store_scaled(f, f.to_mont(host_fr::load32(c)), pow2(f, 261), g.c);
  return g;
}

// eval of a table of 2^k elements at point (k x 32 bytes; point[0] is the TOP bit's variable): level l binds the bits [l t, l t + vars) of the
// index, t = log2(tile); bit b is the variable point[k - 1 - b]
inline std::vector<FrmleEvalArgs> plan_eval(const Field& f, uint32_t tile, int k, const uint8_t* point) {
  const int t = log2_of(tile);
  const size_t levels = k ? (size_t)(k + t - 1) / t : 1;
  std::vector<FrmleEvalArgs> out(levels);
  const Fr radix = pow2(f, 261);
  for (size_t l = 0; l < levels; l++) {
    FrmleEvalArgs& g = out[l];
    memset(&g, 0, sizeof g);
    g.tile = tile;
    const int left = k - (int)l * t;
    g.vars = (uint32_t)(left < t ? left : t);
    for (uint32_t j = 0; j < g.vars; j++) store_scaled(f, f.to_mont(host_fr::load32(point + 32 * (k - 1 - ((int)l * t + (int)j)))), radix, g.z[j]);
  }
  return out;
}

// eq over n = 2^k elements: the tables -- words[8 (16 w + d) ..] = the product of the factors of the bits 2 + 4 w .. 5 + 4 w of the index as the
// bits of d say, times c F for w = 0 and R above, as many windows as the lane numbers of n elements have digits -- and the four factors of the
// bits 0 and 1, times R.  A bit the index does not have has the factors 1 (clear) and 0 (set).
inline FrmleEqArgs plan_eq(const Field& f, size_t n, const uint8_t* point, const uint8_t c[32], bool mont, std::vector<uint32_t>& words) {
  FrmleEqArgs p;
  memset(&p, 0, sizeof p);
  const int k = log2_of(n);
  const size_t lanes = (n + FRMLE_E - 1) / FRMLE_E;
  p.windows = 1;
  while (p.windows < FRMLE_MAX_WINDOWS && ((lanes - 1) >> (FRMLE_WINDOW_BITS * p.windows))) p.windows++;
  const Fr radix = pow2(f, 261);
  const Fr zero = {{0, 0, 0, 0}};
  auto factor = [&](int bit, uint32_t set) -> Fr {
    if (bit >= k) return set ? zero : f.one();
    const Fr pm = f.to_mont(host_fr::load32(point + 32 * (k - 1 - bit)));
    return set ? pm : one_minus_m(f, pm);
  };
  for (uint32_t j = 0; j < FRMLE_E; j++) store_scaled(f, f.mul(factor(1, j >> 1), factor(0, j & 1u)), radix, p.q[j]);
  words.assign((size_t)p.windows * FRMLE_WINDOW_SIZE * 8, 0);
  const Fr first = f.from_mont(f.mul(f.to_mont(host_fr::load32(c)), f.to_mont(form(f, mont))));  // c F
  for (uint32_t w = 0; w < p.windows; w++) {
    for (uint32_t d = 0; d < FRMLE_WINDOW_SIZE; d++) {
      Fr xm = f.one();
      for (int u = 0; u < FRMLE_WINDOW_BITS; u++) xm = f.mul(xm, factor(2 + FRMLE_WINDOW_BITS * (int)w + u, (d >> u) & 1u));
      store_scaled(f, xm, w ? radix : first, words.data() + 8 * (FRMLE_WINDOW_SIZE * w + d));
    }
  }
  return p;
}

// a term as the caller gives it (include/msm_frmle.h: msm_frmle_term), field by field
struct Term {
  const uint8_t* coeff;
  uint32_t degree;
  const uint32_t* rows;
};
// round: the kernel's arguments and words[16 term ..] = the term's constant coeff R^d / F^(d-1) -- the product chain of d factors carries
// F^d / R^(d-1), one product by the constant leaves coeff F prod --, its degree and its rows
inline FrmleRoundArgs plan_round(const Field& f, uint32_t tile, const Term* terms, size_t num_terms, size_t batch, const uint8_t* fold_by, bool mont,
                                 std::vector<uint32_t>& words) {
  FrmleRoundArgs g;
  memset(&g, 0, sizeof g);
  g.tile = tile, g.num_terms = (uint32_t)num_terms, g.batch = (uint32_t)batch, g.fold = fold_by != nullptr;
  if (fold_by) store_scaled(f, f.to_mont(host_fr::load32(fold_by)), pow2(f, 261), g.c);
  words.assign(num_terms * FRMLE_TERM_WORDS, 0);
  uint32_t top = 0;
  for (size_t k = 0; k < num_terms; k++) {
    const int d = (int)terms[k].degree;
    if (terms[k].degree > top) top = terms[k].degree;
    uint32_t* w = words.data() + FRMLE_TERM_WORDS * k;
    store_scaled(f, f.to_mont(host_fr::load32(terms[k].coeff)), pow2(f, mont ? 5 * d + 256 : 261 * d), w);
    w[8] = terms[k].degree;
    for (int j = 0; j < d; j++) w[9 + j] = terms[k].rows[j];
  }
  g.points = top + 1;
  return g;
}

}  // namespace msm_frmle
