// The constants and the level structure of libmsm_frpoly.so's calls: pure host code, no HIP (csrc/frpoly_host.h launches what this plans; the host
// program of tests/test_frpoly_host.py runs the same plan through the same per-lane code on the CPU).  Needs the Frpoly*Args of csrc/frpoly_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "host_fr.h"

namespace msm_frpoly {

using host_fr::Field;
using host_fr::Fr;

inline Fr pow2(const Field& f, int k) {  // 2^k mod r
  Fr x = {{1, 0, 0, 0}};
  for (int i = 0; i < k; i++) x = f.add(x, x);
  return x;
}
inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }

// the device's Montgomery radix is R = 2^261 (csrc/fq29.h); F = 2^256 for mont256 data, 1 otherwise.  Below, values with an m are in the HOST's
// Montgomery form (csrc/host_fr.h: 2^256), whatever the data's form is.
inline Fr form(const Field& f, bool mont) { return mont ? pow2(f, 256) : Fr{{1, 0, 0, 0}}; }
inline Fr restore(const Field& f, bool mont) { return pow2(f, mont ? 266 : 522); }  // R^2 / F
inline Fr pow_m(const Field& f, Fr xm, uint64_t e) {
  Fr acc = f.one();
  for (; e; e >>= 1, xm = f.mul(xm, xm))
    if (e & 1u) acc = f.mul(acc, xm);
  return acc;
}
// xm times the plain value k, as a plain value: what the device reads
inline void store_scaled(const Field& f, const Fr& xm, const Fr& k, uint32_t w[8]) { host_fr::store_words(f.mul(xm, k), w); }

// rows of n elements: level l has len[l] values per row in ceil(len[l] / tile) tiles; the last level has one tile per row (as csrc/frvec_plan.h)
inline std::vector<size_t> plan_levels(size_t n, uint32_t tile) {
  std::vector<size_t> len(1, n);
  while ((len.back() + tile - 1) / tile > 1) len.push_back((len.back() + tile - 1) / tile);
  return len;
}

// Horner at z over `levels` levels of tiles: level l works at the point z_l = z^(tile^l) and folds its lanes with z_l^(4 2^k), k = 0 .. 7
inline std::vector<FrpolyLevelArgs> plan_horner(const Field& f, uint32_t tile, size_t levels, const uint8_t z[32]) {
  std::vector<FrpolyLevelArgs> out(levels);
  const Fr radix = pow2(f, 261);
  Fr zm = f.to_mont(host_fr::load32(z));
  for (size_t l = 0; l < levels; l++) {
    FrpolyLevelArgs& g = out[l];
    memset(&g, 0, sizeof g);
    g.tile = tile, g.mode = FRPOLY_HORNER;
    store_scaled(f, zm, radix, g.z);
    Fr wm = f.mul(zm, zm);
    wm = f.mul(wm, wm);  // z_l^4
    for (int k = 0; k < FRPOLY_STEPS; k++, wm = f.mul(wm, wm)) store_scaled(f, wm, radix, g.w[k]);
    zm = tile == FRPOLY_TILE ? wm : pow_m(f, zm, tile);  // (eight squarings of z^4 leave z^1024)
  }
  return out;
}

// the dot product: level 0 multiplies and restores, the levels above add
inline std::vector<FrpolyLevelArgs> plan_dot(const Field& f, uint32_t tile, size_t levels, bool shared_b, bool mont) {
  std::vector<FrpolyLevelArgs> out(levels);
  for (size_t l = 0; l < levels; l++) {
    FrpolyLevelArgs& g = out[l];
    memset(&g, 0, sizeof g);
    g.tile = tile, g.mode = FRPOLY_DOT;
    g.second = g.restore = l == 0;
    g.shared_b = l == 0 && shared_b;
    host_fr::store_words(restore(f, mont), g.fix);
  }
  return out;
}

// combine: words[8 k ..] = c[k] R
inline void plan_combine(const Field& f, const uint8_t* coeffs, size_t batch, std::vector<uint32_t>& words) {
  words.resize(batch * 8);
  const Fr radix_m = f.to_mont(pow2(f, 261));
  for (size_t k = 0; k < batch; k++) store_scaled(f, radix_m, host_fr::load32(coeffs + 32 * k), words.data() + 8 * k);
}

// powers: the tables -- words[8 (16 w + d) ..] = c g^(4 d) F for w = 0 and g^(4 16^w d) R above, as many windows as the lane numbers of n
// elements have digits -- and g R
inline FrpolyPowersArgs plan_powers(const Field& f, size_t n, const uint8_t g[32], const uint8_t c[32], bool mont, std::vector<uint32_t>& words) {
  FrpolyPowersArgs p;
  memset(&p, 0, sizeof p);
  const size_t lanes = (n + FRPOLY_E - 1) / FRPOLY_E;
  p.windows = 1;
  while (p.windows < FRPOLY_MAX_WINDOWS && ((lanes - 1) >> (FRPOLY_WINDOW_BITS * p.windows))) p.windows++;
  const Fr radix = pow2(f, 261);
  const Fr gm = f.to_mont(host_fr::load32(g));
  store_scaled(f, gm, radix, p.g);
  words.resize((size_t)p.windows * FRPOLY_WINDOW_SIZE * 8);
  Fr step_m = f.mul(gm, gm);
  step_m = f.mul(step_m, step_m);  // g^4
  const Fr first = f.from_mont(f.mul(f.to_mont(host_fr::load32(c)), f.to_mont(form(f, mont))));  // c F
  for (uint32_t w = 0; w < p.windows; w++) {
    Fr xm = f.one();
    for (uint32_t d = 0; d < FRPOLY_WINDOW_SIZE; d++, xm = f.mul(xm, step_m)) store_scaled(f, xm, w ? radix : first, words.data() + 8 * (FRPOLY_WINDOW_SIZE * w + d));
    step_m = xm;  // g^(4 16^(w + 1))
  }
  return p;
}

}  // namespace msm_frpoly
