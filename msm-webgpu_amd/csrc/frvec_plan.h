// The constants and the level structure of libmsm_frvec.so's calls: pure host code, no HIP (csrc/frvec_host.h launches what this plans; the host
// program of tests/test_frvec_host.py runs the same plan through the same per-lane code on the CPU).  Needs the Frvec*Args of csrc/frvec_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "host_fr.h"

namespace msm_frvec {

using host_fr::Field;
using host_fr::Fr;

inline Fr pow2(const Field& f, int k) {  // 2^k mod r
  Fr x = {{1, 0, 0, 0}};
  for (int i = 0; i < k; i++) x = f.add(x, x);
  return x;
}
inline Fr inv_pow2(const Field& f, int k) {  // 2^-k mod r: k halvings of 1 (r odd: x or x + r is even, and x + r < 2^256)
  Fr x = {{1, 0, 0, 0}};
  for (int s = 0; s < k; s++) {
    if (x.v[0] & 1u) {
      unsigned __int128 c = 0;
      for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)x.v[i] + f.modulus().v[i];
        x.v[i] = (uint64_t)c;
        c >>= 64;
      }
    }
    for (int i = 0; i < 4; i++) x.v[i] = (x.v[i] >> 1) | (i < 3 ? x.v[i + 1] << 63 : 0);
  }
  return x;
}
inline Fr times(const Field& f, const Fr& a, const Fr& b) { return f.from_mont(f.mul(f.to_mont(a), f.to_mont(b))); }  // a b mod r, plain values
inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }

// the device's Montgomery radix is R = 2^261 (csrc/fq29.h); F = 2^256 for mont256 data, 1 otherwise
inline Fr form(const Field& f, bool mont) { return mont ? pow2(f, 256) : Fr{{1, 0, 0, 0}}; }
inline Fr restore(const Field& f, bool mont) { return pow2(f, mont ? 266 : 522); }  // R^2 / F

// b_const / c_const: the canonical constants, or NULL for a vector operand
inline FrvecMapArgs plan_map(const Field& f, int op, const uint8_t* b_const, const uint8_t* c_const, bool mont) {
  FrvecMapArgs m;
  memset(&m, 0, sizeof m);
  m.op = (uint32_t)op;
  m.b_const = b_const != nullptr, m.c_const = c_const != nullptr;
  const bool product = op != FRVEC_ADD && op != FRVEC_SUB;
  if (b_const) host_fr::store_words(times(f, host_fr::load32(b_const), product ? pow2(f, 261) : form(f, mont)), m.b);
  if (c_const) host_fr::store_words(times(f, host_fr::load32(c_const), form(f, mont)), m.c);
  host_fr::store_words(restore(f, mont), m.fix);
  return m;
}

inline FrvecInvArgs plan_inverse(const Field& f, uint32_t tile, bool mont) {
  FrvecInvArgs v;
  memset(&v, 0, sizeof v);
  v.tile = tile;
  host_fr::store_words(Field::sub_raw(f.modulus(), Fr{{2, 0, 0, 0}}), v.pm2);
  host_fr::store_words(mont ? pow2(f, 251) : inv_pow2(f, 261), v.scale);  // F^2 / R
  return v;
}

// level 0 of a scan (the data); the levels above it scan tile totals exclusively, in the form the totals are in
inline FrvecScanArgs plan_scan(const Field& f, uint32_t tile, int op, bool exclusive, bool mont) {
  FrvecScanArgs g;
  memset(&g, 0, sizeof g);
  g.tile = tile, g.op = (uint32_t)op, g.exclusive = exclusive;
  g.conv_in = g.conv_out = op == FRVEC_PRODUCT;
  host_fr::store_words(restore(f, mont), g.k_in);
  host_fr::store_words(form(f, mont), g.f_out);
  return g;
}
inline FrvecScanArgs inner_level(FrvecScanArgs g) {
  g.exclusive = 1, g.conv_in = g.conv_out = 0;
  return g;
}

// rows of n elements: level l has len[l] values per row in ceil(len[l] / tile) tiles; the last level has one tile per row
inline std::vector<size_t> plan_levels(size_t n, uint32_t tile) {
  std::vector<size_t> len(1, n);
  while ((len.back() + tile - 1) / tile > 1) len.push_back((len.back() + tile - 1) / tile);
  return len;
}

}  // namespace msm_frvec
