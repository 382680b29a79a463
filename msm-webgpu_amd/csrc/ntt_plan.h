// The plan of a transform and the contents of its factor tables: pure host code, no HIP (csrc/ntt_host.h uploads and caches what this computes;
// the host program of tests/test_ntt_host.py runs the same plan through the same per-element code on the CPU).  Needs NttPass (csrc/ntt_kernels.h).
#pragma once
#include <cstring>
#include <vector>

#include "host_fr.h"

namespace msm_fr {

// digits of (almost) equal width, at most `cap` bits each, the first on top of the index; log_n = 0: one digit of no bits
inline std::vector<uint32_t> plan_digits(int log_n, int cap) {
  const int k = log_n == 0 ? 1 : (log_n + cap - 1) / cap;
  std::vector<uint32_t> w(k);
  for (int q = 0; q < k; q++) w[q] = (uint32_t)(log_n / k + (q < log_n % k ? 1 : 0));
  return w;
}

// the pass structures of a plan (csrc/ntt_kernels.h: NttPass); the factor modes are filled in by the caller
inline std::vector<NttPass> plan_passes(int log_n, const std::vector<uint32_t>& dig) {
  std::vector<NttPass> out;
  uint32_t shift = 0;
  const size_t k = dig.size();
  for (size_t q = 0; q < k; q++) {
    NttPass p;
    memset(&p, 0, sizeof p);
    p.log_n = (uint32_t)log_n;
    p.b = dig[q];
    p.shift = shift;
    shift += dig[q];
    p.lo = (uint32_t)log_n - shift;
    p.first = q == 0;
    p.last = q + 1 == k;
    p.tw_log = dig[0] ? dig[0] : 1;
    p.ndig = (uint32_t)k;
    for (size_t i = 0; i < k; i++) p.dig_w[i] = (uint8_t)dig[i];
    if (!p.last) {  // a strided digit: the columns are the lowest index bits
      p.log_c = p.lo < NTT_COL_BITS ? p.lo : NTT_COL_BITS;
      p.col_at = 0;
      p.ins_at[0] = 0, p.ins_w[0] = p.log_c, p.ins_at[1] = p.lo, p.ins_w[1] = p.b;
    } else if (k > 1) {  // the contiguous digit: the columns are the lowest bits of the first digit
      p.log_c = dig[0] < NTT_COL_BITS ? dig[0] : NTT_COL_BITS;
      p.col_at = (uint32_t)log_n - dig[0];
      p.ins_at[0] = 0, p.ins_w[0] = p.b, p.ins_at[1] = p.col_at, p.ins_w[1] = p.log_c;
    }  // one pass: no columns, nothing to spread (all zero)
    out.push_back(p);
  }
  return out;
}

// x (canonical) -> x 2^261 mod r, canonical words: the form every device factor has
struct FactorForm {
  const host_fr::Field& f;
  host_fr::Fr k;  // 2^261 mod r in the host's Montgomery form
  explicit FactorForm(const host_fr::Field& f_) : f(f_) {
    host_fr::Fr x = {{1, 0, 0, 0}};
    for (int i = 0; i < 261; i++) x = f.add(x, x);
    k = f.to_mont(x);
  }
  void store(const host_fr::Fr& x_mont, uint32_t* w) const { host_fr::store_words(f.from_mont(f.mul(x_mont, k)), w); }
};

// g^e for e < 2^bits, times c = 1 / 2^inv_log_n when inv_log_n > 0, as a two-level table (csrc/ntt_kernels.h: ntt_times_factor): lo[k] = g^k for
// k < 2^lo_bits, hi[k] = c g^(k 2^lo_bits).  g == nullptr: the constant c alone (hi[0]; mode 2).  Entries are 8 words, x 2^261 mod r, canonical.
struct HostTable {
  std::vector<uint32_t> lo, hi;
  uint32_t lo_bits = 0, mode = 0;
};
inline HostTable build_power_table(const host_fr::Field& f, const uint8_t* g, int bits, int inv_log_n) {
  const FactorForm form(f);
  HostTable t;
  t.lo_bits = g ? (uint32_t)(bits < NTT_TABLE_LO_BITS ? bits : NTT_TABLE_LO_BITS) : 31u;
  const size_t n_lo = g ? (size_t)1 << t.lo_bits : 0, n_hi = g ? (size_t)1 << (bits - (int)t.lo_bits) : 1;
  host_fr::Fr c = f.one();
  if (inv_log_n > 0) {
    uint32_t w[8];
    host_fr::inverse_of_n(f, inv_log_n, w);
    host_fr::Fr plain;
    for (int i = 0; i < 4; i++) plain.v[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    c = f.to_mont(plain);
  }
  const bool need_hi = n_hi > 1 || inv_log_n > 0 || !g;
  t.mode = (g ? 1u : 0u) | (need_hi ? 2u : 0u);
  t.lo.resize(8 * n_lo);
  t.hi.resize(need_hi ? 8 * n_hi : 0);
  host_fr::Fr step = f.one();
  if (g) {
    const host_fr::Fr gm = f.to_mont(host_fr::load32(g));
    host_fr::Fr x = f.one();
    for (size_t k = 0; k < n_lo; k++) {
      form.store(x, t.lo.data() + 8 * k);
      x = f.mul(x, gm);
    }
    step = x;  // g^(2^lo_bits)
  }
  if (need_hi) {
    host_fr::Fr x = c;
    for (size_t k = 0; k < n_hi; k++) {
      form.store(x, t.hi.data() + 8 * k);
      x = f.mul(x, step);
    }
  }
  return t;
}

// the powers k < 2^(tw_log - 1) of the primitive 2^tw_log-th root omega^(n / 2^tw_log): the butterflies' twiddles
inline std::vector<uint32_t> build_butterfly_table(const host_fr::Field& f, const uint8_t* omega, int log_n, int tw_log) {
  const FactorForm form(f);
  host_fr::Fr root = f.to_mont(host_fr::load32(omega));
  for (int i = 0; i < log_n - tw_log; i++) root = f.mul(root, root);
  const size_t n = (size_t)1 << (tw_log - 1);
  std::vector<uint32_t> w(8 * n);
  host_fr::Fr x = f.one();
  for (size_t k = 0; k < n; k++) {
    form.store(x, w.data() + 8 * k);
    x = f.mul(x, root);
  }
  return w;
}

inline bool below_r(const host_fr::Field& f, const uint8_t* x) { return !host_fr::Field::geq(host_fr::load32(x), f.modulus()); }

}  // namespace msm_fr
