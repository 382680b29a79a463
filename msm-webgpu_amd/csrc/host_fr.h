// Host arithmetic in the scalar field Fr of a curve, as much of it as the group FFT over the resident bases needs (msm_hip_bases_fft): the
// check that omega is a primitive 2^log_n-th root of unity, the table of its first n / 2 powers -- the twiddles the device reads -- and 1 / n.
// Values are 4 x 64-bit limbs, little-endian; products are Montgomery products with R = 2^256 (CIOS over unsigned __int128), for any odd
// modulus r < 2^255 handed over as 8 32-bit words (a curve unit's FR_R32).  At n = 2^20 the table is 2^19 products: a few milliseconds.
// Host code only; tests/host_harness/fft_harness.cpp builds it against Python's pow.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace host_fr {

struct Fr {
  uint64_t v[4];
};

class Field {
 public:
  explicit Field(const uint32_t r32[8]) {
    for (int i = 0; i < 4; i++) r_.v[i] = (uint64_t)r32[2 * i] | ((uint64_t)r32[2 * i + 1] << 32);
    uint64_t inv = 1;  // r^-1 mod 2^64 by Newton's iteration (r odd); n0 = -r^-1
    for (int i = 0; i < 6; i++) inv *= 2 - r_.v[0] * inv;
    n0_ = ~inv + 1;
    Fr x = {{1, 0, 0, 0}};  // 2^512 mod r by 512 doublings of 1: R^2, which takes a plain value into Montgomery form
    for (int i = 0; i < 512; i++) x = add(x, x);
    r2_ = x;
    one_ = mul(r2_, Fr{{1, 0, 0, 0}});
  }
  const Fr& modulus() const { return r_; }
  const Fr& one() const { return one_; }  // Montgomery form of 1

  static bool geq(const Fr& a, const Fr& b) {
    for (int i = 3; i >= 0; i--)
      if (a.v[i] != b.v[i]) return a.v[i] > b.v[i];
    return true;
  }
  static bool equal(const Fr& a, const Fr& b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }
  static Fr sub_raw(const Fr& a, const Fr& b) {  // a - b over the integers, a >= b
    Fr d;
    uint64_t borrow = 0;
    for (int i = 0; i < 4; i++) {
      const unsigned __int128 t = (unsigned __int128)a.v[i] - b.v[i] - borrow;
      d.v[i] = (uint64_t)t;
      borrow = (uint64_t)(t >> 64) & 1u;
    }
    return d;
  }
  Fr add(const Fr& a, const Fr& b) const {  // a, b < r < 2^255: the sum fits
    Fr s;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (unsigned __int128)a.v[i] + b.v[i];
      s.v[i] = (uint64_t)c;
      c >>= 64;
    }
    return geq(s, r_) ? sub_raw(s, r_) : s;
  }
  // a b / R mod r for a, b < r
  Fr mul(const Fr& a, const Fr& b) const {
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
      unsigned __int128 c = 0;
      for (int j = 0; j < 4; j++) {
        c += (unsigned __int128)a.v[j] * b.v[i] + t[j];
        t[j] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[4] = (uint64_t)c;
      t[5] = (uint64_t)(c >> 64);
      const uint64_t m = t[0] * n0_;
      c = (unsigned __int128)m * r_.v[0] + t[0];
      c >>= 64;
      for (int j = 1; j < 4; j++) {
        c += (unsigned __int128)m * r_.v[j] + t[j];
        t[j - 1] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[3] = (uint64_t)c;
      t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Fr x = {{t[0], t[1], t[2], t[3]}};
    return (t[4] || geq(x, r_)) ? sub_raw(x, r_) : x;
  }
  Fr to_mont(const Fr& plain) const { return mul(plain, r2_); }
  Fr from_mont(const Fr& x) const { return mul(x, Fr{{1, 0, 0, 0}}); }

 private:
  Fr r_, r2_, one_;
  uint64_t n0_;
};

inline Fr load32(const uint8_t b[32]) {  // 32 little-endian bytes
  Fr x;
  for (int i = 0; i < 4; i++) {
    x.v[i] = 0;
    for (int k = 7; k >= 0; k--) x.v[i] = (x.v[i] << 8) | b[8 * i + k];
  }
  return x;
}
inline void store_words(const Fr& x, uint32_t w[8]) {
  for (int i = 0; i < 4; i++) {
    w[2 * i] = (uint32_t)x.v[i];
    w[2 * i + 1] = (uint32_t)(x.v[i] >> 32);
  }
}

// omega (canonical, 32 bytes) is a primitive 2^log_n-th root of unity mod r: omega < r and, for log_n >= 1, omega^(n / 2) == r - 1 (log_n - 1
// squarings); for log_n == 0, omega == 1.
inline bool is_primitive_root(const Field& f, const uint8_t omega[32], int log_n) {
  const Fr w = load32(omega);
  if (log_n < 0 || Field::geq(w, f.modulus())) return false;
  if (log_n == 0) return Field::equal(w, Fr{{1, 0, 0, 0}});
  Fr x = f.to_mont(w);
  for (int i = 0; i < log_n - 1; i++) x = f.mul(x, x);
  return Field::equal(f.from_mont(x), Field::sub_raw(f.modulus(), Fr{{1, 0, 0, 0}}));
}

// the n / 2 twiddles omega^j, j < 2^(log_n - 1), as canonical scalars of 8 words each (log_n >= 1)
inline void twiddle_table(const Field& f, const uint8_t omega[32], int log_n, std::vector<uint32_t>& out) {
  const size_t half = (size_t)1 << (log_n - 1);
  out.resize(half * 8);
  const Fr w = f.to_mont(load32(omega));
  Fr x = f.one();
  for (size_t j = 0; j < half; j++) {
    store_words(f.from_mont(x), out.data() + 8 * j);
    x = f.mul(x, w);
  }
}

// 1 / n mod r for n = 2^log_n dividing r - 1 (which a primitive n-th root of unity shows): r - (r - 1) / n, exact, no inversion
inline void inverse_of_n(const Field& f, int log_n, uint32_t out[8]) {
  Fr q = Field::sub_raw(f.modulus(), Fr{{1, 0, 0, 0}});
  for (int s = 0; s < log_n; s++) {  // (log_n <= 32 < 64: limb-wise shifts by one)
    for (int i = 0; i < 4; i++) q.v[i] = (q.v[i] >> 1) | (i < 3 ? q.v[i + 1] << 63 : 0);
  }
  store_words(Field::sub_raw(f.modulus(), q), out);
}

}  // namespace host_fr
