// What a call of libmsm_frgate.so is made of before any device is asked for: the argument checks, the reduction of every rotation to an offset
// and the term records with their constants.  Pure host code, no HIP (csrc/frgate_host.h launches what this plans; the host program of
// tests/test_frgate_host.py runs the same plan through the same per-lane code on the CPU).  Needs FrgateArgs of csrc/frgate_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "../../include/msm_frgate.h"
#include "host_fr.h"

static_assert(FRGATE_MAX_DEGREE == MSM_FRGATE_MAX_DEGREE && FRGATE_MAX_TERMS == MSM_FRGATE_MAX_TERMS && FRGATE_MAX_ROWS == MSM_FRGATE_MAX_ROWS,
              "csrc/frgate_kernels.h and include/msm_frgate.h disagree on the limits of a call");
static_assert(FRGATE_MAX_DEGREE == 8 && sizeof(msm_frgate_term) == 100, "msm_frgate_term holds eight rows and eight rotations in 100 bytes");

namespace msm_frgate {

using host_fr::Field;
using host_fr::Fr;

constexpr size_t MAX_ELEMENTS = (size_t)1 << 26;
constexpr uint32_t KNOWN_FLAGS = MSM_FRGATE_MONT256 | MSM_FRGATE_ACCUMULATE;

inline Fr pow2(const Field& f, int k) {  // 2^k mod r
  Fr x = {{1, 0, 0, 0}};
  for (int i = 0; i < k; i++) x = f.add(x, x);
  return x;
}
inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }
inline bool power_of_two(size_t n) { return n && !(n & (n - 1)); }

// the element offset of a rotation: rot step mod n, in [0, n); n a power of two <= 2^26, 1 <= step <= n, so the product fits 64 signed bits
inline uint32_t offset_of(int32_t rot, size_t step, size_t n) {
  const int64_t m = (int64_t)n;
  const int64_t p = ((int64_t)rot * (int64_t)step) % m;
  return (uint32_t)(p < 0 ? p + m : p);
}

// everything about the shape, the flags and the terms that can be wrong (the pointers are the caller's to check): true where the call is in range
inline bool args_ok(const Field& f, size_t n, size_t batch, size_t stride, const msm_frgate_term* terms, size_t num_terms, size_t step, bool has_scale, size_t scale_len,
                    uint32_t flags) {
  if (flags & ~KNOWN_FLAGS) return false;
  if (!power_of_two(n) || n > MAX_ELEMENTS) return false;
  if (batch < 1 || batch > MSM_FRGATE_MAX_ROWS || stride < n || stride > MAX_ELEMENTS || batch > MAX_ELEMENTS / stride) return false;
  if (step < 1 || step > n) return false;
  if (has_scale && (!power_of_two(scale_len) || scale_len > n)) return false;
  if (!terms || num_terms < 1 || num_terms > MSM_FRGATE_MAX_TERMS) return false;
  for (size_t t = 0; t < num_terms; t++) {
    if (terms[t].degree < 1 || terms[t].degree > MSM_FRGATE_MAX_DEGREE || !below_r(f, terms[t].coeff)) return false;
    for (uint32_t j = 0; j < terms[t].degree; j++)
      if (terms[t].rows[j] >= batch) return false;
  }
  return true;
}

// the kernel's arguments and words[FRGATE_TERM_WORDS t ..]: the term's constant coeff R^d / F^(d-1) -- times R / F with a scale --, its degree,
// and per factor the first element of its row and its offset (arguments that passed args_ok)
inline FrgateArgs plan_apply(const Field& f, size_t n, size_t stride, const msm_frgate_term* terms, size_t num_terms, size_t step, bool has_scale, size_t scale_len,
                             uint32_t flags, std::vector<uint32_t>& words) {
  FrgateArgs g;
  memset(&g, 0, sizeof g);
  g.n = (uint32_t)n, g.num_terms = (uint32_t)num_terms;
  g.has_scale = has_scale, g.scale_mask = has_scale ? (uint32_t)(scale_len - 1) : 0;
  g.accumulate = (flags & MSM_FRGATE_ACCUMULATE) != 0;
  const bool mont = (flags & MSM_FRGATE_MONT256) != 0;
  words.assign(num_terms * FRGATE_TERM_WORDS, 0);
  for (size_t t = 0; t < num_terms; t++) {
    const int d = (int)terms[t].degree + (has_scale ? 1 : 0);  // (R^d / F^(d-1): 2^(261 d), or 2^(5 d + 256) for F = 2^256)
    uint32_t* w = words.data() + FRGATE_TERM_WORDS * t;
    host_fr::store_words(f.mul(f.to_mont(host_fr::load32(terms[t].coeff)), pow2(f, mont ? 5 * d + 256 : 261 * d)), w);
    w[FRGATE_TERM_DEGREE] = terms[t].degree;
    for (uint32_t j = 0; j < terms[t].degree; j++) {
      w[FRGATE_TERM_BASE + j] = (uint32_t)(terms[t].rows[j] * stride);
      w[FRGATE_TERM_OFF + j] = offset_of(terms[t].rots[j], step, n);
    }
  }
  return g;
}

}  // namespace msm_frgate
