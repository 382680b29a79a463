// The host side of libmsm_frlook.so that needs no HIP: the limits of include/msm_frlook.h, the size of the slot array, the arguments of the
// kernels (2^256 mod r among them), the comparison of host data with r, and the build run serially -- which is how the host form of create
// counts the distinct keys without a device (csrc/frlook_host.h launches what this plans; the host program of tests/test_frlook_host.py runs
// the same plan through the same per-lane code on the CPU).  Needs FrlookArgs and frl_insert of csrc/frlook_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "host_fr.h"

namespace frlook {

using host_fr::Field;

constexpr size_t MAX_TABLE = (size_t)1 << 24;
constexpr size_t MAX_ELEMENTS = (size_t)1 << 26;
constexpr uint32_t FLAG_MONT256 = 2u;  // MSM_FRLOOK_MONT256

inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }
inline bool all_below_r(const Field& f, const uint8_t* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!below_r(f, v + 32 * i)) return false;
  return true;
}

inline bool table_args_ok(size_t n_t, uint32_t flags) { return n_t >= 1 && n_t <= MAX_TABLE && !(flags & ~FLAG_MONT256); }
// batch rows of n scalars, stride apart: 1 <= n <= stride, batch stride <= 2^26 (without a product that wraps)
inline bool count_args_ok(size_t n, size_t batch, size_t stride) { return n >= 1 && batch >= 1 && stride >= n && stride <= MAX_ELEMENTS && batch <= MAX_ELEMENTS / stride; }

// 2 * 2^ceil(log2 n_t): the load is at most 1/2
inline uint32_t slot_count(size_t n_t) {
  uint32_t p = 1;
  while (p < n_t) p <<= 1;
  return 2 * p;
}
inline uint32_t hash_mask_of(uint32_t bits) { return bits == 0 || bits >= 32 ? 0xffffffffu : (1u << bits) - 1; }

inline FrlookArgs plan_args(const Field& f, size_t n_t, uint32_t hash_bits, bool mont) {
  FrlookArgs g;
  g.n_t = (uint32_t)n_t;
  g.slot_mask = slot_count(n_t) - 1;
  g.hash_mask = hash_mask_of(hash_bits);
  g.mont = mont ? 1u : 0u;
  const host_fr::Fr one = f.one();  // 2^256 mod r: the Montgomery form of 1
  for (int i = 0; i < 4; i++) g.t256[2 * i] = (uint32_t)one.v[i], g.t256[2 * i + 1] = (uint32_t)(one.v[i] >> 32);
  return g;
}

// k_frlook_build one lane after the other, j ascending, over keys that are all below r: the slots, and the number of distinct keys
inline size_t build_serial(const FrlookArgs& g, const uint32_t* keys, std::vector<uint32_t>& slots) {
  slots.assign((size_t)g.slot_mask + 1, FRLOOK_EMPTY);
  size_t distinct = 0;
  for (uint32_t j = 0; j < g.n_t; j++) {
    uint32_t w[8];
    frl_load_words(w, keys, j);
    distinct += frl_insert(g, keys, slots.data(), j, w) ? 1 : 0;
  }
  return distinct;
}

}  // namespace frlook
