// What a handle and a call of libmsm_frhash.so are made of before any device is asked for: the argument checks, the table of constants in the
// kernel's representation, the kernel's arguments and the levels of a tree.  Pure host code, no HIP (csrc/frhash_host.h launches what this
// plans; the host program of tests/test_frhash_host.py runs the same plan through the same per-lane code on the CPU).  Needs FrhashArgs of
// csrc/frhash_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "../../include/msm_frhash.h"
#include "host_fr.h"

static_assert(FRHASH_MAX_WIDTH == MSM_FRHASH_MAX_WIDTH && FRHASH_MAX_FULL_ROUNDS == MSM_FRHASH_MAX_FULL_ROUNDS && FRHASH_MAX_PARTIAL_ROUNDS == MSM_FRHASH_MAX_PARTIAL_ROUNDS,
              "csrc/frhash_kernels.h and include/msm_frhash.h disagree on the limits of a permutation");

namespace msm_frhash_plan {

using host_fr::Field;
using host_fr::Fr;

constexpr size_t MAX_ELEMENTS = (size_t)MSM_FRHASH_MAX_ELEMENTS;
constexpr uint32_t KNOWN_FLAGS = MSM_FRHASH_MONT256;                            // of a call
constexpr uint32_t CREATE_FLAGS = MSM_FRHASH_MONT256 | MSM_FRHASH_POSEIDON2;  // of msm_frhash_create

inline Fr pow2(const Field& f, int k) {  // 2^k mod r
  Fr x = {{1, 0, 0, 0}};
  for (int i = 0; i < k; i++) x = f.add(x, x);
  return x;
}
inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }
inline bool all_below_r(const Field& f, const uint8_t* c, size_t count) {
  for (size_t i = 0; i < count; i++)
    if (!below_r(f, c + 32 * i)) return false;
  return true;
}
// c R mod r, R = 2^261, for a canonical c: the kernel's form of a constant
inline void to_kernel(const Field& f, const uint8_t c[32], uint32_t w[8]) { host_fr::store_words(f.mul(f.to_mont(host_fr::load32(c)), pow2(f, 261)), w); }

// the kind of handle the flags of msm_frhash_create ask for (FRHASH_KIND_*)
inline uint32_t kind_of(uint32_t flags) { return (flags & MSM_FRHASH_POSEIDON2) ? FRHASH_KIND_POSEIDON2 : FRHASH_KIND_POSEIDON; }
inline bool poseidon2_width(uint32_t t) { return t == 2 || t == 3 || t == 4 || t == 8 || t == 12; }  // the widths Poseidon2 defines
// the shape of a handle; flags: those of msm_frhash_create
inline bool shape_ok(uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, uint32_t alpha, uint32_t flags) {
  return t >= 2 && t <= MSM_FRHASH_MAX_WIDTH && full_rounds >= 2 && full_rounds <= MSM_FRHASH_MAX_FULL_ROUNDS && full_rounds % 2 == 0 &&
         partial_rounds <= MSM_FRHASH_MAX_PARTIAL_ROUNDS && alpha == 5 && !(flags & ~CREATE_FLAGS) && (kind_of(flags) != FRHASH_KIND_POSEIDON2 || poseidon2_width(t));
}
// how many scalars `round_constants` and `mds` hold: Poseidon t a round and the t x t matrix; Poseidon2 t an external round, one an internal
// round, and the t of mu
inline size_t constants_of(uint32_t kind, uint32_t t, uint32_t full_rounds, uint32_t partial_rounds) {
  return kind == FRHASH_KIND_POSEIDON2 ? (size_t)full_rounds * t + partial_rounds : (size_t)(full_rounds + partial_rounds) * t;
}
inline size_t matrix_of(uint32_t kind, uint32_t t) { return kind == FRHASH_KIND_POSEIDON2 ? t : (size_t)t * t; }
inline size_t table_words(uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, uint32_t kind = FRHASH_KIND_POSEIDON) {
  return FRHASH_TAB_RC + (size_t)8 * (constants_of(kind, t, full_rounds, partial_rounds) + matrix_of(kind, t));
}

// the table: R^2 / F and F for both data forms, then the round constants and the matrix (Poseidon2: mu) as c R (constants that passed all_below_r)
inline void plan_table(const Field& f, uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, const uint8_t* rc, const uint8_t* mds, std::vector<uint32_t>& words,
                       uint32_t kind = FRHASH_KIND_POSEIDON) {
  const size_t n_rc = constants_of(kind, t, full_rounds, partial_rounds), n_m = matrix_of(kind, t);
  words.assign(table_words(t, full_rounds, partial_rounds, kind), 0);
  host_fr::store_words(pow2(f, 2 * 261), words.data() + FRHASH_TAB_IN);
  host_fr::store_words(pow2(f, 0), words.data() + FRHASH_TAB_OUT);
  host_fr::store_words(pow2(f, 2 * 261 - 256), words.data() + FRHASH_TAB_MONT + FRHASH_TAB_IN);
  host_fr::store_words(pow2(f, 256), words.data() + FRHASH_TAB_MONT + FRHASH_TAB_OUT);
  for (size_t i = 0; i < n_rc; i++) to_kernel(f, rc + 32 * i, words.data() + FRHASH_TAB_RC + 8 * i);
  for (size_t i = 0; i < n_m; i++) to_kernel(f, mds + 32 * i, words.data() + FRHASH_TAB_RC + 8 * (n_rc + i));
}

inline FrhashArgs plan_args(uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, size_t n, uint32_t flags, uint32_t tile, uint32_t kind = FRHASH_KIND_POSEIDON) {
  FrhashArgs g;
  memset(&g, 0, sizeof g);
  g.t = t, g.full_rounds = full_rounds, g.partial_rounds = partial_rounds, g.n = (uint32_t)n;
  g.form = (flags & MSM_FRHASH_MONT256) ? FRHASH_TAB_MONT : 0;
  g.tile = tile ? tile : FRHASH_THREADS;
  g.kind = kind;
  return g;
}
inline unsigned blocks_of(const FrhashArgs& g) { return (unsigned)((g.n + g.tile - 1) / g.tile); }

inline bool permute_args_ok(uint32_t t, size_t n, uint32_t flags) { return !(flags & ~KNOWN_FLAGS) && n >= 1 && n <= MAX_ELEMENTS / t; }
// the sponge's shape; the span of a: (rows - 1) stride + len
inline bool hash_args_ok(uint32_t t, size_t rows, size_t len, size_t stride, uint32_t capacity_at, uint32_t out_at, uint32_t flags) {
  if ((flags & ~KNOWN_FLAGS) || capacity_at >= t || out_at >= t) return false;
  if (rows < 1 || len < 1 || stride < len || rows > MAX_ELEMENTS || stride > MAX_ELEMENTS) return false;
  return (rows - 1) <= (MAX_ELEMENTS - len) / stride;
}
// capacity (NULL: 0) as capacity R into the arguments; false where it is not below r
inline bool plan_capacity(const Field& f, const uint8_t* capacity, FrhashArgs& g) {
  const uint8_t zero[32] = {0};
  if (capacity && !below_r(f, capacity)) return false;
  to_kernel(f, capacity ? capacity : zero, g.capacity);
  return true;
}

// The levels of a tree of arity A = t - 1 over n_leaves = A^k leaves (A = 1: a chain of n_leaves levels over one leaf): the number of nodes of
// every level above the leaves, the lowest first.  false where n_leaves is no such number.
inline bool plan_levels(uint32_t t, size_t n_leaves, std::vector<size_t>& levels) {
  const size_t a = t - 1;
  levels.clear();
  if (a == 1) {
    if (n_leaves < 1 || n_leaves > MSM_FRHASH_MAX_LEVELS) return false;
    levels.assign(n_leaves, 1);
    return true;
  }
  if (n_leaves < a || n_leaves > MAX_ELEMENTS) return false;
  for (size_t n = n_leaves; n > 1; n /= a) {
    if (n % a) return false;
    levels.push_back(n / a);
  }
  return true;
}
inline size_t node_count(const std::vector<size_t>& levels) {
  size_t total = 0;
  for (size_t n : levels) total += n;
  return total;
}
inline size_t leaf_count(uint32_t t, size_t n_leaves) { return t == 2 ? 1 : n_leaves; }

}  // namespace msm_frhash_plan
