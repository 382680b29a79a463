// Lookup arguments over the scalar field (libmsm_frlook.so, include/msm_frlook.h), written once and instantiated per field: a unit
// (csrc/frlook_<name>.hip) includes the field's constants (fr_<name>_constants.h) and then this file, inside its own MSM_FIELD_NS.  Everything a
// lane does is an FRL_HD function, which the kernels at the bottom call and which the host program of tests/test_frlook_host.py runs serially on
// the CPU; the atomics go through the small shim below, which has a host definition.
//
// This is the one library of the engine that does no field arithmetic: a key is the 32 bytes as stored (canonical or a 2^256 mod r, both
// bijections of the field), and of the field only r itself is needed -- the comparison of every element read with r -- and 2^256 mod r, for the
// count k written as a scalar of the data's form.  csrc/fq29.h is not included.
//
// The hash table.  slots[2 * 2^ceil(log2 n_t)] words, each FRLOOK_EMPTY or a TABLE INDEX j; load <= 1/2; linear probing from
// hash(key) & slot_mask, where hash is MurmurHash3's 32-bit function over the eight words of the key, so that range tables (which differ in
// word 0 only) and mont-form data (which differ everywhere) spread alike.  Invariants, whatever the order in which the lanes arrive:
//   - a slot never returns to EMPTY, and the index it holds only ever changes to a SMALLER index of the SAME key;
//   - so a lane that passed a slot (another key sits there) would pass it again at any later time, every copy of a key stops at the same slot,
//     a key owns exactly one slot, and no EMPTY slot lies between a key's first probe and its slot;
//   - after the kernel boundary that slot holds the lowest index of the key.
//
//   k_frlook_build   one lane per table entry j: load t[j], compare with r, then per probe atomicCAS(slot, EMPTY, j) at agent scope.  Claimed:
//                    done, and the key is a new distinct value.  Else read the occupant j', compare the 32 bytes t[j'] with t[j] (the keys are
//                    the handle's own copy, written before the launch: plain loads): equal -> atomicMin(slot, j) where j < j', done; different
//                    -> next slot.  No lane waits for another; at most slot_mask + 1 probes, and an EMPTY slot exists because load <= 1/2.
//   k_frlook_count   one lane per looked-up element e = row n + i: load f[row stride + i], compare with r, probe with PLAIN loads (the build
//                    is a kernel boundary away) until the key or EMPTY, write idx[e].  Then the wave aggregates: readfirstlane on j, ballot of
//                    the lanes with that j, ONE atomicAdd(counts[j], popcount) from the first of them, until no lane is left.  A wave takes
//                    FRLOOK_CHUNKS chunks of 64 elements and carries ONE group from chunk to chunk without adding it to memory (frl_credit):
//                    a column of padding (every lane the same j) is one atomic per wave, however many chunks; 64 different j are 64 per
//                    chunk.  `missing` is one 64-bit add per wave and chunk,
//                    `first_missing` one 64-bit atomicMin per wave and chunk (the first missing lane has the chunk's lowest e).  Integer adds
//                    and minima commute: the bytes do not depend on the order of arrival.
//   k_frlook_finish  one lane per table entry: counts[j] -> counts_out[j] and/or m_out[j], the scalar k (canonical) or k 2^256 mod r
//                    (MONT256): 27 doublings and conditional additions of 2^256 mod r in eight 32-bit words (k <= 2^26, r < 2^255).
// counts and the result words are cleared by the host on the stream before each call (csrc/frlook_host.h).
//
// No LDS, no scratch; no kernel waits for another workgroup.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#if defined(FQ_CHECK)
#include <cassert>
#define FRL_ASSERT(c) assert(c)
#else
#define FRL_ASSERT(c) ((void)0)
#endif

#define FRLOOK_THREADS 256
#define FRLOOK_CHUNKS 4            // count: chunks of FRLOOK_THREADS elements per workgroup
#define FRLOOK_EMPTY 0xffffffffu    // slots: nobody here
#define FRLOOK_MISSING 0xffffffffu  // idx: not in the table
// the result buffer: eight words, one copy
#define FRLOOK_RESULT_WORDS 8
#define FRLOOK_RES_ERR 0       // a value that is not below r was read
#define FRLOOK_RES_DISTINCT 1  // build: the slots claimed
#define FRLOOK_RES_MISSING 2   // count: 64 bits (words 2, 3)
#define FRLOOK_RES_FIRST 4     // count: 64 bits (words 4, 5); cleared to all ones

#if defined(__HIPCC__)
#define FRL_HD __host__ __device__ __forceinline__
#else
#define FRL_HD inline
#endif

// what the host plans (csrc/frlook_plan.h) -- plain data, the same for every field's unit
struct FrlookArgs {
  uint32_t n_t;        // table entries, >= 1
  uint32_t slot_mask;  // slots - 1, slots = 2 * 2^ceil(log2 n_t)
  uint32_t hash_mask;  // the bits of the hash in use (the test hook keeps the low ones), all 32 by design
  uint32_t mont;       // the data are a 2^256 mod r
  uint32_t t256[8];    // 2^256 mod r
};

// ---- the atomics: device instructions at agent scope, plain statements on the host (one lane after the other) -------------------------------------
FRL_HD uint32_t frl_atomic_cas(uint32_t* p, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, v);
#else
  const uint32_t was = *p;
  if (was == expect) *p = v;
  return was;
#endif
}
FRL_HD void frl_atomic_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}
FRL_HD void frl_atomic_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, v);
#else
  *p += v;
#endif
}
FRL_HD void frl_atomic_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}
// the 64-bit words of the result buffer (8-byte aligned: words 2 and 4 of a buffer the allocator aligned)
FRL_HD void frl_atomic_add64(uint32_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
#else
  uint64_t x;
  memcpy(&x, p, 8);
  x += v;
  memcpy(p, &x, 8);
#endif
}
FRL_HD void frl_atomic_min64(uint32_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
#else
  uint64_t x;
  memcpy(&x, p, 8);
  if (v < x) memcpy(p, &v, 8);
#endif
}

// ---- the wave: lanes that add to the same word add once ----------------------------------------------------------------------------------------------
// *p += the number of lanes with `flag` (every lane of the wave that is still running comes here)
FRL_HD void frl_wave_add(uint32_t* p, bool flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned long long set = __ballot(flag);
  if (flag && (int)__lane_id() == __ffsll(set) - 1) atomicAdd(p, (uint32_t)__popcll(set));
#else
  if (flag) *p += 1;
#endif
}
// The wave's deferred group: pend.cnt matches of table index pend.j that have not been added to memory yet.  On the device the pair is the same
// in every lane of the wave (it is made of ballots, and every lane of the wave stays in the kernel to its end); the host adds at once.
struct FrlPending {
  uint32_t j, cnt;
};
FRL_HD void frl_flush(uint32_t* counts, FrlPending& pend) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (pend.cnt && __lane_id() == 0) atomicAdd(counts + pend.j, pend.cnt);
#else
  (void)counts;
#endif
  pend.j = FRLOOK_MISSING, pend.cnt = 0;
}
// counts[j] += 1 for every lane with `found` (the whole wave comes here together).  The lanes whose j is the deferred group's only raise its
// count; where no lane is, the group is flushed -- one atomic -- and the group of the first lane that found something is deferred in its place:
// a column's hot value (padding, zeros) costs one atomic per wave and FRLOOK_CHUNKS chunks, not one per chunk.  Every other distinct j of the
// wave is one atomic.
FRL_HD void frl_credit(uint32_t* counts, uint32_t j, bool found, FrlPending& pend) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned long long hot = __ballot(found && j == pend.j);  // (nothing deferred: pend.j is FRLOOK_MISSING, which no lane found)
  bool todo = found && j != pend.j;
  if (hot) {
    pend.cnt += (uint32_t)__popcll(hot);
  } else {
    const unsigned long long rest = __ballot(todo);
    if (rest) {
      frl_flush(counts, pend);
      pend.j = (uint32_t)__shfl((int)j, __ffsll(rest) - 1);
      pend.cnt = (uint32_t)__popcll(__ballot(todo && j == pend.j));
      todo = todo && j != pend.j;
    }
  }
  while (todo) {  // (the lanes that are done have left the loop: readfirstlane and ballot see the others only)
    const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
    const bool mine = j == lead;
    const unsigned long long same = __ballot(mine);
    if (mine) {
      if ((int)__lane_id() == __ffsll(same) - 1) atomicAdd(counts + lead, (uint32_t)__popcll(same));
      todo = false;
    }
  }
#else
  (void)pend;
  if (found) counts[j] += 1;
#endif
}
// the elements that are not in the table: their number, and the lowest flat index e among them (e grows with the lane)
FRL_HD void frl_report_missing(uint32_t* res, bool miss, uint64_t e) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned long long set = __ballot(miss);
  if (miss && (int)__lane_id() == __ffsll(set) - 1) {
    frl_atomic_add64(res + FRLOOK_RES_MISSING, (uint64_t)__popcll(set));
    frl_atomic_min64(res + FRLOOK_RES_FIRST, e);
  }
#else
  if (miss) {
    frl_atomic_add64(res + FRLOOK_RES_MISSING, 1);
    frl_atomic_min64(res + FRLOOK_RES_FIRST, e);
  }
#endif
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------------------------------
FRL_HD void frl_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FRL_HD void frl_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
FRL_HD bool frl_equal(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= a[i] ^ b[i];
  return d == 0;
}
FRL_HD uint32_t frl_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
// MurmurHash3_x86_32 of the 32 bytes (seed 0x9e3779b9), then the bits in use
FRL_HD uint32_t frl_hash(const uint32_t w[8], uint32_t hash_mask) {
  uint32_t h = 0x9e3779b9u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t k = w[i] * 0xcc9e2d51u;
    k = frl_rotl(k, 15) * 0x1b873593u;
    h = frl_rotl(h ^ k, 13) * 5u + 0xe6546b64u;
  }
  h ^= 32u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h & hash_mask;
}

// ---- build and find -----------------------------------------------------------------------------------------------------------------------------------------
// entry j, whose key is w, into the slots: true where the lane claimed an empty slot (the key is a new distinct value)
FRL_HD bool frl_insert(const FrlookArgs& g, const uint32_t* keys, uint32_t* slots, uint32_t j, const uint32_t w[8]) {
  uint32_t s = frl_hash(w, g.hash_mask) & g.slot_mask;
  for (uint32_t probe = 0; probe <= g.slot_mask; probe++) {
    const uint32_t was = frl_atomic_cas(slots + s, FRLOOK_EMPTY, j);
    if (was == FRLOOK_EMPTY) return true;
    FRL_ASSERT(was < g.n_t && was != j);
    uint32_t o[8];
    frl_load_words(o, keys, was);
    if (frl_equal(o, w)) {  // whoever sits here has this key, now and later: the smaller index stays
      if (j < was) frl_atomic_min(slots + s, j);
      return false;
    }
    s = (s + 1) & g.slot_mask;
  }
  FRL_ASSERT(!"the slots are full");  // (load <= 1/2: not reached)
  return false;
}
// the lowest index of the key w, or FRLOOK_MISSING (plain loads: after the build's kernel boundary)
FRL_HD uint32_t frl_find(const FrlookArgs& g, const uint32_t* keys, const uint32_t* slots, const uint32_t w[8]) {
  uint32_t s = frl_hash(w, g.hash_mask) & g.slot_mask;
  for (uint32_t probe = 0; probe <= g.slot_mask; probe++) {
    const uint32_t j = slots[s];
    if (j == FRLOOK_EMPTY) return FRLOOK_MISSING;
    FRL_ASSERT(j < g.n_t);
    uint32_t o[8];
    frl_load_words(o, keys, j);
    if (frl_equal(o, w)) return j;
    s = (s + 1) & g.slot_mask;
  }
  return FRLOOK_MISSING;  // (not reached)
}

// ---- the count as a scalar --------------------------------------------------------------------------------------------------------------------------------
// a + b mod r for a, b < r < 2^255 (the sum fits eight words)
FRL_HD void frl_add_mod(uint32_t a[8], const uint32_t b[8], const uint32_t r[8]) {
  uint32_t s[8], d[8];
  uint64_t carry = 0;
  int64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    carry += (uint64_t)a[i] + b[i];
    s[i] = (uint32_t)carry;
    carry >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    borrow += (int64_t)s[i] - (int64_t)r[i];
    d[i] = (uint32_t)borrow;
    borrow >>= 32;
  }
  FRL_ASSERT(carry == 0);
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = borrow ? s[i] : d[i];  // (a borrow: s < r)
}
// k (canonical) or k 2^256 mod r (mont), k < 2^27
FRL_HD void frl_count_scalar(uint32_t out[8], uint32_t k, const FrlookArgs& g, const uint32_t r[8]) {
  FRL_ASSERT(k < (1u << 27));
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (!g.mont || k == 0) {
    out[0] = k;
    return;
  }
#pragma unroll 1
  for (int bit = 26; bit >= 0; bit--) {
    frl_add_mod(out, out, r);
    if ((k >> bit) & 1u) frl_add_mod(out, g.t256, r);
  }
}

namespace MSM_FIELD_NS {

static_assert(FQ_P32[7] < 0x80000000u, "r < 2^255: a sum of two values below r fits eight words");

FRL_HD bool frl_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}

// build, lane j < n_t: false where t[j] is not below r (the entry is then left out); won: the lane claimed a slot
FRL_HD bool frl_build_lane(const FrlookArgs& g, const uint32_t* keys, uint32_t* slots, uint32_t j, bool& won) {
  uint32_t w[8];
  frl_load_words(w, keys, j);
  won = false;
  if (!frl_below_r(w)) return false;
  won = frl_insert(g, keys, slots, j, w);
  return true;
}
// count, the element at f[at]: its index or FRLOOK_MISSING; false (and FRLOOK_MISSING) where the element is not below r
FRL_HD bool frl_count_lane(const FrlookArgs& g, const uint32_t* keys, const uint32_t* slots, const uint32_t* f, size_t at, uint32_t& j) {
  uint32_t w[8];
  frl_load_words(w, f, at);
  j = FRLOOK_MISSING;
  if (!frl_below_r(w)) return false;
  j = frl_find(g, keys, slots, w);
  return true;
}
// what one looked-up element e does once it has its j (in the kernel: the whole wave together, the lanes behind the last element with
// live = false)
FRL_HD void frl_count_tail(uint32_t* counts, uint32_t* idx_out, uint32_t* res, uint64_t e, uint32_t j, bool live, bool ok, FrlPending& pend) {
  if (live && idx_out) idx_out[e] = j;
  frl_credit(counts, j, live && ok && j != FRLOOK_MISSING, pend);
  frl_report_missing(res, live && ok && j == FRLOOK_MISSING, e);
  if (live && !ok) frl_atomic_or(res + FRLOOK_RES_ERR, 1u);
}
// finish, lane j < n_t
FRL_HD void frl_finish_lane(const FrlookArgs& g, const uint32_t* counts, uint32_t j, uint32_t* m_out, uint32_t* counts_out) {
  const uint32_t k = counts[j];
  if (counts_out) counts_out[j] = k;
  if (m_out) {
    uint32_t w[8];
    frl_count_scalar(w, k, g, FQ_P32);
    frl_store_words(m_out, j, w);
  }
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(FRLOOK_THREADS) k_frlook_build(const uint32_t* keys, uint32_t* slots, const FrlookArgs g, uint32_t* res) {
  const uint32_t j = blockIdx.x * FRLOOK_THREADS + threadIdx.x;
  bool won = false;
  if (j < g.n_t && !frl_build_lane(g, keys, slots, j, won)) atomicOr(res + FRLOOK_RES_ERR, 1u);
  frl_wave_add(res + FRLOOK_RES_DISTINCT, won);
}

// a workgroup owns FRLOOK_CHUNKS chunks of 256 consecutive elements e = row n + i < total = batch n; a wave 64 consecutive ones of each
__global__ void __launch_bounds__(FRLOOK_THREADS) k_frlook_count(const uint32_t* keys, const uint32_t* slots, uint32_t* counts, uint32_t* idx_out, const uint32_t* f,
                                                                 uint32_t n, uint32_t total, size_t stride, const FrlookArgs g, uint32_t* res) {
  FrlPending pend = {FRLOOK_MISSING, 0};
#pragma unroll 1
  for (uint32_t k = 0; k < FRLOOK_CHUNKS; k++) {
    const uint32_t e = (blockIdx.x * FRLOOK_CHUNKS + k) * FRLOOK_THREADS + threadIdx.x;  // (total <= 2^26: no wrap)
    const bool live = e < total;
    uint32_t j = FRLOOK_MISSING;
    bool ok = true;
    if (live) {
      const uint32_t row = e / n, i = e - row * n;
      ok = frl_count_lane(g, keys, slots, f, (size_t)row * stride + i, j);
    }
    frl_count_tail(counts, idx_out, res, e, j, live, ok, pend);
  }
  frl_flush(counts, pend);
}

__global__ void __launch_bounds__(FRLOOK_THREADS) k_frlook_finish(const uint32_t* counts, uint32_t* m_out, uint32_t* counts_out, const FrlookArgs g) {
  const uint32_t j = blockIdx.x * FRLOOK_THREADS + threadIdx.x;
  if (j < g.n_t) frl_finish_lane(g, counts, j, m_out, counts_out);
}

inline void frlook_launch_build(hipStream_t st, const uint32_t* keys, uint32_t* slots, const FrlookArgs* g, uint32_t* res) {
  hipLaunchKernelGGL(k_frlook_build, dim3((g->n_t + FRLOOK_THREADS - 1) / FRLOOK_THREADS), dim3(FRLOOK_THREADS), 0, st, keys, slots, *g, res);
}
inline void frlook_launch_count(hipStream_t st, const uint32_t* keys, const uint32_t* slots, uint32_t* counts, uint32_t* idx_out, const uint32_t* f, uint32_t n, uint32_t total,
                                size_t stride, const FrlookArgs* g, uint32_t* res) {
  hipLaunchKernelGGL(k_frlook_count, dim3((total + FRLOOK_THREADS * FRLOOK_CHUNKS - 1) / (FRLOOK_THREADS * FRLOOK_CHUNKS)), dim3(FRLOOK_THREADS), 0, st, keys, slots, counts, idx_out, f, n, total, stride, *g, res);
}
inline void frlook_launch_finish(hipStream_t st, const uint32_t* counts, uint32_t* m_out, uint32_t* counts_out, const FrlookArgs* g) {
  hipLaunchKernelGGL(k_frlook_finish, dim3((g->n_t + FRLOOK_THREADS - 1) / FRLOOK_THREADS), dim3(FRLOOK_THREADS), 0, st, counts, m_out, counts_out, *g);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS

#if defined(__HIPCC__)
// what the host code (csrc/frlook_host.h) knows of a field's unit
struct FrlookOps {
  const uint32_t* r32;
  void (*build)(hipStream_t st, const uint32_t* keys, uint32_t* slots, const FrlookArgs* g, uint32_t* res);
  void (*count)(hipStream_t st, const uint32_t* keys, const uint32_t* slots, uint32_t* counts, uint32_t* idx_out, const uint32_t* f, uint32_t n, uint32_t total, size_t stride,
                const FrlookArgs* g, uint32_t* res);
  void (*finish)(hipStream_t st, const uint32_t* counts, uint32_t* m_out, uint32_t* counts_out, const FrlookArgs* g);
};
#endif
