// Memory-checking columns (libmsm_frmem.so, include/msm_frmem.h): a stable argsort of integer keys and, from it, the access counters of a memory
// argument.  One translation unit, no field: keys are unsigned words of 4 or 8 bytes.  Everything a lane does is an FRM_HD function, which the
// kernels at the bottom call and which the host program of tests/test_frmem_host.py runs lane by lane and phase by phase on the CPU.
//
// The sort: least significant digit first, 8 bits per pass, payload the 32-bit index (implicit in the first pass), (key, index) ping-pong between
// two buffers.  A pass is
//   k_frmem_hist      one workgroup per tile of `tile` keys (1024 by design): the tile's 256 digit counts -> hist[digit][tile].  The first pass
//                     also checks every key against the caller's bound and sets the error word: every later launch that writes reads it first.
//   k_frmem_sums /    the exclusive prefix sums of those 256 * tiles words, level by level over tiles of `tile` words exactly as
//   k_frmem_scan      csrc/frcol_kernels.h scans its counts: sums upwards, scans from the top level down, in place.
//   k_frmem_scatter   the workgroup reads its tile again and puts every key at base[digit][tile] + its stable rank among the tile's equal digits.
// The rank inside a tile depends on positions only.  Wave w of the workgroup owns positions w * 256 .. w * 256 + 255 of the tile, in four rounds of
// 64; in a round, the lanes with the same digit find one another by eight ballots (one per digit bit), a lane's rank among them is the
// population count of the lanes below it, and the lowest of them adds the group's size to cnt[w][digit] in LDS -- one writer per word, no atomic.
// After the rounds lane d turns column d of cnt into the waves' starting offsets, in wave order.
//
// access: the sort, then ONE inclusive max-scan over the sorted keys of (is head of a run, its position) -- the sum counts the heads, the max is
// the run's start -- through the same two scan kernels, then k_frmem_access, one lane per sorted position k: rank[perm[k]] = k - start[k],
// prev[perm[k]] = perm[k - 1] inside a run, and at a run's tail counts[key] and last[key], which k_frmem_fill set to 0 and MISSING before.
// No atomics; no kernel waits for another workgroup; every store to an output is guarded by its own index.
#pragma once
#include <cstddef>
#include <cstdint>

#define FRMEM_THREADS 256
#define FRMEM_PER_LANE 4                             // entries of a tile per lane: a tile holds at most 1024
#define FRMEM_TILE (FRMEM_THREADS * FRMEM_PER_LANE)  // 1024
#define FRMEM_WAVE 64
#define FRMEM_WAVES (FRMEM_THREADS / FRMEM_WAVE)  // 4
#define FRMEM_DIGIT_BITS 8
#define FRMEM_DIGITS 256      // == FRMEM_THREADS: lane d owns digit d
#define FRMEM_SCAN_STEPS 8    // log2 FRMEM_THREADS
#define FRMEM_MISSING 0xffffffffu
// the result buffer: eight words, one copy
#define FRMEM_RESULT_WORDS 8
#define FRMEM_RES_ERR 0       // a key above the caller's bound
#define FRMEM_RES_TOTAL 2     // the digit counts of the last pass, added up: n
#define FRMEM_RES_DISTINCT 4  // access: the heads of runs
// what a scan's leaf is
#define FRMEM_INNER 0  // nodes, in place
#define FRMEM_WORDS 1  // 32-bit counts, in place: exclusive sums
#define FRMEM_HEADS 2  // sorted keys: (head of a run, its position) -> start[], inclusive

#if defined(__HIPCC__)
#define FRM_HD __host__ __device__ __forceinline__
#else
#define FRM_HD inline
#endif

struct FrmNode {  // a tile's sum and maximum; after its level's scan, those of everything before the tile
  uint32_t sum, max;
};
struct FrmemArgs {   // what the host plans (csrc/frmem_plan.h) for one pass
  uint32_t n;        // keys, >= 1
  uint32_t tile;     // keys per tile, 2 .. 1024
  uint32_t tiles;    // ceil(n / tile)
  uint32_t shift;    // 8 * pass
  uint32_t first;    // the first pass: the keys are checked
  uint32_t pad;
  uint64_t max_key;  // 2^key_bits - 1, or n_t - 1 where that is less
};
template <class KEY>
struct FrmLane {  // what a lane keeps between the phases of k_frmem_hist and k_frmem_scatter
  KEY key[FRMEM_PER_LANE];
  uint32_t idx[FRMEM_PER_LANE], digit[FRMEM_PER_LANE], rank[FRMEM_PER_LANE];
  uint32_t valid;  // bit e: entry e lies in the tile and below n
};
struct FrmScanLane {  // ... of k_frmem_sums and k_frmem_scan
  FrmNode v[FRMEM_PER_LANE], sum;
};

FRM_HD uint32_t frm_popcount(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
FRM_HD FrmNode frm_join(const FrmNode& a, const FrmNode& b) { return FrmNode{a.sum + b.sum, a.max > b.max ? a.max : b.max}; }

// ---- a tile of keys: k_frmem_hist, k_frmem_scatter ---------------------------------------------------------------------------------------------------------
// where entry e of `lane` lies in its tile: wave w owns w * 256 .. w * 256 + 255, round e the 64 positions from e * 64
FRM_HD uint32_t frm_pos(uint32_t lane, uint32_t e) { return (lane / FRMEM_WAVE) * (FRMEM_WAVE * FRMEM_PER_LANE) + e * FRMEM_WAVE + lane % FRMEM_WAVE; }
FRM_HD void frm_zero(uint32_t* cnt, uint32_t lane) {
#pragma unroll
  for (uint32_t w = 0; w < FRMEM_WAVES; w++) cnt[w * FRMEM_DIGITS + lane] = 0;
}
// the lane's keys with their indices and this pass's digits; false where the first pass meets a key above the bound
template <class KEY>
FRM_HD bool frm_load(const FrmemArgs& g, const KEY* keys, const uint32_t* idx, size_t tile_at, uint32_t lane, FrmLane<KEY>& s) {
  bool ok = true;
  s.valid = 0;
#pragma unroll
  for (uint32_t e = 0; e < FRMEM_PER_LANE; e++) {
    const uint32_t in_tile = frm_pos(lane, e);
    const size_t at = tile_at * g.tile + in_tile;
    s.key[e] = 0, s.idx[e] = 0, s.digit[e] = 0, s.rank[e] = 0;
    if (in_tile < g.tile && at < g.n) {
      s.valid |= 1u << e;
      s.key[e] = keys[at];
      s.idx[e] = idx ? idx[at] : (uint32_t)at;  // (no indices: the first pass's scatter, whose index is the position, and every hist)
      s.digit[e] = (uint32_t)((uint64_t)s.key[e] >> g.shift) & (FRMEM_DIGITS - 1);
      if (g.first && (uint64_t)s.key[e] > g.max_key) ok = false;
    }
  }
  return ok;
}
// the lanes of the wave whose entry has this lane's digit: bal[b] holds the lanes whose digit has bit b, `in` those with an entry at all
FRM_HD uint64_t frm_peers(const uint64_t* bal, uint64_t in, uint32_t digit) {
  uint64_t m = in;
#pragma unroll
  for (uint32_t b = 0; b < FRMEM_DIGIT_BITS; b++) m &= (digit >> b & 1u) ? bal[b] : ~bal[b];
  return m;
}
// round e, before the barrier: the lane's rank among the wave's entries with its digit so far (earlier rounds: cnt; this round: the peers below)
template <class KEY>
FRM_HD void frm_rank(const uint32_t* cnt, uint32_t lane, uint32_t e, uint64_t peers, FrmLane<KEY>& s) {
  if (!(s.valid >> e & 1u)) return;
  const uint64_t below = peers & (((uint64_t)1 << (lane % FRMEM_WAVE)) - 1);
  s.rank[e] = cnt[(lane / FRMEM_WAVE) * FRMEM_DIGITS + s.digit[e]] + frm_popcount(below);
}
// round e, after it: the lowest lane of a group adds the group to its wave's count of the digit (one writer per word)
template <class KEY>
FRM_HD void frm_count(uint32_t* cnt, uint32_t lane, uint32_t e, uint64_t peers, const FrmLane<KEY>& s) {
  if (!(s.valid >> e & 1u)) return;
  if (peers & (((uint64_t)1 << (lane % FRMEM_WAVE)) - 1)) return;
  cnt[(lane / FRMEM_WAVE) * FRMEM_DIGITS + s.digit[e]] += frm_popcount(peers);
}
// hist, after the rounds: lane d writes the tile's count of digit d, digit-major
FRM_HD void frm_store_hist(const FrmemArgs& g, const uint32_t* cnt, uint32_t* hist, size_t tile_at, uint32_t lane) {
  uint32_t total = 0;
#pragma unroll
  for (uint32_t w = 0; w < FRMEM_WAVES; w++) total += cnt[w * FRMEM_DIGITS + lane];
  if (tile_at < g.tiles) hist[(size_t)lane * g.tiles + tile_at] = total;
}
// scatter, after the rounds: lane d turns the waves' counts of digit d into where each wave's first entry of that digit goes
FRM_HD void frm_offsets(const FrmemArgs& g, uint32_t* cnt, const uint32_t* base, size_t tile_at, uint32_t lane) {
  uint32_t run = tile_at < g.tiles ? base[(size_t)lane * g.tiles + tile_at] : 0;
#pragma unroll
  for (uint32_t w = 0; w < FRMEM_WAVES; w++) {
    const uint32_t c = cnt[w * FRMEM_DIGITS + lane];
    cnt[w * FRMEM_DIGITS + lane] = run;
    run += c;
  }
}
// ... and, after one more barrier, every entry goes to its place
template <class KEY>
FRM_HD void frm_place(const FrmemArgs& g, const uint32_t* cnt, KEY* keys_dst, uint32_t* idx_dst, uint32_t lane, const FrmLane<KEY>& s) {
#pragma unroll
  for (uint32_t e = 0; e < FRMEM_PER_LANE; e++) {
    if (!(s.valid >> e & 1u)) continue;
    const uint32_t to = cnt[(lane / FRMEM_WAVE) * FRMEM_DIGITS + s.digit[e]] + s.rank[e];
    if (to >= g.n) continue;  // (hist and base are this call's own: never taken)
    if (keys_dst) keys_dst[to] = s.key[e];
    idx_dst[to] = s.idx[e];
  }
}

// ---- phases of k_frmem_sums and k_frmem_scan ---------------------------------------------------------------------------------------------------------------
// the lane's entries of tile `tile_at` of a level of `len` entries: lane * 4 + e < tile, inside the level
template <int KIND, class KEY>
FRM_HD void frm_scan_load(uint32_t tile, const void* leaf, size_t len, size_t tile_at, uint32_t lane, FrmScanLane& s) {
  s.sum = FrmNode{0, 0};
#pragma unroll
  for (uint32_t e = 0; e < FRMEM_PER_LANE; e++) {
    const uint32_t in_tile = lane * FRMEM_PER_LANE + e;
    const size_t at = tile_at * tile + in_tile;
    s.v[e] = FrmNode{0, 0};
    if (in_tile < tile && at < len) {
      if (KIND == FRMEM_INNER) {
        s.v[e] = static_cast<const FrmNode*>(leaf)[at];
      } else if (KIND == FRMEM_WORDS) {
        s.v[e].sum = static_cast<const uint32_t*>(leaf)[at];
      } else {
        const KEY* keys = static_cast<const KEY*>(leaf);
        if (at == 0 || keys[at] != keys[at - 1]) s.v[e] = FrmNode{1u, (uint32_t)at};
      }
    }
    s.sum = frm_join(s.sum, s.v[e]);
  }
}
FRM_HD void frm_put(FrmNode* lds, uint32_t lane, const FrmScanLane& s) { lds[lane] = s.sum; }
// one Hillis-Steele step: what the lane takes in (read before the barrier), then the join (after it)
FRM_HD FrmNode frm_peek(const FrmNode* lds, uint32_t lane, uint32_t step) {
  const uint32_t d = 1u << step;
  return lane >= d ? lds[lane - d] : FrmNode{0, 0};
}
FRM_HD void frm_add(FrmNode* lds, uint32_t lane, const FrmNode& v) { lds[lane] = frm_join(lds[lane], v); }
// sums: the tile's node of the level above (lane 0, after the scan: the last word of the LDS holds the tile's total)
FRM_HD void frm_store_sum(const FrmNode* lds, FrmNode* above, size_t tile_at, size_t len_above) {
  if (tile_at < len_above) above[tile_at] = lds[FRMEM_THREADS - 1];
}
// the top level's total (lane 0, after the scan): the sum, into word `res_at` of the result
FRM_HD void frm_store_total(const FrmNode* lds, uint32_t* res, uint32_t res_at) { res[res_at] = lds[FRMEM_THREADS - 1].sum; }
// scan: what precedes the lane's entries (the tile's node of the level above, nothing above the top; the lanes below), then entry by entry.
// INNER and WORDS write what precedes the entry, in place; HEADS writes start[at], the entry's own head included.
template <int KIND>
FRM_HD void frm_scan_store(uint32_t tile, const FrmNode* lds, const FrmNode* above, void* leaf, uint32_t* start, size_t len, size_t tile_at, uint32_t lane, const FrmScanLane& s) {
  FrmNode run = lane ? lds[lane - 1] : FrmNode{0, 0};
  if (above) run = frm_join(above[tile_at], run);
#pragma unroll
  for (uint32_t e = 0; e < FRMEM_PER_LANE; e++) {
    const uint32_t in_tile = lane * FRMEM_PER_LANE + e;
    const size_t at = tile_at * tile + in_tile;
    const FrmNode with = frm_join(run, s.v[e]);
    if (in_tile < tile && at < len) {
      if (KIND == FRMEM_INNER) static_cast<FrmNode*>(leaf)[at] = run;
      else if (KIND == FRMEM_WORDS) static_cast<uint32_t*>(leaf)[at] = run.sum;
      else start[at] = with.max;
    }
    run = with;
  }
}

// ---- access ------------------------------------------------------------------------------------------------------------------------------------------------
// counts and last before the runs' tails are written: entry j < n_t
FRM_HD void frm_fill_lane(const uint32_t* res, uint32_t* counts, uint32_t* last, uint32_t n_t, uint32_t j) {
  if (j >= n_t || res[FRMEM_RES_ERR]) return;
  if (counts) counts[j] = 0;
  if (last) last[j] = FRMEM_MISSING;
}
// sorted position k < n: the access perm[k] is number k - start[k] of its run
template <class KEY>
FRM_HD void frm_access_lane(uint32_t n, uint32_t n_t, const uint32_t* res, const KEY* keys, const uint32_t* perm, const uint32_t* start, uint32_t* rank, uint32_t* prev,
                            uint32_t* counts, uint32_t* last, uint32_t k) {
  if (k >= n || res[FRMEM_RES_ERR]) return;
  const uint32_t i = perm[k], s = start[k];
  if (i >= n || s > k) return;  // (perm and start are this call's own: never taken)
  if (rank) rank[i] = k - s;
  if (prev) prev[i] = k > s ? perm[k - 1] : FRMEM_MISSING;
  if (!counts && !last) return;
  const KEY key = keys[k];
  if (k + 1 < n && keys[k + 1] == key) return;  // not the run's tail
  if ((uint64_t)key >= n_t) return;             // (the first pass refused such a key)
  if (counts) counts[(size_t)key] = k - s + 1;
  if (last) last[(size_t)key] = i;
}

#if defined(__HIPCC__)
namespace frmem {

// the rounds of a tile, shared by the two kernels: afterwards cnt[w][d] counts wave w's entries with digit d and s.rank their ranks inside the wave
template <class KEY>
__device__ __forceinline__ void tile_ranks(uint32_t* cnt, uint32_t lane, FrmLane<KEY>& s) {
  frm_zero(cnt, lane);
  __syncthreads();
#pragma unroll  // (e indexes the lane's arrays: unrolled, they stay in registers)
  for (uint32_t e = 0; e < FRMEM_PER_LANE; e++) {
    const bool in = s.valid >> e & 1u;
    uint64_t bal[FRMEM_DIGIT_BITS];
#pragma unroll
    for (uint32_t b = 0; b < FRMEM_DIGIT_BITS; b++) bal[b] = __ballot(in && (s.digit[e] >> b & 1u));
    const uint64_t peers = frm_peers(bal, __ballot(in), s.digit[e]);
    frm_rank(cnt, lane, e, peers, s);
    __syncthreads();
    frm_count(cnt, lane, e, peers, s);
    __syncthreads();
  }
}

template <class KEY>
__global__ void __launch_bounds__(FRMEM_THREADS) k_frmem_hist(const KEY* keys, uint32_t* hist, uint32_t* res, const FrmemArgs g) {
  __shared__ uint32_t cnt[FRMEM_WAVES * FRMEM_DIGITS];
  FrmLane<KEY> s;
  if (!frm_load<KEY>(g, keys, nullptr, blockIdx.x, threadIdx.x, s)) res[FRMEM_RES_ERR] = 1u;  // (every lane that writes it writes the same word)
  tile_ranks(cnt, threadIdx.x, s);
  frm_store_hist(g, cnt, hist, blockIdx.x, threadIdx.x);
}

template <class KEY>
__global__ void __launch_bounds__(FRMEM_THREADS) k_frmem_scatter(const KEY* keys, const uint32_t* idx, const uint32_t* base, KEY* keys_dst, uint32_t* idx_dst, const uint32_t* res,
                                                                  const FrmemArgs g) {
  __shared__ uint32_t cnt[FRMEM_WAVES * FRMEM_DIGITS];
  if (res[FRMEM_RES_ERR]) return;  // (the whole grid alike: the first pass's hist has completed)
  FrmLane<KEY> s;
  frm_load<KEY>(g, keys, idx, blockIdx.x, threadIdx.x, s);
  tile_ranks(cnt, threadIdx.x, s);
  frm_offsets(g, cnt, base, blockIdx.x, threadIdx.x);
  __syncthreads();
  frm_place<KEY>(g, cnt, keys_dst, idx_dst, threadIdx.x, s);
}

// the inclusive scan of the 256 lane sums in LDS: afterwards lds[lane] covers lanes 0 .. lane
__device__ __forceinline__ void block_scan(FrmNode* lds, uint32_t lane, const FrmScanLane& s) {
  frm_put(lds, lane, s);
  __syncthreads();
#pragma unroll 1
  for (uint32_t step = 0; step < FRMEM_SCAN_STEPS; step++) {
    const FrmNode v = frm_peek(lds, lane, step);
    __syncthreads();
    frm_add(lds, lane, v);
    __syncthreads();
  }
}

// level l -> level l + 1: a workgroup per tile of level l
template <int KIND, class KEY>
__global__ void __launch_bounds__(FRMEM_THREADS) k_frmem_sums(const void* leaf, FrmNode* above, uint32_t len, uint32_t len_above, uint32_t tile) {
  __shared__ FrmNode lds[FRMEM_THREADS];
  FrmScanLane s;
  frm_scan_load<KIND, KEY>(tile, leaf, len, blockIdx.x, threadIdx.x, s);
  block_scan(lds, threadIdx.x, s);
  if (threadIdx.x == 0) frm_store_sum(lds, above, blockIdx.x, len_above);
}

// level l scanned, a workgroup per tile; above: the scanned level l + 1, or null at the top, whose one workgroup writes the total
template <int KIND, class KEY>
__global__ void __launch_bounds__(FRMEM_THREADS) k_frmem_scan(void* leaf, const FrmNode* above, uint32_t len, uint32_t* start, uint32_t* res, uint32_t res_at, uint32_t tile) {
  __shared__ FrmNode lds[FRMEM_THREADS];
  FrmScanLane s;
  frm_scan_load<KIND, KEY>(tile, leaf, len, blockIdx.x, threadIdx.x, s);
  block_scan(lds, threadIdx.x, s);
  frm_scan_store<KIND>(tile, lds, above, leaf, start, len, blockIdx.x, threadIdx.x, s);
  if (!above && threadIdx.x == 0) frm_store_total(lds, res, res_at);
}

__global__ void __launch_bounds__(FRMEM_THREADS) k_frmem_fill(const uint32_t* res, uint32_t* counts, uint32_t* last, uint32_t n_t) {
  frm_fill_lane(res, counts, last, n_t, blockIdx.x * FRMEM_THREADS + threadIdx.x);  // (n_t <= 2^26: no wrap)
}
template <class KEY>
__global__ void __launch_bounds__(FRMEM_THREADS) k_frmem_access(uint32_t n, uint32_t n_t, const uint32_t* res, const KEY* keys, const uint32_t* perm, const uint32_t* start,
                                                                 uint32_t* rank, uint32_t* prev, uint32_t* counts, uint32_t* last) {
  frm_access_lane<KEY>(n, n_t, res, keys, perm, start, rank, prev, counts, last, blockIdx.x * FRMEM_THREADS + threadIdx.x);
}

}  // namespace frmem
#endif  // __HIPCC__
