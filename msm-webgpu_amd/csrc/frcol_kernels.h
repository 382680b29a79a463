// Lookup columns from counts (libmsm_frcol.so, include/msm_frcol.h): run expansion, halo2's permuted pair, gather.  One translation unit for all
// curves: a scalar is 32 bytes moved AS STORED -- no field arithmetic, no comparison with r, no constants.  Everything a lane does is an FRC_HD
// function, which the kernels at the bottom call and which the host program of tests/test_frcol_host.py runs lane by lane and phase by phase on
// the CPU.
//
// The scan.  With w[j] = counts[j] + bias (64 bits) and u[j] = (counts[j] > 0), the exclusive prefix sums of (w, u) over the table are formed level by
// level over tiles of `tile` entries (1024 by design), as in csrc/frvec_kernels.h: level 0 is the table, level l + 1 holds one node per tile of
// level l.  Nodes are pairs of 64-bit words: four counts of 0x80000000 add up to 2^33, not to 0.
//   k_frcol_sums<LEAF>   one workgroup per tile: the tile's sum of (w, u) -> its node of the level above
//   k_frcol_scan<LEAF>   one workgroup per tile, from the top level down: the exclusive prefix inside the tile plus the tile's node of the level
//                        above (already final).  The top level (one tile) also writes the grand totals to the result words.  Inner levels
//                        scan their nodes in place.  LEAF (level 0) writes, per entry, rel[j] -- the offset of run j inside its tile, saturated
//                        at 2^32 - 1 --, used[j] = #{j' < j : counts[j'] > 0}, and -- compaction -- z[j - used[j]] = j where counts[j] = 0.
//   k_frcol_expand       one lane per OUTPUT k < n_out: nothing is written unless the total equals n_out; then two binary searches --
//   k_frcol_pair         the level-1 nodes (tile bases) for the last tile with base <= k, rel[] of that tile for the last run with
//                        rel <= k - base -- give j, and the lane copies t[j].  The cost of a lane does not depend on the counts: one run of n,
//                        n runs of one and a table of zeros take the same two searches.  pair also writes s_out: t[j] at the head of a run,
//                        else the filler t[z[k - used[j] - 1]].
//   k_frcol_gather       one lane per output: a[idx[i]], zero for 0xFFFFFFFF, zero and the error word for any other idx >= n_a.
// No atomics; a workgroup's 256 partial sums are scanned in LDS (Hillis-Steele, eight steps); no kernel waits for another workgroup.  Every
// store to an output is guarded by its own index, every load of t by j < n_t.
#pragma once
#include <cstddef>
#include <cstdint>

#define FRCOL_THREADS 256
#define FRCOL_PER_LANE 4                             // entries of a tile per lane: a tile holds at most 1024
#define FRCOL_TILE (FRCOL_THREADS * FRCOL_PER_LANE)  // 1024
#define FRCOL_SCAN_STEPS 8                           // log2 FRCOL_THREADS
#define FRCOL_MISSING 0xffffffffu                    // gather: 32 zero bytes
// the result buffer: eight words, one copy
#define FRCOL_RESULT_WORDS 8
#define FRCOL_RES_ERR 0    // gather: an index that is neither below n_a nor FRCOL_MISSING
#define FRCOL_RES_TOTAL 2  // 64 bits (words 2, 3): the sum of w
#define FRCOL_RES_USED 4   // 64 bits (words 4, 5): the entries with counts > 0

#if defined(__HIPCC__)
#define FRC_HD __host__ __device__ __forceinline__
#else
#define FRC_HD inline
#endif

struct FrcNode {  // a tile's sums; after its level's scan, the sums of everything before the tile
  uint64_t w, u;
};
struct FrcolArgs {  // what the host plans (csrc/frcol_plan.h)
  uint32_t n_t;     // table entries, >= 1
  uint32_t tile;    // entries per tile, 2 .. 1024
  uint32_t bias;    // 0 or 1
  uint32_t n_out;   // outputs, >= 1
  uint32_t tiles;   // level-1 nodes: ceil(n_t / tile)
  uint32_t pair;    // the leaf also writes used[] and z[]
};
struct FrcLane {  // what a lane keeps between the phases of a sums or scan kernel
  uint64_t w[FRCOL_PER_LANE], u[FRCOL_PER_LANE];
  FrcNode sum;
};

// ---- phases of k_frcol_sums and k_frcol_scan -------------------------------------------------------------------------------------------------------------
// the lane's entries of tile `tile_at` of a level of `len` entries: lane * 4 + e < g.tile, inside the level.  LEAF: counts; else nodes.
template <bool LEAF>
FRC_HD void frc_load(const FrcolArgs& g, const uint32_t* counts, const FrcNode* nodes, size_t len, size_t tile_at, uint32_t lane, FrcLane& s) {
  s.sum.w = s.sum.u = 0;
#pragma unroll
  for (uint32_t e = 0; e < FRCOL_PER_LANE; e++) {
    const uint32_t in_tile = lane * FRCOL_PER_LANE + e;
    const size_t at = tile_at * g.tile + in_tile;
    s.w[e] = s.u[e] = 0;
    if (in_tile < g.tile && at < len) {
      if (LEAF) {
        const uint32_t c = counts[at];
        s.w[e] = (uint64_t)c + g.bias, s.u[e] = c != 0;
      } else {
        s.w[e] = nodes[at].w, s.u[e] = nodes[at].u;
      }
    }
    s.sum.w += s.w[e], s.sum.u += s.u[e];
  }
}
FRC_HD void frc_put(FrcNode* lds, uint32_t lane, const FrcLane& s) { lds[lane] = s.sum; }
// one Hillis-Steele step: what the lane adds (read before the barrier), then the addition (after it)
FRC_HD FrcNode frc_peek(const FrcNode* lds, uint32_t lane, uint32_t step) {
  const uint32_t d = 1u << step;
  return lane >= d ? lds[lane - d] : FrcNode{0, 0};
}
FRC_HD void frc_add(FrcNode* lds, uint32_t lane, const FrcNode& v) { lds[lane].w += v.w, lds[lane].u += v.u; }
// sums: the tile's node of the level above (lane 0, after the scan: the last word of the LDS holds the tile's total)
FRC_HD void frc_store_sum(const FrcNode* lds, FrcNode* above, size_t tile_at, size_t len_above) {
  if (tile_at < len_above) above[tile_at] = lds[FRCOL_THREADS - 1];
}
// scan of an inner level, in place: base (the tile's node of the level above; nothing above the top) + what precedes the entry in its tile
FRC_HD void frc_store_inner(const FrcolArgs& g, const FrcNode* lds, const FrcNode* above, FrcNode* nodes, size_t len, size_t tile_at, uint32_t lane, const FrcLane& s) {
  FrcNode run = {lds[lane].w - s.sum.w, lds[lane].u - s.sum.u};
  if (above) run.w += above[tile_at].w, run.u += above[tile_at].u;
#pragma unroll
  for (uint32_t e = 0; e < FRCOL_PER_LANE; e++) {
    const uint32_t in_tile = lane * FRCOL_PER_LANE + e;
    const size_t at = tile_at * g.tile + in_tile;
    if (in_tile < g.tile && at < len) nodes[at] = run;
    run.w += s.w[e], run.u += s.u[e];
  }
}
// the top level's totals (lane 0, after the scan)
FRC_HD void frc_store_totals(const FrcNode* lds, uint32_t* res) {
  const FrcNode t = lds[FRCOL_THREADS - 1];
  res[FRCOL_RES_TOTAL] = (uint32_t)t.w, res[FRCOL_RES_TOTAL + 1] = (uint32_t)(t.w >> 32);
  res[FRCOL_RES_USED] = (uint32_t)t.u, res[FRCOL_RES_USED + 1] = (uint32_t)(t.u >> 32);
}
// scan of the table: rel[j] inside the tile (saturated: a lane looks for k - base < 2^26), and for the pair used[j] and z
FRC_HD void frc_store_leaf(const FrcolArgs& g, const FrcNode* lds, const FrcNode* above, uint32_t* rel, uint32_t* used, uint32_t* z, size_t tile_at, uint32_t lane,
                           const FrcLane& s) {
  uint64_t run_w = lds[lane].w - s.sum.w;
  uint64_t run_u = lds[lane].u - s.sum.u + above[tile_at].u;  // (at most n_t)
#pragma unroll
  for (uint32_t e = 0; e < FRCOL_PER_LANE; e++) {
    const uint32_t in_tile = lane * FRCOL_PER_LANE + e;
    const size_t at = tile_at * g.tile + in_tile;
    if (in_tile < g.tile && at < g.n_t) {
      rel[at] = run_w > 0xffffffffull ? 0xffffffffu : (uint32_t)run_w;
      if (g.pair) {
        used[at] = (uint32_t)run_u;
        const size_t zat = at - (size_t)run_u;  // the entries before this one with counts == 0
        if (!s.u[e] && zat < g.n_t) z[zat] = (uint32_t)at;
      }
    }
    run_w += s.w[e], run_u += s.u[e];
  }
}

// ---- an output's run ------------------------------------------------------------------------------------------------------------------------------------------
// The run that holds output k, given that the total is n_out > k: j, and d = k - off[j].  bases: the level-1 nodes after their scan (bases[0].w = 0).
// The last tile with base <= k has base + sum > k, and the last entry of it with rel <= k - base has w > 0: entries of weight 0 share their
// successor's offset and are passed over.  false where no run is found (the counts changed under the call: nothing is read or written then).
FRC_HD bool frc_find(const FrcolArgs& g, const FrcNode* bases, const uint32_t* rel, uint32_t k, uint32_t& j, uint32_t& d) {
  uint32_t lo = 0, hi = g.tiles;  // bases[lo].w <= k < bases[hi].w (hi == tiles: the end)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (bases[mid].w <= k) lo = mid; else hi = mid;
  }
  const uint32_t in = k - (uint32_t)bases[lo].w;
  const uint32_t first = lo * g.tile;
  const uint32_t end = g.n_t - first < g.tile ? g.n_t - first : g.tile;
  uint32_t a = 0, b = end;  // rel[first + a] <= in < rel[first + b]
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (rel[first + mid] <= in) a = mid; else b = mid;
  }
  j = first + a;
  if (j >= g.n_t || rel[j] > in) return false;
  d = in - rel[j];
  return true;
}

// 32 bytes as two 16-byte vector accesses on the device
FRC_HD void frc_copy32(uint32_t* dst, size_t to, const uint32_t* src, size_t from) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  const uint4 q0 = s4[2 * from], q1 = s4[2 * from + 1];
  d4[2 * to] = q0, d4[2 * to + 1] = q1;
#else
  for (int i = 0; i < 8; i++) dst[8 * to + i] = src[8 * from + i];
#endif
}
FRC_HD void frc_zero32(uint32_t* dst, size_t to) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * to] = d4[2 * to + 1] = make_uint4(0, 0, 0, 0);
#else
  for (int i = 0; i < 8; i++) dst[8 * to + i] = 0;
#endif
}
FRC_HD uint64_t frc_total(const uint32_t* res) { return (uint64_t)res[FRCOL_RES_TOTAL] | (uint64_t)res[FRCOL_RES_TOTAL + 1] << 32; }

// expand, output k
FRC_HD void frc_expand_lane(const FrcolArgs& g, const uint32_t* res, const FrcNode* bases, const uint32_t* rel, const uint32_t* t, uint32_t* out, uint32_t k) {
  uint32_t j, d;
  if (k >= g.n_out || frc_total(res) != g.n_out || !frc_find(g, bases, rel, k, j, d)) return;
  frc_copy32(out, k, t, j);
}
// pair, output k (n_out = n_t): the run's value, and the run's value or a filler
FRC_HD void frc_pair_lane(const FrcolArgs& g, const uint32_t* res, const FrcNode* bases, const uint32_t* rel, const uint32_t* used, const uint32_t* z, const uint32_t* t,
                          uint32_t* a_out, uint32_t* s_out, uint32_t k) {
  uint32_t j, d;
  if (k >= g.n_out || frc_total(res) != g.n_out || !frc_find(g, bases, rel, k, j, d)) return;
  uint32_t from = j;
  if (d) {  // the (k - used[j] - 1)-th output that is no head of a run takes the entry of that rank among those never looked up
    const uint32_t rank = k - used[j] - 1;
    if (rank >= g.n_t) return;
    from = z[rank];
    if (from >= g.n_t) return;
  }
  frc_copy32(a_out, k, t, j);
  frc_copy32(s_out, k, t, from);
}
// gather, output i < n
FRC_HD void frc_gather_lane(const uint32_t* a, uint32_t n_a, const uint32_t* idx, uint32_t n, uint32_t* out, uint32_t* res, uint32_t i) {
  if (i >= n) return;
  const uint32_t at = idx[i];
  if (at < n_a) {
    frc_copy32(out, i, a, at);
    return;
  }
  frc_zero32(out, i);
  if (at != FRCOL_MISSING) res[FRCOL_RES_ERR] = 1u;  // (every lane that writes it writes the same word)
}

#if defined(__HIPCC__)
namespace frcol {

// the inclusive scan of the 256 lane sums in LDS: afterwards lds[lane] covers lanes 0 .. lane
__device__ __forceinline__ void block_scan(FrcNode* lds, uint32_t lane, const FrcLane& s) {
  frc_put(lds, lane, s);
  __syncthreads();
#pragma unroll 1
  for (uint32_t step = 0; step < FRCOL_SCAN_STEPS; step++) {
    const FrcNode v = frc_peek(lds, lane, step);
    __syncthreads();
    frc_add(lds, lane, v);
    __syncthreads();
  }
}

// level l -> level l + 1: a workgroup per tile of level l
template <bool LEAF>
__global__ void __launch_bounds__(FRCOL_THREADS) k_frcol_sums(const uint32_t* counts, const FrcNode* nodes, FrcNode* above, uint32_t len, uint32_t len_above, const FrcolArgs g) {
  __shared__ FrcNode lds[FRCOL_THREADS];
  FrcLane s;
  frc_load<LEAF>(g, counts, nodes, len, blockIdx.x, threadIdx.x, s);
  block_scan(lds, threadIdx.x, s);
  if (threadIdx.x == 0) frc_store_sum(lds, above, blockIdx.x, len_above);
}

// level l scanned, a workgroup per tile; above: the scanned level l + 1, or null at the top, whose one workgroup writes the totals
template <bool LEAF>
__global__ void __launch_bounds__(FRCOL_THREADS) k_frcol_scan(const uint32_t* counts, FrcNode* nodes, const FrcNode* above, uint32_t len, uint32_t* rel, uint32_t* used,
                                                               uint32_t* z, uint32_t* res, const FrcolArgs g) {
  __shared__ FrcNode lds[FRCOL_THREADS];
  FrcLane s;
  frc_load<LEAF>(g, counts, nodes, len, blockIdx.x, threadIdx.x, s);
  block_scan(lds, threadIdx.x, s);
  if (LEAF) {
    frc_store_leaf(g, lds, above, rel, used, z, blockIdx.x, threadIdx.x, s);
  } else {
    frc_store_inner(g, lds, above, nodes, len, blockIdx.x, threadIdx.x, s);
    if (!above && threadIdx.x == 0) frc_store_totals(lds, res);
  }
}

__global__ void __launch_bounds__(FRCOL_THREADS) k_frcol_expand(const uint32_t* res, const FrcNode* bases, const uint32_t* rel, const uint32_t* t, uint32_t* out, const FrcolArgs g) {
  frc_expand_lane(g, res, bases, rel, t, out, blockIdx.x * FRCOL_THREADS + threadIdx.x);  // (n_out <= 2^26: no wrap)
}
__global__ void __launch_bounds__(FRCOL_THREADS) k_frcol_pair(const uint32_t* res, const FrcNode* bases, const uint32_t* rel, const uint32_t* used, const uint32_t* z,
                                                               const uint32_t* t, uint32_t* a_out, uint32_t* s_out, const FrcolArgs g) {
  frc_pair_lane(g, res, bases, rel, used, z, t, a_out, s_out, blockIdx.x * FRCOL_THREADS + threadIdx.x);
}
__global__ void __launch_bounds__(FRCOL_THREADS) k_frcol_gather(const uint32_t* a, uint32_t n_a, const uint32_t* idx, uint32_t n, uint32_t* out, uint32_t* res) {
  frc_gather_lane(a, n_a, idx, n, out, res, blockIdx.x * FRCOL_THREADS + threadIdx.x);
}

}  // namespace frcol
#endif  // __HIPCC__
