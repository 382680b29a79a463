// The recode and the sort of the MSM pipeline: from the scalars of a launch to val_idxs / col_ptr and the SMVP's chunk table.  No field, curve
// or endomorphism header enters (recode.h and msm_layout.h are all it needs), so these kernels are compiled ONCE, by msm_hip.hip, for every
// curve.  The sort's first pass, k_count, is in recode.h: endomorphism launches split their scalars in it, the one place where a curve enters,
// and those instantiations belong to the curve units (CurveOps::count_split).
// The HBM arrays of this stage: see the layout at the top of msm_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "recode.h"

namespace msm_sort {
using namespace msm_layout;
using namespace msm_recode;

// ------------------------------------------------------------------------------------------------ stage 1+2: recode + sort
// Signed 16-bit digit recode (≙ decompose_scalars.template.wgsl:83-112, CPU model test/utils.rs:121-161):
//   d = raw + carry; if d >= 2^15 { d -= 2^16; carry = 1 }  -- computed per window without the serial carry chain.  Signed-magnitude code = sign << 15 | (|d| & 0x7fff):
//   0 = digit 0 (contributes nothing), 0x8000 = digit -2^15 (bucket slot 0).
//
// The reference's transpose (transpose.template.wgsl:32-76) is a counting sort run by 16 threads.  Here it is a
// two-level LDS counting sort over the 15-bit bucket slot, and the recode is fused into both of its global passes
// (scalars are re-read instead of materialising 16 digit planes: 32 B per scalar either way):
//   k_count          per tile of scalars: LDS histogram of the 128 coarse bins (slot >> 8) of every window; the tile's place inside every bin
//                    (a returning atomic on the bin's fill) and, with the last tile, the bin totals
//   k_scan_tiles     (wide and list passes only) per (window, coarse bin): prefix over tiles, bin totals
//   k_scatter_coarse per tile: LDS-ranked scatter of (index | sign << 31, slot & 255) into coarse-bin order
//   k_sort_fine      per (window, coarse bin): LDS counting sort over its 256 slots -> val_idxs + col_ptr
// Order inside a slot is the arrival order of LDS atomics; the group sum does not depend on it.

// A launch over a base set with identity records (k_convert_points_zero_id): its scalars -- `nvec` (grid.y) contiguous vectors of n elements of NB
// bytes -- copied to `out` with zeros where the base is the identity.  Input j of a vector is base base_off + j or, sparse (idx != null), base
// idx[j]; an index not below n_bases is left to the sort's ERRBIT_BAD_INDEX path and reads no bitmap word.  It runs before any pass validates,
// converts or splits the scalars, so a scalar paired with the identity is ignored exactly as a zero scalar is.
template <int NB>
__global__ void __launch_bounds__(256) k_mask_identity(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, size_t n, size_t base_off,
                                                       const uint64_t* __restrict__ id_bits, uint32_t n_bases, const uint32_t* __restrict__ idx) {
  static_assert(NB == 1 || NB == 2 || NB == 4 || NB == 8 || NB == 16 || NB == 32, "scalar width");
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t e = (size_t)blockIdx.y * n + j;
  bool zero;
  if (idx) {
    const uint32_t b = idx[j];
    zero = b < n_bases && ((id_bits[b >> 6] >> (b & 63u)) & 1u);
  } else {
    const size_t b = base_off + j;
    zero = (id_bits[b >> 6] >> (b & 63u)) & 1u;
  }
  if constexpr (NB == 32) {
    const uint4* s = reinterpret_cast<const uint4*>(in) + 2 * e;
    uint4* d = reinterpret_cast<uint4*>(out) + 2 * e;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (!zero) {
      a = s[0];
      b = s[1];
    }
    d[0] = a;
    d[1] = b;
  } else if constexpr (NB == 16) {
    uint4 a = make_uint4(0u, 0u, 0u, 0u);
    if (!zero) a = reinterpret_cast<const uint4*>(in)[e];
    reinterpret_cast<uint4*>(out)[e] = a;
  } else {
    using T = std::conditional_t<NB == 1, uint8_t, std::conditional_t<NB == 2, uint16_t, std::conditional_t<NB == 4, uint32_t, uint64_t>>>;
    T v = 0;
    if (!zero) v = reinterpret_cast<const T*>(in)[e];
    reinterpret_cast<T*>(out)[e] = v;
  }
}

// (The passes whose first kernel is not k_count -- wide and list shares -- still scan the tiles here.)
// One wave per (window, coarse bin): in place, counts[lw][tile][bin] becomes the number of entries of that bin in earlier
// tiles; bin_total[lw][bin] receives the bin's size.  (The 128 totals of a window are turned into bin starts by every
// workgroup of k_scatter_coarse for itself: a last-block hand-off here needs agent-scope releases, i.e. L2 write-backs,
// which cost 70 us.)
__global__ void __launch_bounds__(256) k_scan_tiles(uint32_t* __restrict__ counts, uint32_t tiles, uint32_t* __restrict__ bin_total) {
  const int lw = blockIdx.y, lane = threadIdx.x & 63;
  const int bin = blockIdx.x * 4 + (threadIdx.x >> 6);
  uint32_t* c = counts + (size_t)lw * tiles * NCOARSE + bin;
  uint32_t run = 0;
  for (uint32_t t0 = 0; t0 < tiles; t0 += 64) {
    const uint32_t t = t0 + lane;
    const uint32_t v = t < tiles ? c[(size_t)t * NCOARSE] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (t < tiles) c[(size_t)t * NCOARSE] = run + x - v;
    run += __shfl(x, 63);
  }
  if (lane == 0) bin_total[lw * NCOARSE + bin] = run;
}

// The SMVP's chunk length is chosen on the DEVICE from the number of entries the sort actually produced: the host sizes the chunk
// arrays and grids for n entries per window (`chunks` lanes of `host_len` entries), but zero digits produce no entry -- witness-like
// scalar vectors (many zeros and ones) fill a fraction of that, and with the host's length most lanes would find nothing to do while
// the rest carry full-length chunks.  Every kernel that uses the chunk structure (k_sort_fine's chunk table, k_smvp_chunks, the
// stitch kernels) uses the same length: the largest window's entries spread over all `chunks` lanes.  It is computed ONCE per launch, by
// workgroup 0 of k_scatter_coarse (which scans the windows' bin totals anyway), into a word of the launch's slot (`chunk_len_dev`);
// the consumers load that one word (deriving it per workgroup from the 16 .. 64 window totals cost every SMVP workgroup a chain of
// scalar loads at its start: +1 % on the whole MSM).
// (rounds 1 - 2 kept chunk lengths multiples of 4 for the index loads of that time; any length works since the SMVP loads one index per entry,
//  and the host now picks the length by the workgroups-per-CU count it produces: msm_plan.h, chunk_len_for)
constexpr uint32_t SMVP_CHUNK_ROUND = 1;
__device__ __forceinline__ uint32_t smvp_chunk_len(uint32_t mx, uint32_t chunks, uint32_t host_len) {
  uint32_t len = (uint32_t)(((uint64_t)mx + chunks - 1) / chunks);
  len = (len + (SMVP_CHUNK_ROUND - 1u)) / SMVP_CHUNK_ROUND * SMVP_CHUNK_ROUND;
  if (len < (uint32_t)SMVP_CHUNK_MIN_ENTRIES) len = SMVP_CHUNK_MIN_ENTRIES;
  return len < host_len ? len : host_len;
}
// Both scatter kernels stage their output through LDS: the block ranks its items per destination bin with LDS atomics,
// lays them out bin-major in LDS, and writes them out in LDS order, so consecutive lanes store to consecutive global
// addresses inside each (tile, bin) run instead of 64 unrelated 4-byte stores per wave instruction.
constexpr int SCAT_SUB = 2048;  // scalars staged per block iteration (8 per thread)

// (round 5) The run cursors (gpos) live in dynamic LDS, as many as the launch has local windows (512 B each): with the 32 KB of a 64-window launch
// declared statically, three workgroups fitted a CU whatever the launch's size; the half-scalar form is held to 128 registers (four waves per SIMD):
// 1290 -> 1148 us at 2^24.  (Tried and dropped: splitting the scalars again here instead of reading the halves the first pass wrote -- 1 GB less
// traffic at 2^24, and 1522 us instead of 1148 with the first pass no faster: profiles/r05_sort.txt.)
// NB != 0: narrow scalars (the layout of k_count<C, SW, void, NB>; vec_stride in bytes; NB < 0: signed, the sign in `negs`)
// Sparse (a SparseIdx argument): input i carries base idx[i] (halves: idx[i / 2], + half_shift for k2) instead of its position, and an input
// whose index is out of range reads as a zero scalar, as in k_count
template <int C, int SW, int NB = 0, typename... Sparse>
__global__ void __launch_bounds__(256, (SW == 4 || NB != 0 ? 4 : 1)) k_scatter_coarse(const uint32_t* __restrict__ scalars, size_t n, size_t stride, uint32_t tile_len,
                                                        uint32_t tiles, int w_begin, int w_count, int nvec, size_t vec_stride,
                                                        const uint32_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ bin_total, uint32_t* __restrict__ coarse_ptr,
                                                        uint32_t* __restrict__ tmp_val,
                                                        uint8_t* __restrict__ tmp_fine, size_t merge_nb, uint32_t half_n, uint32_t half_shift,
                                                        uint32_t chunks, uint32_t host_chunk_len, uint32_t* __restrict__ chunk_len_dev,
                                                        Sparse... sparse) {
  constexpr bool SPARSE = sizeof...(Sparse) != 0;
  const SparseIdx sp = sparse_arg(sparse...);
  // scalars a thread holds (biased, in registers) per block iteration: 8 halves of 4 words, or 4 full scalars of 8 words -- 8 of those cost
  // 282 VGPRs + 26 AGPRs at 16 bits (one wave per SIMD) and a 304-byte scratch object at 12 bits (round 3)
  constexpr int PER = SW == 8 ? 4 : 8;
  constexpr int SUB = 256 * PER;
  using Cfg = WinCfg<C, SW, narrow_width(NB)>;
  constexpr bool HALVES = SW == 4 && NB == 0;  // (128-bit narrow scalars have 4 words too)
  static_assert(SUB <= SCAT_SUB, "LDS staging arrays");
  // SW = 4 (endomorphism halves, interleaved by k_count<C, 4, Split>): input 2 j is k1 of scalar j and multiplies base j; input 2 j + 1 is
  // k2 and multiplies phi(P_j), record half_shift = n_bases + j
  extern __shared__ uint32_t gpos[];  // [local windows of the launch][NCOARSE]: global write cursor of every (window, coarse bin) run of this tile
  __shared__ uint32_t hist[NCOARSE];
  __shared__ uint32_t lstart[NCOARSE];
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t st_val[SCAT_SUB];
  __shared__ uint32_t st_dst[SCAT_SUB];
  __shared__ uint8_t st_fine[SCAT_SUB];
  __shared__ uint32_t max_total;  // entries of the fullest local window (workgroup 0: -> chunk_len_dev)
  const int tid = threadIdx.x;
  if (tid == 0) max_total = 0;
  __syncthreads();
  // start of every (window, coarse bin): exclusive scan of the window's 128 bin totals -- a pair of waves per window, two
  // windows per step; workgroup 0 also publishes them as coarse_ptr[lw][0..128] for k_sort_fine
  // grid (tiles, nvec): a workgroup scatters one tile of ONE scalar vector and needs the starts of that vector's windows only; workgroup (0, 0)
  // scans the windows of every vector: it publishes all of them and the launch's chunk length
  const int w_eff = merge_nb ? nvec : nvec * w_count;  // local windows of all vectors of this launch
  const int v = blockIdx.y;
  const bool publisher = blockIdx.x == 0 && blockIdx.y == 0;
  const int le0 = publisher ? 0 : (merge_nb ? v : v * w_count), le1 = publisher ? w_eff : le0 + (merge_nb ? 1 : w_count);
  for (int i0 = le0 * NCOARSE; i0 < le1 * NCOARSE; i0 += 256) {
    const int i = i0 + tid, lw = i / NCOARSE, bin = i % NCOARSE, lane = tid & 63;
    const bool live = i < le1 * NCOARSE;  // odd window counts: the last step has one idle pair of waves
    const uint32_t bt = live ? bin_total[i] : 0u;
    uint32_t x = bt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[tid >> 6] = x;
    __syncthreads();
    const uint32_t incl = x + ((tid >> 6) & 1 ? wave_tot[(tid >> 6) - 1] : 0u);
    if (live) gpos[i] = incl - bt + counts[((size_t)lw * tiles + blockIdx.x) * NCOARSE + bin];
    if (live && publisher) {
      coarse_ptr[(size_t)lw * (NCOARSE + 1) + bin] = incl - bt;
      if (bin == NCOARSE - 1) {
        coarse_ptr[(size_t)lw * (NCOARSE + 1) + NCOARSE] = incl;
        atomicMax(&max_total, incl);
      }
    }
    __syncthreads();
  }
  if (publisher && tid == 0) *chunk_len_dev = smvp_chunk_len(max_total, chunks, host_chunk_len);
  const size_t tile_base = (size_t)blockIdx.x * tile_len;
  const size_t tile_end = tile_base + tile_len < n ? tile_base + tile_len : n;
  for (size_t sub = tile_base; sub < tile_end; sub += SUB) {
    // this thread's PER biased scalars stay in registers; every window's digit code is read from them
    uint32_t sc[PER][Cfg::WORDS];
    uint32_t negs = 0;  // bit j: scalar j is a negative half (its digits' signs are flipped)
    uint32_t rec[PER];  // sparse: the record input j feeds
#pragma unroll
    for (int j = 0; j < PER; j++) {
      const size_t i = sub + (size_t)j * 256 + tid;
      uint32_t raw[SW], neg = 0;
#pragma unroll
      for (int k = 0; k < SW; k++) raw[k] = 0;  // an all-zero scalar recodes to all-zero digits: no entries
      bool live = i < tile_end;
      if constexpr (SPARSE) {
        const uint32_t x = live ? sp.idx[HALVES ? i >> 1 : i] : 0u;
        live = live && x < sp.n_bases;
        rec[j] = x + ((HALVES && (i & 1u)) ? half_shift : 0u);
      }
      if constexpr (NB != 0) {
        if (live) ld_narrow_fmt<NB>(reinterpret_cast<const uint8_t*>(scalars) + (size_t)v * vec_stride, i, raw, neg);
      } else {
        if (live) ld_scalar<SW>(scalars + (size_t)v * vec_stride + i * SW, raw, neg);
      }
      negs |= neg << j;
      (void)bias_scalar<C, SW, narrow_width(NB)>(raw, sc[j]);
    }
#pragma unroll
    for (int w = 0; w < Cfg::NWIN; w++) {
      if (w < w_begin || w >= w_begin + w_count) continue;  // block-uniform
      // fixed-base tables: window w of point i is table entry w * merge_nb + i, and all windows share local window v
      const int lw = merge_nb ? v : v * w_count + (w - w_begin);
      const uint32_t idx_base = merge_nb ? (uint32_t)(w * merge_nb) : 0u;
      if (tid < NCOARSE) hist[tid] = 0;
      __syncthreads();
      uint32_t rank[PER];
#pragma unroll
      for (int j = 0; j < PER; j++) {
        const uint32_t code = code_of_window<C>(sc[j], w);
        rank[j] = code ? atomicAdd(&hist[(code & 0x7fffu) >> 8], 1u) : 0u;
      }
      __syncthreads();
      const uint32_t mine = tid < NCOARSE ? hist[tid] : 0u;
      const uint32_t excl = block_excl_scan_256(mine, wave_tot);
      if (tid < NCOARSE) lstart[tid] = excl;
      __syncthreads();
      const uint32_t total = lstart[NCOARSE - 1] + hist[NCOARSE - 1];
#pragma unroll
      for (int j = 0; j < PER; j++) {
        const uint32_t code = code_of_window<C>(sc[j], w);
        if (code) {
          const uint32_t slot = code & 0x7fffu, bin = slot >> 8;
          const uint32_t e = lstart[bin] + rank[j];
          uint32_t pos = (uint32_t)(sub + (size_t)j * 256 + tid);
          if constexpr (SPARSE) pos = rec[j];
          else if constexpr (HALVES) pos = (pos >> 1) + ((pos & 1u) ? half_shift : 0u);
          st_val[e] = (idx_base + pos) | (((code >> 15) ^ ((negs >> j) & 1u)) << 31);
          st_fine[e] = (uint8_t)(slot & 0xffu);
          st_dst[e] = gpos[lw * NCOARSE + bin] + rank[j];
        }
      }
      __syncthreads();
      uint32_t* ov = tmp_val + (size_t)lw * stride;
      uint8_t* of = tmp_fine + (size_t)lw * stride;
      for (uint32_t e = tid; e < total; e += 256) {
        const uint32_t d = st_dst[e];
        ov[d] = st_val[e];
        of[d] = st_fine[e];
      }
      if (tid < NCOARSE) gpos[lw * NCOARSE + tid] += hist[tid];
      __syncthreads();
    }
  }
}

// ---- byte windows (narrow U8 / U16 scalars: MSM_HIP_SCALARS_U8, MSM_HIP_SCALARS_U16, and their signed forms) -------------------------------
// A window is one byte of the scalar (U8: 1 window, U16: 2 -- low byte, high byte), its digit the byte itself: unsigned, bucket slot = value
// (1 .. 255; a zero byte emits no entry).  With 256 slots a one-level counting sort suffices -- no coarse bins, so a few-distinct-values vector
// (booleans: every entry in slot 1) never meets k_sort_fine's huge-bin fallback.  The four kernels leave exactly what k_sort_fine leaves:
// val_idxs grouped by slot (point index, sign bit 0), col_ptr over the launch's whole bucket grid (slots 256 .. half hold the window's total:
// empty), the SMVP's chunk table and chunk-length word.  Everything behind them (SMVP, stitch, bucket reduce on the 12-bit grid) is unchanged;
// the host weighs window j by 2^(8 j).
// Signed forms (NB = -1, -2: I8 / I16): the digits are the bytes of |v| -- at most 128 in I8's byte and I16's high byte, so the 255 slots
// suffice -- and every entry of a negative value carries its sign in bit 31, which the SMVP subtracts on.
// Layouts: counts[lw][tile][256] and bin_total[lw][256] in the arrays of the coarse sort, which hold BYTE_MAXLW windows of 256 bins.
template <int NB>
__device__ __forceinline__ uint32_t ld_byte_scalar(const uint8_t* v, size_t i) {
  static_assert(NB == 1 || NB == 2, "byte windows: U8 / U16");
  if constexpr (NB == 1) return v[i];
  else return reinterpret_cast<const uint16_t*>(v)[i];
}
// ... of the format NB names (narrow_width): the magnitude, and the sign in `neg`
template <int NB>
__device__ __forceinline__ uint32_t ld_byte_scalar_fmt(const uint8_t* v, size_t i, uint32_t& neg) {
  uint32_t s = ld_byte_scalar<narrow_width(NB)>(v, i);
  neg = 0;
  if constexpr (NB < 0) {
    neg = s >> (8 * -NB - 1);
    if (neg) s = (0u - s) & ((1u << (8 * -NB)) - 1u);
  }
  return s;
}
// counting pass: grid (tiles, nvec); a 256-bin LDS histogram per (tile, window).  scalars: nvec x n x |NB| bytes (NB < 0: signed -- the bytes of |v|).
// Sparse (a SparseIdx argument, as k_count): an entry whose index is out of range counts as a zero scalar and sets ERRBIT_BAD_INDEX in sp.err
template <int NB, typename... Sparse>
__global__ void __launch_bounds__(256) k_byte_count(const uint8_t* __restrict__ scalars, size_t n, uint32_t tile_len, uint32_t tiles,
                                                    uint32_t* __restrict__ counts, Sparse... sparse) {
  constexpr bool SPARSE = sizeof...(Sparse) != 0;
  constexpr int NW = narrow_width(NB);
  const SparseIdx sp = sparse_arg(sparse...);
  __shared__ uint32_t hist[NW * BYTE_BINS];
  const int tid = threadIdx.x, v = blockIdx.y;
#pragma unroll
  for (int j = 0; j < NW; j++) hist[j * BYTE_BINS + tid] = 0;
  __syncthreads();
  const uint8_t* sv = scalars + (size_t)v * n * NW;
  const size_t base = (size_t)blockIdx.x * tile_len, end = base + tile_len < n ? base + tile_len : n;
  for (size_t i = base + tid; i < end; i += 256) {
    if constexpr (SPARSE) {
      if (sp.idx[i] >= sp.n_bases) {
        atomicOr(sp.err, ERRBIT_BAD_INDEX);
        continue;
      }
    }
    uint32_t neg;
    const uint32_t s = ld_byte_scalar_fmt<NB>(sv, i, neg);
#pragma unroll
    for (int j = 0; j < NW; j++) {
      const uint32_t b = (s >> (8 * j)) & 0xffu;
      if (b) atomicAdd(&hist[j * BYTE_BINS + b], 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NW; j++) counts[((size_t)(v * NW + j) * tiles + blockIdx.x) * BYTE_BINS + tid] = hist[j * BYTE_BINS + tid];
}
// scan over the tiles: one wave per (window, bin) -- counts[lw][tile][bin] becomes the bin's entries in earlier tiles, bin_total[lw][bin] its size
__global__ void __launch_bounds__(256) k_byte_scan(uint32_t* __restrict__ counts, uint32_t tiles, uint32_t* __restrict__ bin_total) {
  const int lw = blockIdx.y, lane = threadIdx.x & 63;
  const int bin = blockIdx.x * 4 + (threadIdx.x >> 6);
  uint32_t* c = counts + (size_t)lw * tiles * BYTE_BINS + bin;
  uint32_t run = 0;
  for (uint32_t t0 = 0; t0 < tiles; t0 += 64) {
    const uint32_t t = t0 + lane;
    const uint32_t v = t < tiles ? c[(size_t)t * BYTE_BINS] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (t < tiles) c[(size_t)t * BYTE_BINS] = run + x - v;
    run += __shfl(x, 63);
  }
  if (lane == 0) bin_total[lw * BYTE_BINS + bin] = run;
}
// scatter pass: grid (tiles, nvec).  Every workgroup turns its windows' 256 bin totals into slot starts; workgroup (0, v) publishes col_ptr of
// vector v's windows over the whole grid of `half` slots, workgroup (0, 0) the launch's SMVP chunk length (the fullest of its w_count windows).
// Entries are placed with LDS cursors (order within a slot: unspecified, as everywhere).
// Sparse (a SparseIdx argument): entry i carries base idx[i]; an out-of-range one is skipped, as k_byte_count skipped it.
// NB < 0 (I8 / I16): the entries of a negative value carry bit 31.
template <int NB, typename... Sparse>
__global__ void __launch_bounds__(256) k_byte_scatter(const uint8_t* __restrict__ scalars, size_t n, size_t stride, uint32_t tile_len, uint32_t tiles,
                                                      int w_count, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ bin_total,
                                                      uint32_t* __restrict__ col_ptr, uint32_t half, uint32_t* __restrict__ val_idxs,
                                                      uint32_t chunks, uint32_t host_chunk_len, uint32_t* __restrict__ chunk_len_dev,
                                                      Sparse... sparse) {
  constexpr bool SPARSE = sizeof...(Sparse) != 0;
  constexpr int NW = narrow_width(NB);
  const SparseIdx sp = sparse_arg(sparse...);
  __shared__ uint32_t cur[NW * BYTE_BINS];
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t wtotal, max_total;
  const int tid = threadIdx.x, v = blockIdx.y;
  if (tid == 0) max_total = 0;
  for (int j = 0; j < NW; j++) {
    const int lw = v * NW + j;
    const uint32_t bt = bin_total[lw * BYTE_BINS + tid];
    const uint32_t excl = block_excl_scan_256(bt, wave_tot);
    cur[j * BYTE_BINS + tid] = excl + counts[((size_t)lw * tiles + blockIdx.x) * BYTE_BINS + tid];
    if (tid == BYTE_BINS - 1) wtotal = excl + bt;
    __syncthreads();
    if (blockIdx.x == 0) {
      uint32_t* cp = col_ptr + (size_t)lw * (half + 1);
      cp[tid] = excl;  // (slot 0: no entries, start 0)
      for (uint32_t k = BYTE_BINS + tid; k <= half; k += 256) cp[k] = wtotal;
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && blockIdx.y == 0) {  // the chunk length: the fullest window of the launch spread over all `chunks` lanes
    for (int lw = 0; lw < w_count; lw++) {
      const uint32_t excl = block_excl_scan_256(bin_total[lw * BYTE_BINS + tid], wave_tot);
      if (tid == BYTE_BINS - 1) atomicMax(&max_total, excl + bin_total[lw * BYTE_BINS + tid]);
    }
    __syncthreads();
    if (tid == 0) *chunk_len_dev = smvp_chunk_len(max_total, chunks, host_chunk_len);
  }
  const uint8_t* sv = scalars + (size_t)v * n * NW;
  const size_t base = (size_t)blockIdx.x * tile_len, end = base + tile_len < n ? base + tile_len : n;
  for (size_t i = base + tid; i < end; i += 256) {
    uint32_t rec = (uint32_t)i;
    if constexpr (SPARSE) {
      rec = sp.idx[i];
      if (rec >= sp.n_bases) continue;
    }
    uint32_t neg;
    const uint32_t s = ld_byte_scalar_fmt<NB>(sv, i, neg);
    rec |= neg << 31;
#pragma unroll
    for (int j = 0; j < NW; j++) {
      const uint32_t b = (s >> (8 * j)) & 0xffu;
      if (b) val_idxs[(size_t)(v * NW + j) * stride + atomicAdd(&cur[j * BYTE_BINS + b], 1u)] = rec;
    }
  }
}
// the SMVP's chunk table: chunk c of window lw starts at entry c * chunk_len; its slot is the last of 1 .. 255 whose run starts at or before it
__global__ void __launch_bounds__(256) k_byte_chunks(const uint32_t* __restrict__ col_ptr, uint32_t half, uint32_t chunks,
                                                     const uint32_t* __restrict__ chunk_len_dev, uint32_t* __restrict__ chunk_slot) {
  __shared__ uint32_t cp[BYTE_BINS + 1];
  const int lw = blockIdx.y, tid = threadIdx.x;
  const uint32_t* src = col_ptr + (size_t)lw * (half + 1);
  cp[tid] = src[tid];
  if (tid == 0) cp[BYTE_BINS] = src[BYTE_BINS];
  __syncthreads();
  const uint32_t c = blockIdx.x * 256 + tid;
  const uint64_t e = (uint64_t)c * *chunk_len_dev;
  if (c >= chunks || e >= cp[BYTE_BINS]) return;
  uint32_t lo = 1, hi = BYTE_BINS - 1;  // cp[lo] <= e (cp[1] = 0); find the largest such slot
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (cp[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  chunk_slot[(size_t)lw * chunks + c] = lo;
}

// ---- wide fixed-base tables (round 4; SURVEY.md 8f-2, MSM_HIP_BASES_PRECOMPUTE_WIDE) ------------------------------------------------
// With tables T_w[i] = 2^(C w) P_i the number of bucket additions of an MSM is ceil(255 / C) * n and nothing ties C to the bucket count of
// a window any more -- there is one bucket set of 2^(C-1) slots.  C = 17 / 19 / 20: 15 / 14 / 13 additions per point instead of 16 (the SMVP,
// the dominant kernel, shrinks by that much).  The slot of magnitude m (1 .. 2^(C-1)) is split as
//     m = hi * 2^15 + value(slot),   hi = (m - 1) >> 15,   slot = m & 0x7fff,   value(slot) = slot, or 2^15 for slot 0
// and `hi` is handled as a VIRTUAL WINDOW: local window hi holds the 2^15 slots of that range, so that everything behind the two
// scalar-reading passes -- fine sort, SMVP, stitch, row / column sums -- runs unchanged on 2^(C-16) local windows of 2^15 slots.  The reduce leaves,
// per virtual window, the weighted sum W_hi = sum_slot value(slot) B[hi][slot] AND the plain total TC_hi = sum_slot B[hi][slot] (the column
// total of the bit-plane sums, k_bpr_planes), and the host finishes  sum_hi W_hi + 2^15 * sum_hi hi * TC_hi  (host_g1.h: combine_wide).
// The entries of virtual window hi are stored at tmp_val[hi][...]: with skewed scalars one virtual window may receive all T n entries, so
// the per-window stride is T n (the host sizes the arrays for it); the lanes of the SMVP are sized for the uniform case and the device
// picks the chunk length from the fullest window as always (smvp_chunk_len).
// Which C (profiles/r04_wide_tables.txt): what an MSM costs in the pipeline is sort + SMVP + the stitch / reduce work that runs beside the
// next launch, and that grows with the bucket sets -- 20 bits (16 of them) loses to the endomorphism mode at 2^20 although its SMVP is 0.85 ms
// alone against 0.99, and wins by 18 % at 2^24; 17 bits (2 of them) wins at 2^20.
// The digit width C is a template parameter of the two kernels (the tables are built for it when the bases are set: msm_plan.h, pick_wide_bits, picks it from
// the number of bases -- 16 bits up to 2^16 points and 17 up to 2^20, where the bucket sets' stitch / reduce still counts, 20 beyond).
template <int C>
struct WideCfg {
  static_assert(C >= 16 && C <= 20, "digit bits of the wide tables");
  static constexpr int BITS = C;
  static constexpr int TABLES = WinCfg<C>::NWIN;  // 16 / 15 / 15 / 14 / 13 tables 2^(C w) P_i at 16 / 17 / 18 / 19 / 20 bits
  static constexpr int VWIN = 1 << (C - WBITS);   // 1 / 2 / 4 / 8 / 16 virtual windows of 2^15 slots
  static constexpr int KEYS = VWIN * NCOARSE;     // (virtual window, coarse bin) runs
  static_assert(VWIN <= MAXLW, "virtual windows are local windows");
};
// The top digit.  The last window holds what is left of the scalar above bit C (T - 1) -- 16 / 7 / 14 bits at C = 17 / 19 / 20 -- so its
// magnitudes would all fall into the lowest virtual windows, which would then carry far more entries than the others, and the SMVP's lanes are
// as long as the fullest window makes them (first measurement at 20 bits: SMVP 1.06 ms instead of 0.85).  The top table is therefore
// 2^(C (T - 1) - top_shift) P_i and the top digit is used as d << top_shift: the same product for any point (exact integer arithmetic: no
// assumption on the point's order), spread over the virtual windows.  top_shift (msm_plan.h: wide_top_shift) is the largest for which the top
// digit of every scalar below the scalar field's modulus stays within 2^(C-1): for BN254 0 / 11 / 5 at 17 / 19 / 20 bits.  A scalar whose
// shifted top digit passes that -- at or above the modulus -- is rejected like one that overflows the reference's recode (ERRBIT_SCALAR_CARRY).
// signed C-bit digit of window w of the biased scalar t (WinCfg<C>::WORDS words): its magnitude 1 .. 2^(C - 1) (0: no entry) and sign
template <int C>
__device__ __forceinline__ uint32_t wide_digit(const uint32_t* t, int w, int top_shift, uint32_t& sign, uint32_t& overflow) {
  constexpr uint32_t H = 1u << (C - 1);
  const int bit = C * w, i = bit >> 5, sh = bit & 31;
  uint32_t b = t[i] >> sh;
  if (sh + C > 32 && i + 1 < WinCfg<C>::WORDS) b |= t[i + 1] << (32 - sh);
  if (w == WideCfg<C>::TABLES - 1) {
    // the top digit: never negative (nothing above it carries into it), so its field is read with everything above it -- a digit of exactly
    // 2^(C-1), which the C-bit field cannot hold (17-bit digits of a scalar of 2^254 or more: Pallas, Vesta), is the bucket magnitude 2^(C-1) like
    // any other; beyond that, or beyond it after the shift, the scalar is rejected
    sign = 0;
    const uint32_t d = b - H;  // (b >= H: the bias bit of this window is set and the digit is not negative)
    if (d > (H >> top_shift)) {
      overflow = 1;
      return 0;
    }
    return d << top_shift;
  }
  b &= (1u << C) - 1u;
  sign = b < H ? 1u : 0u;
  return b >= H ? b - H : H - b;
}
// Magnitude m (1 .. 2^(C-1)) -> virtual window and bucket slot, INTERLEAVED (round 5):  vw = (m - 1) mod VWIN,  value(slot) = (m - 1) / VWIN + 1
// (1 .. 2^15; slot = value mod 2^15, i.e. slot 0 carries 2^15 as in every window).  Consecutive magnitudes go to consecutive virtual windows, so
// ANY smooth distribution of magnitudes -- the narrow top digit's included -- fills the virtual windows evenly: the shares of a window-sharded
// run (one virtual window per rank at 19 bits and 8 GPUs) are balanced, a whole MSM's windows need the same chunk length, and the top digit
// needs no shift.  (Rounds 4's contiguous ranges, vw = (m - 1) >> 15, put the whole top digit into the lowest windows; its shift spread it as
// multiples of 2^shift -- every 32nd slot of a 20-bit set four times as full as its neighbours, which a stitch wave pays for in all 64 lanes.)
// The window's weighted sum W_vw = sum_slot value(slot) B[slot] and plain total TC_vw give  sum_m m B_m = VWIN W_vw - (VWIN - 1 - vw) TC_vw.
template <int C>
__device__ __forceinline__ uint32_t wide_slot(uint32_t mag) { return (((mag - 1u) >> (C - WBITS)) + 1u) & 0x7fffu; }
template <int C>
__device__ __forceinline__ uint32_t wide_key(uint32_t mag) {  // (virtual window, coarse bin); mag = 0 gives garbage: callers test mag first
  return (((mag - 1u) & (uint32_t)(WideCfg<C>::VWIN - 1)) << 7) | (wide_slot<C>(mag) >> 8);
}

// first pass: counts[lw][tile][bin] (the layout of k_count), local window lw = v * VWIN + hi for scalar vector v of the launch's nvec
// (vec_stride words apart: several whole MSMs over the same tables share one kernel sequence, as in k_count)
// Virtual-window SHARES (round 5: the wide tables behind the window-sharded / multi-GPU entry points): a launch may take only the virtual
// windows [v_begin, v_begin + v_count) of every vector -- a rank of an 8-GPU run at 19-bit digits takes ONE of the 8: a bucket set of 2^15
// slots and, for uniform scalars, 14 n / 8 entries instead of the 2 n entries and two bucket sets of two 16-bit windows.  Both passes still
// recode every digit of every scalar (the carry chain runs across the digits; 32 B per scalar) and drop the digits whose magnitude falls
// outside the range; local window lw = v * v_count + (hi - v_begin).  Whole MSMs: v_begin = 0, v_count = VWIN.
template <int C>
__global__ void __launch_bounds__(256) k_count_wide(const uint32_t* __restrict__ scalars, size_t n, uint32_t tile_len, uint32_t tiles, int nvec,
                                                    size_t vec_stride, uint32_t* __restrict__ counts, uint32_t* __restrict__ err, int top_shift,
                                                    int v_begin, int v_count) {
  constexpr int SW = 8;  // full-length scalars
  constexpr int WIDE_KEYS = WideCfg<C>::KEYS, WIDE_TABLES = WideCfg<C>::TABLES;
  __shared__ uint32_t cnt[WIDE_KEYS];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * tile_len;
  const size_t end = base + tile_len < n ? base + tile_len : n;
  uint32_t bad = 0;
  const int v = blockIdx.y;  // grid (tiles, nvec): one tile of one scalar vector per workgroup (as k_count)
  (void)nvec;
  const uint32_t keys = (uint32_t)v_count * NCOARSE;  // (virtual window, coarse bin) runs of this launch's share (<= WIDE_KEYS)
  for (int i = tid; i < WIDE_KEYS; i += 256) cnt[i] = 0;
  __syncthreads();
  for (size_t i0 = base; i0 < end; i0 += 256) {
    const size_t i = i0 + tid;
    if (i >= end) continue;
    uint32_t s[SW], tb[WinCfg<C, SW>::WORDS], t16[8], neg = 0;
    ld_scalar<SW>(scalars + (size_t)v * vec_stride + i * SW, s, neg);
    (void)bias_scalar<C, SW>(s, tb);  // (a top digit beyond the recode's range is caught where it is read: wide_digit)
    bad |= bias_scalar<16>(s, t16);   // the input contract of every mode: what overflows the reference's 16-bit recode is rejected (test/utils.rs:150-152)
#pragma unroll
    for (int w = 0; w < WIDE_TABLES; w++) {
      uint32_t sign;
      const uint32_t mag = wide_digit<C>(tb, w, top_shift, sign, bad);
      const uint32_t key = wide_key<C>(mag) - ((uint32_t)v_begin << 7);  // (mag = 0: no entry, whatever the key says)
      if (mag && key < keys) atomicAdd(&cnt[key], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < (int)keys; i += 256)
    counts[((size_t)(v * v_count + i / NCOARSE) * tiles + blockIdx.x) * NCOARSE + (i % NCOARSE)] = cnt[i];
  if (bad) atomicOr(err, ERRBIT_SCALAR_CARRY);
}

// ---- shares of a few virtual windows: the first pass leaves a COMPACT LIST of the share's entries (round 5) ---------------------------------
// A rank of a window-sharded run keeps an eighth of the digits (one of 8 virtual windows at 19 bits, two of 16 at 20).  Ranking and staging
// them where they are found -- 13 x 8 digit positions per thread, an eighth of the lanes active at each -- made the second pass the longest
// kernel of the sort (310 - 540 us per launch of 8 vectors against 153 for the digit-plane scatter of two 16-bit windows,
// profiles/r05_wide_shares.txt).  So the divergent work is done ONCE, here: every kept digit is appended (wave-aggregated: one LDS atomic per
// wave, digit position and virtual window) to the list of its (local window, sub-tile of LIST_SUB scalars), and the second pass
// (k_scatter_list) reads the lists with every lane busy.
//   entry  = position within the sub-tile (11 bits) | table w << 11 | sign << 15 | bucket slot << 16   (the virtual window is the list's)
//   list of (lw, sub-tile q): list[lw * stride + q * LIST_SUB * TABLES ...], list_len[lw * subtiles + q] entries -- the arrays of the final
//   slot order (val_idxs), free until the fine sort writes them, sized for a share that receives every digit (stride >= n TABLES).
template <int C>
__global__ void __launch_bounds__(256) k_count_wide_list(const uint32_t* __restrict__ scalars, size_t n, uint32_t tile_len, uint32_t tiles, int nvec,
                                                         size_t vec_stride, uint32_t* __restrict__ counts, uint32_t* __restrict__ err, int top_shift,
                                                         int v_begin, int v_count, uint32_t* __restrict__ list, uint32_t* __restrict__ list_len,
                                                         size_t stride, uint32_t subtiles) {
  constexpr int SW = 8;
  constexpr int WIDE_TABLES = WideCfg<C>::TABLES;
  constexpr int KEYS_MAX = WIDE_SHARE_VWIN_MAX * NCOARSE;
  __shared__ uint32_t cnt[KEYS_MAX];
  __shared__ uint32_t lcount[WIDE_SHARE_VWIN_MAX];
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t base = (size_t)blockIdx.x * tile_len;  // (tile_len is a multiple of LIST_SUB or the only tile's: sub-tiles never straddle tiles)
  const size_t end = base + tile_len < n ? base + tile_len : n;
  uint32_t bad = 0;
  const int v = blockIdx.y;
  (void)nvec;
  const uint32_t keys = (uint32_t)v_count * NCOARSE;
  for (int i = tid; i < KEYS_MAX; i += 256) cnt[i] = 0;
  if (tid < WIDE_SHARE_VWIN_MAX) lcount[tid] = 0;
  __syncthreads();
  for (size_t sub = base; sub < end; sub += LIST_SUB) {
    const size_t sub_end = sub + LIST_SUB < end ? sub + LIST_SUB : end;
    const uint32_t q = (uint32_t)(sub / LIST_SUB);
    for (size_t i0 = sub; i0 < sub_end; i0 += 256) {
      const size_t i = i0 + tid;
      const bool valid = i < sub_end;
      uint32_t s[SW], tb[WinCfg<C, SW>::WORDS], t16[8], neg = 0;
#pragma unroll
      for (int k = 0; k < SW; k++) s[k] = 0;  // (a lane beyond the end recodes zero: no entries)
      if (valid) ld_scalar<SW>(scalars + (size_t)v * vec_stride + i * SW, s, neg);
      (void)bias_scalar<C, SW>(s, tb);
      bad |= bias_scalar<16>(s, t16);   // the input contract of every mode (test/utils.rs:150-152)
      // every kept digit's entry and its place among the wave's kept digits of the same local window (ballots only: no LDS round trip) ...
      uint32_t ent[WIDE_TABLES], place[WIDE_TABLES];  // place: local window << 28 | position within the wave's block of that window; 0xffffffff: not kept
      uint32_t wave_cnt[WIDE_SHARE_VWIN_MAX];         // wave-uniform running counts
#pragma unroll
      for (int vw = 0; vw < WIDE_SHARE_VWIN_MAX; vw++) wave_cnt[vw] = 0;
#pragma unroll
      for (int w = 0; w < WIDE_TABLES; w++) {
        uint32_t sign;
        const uint32_t mag = wide_digit<C>(tb, w, top_shift, sign, bad);
        const uint32_t key = wide_key<C>(mag) - ((uint32_t)v_begin << 7);
        const bool keep = mag && key < keys;
        if (keep) atomicAdd(&cnt[key], 1u);
        ent[w] = (uint32_t)(i - sub) | ((uint32_t)w << 11) | (sign << 15) | (wide_slot<C>(mag) << 16);
        place[w] = 0xffffffffu;
#pragma unroll
        for (int vw = 0; vw < WIDE_SHARE_VWIN_MAX; vw++) {
          if (vw >= v_count) break;  // wave-uniform
          const bool mine = keep && (key >> 7) == (uint32_t)vw;
          const unsigned long long mm = __ballot(mine);
          if (mine) place[w] = ((uint32_t)vw << 28) | (wave_cnt[vw] + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull)));
          wave_cnt[vw] += (uint32_t)__popcll(mm);
        }
      }
      // ... ONE reservation per wave and local window for all of them (one LDS round trip instead of one per digit position), then the stores
      uint32_t wave_base[WIDE_SHARE_VWIN_MAX];
#pragma unroll
      for (int vw = 0; vw < WIDE_SHARE_VWIN_MAX; vw++) {
        wave_base[vw] = 0;
        if (vw < v_count && lane == 0 && wave_cnt[vw]) wave_base[vw] = atomicAdd(&lcount[vw], wave_cnt[vw]);
      }
#pragma unroll
      for (int vw = 0; vw < WIDE_SHARE_VWIN_MAX; vw++) wave_base[vw] = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_base[vw]);
#pragma unroll
      for (int w = 0; w < WIDE_TABLES; w++) {
        if (place[w] != 0xffffffffu) {
          const uint32_t vw = place[w] >> 28;
          const uint32_t b = vw == 0 ? wave_base[0] : vw == 1 ? wave_base[1] : vw == 2 ? wave_base[2] : wave_base[3];
          list[(size_t)(v * v_count + vw) * stride + (size_t)q * (LIST_SUB * WIDE_TABLES) + b + (place[w] & 0x0fffffffu)] = ent[w];
        }
      }
    }
    __syncthreads();
    if (tid < v_count) {
      list_len[(size_t)(v * v_count + tid) * subtiles + q] = lcount[tid];
      lcount[tid] = 0;
    }
    __syncthreads();
  }
  for (int i = tid; i < (int)keys; i += 256)
    counts[((size_t)(v * v_count + i / NCOARSE) * tiles + blockIdx.x) * NCOARSE + (i % NCOARSE)] = cnt[i];
  if (bad) atomicOr(err, ERRBIT_SCALAR_CARRY);
}

// second pass of a share: grid (tiles, local windows) -- a workgroup takes the lists of ONE local window over its tile, LIST_CHUNK entries at a
// time: histogram of the coarse bins, scan, cursor placement into the LDS staging, coalesced write-out (k_scatter_coarse's scheme with every lane
// busy).
constexpr int LIST_CHUNK = 4096;
__global__ void __launch_bounds__(256) k_scatter_list(const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_len, size_t stride, uint32_t region,
                                                      uint32_t subtiles, size_t n, uint32_t tile_len, uint32_t tiles, int w_eff,
                                                      const uint32_t* __restrict__ counts, const uint32_t* __restrict__ bin_total,
                                                      uint32_t* __restrict__ coarse_ptr, uint32_t* __restrict__ tmp_val, uint8_t* __restrict__ tmp_fine,
                                                      size_t table_stride, uint32_t chunks, uint32_t host_chunk_len, uint32_t* __restrict__ chunk_len_dev) {
  __shared__ uint32_t gpos[NCOARSE];
  __shared__ uint32_t hist[NCOARSE];
  __shared__ uint32_t lstart[NCOARSE];
  __shared__ uint32_t cur[NCOARSE];
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t st_val[LIST_CHUNK];
  __shared__ uint32_t st_dst[LIST_CHUNK];
  __shared__ uint8_t st_fine[LIST_CHUNK];
  __shared__ uint32_t max_total;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lw = blockIdx.y;
  if (tid == 0) max_total = 0;
  __syncthreads();
  // start of every coarse bin's run of this tile (exclusive scan of the window's 128 bin totals + what earlier tiles put there); workgroup
  // (0, 0) does it for every local window of the launch (its own last): it publishes all bin starts and the launch's chunk length
  const bool publisher = blockIdx.x == 0 && blockIdx.y == 0;
  for (int pl = publisher ? w_eff - 1 : lw; pl >= lw; pl--) {
    const int bin = tid;  // threads 0 .. 127: one bin each (two waves)
    const bool live = tid < NCOARSE;
    const uint32_t v = live ? bin_total[pl * NCOARSE + bin] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[wid] = x;
    __syncthreads();
    const uint32_t incl = x + ((wid & 1) ? wave_tot[wid - 1] : 0u);
    if (live) gpos[bin] = incl - v + counts[((size_t)pl * tiles + blockIdx.x) * NCOARSE + bin];
    if (live && publisher) {
      coarse_ptr[(size_t)pl * (NCOARSE + 1) + bin] = incl - v;
      if (bin == NCOARSE - 1) {
        coarse_ptr[(size_t)pl * (NCOARSE + 1) + NCOARSE] = incl;
        atomicMax(&max_total, incl);
      }
    }
    __syncthreads();
  }
  if (publisher && tid == 0) *chunk_len_dev = smvp_chunk_len(max_total, chunks, host_chunk_len);
  const size_t tile_base = (size_t)blockIdx.x * tile_len;
  const size_t tile_end = tile_base + tile_len < n ? tile_base + tile_len : n;
  uint32_t* ov = tmp_val + (size_t)lw * stride;
  uint8_t* of = tmp_fine + (size_t)lw * stride;
  for (size_t sub = tile_base; sub < tile_end; sub += LIST_SUB) {
    const uint32_t q = (uint32_t)(sub / LIST_SUB);
    const uint32_t len = list_len[(size_t)lw * subtiles + q];
    const uint32_t* src = list + (size_t)lw * stride + (size_t)q * region;
    for (uint32_t lo = 0; lo < len; lo += LIST_CHUNK) {
      const uint32_t cnt = len - lo < (uint32_t)LIST_CHUNK ? len - lo : (uint32_t)LIST_CHUNK;
      if (tid < NCOARSE) hist[tid] = 0;
      __syncthreads();
      uint32_t ent[LIST_CHUNK / 256];
#pragma unroll
      for (int j = 0; j < LIST_CHUNK / 256; j++) {
        const uint32_t e = (uint32_t)j * 256 + tid;
        ent[j] = e < cnt ? src[lo + e] : 0xffffffffu;     // (a slot is 15 bits: no entry has bit 31 set)
        if (e < cnt) atomicAdd(&hist[ent[j] >> 24], 1u);  // coarse bin = slot >> 8 = entry >> 24
      }
      __syncthreads();
      const uint32_t mine = tid < NCOARSE ? hist[tid] : 0u;
      const uint32_t excl = block_excl_scan_256(mine, wave_tot);
      if (tid < NCOARSE) {
        lstart[tid] = excl;
        cur[tid] = excl;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < LIST_CHUNK / 256; j++) {
        if (ent[j] != 0xffffffffu) {
          const uint32_t bin = ent[j] >> 24;
          const uint32_t e = atomicAdd(&cur[bin], 1u);
          // window w of point i = record w * n_bases + i
          st_val[e] = ((uint32_t)(((ent[j] >> 11) & 15u) * table_stride) + (uint32_t)sub + (ent[j] & 2047u)) | (((ent[j] >> 15) & 1u) << 31);
          st_fine[e] = (uint8_t)((ent[j] >> 16) & 0xffu);
          st_dst[e] = gpos[bin] + (e - lstart[bin]);
        }
      }
      __syncthreads();
      for (uint32_t e = tid; e < cnt; e += 256) {
        const uint32_t d = st_dst[e];
        ov[d] = st_val[e];
        of[d] = st_fine[e];
      }
      if (tid < NCOARSE) gpos[tid] += hist[tid];
      __syncthreads();
    }
  }
}

// second pass: the LDS-ranked, LDS-staged scatter of k_scatter_coarse over all (virtual window, coarse bin) runs at once -- 256 / 1024 / 2048
// of them at 17 / 19 / 20 bits.  ALL digits of the 2048 scalars of a block iteration are staged together (30 720 / 28 672 / 26 624 entries:
// 120 / 28 / 13 per run): ranked per window as k_scatter_coarse does, a run would receive a fraction of that per iteration and every 4-byte
// store would be a memory transaction of its own.  One workgroup of 512 threads per CU.  (With 1024 scalars per iteration the kernel took
// 244 / 351 / 471 us at 2^22 points: the shorter the runs, the worse the stores coalesce.)
//
// Two shapes of the same kernel (WideShape<C, SHARE>):
//   whole MSMs   512 threads, 4 scalars per thread and iteration (3 at 16 bits), every run of the bucket set, LDS for every entry the iteration's
//                scalars can produce (153 - 158 KB: one workgroup per CU)
//   shares       (round 5: a rank's virtual windows, k_count_wide) -- at most 4 virtual windows, an eighth of the entries for uniform scalars at 8
//                ranks: with the whole-MSM shape the 4096 workgroups of a launch of 8 vectors ran one per CU, sixteen rounds of a latency-bound
//                kernel (385 - 544 us per launch against 153 for the digit-plane scatter of two 16-bit windows, profiles/r05_wide_shares.txt).
//                256 threads, 8 scalars per thread, LDS for WIDE_SHARE_CAP entries (38 KB: four workgroups per CU), no ranks in registers.  Skewed
//                scalars may put EVERY digit of an iteration into the share (14 x 2048 entries): an iteration whose entries pass the staging is
//                redone one scalar per thread at a time.
#ifndef WIDE_SHARE_REREAD
#define WIDE_SHARE_REREAD 1  // A/B aid (same-box pairs, profiles/r05_wide_shares.txt: 0.2198 - 0.2231 vs 0.2242 - 0.2256 ms per MSM share): 1 = the scalars are read again for the second pass (one at a time) instead of staying in registers
#endif
constexpr int WIDE_THREADS = 512;
constexpr int WIDE_SHARE_THREADS = 256, WIDE_SHARE_CAP = 6144;
template <int C, bool SHARE>
struct WideScatterShape {
  static constexpr int THREADS = SHARE ? WIDE_SHARE_THREADS : WIDE_THREADS;
  static constexpr int PER = SHARE ? 8 : (C == 16 ? 3 : 4);                    // scalars per thread and block iteration
  static constexpr int SUB = THREADS * PER;                                    // scalars staged per block iteration
  static constexpr int KEYS = SHARE ? (WideCfg<C>::VWIN < WIDE_SHARE_VWIN_MAX ? WideCfg<C>::VWIN : WIDE_SHARE_VWIN_MAX) * NCOARSE : WideCfg<C>::KEYS;
  static constexpr int STAGE = SHARE ? WIDE_SHARE_CAP : SUB * WideCfg<C>::TABLES;  // entries the LDS staging holds
  static_assert(SUB <= 2048 && WideCfg<C>::TABLES <= 16, "sign | window | position in 16 bits");
  static_assert(STAGE * 5 + KEYS * (SHARE ? 16 : 12) + 64 <= 160 * 1024, "LDS of a workgroup");
};
template <int C, bool SHARE>
__global__ void __launch_bounds__((WideScatterShape<C, SHARE>::THREADS), (SHARE ? (WIDE_SHARE_REREAD ? 4 : 3) : 1)) k_scatter_wide(const uint32_t* __restrict__ scalars, size_t n, size_t stride, uint32_t tile_len,
                                                               uint32_t tiles, int nvec, size_t vec_stride, const uint32_t* __restrict__ counts,
                                                               const uint32_t* __restrict__ bin_total, uint32_t* __restrict__ coarse_ptr,
                                                               uint32_t* __restrict__ tmp_val, uint8_t* __restrict__ tmp_fine, size_t table_stride,
                                                               uint32_t chunks, uint32_t host_chunk_len, uint32_t* __restrict__ chunk_len_dev, int top_shift,
                                                               int v_begin, int v_count) {
  using Shape = WideScatterShape<C, SHARE>;
  constexpr int SW = 8;  // full-length scalars
  constexpr int WIDE_KEYS = Shape::KEYS, WIDE_TABLES = WideCfg<C>::TABLES, THREADS = Shape::THREADS;
  const int keys = v_count * NCOARSE;                // runs of this launch's share of the virtual windows (k_count_wide); WIDE_KEYS for whole MSMs
  const uint32_t key0 = (uint32_t)v_begin << 7;
  // 5 bytes of LDS per staged entry -- its (virtual window, coarse bin) run, its fine slot, and sign | window | position within the iteration's
  // scalars (16 bits: the record index is put together when the entry is written out) -- so that 2048 scalars (1536 at 16 bits) fit one
  // iteration: twice the run length of the 4-byte index staged before (153 - 158 KB of the 160 KB a workgroup may hold)
  constexpr int WIDE_PER = Shape::PER;
  constexpr int WIDE_SUB = Shape::SUB;      // scalars staged per block iteration
  constexpr int WIDE_STAGE = Shape::STAGE;  // entries staged at a time
  __shared__ uint32_t gpos[WIDE_KEYS];    // write cursor of every run of this tile, relative to its virtual window's array
  __shared__ uint32_t hist[WIDE_KEYS];
  __shared__ uint32_t lstart[WIDE_KEYS];
  __shared__ uint32_t cur[SHARE ? WIDE_KEYS : 1];  // share shape: cursor of every run while an iteration's entries are staged
  __shared__ uint16_t st_loc[WIDE_STAGE];
  __shared__ uint16_t st_key[WIDE_STAGE];
  __shared__ uint8_t st_fine[WIDE_STAGE];
  __shared__ uint32_t wave_tot[THREADS / 64];
  __shared__ uint32_t max_total;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) max_total = 0;
  __syncthreads();
  const size_t tile_base = (size_t)blockIdx.x * tile_len;
  const size_t tile_end = tile_base + tile_len < n ? tile_base + tile_len : n;
  // grid (tiles, nvec): a workgroup scatters one tile of ONE scalar vector (one MSM of the launch), whose v_count local windows start at lw0.
  // Start of every run: exclusive scan of each virtual window's 128 bin totals (a pair of waves per window) + what
  // earlier tiles put there.  Workgroup (0, 0) does this for every vector of the launch (its own last: gpos keeps the last one scanned): it
  // publishes all bin starts (coarse_ptr[lw][0 .. 128]) and the launch's chunk length.
  const bool publisher = blockIdx.x == 0 && blockIdx.y == 0;
  const int lw0 = (int)blockIdx.y * v_count;
  const uint32_t* sv = scalars + (size_t)blockIdx.y * vec_stride;
  for (int pv = publisher ? nvec - 1 : (int)blockIdx.y; pv >= (int)blockIdx.y; pv--)
  for (int i0 = 0; i0 < keys; i0 += THREADS) {
    const int i = i0 + tid, lw = pv * v_count + i / NCOARSE, bin = i % NCOARSE;
    const bool live = i < keys;  // (fewer runs than threads: 17-bit digits, shares of a few virtual windows)
    const uint32_t v = live ? bin_total[lw * NCOARSE + bin] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[wid] = x;
    __syncthreads();
    const uint32_t incl = x + ((wid & 1) ? wave_tot[wid - 1] : 0u);
    if (live) gpos[i] = incl - v + counts[((size_t)lw * tiles + blockIdx.x) * NCOARSE + bin];
    if (live && publisher) {
      coarse_ptr[(size_t)lw * (NCOARSE + 1) + bin] = incl - v;
      if (bin == NCOARSE - 1) {
        coarse_ptr[(size_t)lw * (NCOARSE + 1) + NCOARSE] = incl;
        atomicMax(&max_total, incl);
      }
    }
    __syncthreads();
  }
  if (publisher && tid == 0) *chunk_len_dev = smvp_chunk_len(max_total, chunks, host_chunk_len);
  // this thread's scalar j of the block iteration at `sub`, biased for the recode.  The scalars are read twice -- for the counts and for the
  // entries (the second time from the L2) --: held in registers across the scan they and the ranks passed the 256 registers a wave may have
  auto biased = [&](size_t sub, int j, uint32_t* tb) {
    const size_t i = sub + (size_t)j * THREADS + tid;
    uint32_t raw[SW], neg = 0;
#pragma unroll
    for (int k = 0; k < SW; k++) raw[k] = 0;  // an all-zero scalar recodes to all-zero digits: no entries
    if (i < tile_end) ld_scalar<SW>(sv + i * SW, raw, neg);
    (void)bias_scalar<C, SW>(raw, tb);
  };
  // exclusive scan of the run lengths hist[] -> lstart[]: KPT consecutive keys per thread (with fewer runs than threads, the first WIDE_KEYS threads
  // take one each); ends with a barrier
  auto scan_runs = [&]() {
    constexpr int KPT = WIDE_KEYS >= THREADS ? WIDE_KEYS / THREADS : 1;
    static_assert(KPT * THREADS == WIDE_KEYS || WIDE_KEYS < THREADS, "keys per thread");
    const bool mine = KPT * tid < WIDE_KEYS;
    uint32_t h[KPT], sum = 0;
#pragma unroll
    for (int k = 0; k < KPT; k++) {
      h[k] = mine ? hist[KPT * tid + k] : 0u;
      sum += h[k];
    }
    uint32_t x = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[wid] = x;
    __syncthreads();
    uint32_t run = x - sum;
    for (int k = 0; k < wid; k++) run += wave_tot[k];
#pragma unroll
    for (int k = 0; k < KPT; k++) {
      if (mine) lstart[KPT * tid + k] = run;
      run += h[k];
    }
    __syncthreads();
  };
  // the staged entries 0 .. cnt-1 (bin-major) to their runs; ends with a barrier
  auto write_out = [&](size_t sub, uint32_t cnt) {
    for (uint32_t e = tid; e < cnt; e += THREADS) {
      const uint32_t key = st_key[e];
      const size_t d = (size_t)(lw0 + (key >> 7)) * stride + gpos[key] + (e - lstart[key]);
      const uint32_t loc = st_loc[e];
      // window w of point i = record w * n_bases + i
      tmp_val[d] = ((uint32_t)(((loc >> 11) & 15u) * table_stride) + (uint32_t)sub + (loc & 2047u)) | ((loc >> 15) << 31);
      tmp_fine[d] = st_fine[e];
    }
    __syncthreads();
  };
  for (size_t sub = tile_base; sub < tile_end; sub += WIDE_SUB) {
    if constexpr (SHARE) {
      // Share shape: no ranks are kept -- an entry's place inside its run is drawn from a cursor when it is staged (any order inside a run is as
      // good as another) -- and the iteration's biased scalars stay in registers across both passes (8 x 9 words; their 8 loads are in flight
      // together): nothing is read twice, and the LDS alone bounds the workgroups per CU.
#if WIDE_SHARE_REREAD
#define WIDE_SHARE_UNROLL _Pragma("unroll 1")
#define WIDE_SHARE_TB(j) tb1
#define WIDE_SHARE_LOAD(j) uint32_t tb1[WinCfg<C, SW>::WORDS]; biased(sub, j, tb1)
#else
#define WIDE_SHARE_UNROLL _Pragma("unroll")
#define WIDE_SHARE_TB(j) tbs[j]
#define WIDE_SHARE_LOAD(j)
      uint32_t tbs[WIDE_PER][WinCfg<C, SW>::WORDS];
#pragma unroll
      for (int j = 0; j < WIDE_PER; j++) biased(sub, j, tbs[j]);
#endif
      for (int k = tid; k < WIDE_KEYS; k += THREADS) hist[k] = 0;
      __syncthreads();
      WIDE_SHARE_UNROLL
      for (int j = 0; j < WIDE_PER; j++) {
        WIDE_SHARE_LOAD(j);
#pragma unroll
        for (int w = 0; w < WIDE_TABLES; w++) {
          uint32_t sign, over = 0;
          const uint32_t mag = wide_digit<C>(WIDE_SHARE_TB(j), w, top_shift, sign, over);  // (an overflowing top digit: no entry here as in k_count_wide, which reports it)
          const uint32_t key = wide_key<C>(mag) - key0;                            // (outside this launch's virtual windows: no entry)
          if (mag && key < (uint32_t)keys) atomicAdd(&hist[key], 1u);
        }
        __builtin_amdgcn_sched_barrier(0);  // one scalar's digits at a time: hoisted together, the 8 x 14 digits and keys take 400 registers
      }
      __syncthreads();
      scan_runs();
      const uint32_t total = lstart[WIDE_KEYS - 1] + hist[WIDE_KEYS - 1];
      if (total <= (uint32_t)WIDE_STAGE) {  // block-uniform
        for (int k = tid; k < WIDE_KEYS; k += THREADS) cur[k] = lstart[k];
        __syncthreads();
        // (the digits are extracted AGAIN from the biased scalars: kept from the counting pass -- which is what the compiler does when it can
        //  see that the values are the same -- the 8 x 14 magnitudes, keys and signs take 400 registers; the asm makes the words opaque)
#if !WIDE_SHARE_REREAD
#pragma unroll
        for (int j = 0; j < WIDE_PER; j++)
#pragma unroll
          for (int k = 0; k < WinCfg<C, SW>::WORDS; k++) asm volatile("" : "+v"(tbs[j][k]));
#endif
        WIDE_SHARE_UNROLL
        for (int j = 0; j < WIDE_PER; j++) {
          WIDE_SHARE_LOAD(j);
#pragma unroll
          for (int w = 0; w < WIDE_TABLES; w++) {
            uint32_t sign, over = 0;
            const uint32_t mag = wide_digit<C>(WIDE_SHARE_TB(j), w, top_shift, sign, over);
            const uint32_t key = wide_key<C>(mag) - key0;
            if (mag && key < (uint32_t)keys) {
              const uint32_t e = atomicAdd(&cur[key], 1u);
              st_loc[e] = (uint16_t)((sign << 15) | ((uint32_t)w << 11) | (uint32_t)(j * THREADS + tid));
              st_key[e] = (uint16_t)key;
              st_fine[e] = (uint8_t)(wide_slot<C>(mag) & 0xffu);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        write_out(sub, total);
        for (int k = tid; k < WIDE_KEYS; k += THREADS) gpos[k] += hist[k];
        __syncthreads();
      } else {
        // Skewed scalars put more of the iteration's digits into this share than the staging holds (every digit, at worst): the iteration is
        // redone one scalar per thread at a time (THREADS x TABLES entries at most), each read again (the rare path keeps nothing in registers)
        static_assert(THREADS * WIDE_TABLES <= WIDE_STAGE, "one scalar per thread fits the staging");
        __syncthreads();  // (everyone has read `total` before hist / lstart are rebuilt)
#pragma unroll 1
        for (int j = 0; j < WIDE_PER; j++) {
          for (int k = tid; k < WIDE_KEYS; k += THREADS) hist[k] = 0;
          __syncthreads();
          uint32_t tb[WinCfg<C, SW>::WORDS];
          biased(sub, j, tb);
#pragma unroll 1
          for (int w = 0; w < WIDE_TABLES; w++) {
            uint32_t sign, over = 0;
            const uint32_t mag = wide_digit<C>(tb, w, top_shift, sign, over);
            const uint32_t key = wide_key<C>(mag) - key0;
            if (mag && key < (uint32_t)keys) atomicAdd(&hist[key], 1u);
          }
          __syncthreads();
          scan_runs();
          const uint32_t part = lstart[WIDE_KEYS - 1] + hist[WIDE_KEYS - 1];
          for (int k = tid; k < WIDE_KEYS; k += THREADS) cur[k] = lstart[k];
          __syncthreads();
#pragma unroll 1
          for (int w = 0; w < WIDE_TABLES; w++) {
            uint32_t sign, over = 0;
            const uint32_t mag = wide_digit<C>(tb, w, top_shift, sign, over);
            const uint32_t key = wide_key<C>(mag) - key0;
            if (mag && key < (uint32_t)keys) {
              const uint32_t e = atomicAdd(&cur[key], 1u);
              st_loc[e] = (uint16_t)((sign << 15) | ((uint32_t)w << 11) | (uint32_t)(j * THREADS + tid));
              st_key[e] = (uint16_t)key;
              st_fine[e] = (uint8_t)(wide_slot<C>(mag) & 0xffu);
            }
          }
          __syncthreads();
          write_out(sub, part);
          for (int k = tid; k < WIDE_KEYS; k += THREADS) gpos[k] += hist[k];
          __syncthreads();
        }
      }
    } else {
    for (int k = tid; k < WIDE_KEYS; k += THREADS) hist[k] = 0;
    __syncthreads();
    uint32_t rank[WIDE_PER][(WIDE_TABLES + 1) / 2];  // two 16-bit ranks per register (a run holds fewer than 2^16 entries)
#pragma unroll
    for (int j = 0; j < WIDE_PER; j++) {
      uint32_t tb[WinCfg<C, SW>::WORDS];
      biased(sub, j, tb);
#pragma unroll
      for (int w = 0; w < WIDE_TABLES; w++) {
        uint32_t sign, over = 0;
        const uint32_t mag = wide_digit<C>(tb, w, top_shift, sign, over);  // (an overflowing top digit: no entry here as in k_count_wide, which reports it)
        const uint32_t key = wide_key<C>(mag) - key0;                           // (outside this launch's virtual windows: no entry)
        const uint32_t r = mag && key < (uint32_t)keys ? atomicAdd(&hist[key], 1u) : 0u;
        if (w & 1) rank[j][w >> 1] |= r << 16;
        else rank[j][w >> 1] = r;
      }
    }
    __syncthreads();
    scan_runs();
    const uint32_t total = lstart[WIDE_KEYS - 1] + hist[WIDE_KEYS - 1];
#pragma unroll
    for (int j = 0; j < WIDE_PER; j++) {
      uint32_t tb[WinCfg<C, SW>::WORDS];
      biased(sub, j, tb);
#pragma unroll
      for (int w = 0; w < WIDE_TABLES; w++) {
        uint32_t sign, over = 0;
        const uint32_t mag = wide_digit<C>(tb, w, top_shift, sign, over);
        const uint32_t key = wide_key<C>(mag) - key0;
        if (mag && key < (uint32_t)keys) {
          const uint32_t e = lstart[key] + ((rank[j][w >> 1] >> ((w & 1) * 16)) & 0xffffu);
          st_loc[e] = (uint16_t)((sign << 15) | ((uint32_t)w << 11) | (uint32_t)(j * THREADS + tid));
          st_key[e] = (uint16_t)key;
          st_fine[e] = (uint8_t)(wide_slot<C>(mag) & 0xffu);
        }
      }
    }
    __syncthreads();
    write_out(sub, total);
    for (int k = tid; k < WIDE_KEYS; k += THREADS) gpos[k] += hist[k];
    __syncthreads();
    }
  }
}

// The second pass of a launch whose first pass left digit planes (k_count with negbits != null): the same LDS-ranked, LDS-staged
// scatter as k_scatter_coarse, reading 2 B per (input, local window) from the planes.  No scalar arithmetic and no scalars in
// registers.  `w_eff` local windows of `w_count_vec` windows per scalar vector.  negbits == null: input `pos` is scalar `pos` and multiplies
// base `pos`.  Endomorphism halves (k_count<C, 4, Split>): input 2 j + h is half h of scalar j, its sign bit j of negbits[v][h], and it
// multiplies record j + h * half_shift (half_shift = n_bases).
__global__ void __launch_bounds__(256) k_scatter_planes(const uint16_t* __restrict__ planes, const uint64_t* __restrict__ negbits, size_t n,
                                                        size_t stride, uint32_t tile_len, uint32_t tiles, int w_eff, int w_count_vec,
                                                        const uint32_t* __restrict__ counts, const uint32_t* __restrict__ bin_total,
                                                        uint32_t* __restrict__ coarse_ptr, uint32_t* __restrict__ tmp_val,
                                                        uint8_t* __restrict__ tmp_fine, uint32_t half_shift,
                                                        uint32_t chunks, uint32_t host_chunk_len, uint32_t* __restrict__ chunk_len_dev) {
  __shared__ uint32_t gpos[MAXLW * NCOARSE];
  __shared__ uint32_t hist[NCOARSE];
  __shared__ uint32_t lstart[NCOARSE];
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t st_val[SCAT_SUB];
  __shared__ uint32_t st_dst[SCAT_SUB];
  __shared__ uint8_t st_fine[SCAT_SUB];
  __shared__ uint32_t max_total;
  const int tid = threadIdx.x;
  if (tid == 0) max_total = 0;
  __syncthreads();
  for (int i0 = 0; i0 < w_eff * NCOARSE; i0 += 256) {  // bin starts of every local window: as k_scatter_coarse
    const int i = i0 + tid, lw = i / NCOARSE, bin = i % NCOARSE, lane = tid & 63;
    const bool live = i < w_eff * NCOARSE;
    const uint32_t v = live ? bin_total[i] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[tid >> 6] = x;
    __syncthreads();
    const uint32_t incl = x + ((tid >> 6) & 1 ? wave_tot[(tid >> 6) - 1] : 0u);
    if (live) gpos[i] = incl - v + counts[((size_t)lw * tiles + blockIdx.x) * NCOARSE + bin];
    if (live && blockIdx.x == 0) {
      coarse_ptr[(size_t)lw * (NCOARSE + 1) + bin] = incl - v;
      if (bin == NCOARSE - 1) {
        coarse_ptr[(size_t)lw * (NCOARSE + 1) + NCOARSE] = incl;
        atomicMax(&max_total, incl);
      }
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && tid == 0) *chunk_len_dev = smvp_chunk_len(max_total, chunks, host_chunk_len);
  const size_t tile_base = (size_t)blockIdx.x * tile_len;
  const size_t tile_end = tile_base + tile_len < n ? tile_base + tile_len : n;
  const size_t neg_words = (n / 2 + 63) / 64;
  for (int lw = 0; lw < w_eff; lw++) {
    const uint16_t* pl = planes + (size_t)lw * n;
    const uint64_t* nb = negbits ? negbits + (size_t)(lw / w_count_vec) * 2 * neg_words : nullptr;
    uint32_t* ov = tmp_val + (size_t)lw * stride;
    uint8_t* of = tmp_fine + (size_t)lw * stride;
    for (size_t sub = tile_base; sub < tile_end; sub += SCAT_SUB) {
      uint32_t code[8];
      uint32_t negs = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const size_t i = sub + (size_t)j * 256 + tid;
        code[j] = i < tile_end ? pl[i] : 0u;
        if (nb && i < tile_end) negs |= (uint32_t)((nb[(i & 1) * neg_words + (i >> 1) / 64] >> ((i >> 1) & 63)) & 1ull) << j;
      }
      if (tid < NCOARSE) hist[tid] = 0;
      __syncthreads();
      uint32_t rank[8];
#pragma unroll
      for (int j = 0; j < 8; j++) rank[j] = code[j] ? atomicAdd(&hist[(code[j] & 0x7fffu) >> 8], 1u) : 0u;
      __syncthreads();
      const uint32_t mine = tid < NCOARSE ? hist[tid] : 0u;
      const uint32_t excl = block_excl_scan_256(mine, wave_tot);
      if (tid < NCOARSE) lstart[tid] = excl;
      __syncthreads();
      const uint32_t total = lstart[NCOARSE - 1] + hist[NCOARSE - 1];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (code[j]) {
          const uint32_t slot = code[j] & 0x7fffu, bin = slot >> 8;
          const uint32_t e = lstart[bin] + rank[j];
          uint32_t pos = (uint32_t)(sub + (size_t)j * 256 + tid);
          if (nb) pos = (pos >> 1) + ((pos & 1u) ? half_shift : 0u);
          st_val[e] = pos | (((code[j] >> 15) ^ ((negs >> j) & 1u)) << 31);
          st_fine[e] = (uint8_t)(slot & 0xffu);
          st_dst[e] = gpos[lw * NCOARSE + bin] + rank[j];
        }
      }
      __syncthreads();
      for (uint32_t e = tid; e < total; e += 256) {
        const uint32_t d = st_dst[e];
        ov[d] = st_val[e];
        of[d] = st_fine[e];
      }
      if (tid < NCOARSE) gpos[lw * NCOARSE + tid] += hist[tid];
      __syncthreads();
    }
  }
}

#ifndef MSM_FINE_CHUNK
#define MSM_FINE_CHUNK 4096
#endif
constexpr int FINE_CHUNK = MSM_FINE_CHUNK;  // entries staged per block iteration (16 per thread; 8192 -- runs of 32 entries per slot -- measured slower:
                                            // 1.55 -> 1.69 ms at 2^24, 0.092 -> 0.106 at 2^20, profiles/r05_sort.txt)
constexpr int FINE_PER = FINE_CHUNK / 256;  // entries per thread and iteration

// counter[key] += 1 for every active lane, returning the lane's rank (old value).  All lanes that share the key of the
// wave's first active lane are served by ONE LDS atomic (ballot + popcount): with heavily skewed scalars (many equal
// digits) nearly the whole wave shares a key and a plain ds_add would serialise 64-fold; with uniform digits this costs
// one ballot.  Must be called with the same `valid` pattern by whole waves (inactive lanes pass valid = false).
__device__ __forceinline__ uint32_t lds_count_rank(uint32_t* counter, uint32_t key, bool valid) {
  const unsigned long long vm = __ballot(valid);
  if (vm == 0) return 0;
  const int first = __ffsll((long long)vm) - 1;  // wave-uniform: v_readlane, no LDS round trip
  const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
  const bool same = valid && key == k0;
  const unsigned long long sm = __ballot(same);
  const int lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == first) base = atomicAdd(&counter[k0], (uint32_t)__popcll(sm));
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, first);
  uint32_t rank = base + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
  if (valid && !same) rank = atomicAdd(&counter[key], 1u);
  return rank;
}
// the same without the rank: no atomic has to return, so consecutive calls do not wait for each other
__device__ __forceinline__ void lds_count_only(uint32_t* counter, uint32_t key, bool valid) {
  const unsigned long long vm = __ballot(valid);
  if (vm == 0) return;
  const int first = __ffsll((long long)vm) - 1;
  const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
  const bool same = valid && key == k0;
  const unsigned long long sm = __ballot(same);
  if ((int)(threadIdx.x & 63) == first) atomicAdd(&counter[k0], (uint32_t)__popcll(sm));
  if (valid && !same) atomicAdd(&counter[key], 1u);
}

// A coarse bin with more than FINE_BIG entries (heavily skewed scalars: e.g. all entries of a window in one slot) is shared
// by FINE_SPLIT workgroups WITHOUT any cross-block communication: each of them histograms the whole bin (1 byte per entry)
// and, in the same sweep, the part in front of its own contiguous sub-range -- that gives it the start of every slot and
// its own offset inside every slot -- and then scatters only its sub-range.  Normal bins are handled by workgroup 0 alone
// (the other FINE_SPLIT - 1 exit at once).
static_assert(FINE_BIG % FINE_CHUNK == 0, "sub-ranges are whole chunks");

// Histograms of the FINE_SPLIT sub-ranges of every coarse bin that exceeds FINE_BIG (part_hist[lw][bin][part][256]); launched
// ahead of k_sort_fine when n is large enough for uniform scalars to produce such bins (the host decides), so that the
// FINE_SPLIT workgroups of a bin do not each histogram the whole bin.  Smaller bins: nothing to do.
__global__ void __launch_bounds__(256) k_fine_hist(const uint8_t* __restrict__ tmp_fine, size_t stride,
                                                   const uint32_t* __restrict__ coarse_ptr, uint32_t* __restrict__ part_hist) {
  __shared__ uint32_t hist[FINE];
  const int bin = blockIdx.x, part = blockIdx.z, lw = blockIdx.y, tid = threadIdx.x;
  const uint32_t begin = coarse_ptr[(size_t)lw * (NCOARSE + 1) + bin], end = coarse_ptr[(size_t)lw * (NCOARSE + 1) + bin + 1];
  if (end - begin <= FINE_BIG) return;
  uint32_t per = (end - begin + FINE_SPLIT - 1) / FINE_SPLIT;
  per = (per + FINE_CHUNK - 1) / FINE_CHUNK * FINE_CHUNK;
  const uint32_t my_begin = begin + (uint32_t)part * per < end ? begin + (uint32_t)part * per : end;
  const uint32_t my_end = my_begin + per < end ? my_begin + per : end;
  const uint8_t* tf = tmp_fine + (size_t)lw * stride;
  hist[tid] = 0;
  __syncthreads();
  for (uint32_t base = my_begin; base < my_end; base += FINE_CHUNK) {
    uint32_t f[FINE_PER];
#pragma unroll
    for (int j = 0; j < FINE_PER; j++) {
      const uint32_t i = base + j * 256 + tid;
      f[j] = i < my_end ? tf[i] : 0xffffffffu;
    }
#pragma unroll
    for (int j = 0; j < FINE_PER; j++) lds_count_only(hist, f[j] & 0xffu, f[j] != 0xffffffffu);
  }
  __syncthreads();
  part_hist[(((size_t)lw * NCOARSE + bin) * FINE_SPLIT + part) * FINE + tid] = hist[tid];
}

__global__ void __launch_bounds__(256) k_sort_fine(const uint32_t* __restrict__ tmp_val, const uint8_t* __restrict__ tmp_fine, size_t stride,
                                                   const uint32_t* __restrict__ coarse_ptr, uint32_t* __restrict__ col_ptr,
                                                   uint32_t* __restrict__ val_idxs, uint32_t chunks, const uint32_t* __restrict__ chunk_len_dev,
                                                   uint32_t* __restrict__ chunk_slot, const uint32_t* __restrict__ part_hist, uint32_t* __restrict__ info,
                                                   uint32_t* __restrict__ bin_fill) {
  const uint32_t chunk_len = *chunk_len_dev;
  __shared__ uint32_t hist[FINE];
  __shared__ uint32_t before[FINE];  // entries of every slot in front of this workgroup's sub-range
  __shared__ uint32_t lstart[FINE];
  __shared__ uint32_t gpos[FINE];
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t st_val[FINE_CHUNK];
  __shared__ uint8_t st_slot[FINE_CHUNK];  // (round 5: an entry's destination is its run's cursor + its place in the staged run -- recomputed at the
                                           //  write-out from the slot, 1 B, instead of staged as 4 B: 24.6 KB instead of 36.9 -- six workgroups per CU, not four)
  __shared__ uint32_t long_c0[FINE], long_c1[FINE], long_slot[FINE];  // (the chunk table's long runs: at most one per slot)
  __shared__ uint32_t skew_flag, long_count;
  const int bin = blockIdx.x, part = blockIdx.z, lw = blockIdx.y, tid = threadIdx.x;
  const uint32_t half = gridDim.x * FINE;  // bucket slots per window: the grid covers exactly the window's coarse bins
  const uint32_t begin = coarse_ptr[(size_t)lw * (NCOARSE + 1) + bin], end = coarse_ptr[(size_t)lw * (NCOARSE + 1) + bin + 1];
  const bool big = end - begin > FINE_BIG;
  if (!big && part != 0) return;
  // k_count's fill word of this bin (null: the launch's first pass was another kernel): read for the last time by k_scatter_coarse, zero for the next launch
  if (bin_fill && part == 0 && tid == 0) bin_fill[lw * NCOARSE + bin] = 0;
  // The host's cue for k_fine_hist (INFOBIT_HUGE_BIN) is for SKEWED scalars: a bin beyond FINE_BIG that also holds more than HUGE_BIN_MEANS times
  // the window's mean bin.  The top window of endomorphism halves is not uniform -- its bins reach twice the mean, which at 2^20 points is FINE_BIG
  // itself -- and used to keep the histograms on for every launch of uniform scalars (22 us each).  Such a bin costs its sharers little without them:
  // each sweeps at most 4 mean bins of one-byte keys and scatters an eighth of it, about what the workgroup of an ordinary bin does in its two passes.
  const uint32_t win_total = coarse_ptr[(size_t)lw * (NCOARSE + 1) + NCOARSE];  // (the window's first bin starts at 0)
  const bool skew_cue = big && (uint64_t)(end - begin) * gridDim.x > (uint64_t)HUGE_BIN_MEANS * win_total;
  // this workgroup's sub-range [my_begin, my_end): the whole bin, or one of FINE_SPLIT pieces (multiples of FINE_CHUNK)
  uint32_t my_begin = begin, my_end = end;
  if (big) {
    uint32_t per = (end - begin + FINE_SPLIT - 1) / FINE_SPLIT;
    per = (per + FINE_CHUNK - 1) / FINE_CHUNK * FINE_CHUNK;
    my_begin = begin + (uint32_t)part * per < end ? begin + (uint32_t)part * per : end;
    my_end = my_begin + per < end ? my_begin + per : end;
  }
  const uint32_t* tv = tmp_val + (size_t)lw * stride;
  const uint8_t* tf = tmp_fine + (size_t)lw * stride;
  uint32_t* out = val_idxs + (size_t)lw * stride;
  // pass 1: slot histogram of the whole coarse bin (and of the part in front of the sub-range)
  hist[tid] = 0;
  before[tid] = 0;
  if (tid == 0) {
    skew_flag = 0;
    long_count = 0;
  }
  __syncthreads();
  if (!big) {
    for (uint32_t base = begin; base < end; base += FINE_CHUNK) {  // 16 independent byte loads in flight per thread
      uint32_t f[FINE_PER];
#pragma unroll
      for (int j = 0; j < FINE_PER; j++) {
        const uint32_t i = base + j * 256 + tid;
        f[j] = i < end ? tf[i] : 0xffffffffu;
      }
#pragma unroll
      for (int j = 0; j < FINE_PER; j++)
        if (f[j] != 0xffffffffu) atomicAdd(&hist[f[j]], 1u);
    }
  } else if (part_hist) {
    // the sub-range histograms were made by k_fine_hist: sum them (and the ones in front of this workgroup's sub-range)
    if (tid == 0 && part == 0 && skew_cue) atomicOr(info, INFOBIT_HUGE_BIN);
    const uint32_t* ph = part_hist + ((size_t)lw * NCOARSE + bin) * FINE_SPLIT * FINE + tid;
    uint32_t all = 0, front = 0;
#pragma unroll
    for (int q = 0; q < FINE_SPLIT; q++) {
      const uint32_t c = ph[q * FINE];
      all += c;
      if (q < part) front += c;
    }
    hist[tid] = all;
    before[tid] = front;
  } else {
    if (tid == 0 && part == 0 && skew_cue) atomicOr(info, INFOBIT_HUGE_BIN);  // (a huge bin without k_fine_hist's histograms: every sharer sweeps the bin up to its own end)
    // FINE_CHUNK entries per sweep step, 16 independent byte loads per thread in flight; a step lies wholly in front of
    // the sub-range or not (my_begin - begin is a multiple of FINE_CHUNK), so every entry is counted once
    uint32_t f[FINE_PER], g[FINE_PER];  // double buffered: the loads of step k + 1 are in flight while step k is counted
#pragma unroll
    for (int j = 0; j < FINE_PER; j++) {
      const uint32_t i = begin + j * 256 + tid;
      f[j] = i < end ? tf[i] : 0xffffffffu;
    }
    for (uint32_t base = begin; base < end; base += FINE_CHUNK) {
#pragma unroll
      for (int j = 0; j < FINE_PER; j++) {
        const uint32_t i = base + FINE_CHUNK + j * 256 + tid;
        g[j] = i < end ? tf[i] : 0xffffffffu;
      }
      uint32_t* counter = base < my_begin ? before : hist;
      if (skew_cue) {  // (block-uniform) many entries per slot: wave-aggregated counting
#pragma unroll
        for (int j = 0; j < FINE_PER; j++) lds_count_only(counter, f[j] & 0xffu, f[j] != 0xffffffffu);
      } else {  // a bin of a few means: counted as an ordinary bin is
#pragma unroll
        for (int j = 0; j < FINE_PER; j++)
          if (f[j] != 0xffffffffu) atomicAdd(&counter[f[j]], 1u);
      }
#pragma unroll
      for (int j = 0; j < FINE_PER; j++) f[j] = g[j];
    }
    __syncthreads();
    hist[tid] += before[tid];
  }
  __syncthreads();
  // a slot holding more than a quarter of the bin means skewed scalars: pass 2 then ranks with wave-aggregated atomics
  if (hist[tid] > (end - begin) / 4 && end - begin > (uint32_t)FINE_CHUNK) skew_flag = 1;
  {
    const uint32_t excl = block_excl_scan_256(hist[tid], wave_tot);
    gpos[tid] = begin + excl + before[tid];
    if (part == 0) {
      col_ptr[(size_t)lw * (half + 1) + bin * FINE + tid] = begin + excl;
      if (bin == (int)gridDim.x - 1 && tid == FINE - 1) col_ptr[(size_t)lw * (half + 1) + half] = end;
    }
    // SMVP chunks whose first entry lies in this slot's run [first, last): short runs are tabulated by their own thread
    // (of workgroup 0), long ones (skewed scalars) by all threads of all workgroups of the bin together
    const uint32_t first = begin + excl, last = first + hist[tid];
    uint32_t c0 = (first + chunk_len - 1) / chunk_len;
    uint32_t c1 = (uint32_t)(((uint64_t)last + chunk_len - 1) / chunk_len);
    if (c1 > chunks) c1 = chunks;
    if (c0 > c1) c0 = c1;
    const bool long_run = c1 - c0 > 16;
    if (part == 0 && !long_run)
      for (uint32_t c = c0; c < c1; c++) chunk_slot[(size_t)lw * chunks + c] = (uint32_t)(bin * FINE + tid);
    if (long_run) {
      const uint32_t k = atomicAdd(&long_count, 1u);
      long_c0[k] = c0;
      long_c1[k] = c1;
      long_slot[k] = (uint32_t)(bin * FINE + tid);
    }
  }
  __syncthreads();
  {
    const uint32_t nl = long_count, nparts = big ? FINE_SPLIT : 1;
    for (uint32_t k = 0; k < nl; k++)
      for (uint32_t c = long_c0[k] + part * 256 + tid; c < long_c1[k]; c += nparts * 256) chunk_slot[(size_t)lw * chunks + c] = long_slot[k];
  }
  __syncthreads();
  // pass 2: LDS-staged scatter of the sub-range, FINE_CHUNK entries at a time
  const bool skewed = skew_flag != 0;  // block-uniform (read after the barriers of the scan above)
  for (uint32_t base = my_begin; base < my_end; base += FINE_CHUNK) {
    hist[tid] = 0;
    __syncthreads();
    uint32_t v[FINE_PER], fr[FINE_PER];  // value; slot | rank << 8
#pragma unroll
    for (int j = 0; j < FINE_PER; j++) {
      const uint32_t i = base + j * 256 + tid;
      const bool valid = i < my_end;
      const uint32_t f = valid ? tf[i] : 0u;
      const uint32_t rank = skewed ? lds_count_rank(hist, f, valid) : (valid ? atomicAdd(&hist[f], 1u) : 0u);
      if (valid) {
        v[j] = tv[i];
        fr[j] = f | (rank << 8);
      } else {
        fr[j] = 0xffffffffu;
      }
    }
    __syncthreads();
    const uint32_t excl = block_excl_scan_256(hist[tid], wave_tot);
    lstart[tid] = excl;
    __syncthreads();
    const uint32_t total = (my_end - base) < (uint32_t)FINE_CHUNK ? (my_end - base) : (uint32_t)FINE_CHUNK;
#pragma unroll
    for (int j = 0; j < FINE_PER; j++) {
      if (fr[j] != 0xffffffffu) {
        const uint32_t f = fr[j] & 0xffu, r = fr[j] >> 8;
        const uint32_t e = lstart[f] + r;
        st_val[e] = v[j];
        st_slot[e] = (uint8_t)f;
      }
    }
    __syncthreads();
    for (uint32_t e = tid; e < total; e += 256) {
      const uint32_t f = st_slot[e];
      out[gpos[f] + (e - lstart[f])] = st_val[e];
    }
    __syncthreads();
    gpos[tid] += hist[tid];
    __syncthreads();
  }
}

// Deterministic mode of the transpose (the reference's stage test asserts the exact val_idxs,
// tests/transpose_shader.rs:198-199): the order inside a slot is the arrival order of LDS atomics -- the group sum does not depend on it,
// but a stage-level comparison does.  With the debug switch on (msm_hip_set_debug), every slot's run is put into ascending order of its
// entries (index | sign << 31: the positive digits' points by index, then the negative digits') by a rank sort: one lane per entry finds
// its slot (binary search of col_ptr), counts the entries of its run that are smaller (they are distinct) and writes itself to that
// position of a scratch copy (`tmp`, the coarse-order array, free by then); a second kernel copies the scratch back.  O(sum of run
// length^2): runs beyond ORDER_RUN_MAX entries (heavily skewed inputs) keep their arrival order.
constexpr uint32_t ORDER_RUN_MAX = 1u << 15;  // (2^30 comparisons for one such run)
__global__ void __launch_bounds__(256) k_order_runs(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ val_idxs, uint32_t* __restrict__ tmp,
                                                    size_t stride, uint32_t half) {
  const int lw = blockIdx.y;
  const uint32_t* cp = col_ptr + (size_t)lw * (half + 1);
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= cp[half]) return;
  uint32_t lo = 0, hi = half - 1;  // the slot whose run holds entry e: cp[s] <= e < cp[s + 1]
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cp[mid + 1] > e) hi = mid;
    else lo = mid + 1;
  }
  const uint32_t b = cp[lo], end = cp[lo + 1];
  const uint32_t* v = val_idxs + (size_t)lw * stride;
  const uint32_t x = v[e];
  uint32_t pos = e;
  if (end - b <= ORDER_RUN_MAX) {
    uint32_t rank = 0;
    for (uint32_t j = b; j < end; j++) rank += v[j] < x ? 1u : 0u;
    pos = b + rank;
  }
  tmp[(size_t)lw * stride + pos] = x;
}
__global__ void __launch_bounds__(256) k_copy_runs(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ tmp, uint32_t* __restrict__ val_idxs,
                                                   size_t stride, uint32_t half) {
  const int lw = blockIdx.y;
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e < col_ptr[(size_t)lw * (half + 1) + half]) val_idxs[(size_t)lw * stride + e] = tmp[(size_t)lw * stride + e];
}
}  // namespace msm_sort
