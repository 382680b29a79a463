// The curve-neutral device code that the sort (sort_kernels.h) and the curve units (msm_kernels.h) share: scalar loads, the signed-digit recode,
// a block-wide scan, and the sort's first pass, k_count.  No field, curve or endomorphism header enters.  k_count is here and not in
// sort_kernels.h because endomorphism launches split their scalars in it: a curve unit instantiates it over its own split functor; every
// other instantiation is msm_hip.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "msm_layout.h"

namespace msm_recode {
using namespace msm_layout;

// Window size as a parameter (the reference hard-codes c, src/cuzk/msm.rs:79-82): C-bit signed digits,
// 2^(C-1) bucket slots per window, NWIN = ceil(255 / C) windows (254-bit scalars + one bit for the recode's carry).
// Small MSMs are dominated by the bucket reduce of 16 x 2^15 mostly empty buckets; a smaller C trades a few more
// additions per point for 16 x / 4 x fewer buckets.  The host picks C from n (msm_plan.h: pick_window_bits).
// SW = words per scalar the recode reads: 8 (a 254-bit scalar) or 4 (one 127-bit half of the endomorphism split, csrc/glv.h:
// magnitude in bits 0 .. 126, sign in bit 127).
// NB != 0: narrow scalars (MSM_HIP_SCALARS_U8 .. U64, MSM_HIP_SCALAR_U128) of NB bytes, unsigned, in SW = 1 (NB <= 4), 2 (NB = 8) or 4 (NB = 16)
// words: 8 NB bits, and NWIN = (8 NB + C) / C windows -- 1 / 2 / 3 / 5 / 9 at 16 bits (NB = 16: 10 at 14 bits, 11 at 12); the top window of
// U16 .. U128 holds only the recode's carry.  NB = 16 is not the SW = 4 half-scalar (NB = 0: 127 bits, its sign in bit 127).
// The signed formats (MSM_HIP_SCALAR_SIGNED) recode the MAGNITUDE |v| <= 2^(8 NB - 1) with the configuration of their width; the kernels that
// load scalars name such a format by a negative NB (narrow_width below) and carry the sign where the endomorphism's halves carry theirs.
template <int C, int SW = 8, int NB = 0>
struct WinCfg {
  static_assert((C >= 10 && C <= 16) || (C >= 17 && C <= 20), "window bits (17 .. 20: the digits of the wide fixed-base tables, k_count_wide)");
  static_assert(NB ? (SW == (NB + 3) / 4 && (NB == 1 || NB == 2 || NB == 4 || NB == 8 || NB == 16)) : (SW == 8 || SW == 4), "scalar words");
  static constexpr int BITS = C;
  static constexpr int SBITS = NB ? 8 * NB : SW == 8 ? 254 : 127;  // bits of the scalar (magnitude)
  static constexpr int NWIN = (SBITS + C) / C;             // 16: 16 | 8, 14: 19 | 10, 12: 22 | 11
  static constexpr int HALF = 1 << (C - 1);                // bucket slots per window
  static constexpr int TBITS = NWIN * C;                   // bits of the biased scalar that carry digits
  static constexpr int WORDS = (TBITS + 31) / 32;          // 8 or 9 | 4 or 5
};

__device__ __forceinline__ void ld8(const uint32_t* p, uint32_t w[8]) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0];
  const uint4 b = reinterpret_cast<const uint4*>(p)[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void st8(uint32_t* p, const uint32_t w[8]) {
  reinterpret_cast<uint4*>(p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// Adding 0x8000 to every 16-bit halfword of the 256-bit scalar (one multiword addition) performs the whole carry chain
// at once: halfword w of t = s + 0x8000...8000 is the reference's biased digit d_w + 2^15 (decompose_scalars.template.wgsl:
// 105-112), and the carry out of bit 255 is its "final carry".  Each window's digit is then read independently.
// The same for C-bit windows: the bias constant has bit C w + C - 1 set for every window w (word i of it below), the biased
// scalar t has WinCfg<C>::WORDS words, and the recode overflows iff t has a bit at or above C * NWIN.
template <int C, int SW = 8, int NB = 0>
__host__ __device__ constexpr uint32_t bias_word(int i) {
  uint32_t v = 0;
  for (int w = 0; w < WinCfg<C, SW, NB>::NWIN; w++) {
    const int bit = C * w + C - 1;
    if (bit / 32 == i) v |= 1u << (bit % 32);
  }
  return v;
}
template <int C, int SW = 8, int NB = 0>
__device__ __forceinline__ uint32_t bias_scalar(const uint32_t s[SW], uint32_t t[WinCfg<C, SW, NB>::WORDS]) {
  constexpr int WORDS = WinCfg<C, SW, NB>::WORDS;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < WORDS; i++) {
    c += (uint64_t)(i < SW ? s[i] : 0u) + bias_word<C, SW, NB>(i);
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  // 1: the recode does not fit NWIN windows ("final carry is 1", test/utils.rs:150-152; never for a narrow scalar: NWIN C > 8 NB)
  if constexpr (WinCfg<C, SW, NB>::TBITS == 32 * WORDS) return (uint32_t)c;
  else return (t[WORDS - 1] >> (WinCfg<C, SW, NB>::TBITS - 32 * (WORDS - 1))) != 0u ? 1u : 0u;
}
// scalar i of a vector of narrow NB-byte scalars (unsigned little-endian, packed: the vector is n x NB bytes), zero-extended into SW words
template <int NB>
__device__ __forceinline__ void ld_narrow(const uint8_t* v, size_t i, uint32_t s[(NB + 3) / 4]) {
  if constexpr (NB == 1) s[0] = v[i];
  else if constexpr (NB == 2) s[0] = reinterpret_cast<const uint16_t*>(v)[i];
  else if constexpr (NB == 4) s[0] = reinterpret_cast<const uint32_t*>(v)[i];
  else if constexpr (NB == 8) {
    const uint2 a = reinterpret_cast<const uint2*>(v)[i];
    s[0] = a.x;
    s[1] = a.y;
  } else {
    static_assert(NB == 16, "narrow scalar width");
    const uint4 a = reinterpret_cast<const uint4*>(v)[i];
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
  }
}
// the same for NB-byte two's-complement integers: s receives the magnitude |v| (the minimum's, 2^(8 NB - 1), fits the NB bytes unsigned),
// `neg` the sign
template <int NB>
__device__ __forceinline__ void ld_narrow_signed(const uint8_t* v, size_t i, uint32_t s[(NB + 3) / 4], uint32_t& neg) {
  constexpr int SW = (NB + 3) / 4;
  ld_narrow<NB>(v, i, s);
  neg = (s[SW - 1] >> ((8 * NB - 1) & 31)) & 1u;
  uint64_t c = neg;  // -v = ~v + 1 within 8 NB bits
#pragma unroll
  for (int k = 0; k < SW; k++) {
    c += s[k] ^ (0u - neg);
    s[k] = (uint32_t)c;
    c >>= 32;
  }
  if constexpr (NB < 4) s[0] &= (1u << (8 * NB)) - 1u;
}
// scalar i of a narrow vector in the format NB names (narrow_width): magnitude and sign
template <int NB>
__device__ __forceinline__ void ld_narrow_fmt(const uint8_t* v, size_t i, uint32_t s[(narrow_width(NB) + 3) / 4], uint32_t& neg) {
  if constexpr (NB < 0) ld_narrow_signed<-NB>(v, i, s, neg);
  else {
    ld_narrow<NB>(v, i, s);
    neg = 0;
  }
}
// the recode's input: a scalar (8 words) or one half of the endomorphism split (4 words; `neg` receives its sign)
template <int SW>
__device__ __forceinline__ void ld_scalar(const uint32_t* p, uint32_t s[SW], uint32_t& neg) {
  if constexpr (SW == 8) {
    ld8(p, s);
    neg = 0;
  } else {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    s[0] = a.x; s[1] = a.y; s[2] = a.z;
    s[3] = a.w & 0x7fffffffu;
    neg = a.w >> 31;
  }
}
// biased digit b = d + 2^(C-1) of window w  ->  signed-magnitude code: sign << 15 | (|d| mod 2^(C-1))
template <int C>
__device__ __forceinline__ uint32_t code_of_window(const uint32_t* t, int w) {  // t: WinCfg<C, SW>::WORDS words
  constexpr uint32_t H = (uint32_t)WinCfg<C>::HALF;
  const int bit = C * w, i = bit >> 5, sh = bit & 31;
  uint32_t b = t[i] >> sh;
  if (sh + C > 32) b |= t[i + 1] << (32 - sh);  // (only then is i + 1 < WORDS)
  b &= (1u << C) - 1u;
  if (b >= H) return b - H;                       // d = 0 .. 2^(C-1) - 1 (0: no entry)
  return 0x8000u | ((H - b) & (H - 1u));          // d = -(2^(C-1) - b): magnitude 1 .. 2^(C-1) (2^(C-1) -> slot 0)
}

// Exclusive prefix sum of one value per thread over a 256-thread block (4 waves); `wave_tot` is 4 words of LDS.
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t* wave_tot) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  if (lane == 63) wave_tot[wid] = x;
  __syncthreads();
  uint32_t add = 0;
  for (int k = 0; k < wid; k++) add += wave_tot[k];
  __syncthreads();
  return x - v + add;
}

// ---- the sort's first pass: a workgroup's tile of scalars recoded and counted per (local window, coarse bin)
// `nvec` scalar vectors (vec_stride words apart) may share one launch: vector v, window w is handled as local window
// lw = v * w_count + (w - w_begin), nvec * w_count <= MAXLW -- several MSMs over the same bases sorted, accumulated and reduced
// by one kernel sequence (used by the window-sharded multi-GPU pipeline, where one MSM's share is too small to fill a GPU).
//
// Digit planes.  `planes` receives every local window's digit code, u16 planes[lw][n] (PLANE_MODE below): for the debug read-back
// (msm_hip_read_digits), or as the input of the launch's second pass (k_scatter_planes reads them instead of the scalars).
// A rank of a window-sharded run needs 1 - 4 of a scalar's 16 digits: its second pass then reads 2 - 8 B per scalar instead of 32,
// and keeps no scalar in registers (the scalar-reading scatter holds 8 biased scalars per thread: 282 VGPRs at 16 bits).
// PLANE_MODE of k_count's `planes` output: 0 none; 1 debug read-back (the half's sign folded into bit 15); 2 raw codes for k_scatter_planes
// (with the signs of the halves, if any, in `negbits`).
// Split != void (endomorphism launches, SW = 4): `scalars` are the nvec x n / 2 full 8-word scalars; the kernel splits each into its two halves
// (csrc/glv.h) itself -- the separate pass of round 2 (k_glv_split: 32 B read + 32 B written per scalar and a kernel of its own in front of
// every launch) is gone -- and treats them as inputs 2 j (k1, multiplies P_j) and 2 j + 1 (k2, multiplies phi(P_j)) of the 2n-input problem:
// INTERLEAVED positions, so that a tile of positions is a tile of scalars and one LDS histogram serves both halves.  The halves go to
// `halves_out` (position p at word 4 p: the same 32 B the scalar took) for k_scatter_coarse<C, 4>; negbits[v][h][n / 128 rounded up]: bit j of
// half h's array is the sign of half h of scalar j.
// NB != 0 (narrow scalars, MSM_HIP_SCALARS_U8 .. U64, MSM_HIP_SCALAR_U128): `scalars` holds nvec x n x |NB| packed bytes, `vec_stride` counts BYTES,
// SW = (|NB| + 3) / 4.  NB < 0 (MSM_HIP_SCALAR_SIGNED): two's-complement values -- the magnitude is recoded, the sign goes where a half's goes.
// Sparse (a SparseIdx argument; one vector): scalar j whose index is out of range reads as zero, and the launch's error word gets ERRBIT_BAD_INDEX.
__device__ __forceinline__ SparseIdx sparse_arg() { return SparseIdx{nullptr, 0u, nullptr}; }  // (a dense instantiation: never read)
__device__ __forceinline__ SparseIdx sparse_arg(SparseIdx s) { return s; }
// Split: void, or a curve unit's stateless functor around its endomorphism split -- bool operator()(k[8], h1[4], h2[4]) (csrc/glv.h: glv_split;
// msm_kernels.h: glv_split_fn).  It is the one place where a curve enters the recode, so the instantiations with a functor are the curve unit's
// (CurveOps::count_split) and those with void are msm_hip.hip's, built once.
template <int C, int SW, typename Split = void, int NB = 0, typename... Sparse>
__global__ void __launch_bounds__(256) k_count(const uint32_t* __restrict__ scalars, size_t n, uint32_t tile_len, uint32_t tiles,
                                               int w_begin, int w_count, int nvec, size_t vec_stride,
                                               uint32_t* __restrict__ counts, uint32_t* __restrict__ bin_fill, uint16_t* __restrict__ planes, int plane_mode,
                                               uint64_t* __restrict__ negbits, uint32_t* __restrict__ halves_out,
                                               uint32_t* __restrict__ err, size_t merge_nb, Sparse... sparse) {
  constexpr bool SPLIT = !std::is_void_v<Split>;
  static_assert(!SPLIT || SW == 4, "the split produces 4-word halves");
  static_assert(!SPLIT || NB == 0, "narrow scalars are never split");
  constexpr bool SPARSE = sizeof...(Sparse) != 0;
  constexpr int NW = narrow_width(NB);  // bytes of a narrow scalar, whatever its signedness
  const SparseIdx sp = sparse_arg(sparse...);
  uint32_t bad_idx = 0;
  // merge_nb != 0 (fixed-base tables, see k_precompute_tables): every window of vector v feeds ONE bucket set, local window v
  // grid (tiles, nvec): a workgroup counts one tile of ONE scalar vector (round 4: with the vectors looped over inside the workgroup a
  // grouped launch of small MSMs kept a quarter of the CUs busy -- 64 tiles at 2^16 -- for nvec times as long)
  __shared__ uint32_t cnt[MAXLW * NCOARSE];
  const int tid = threadIdx.x;
  const int v = blockIdx.y;
  const int le0 = merge_nb ? v : v * w_count, le_n = merge_nb ? 1 : w_count;  // this vector's local windows
  (void)nvec;
  for (int i = tid; i < le_n * NCOARSE; i += 256) cnt[le0 * NCOARSE + i] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * tile_len;
  const size_t end = base + tile_len < n ? base + tile_len : n;
  uint32_t bad = 0;
  // one recoded input: histogram and plane entries of its local windows
  auto emit = [&](int v, size_t pos, const uint32_t* tb, uint32_t neg) {
#pragma unroll
    for (int w = 0; w < WinCfg<C, SW, NW>::NWIN; w++) {
      const int lw = w - w_begin;
      if (lw >= 0 && lw < w_count) {
        const int le = merge_nb ? v : v * w_count + lw;
        const uint32_t code = code_of_window<C>(tb, w);
        if (code != 0) atomicAdd(&cnt[le * NCOARSE + ((code & 0x7fffu) >> 8)], 1u);
        if (plane_mode) planes[((size_t)v * w_count + lw) * n + pos] = (uint16_t)(plane_mode == 2 ? code : (code ? code ^ (neg << 15) : 0u));
      }
    }
  };
  {
    const uint32_t* sv = scalars + (size_t)v * vec_stride;
    if constexpr (SPLIT) {
      const size_t nsc = n / 2, neg_words = (nsc + 63) / 64;
      for (size_t j0 = base / 2; j0 < end / 2; j0 += 256) {  // (tile_len is a multiple of 256 positions: a wave's 64 scalars share a word of negbits)
        const size_t j = j0 + tid;
        const bool valid = j < end / 2;
        uint32_t k[8], h[2][4];
#pragma unroll
        for (int q = 0; q < 8; q++) k[q] = 0;
        bool live = valid;
        if constexpr (SPARSE) {
          if (valid && sp.idx[j] >= sp.n_bases) live = false, bad_idx = 1;  // (a zero scalar: zero halves, no entries)
        }
        if (live) ld8(sv + j * 8, k);
        // the input contract of the plain path: scalars that overflow the reference's 16-bit recode are rejected (test/utils.rs:150-152)
        uint64_t c = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) c = (c + k[q] + 0x80008000u) >> 32;
        const bool ok = Split{}(k, h[0], h[1]);
        if (c != 0 || !ok) bad = 1;
        if (negbits) {
#pragma unroll
          for (int hh = 0; hh < 2; hh++) {
            const unsigned long long nb = __ballot((h[hh][3] >> 31) != 0u);
            if ((tid & 63) == 0 && valid) negbits[((size_t)v * 2 + hh) * neg_words + j / 64] = nb;
          }
        }
        if (!valid) continue;
        if (halves_out) {
          uint4* o = reinterpret_cast<uint4*>(halves_out + ((size_t)v * nsc + j) * 8);
          o[0] = make_uint4(h[0][0], h[0][1], h[0][2], h[0][3]);
          o[1] = make_uint4(h[1][0], h[1][1], h[1][2], h[1][3]);
        }
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
          uint32_t s[4] = {h[hh][0], h[hh][1], h[hh][2], h[hh][3] & 0x7fffffffu}, tb[WinCfg<C, 4>::WORDS];
          bad |= bias_scalar<C, 4>(s, tb);
          emit(v, 2 * j + hh, tb, h[hh][3] >> 31);
        }
      }
    } else if constexpr (NB != 0) {
      const uint8_t* nv = reinterpret_cast<const uint8_t*>(scalars) + (size_t)v * vec_stride;
      for (size_t i0 = base; i0 < end; i0 += 256) {
        const size_t i = i0 + tid;
        if (i >= end) continue;
        uint32_t s[SW], tb[WinCfg<C, SW, NW>::WORDS], neg;
        ld_narrow_fmt<NB>(nv, i, s, neg);
        if constexpr (SPARSE) {
          if (sp.idx[i] >= sp.n_bases) {
            bad_idx = 1;
            neg = 0;
#pragma unroll
            for (int k = 0; k < SW; k++) s[k] = 0;
          }
        }
        (void)bias_scalar<C, SW, NW>(s, tb);  // (every NB-byte value or magnitude fits: no input is rejected)
        emit(v, i, tb, neg);
      }
    } else {
      for (size_t i0 = base; i0 < end; i0 += 256) {
        const size_t i = i0 + tid;
        if (i >= end) continue;
        uint32_t s[SW], tb[WinCfg<C, SW>::WORDS], neg = 0;
        ld_scalar<SW>(sv + i * SW, s, neg);
        if constexpr (SPARSE) {
          if (sp.idx[i] >= sp.n_bases) {
            bad_idx = 1;
            neg = 0;
#pragma unroll
            for (int k = 0; k < SW; k++) s[k] = 0;
          }
        }
        bad |= bias_scalar<C, SW>(s, tb);
        if constexpr (C != 16 && SW == 8) {  // the same input contract for every window size: scalars that overflow the reference's
          uint32_t t16[8];                   // 16-bit recode ("final carry is 1", test/utils.rs:150-152) are rejected
          bad |= bias_scalar<16>(s, t16);
        }
        emit(v, i, tb, neg);
      }
    }
  }
  if (bad) atomicOr(err, ERRBIT_SCALAR_CARRY);
  if constexpr (SPARSE) {
    if (bad_idx) atomicOr(err, ERRBIT_BAD_INDEX);
  }
  __syncthreads();
  // counts[lw][tile][bin]: where this tile's entries of the bin start inside the bin -- the bin's fill when this workgroup arrives (one returning
  // device-scope atomic per non-empty (window, bin): bin_fill[lw][bin], zero at launch, ends as the bin's size).  The prefix over tiles that
  // k_scan_tiles made as a launch of its own (18 - 23 us of every launch's main stream for 2 MB of counters) is gone: the tiles of a bin then lie in
  // ARRIVAL order instead of tile order, which nothing downstream asks about (the order inside a slot is the arrival order of LDS atomics already).
  // No workgroup waits for another and none fences: the consumers are later kernels.  k_sort_fine zeroes the word again for the next launch.
  // (four atomics in flight per thread -- the 8 windows of a launch of halves in one round trip, not four)
  for (int i0 = tid; i0 < le_n * NCOARSE; i0 += 4 * 256) {
    uint32_t at[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = i0 + k * 256;
      const uint32_t c = i < le_n * NCOARSE ? cnt[le0 * NCOARSE + i] : 0u;
      at[k] = c ? atomicAdd(&bin_fill[le0 * NCOARSE + i], c) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = i0 + k * 256;
      if (i < le_n * NCOARSE) counts[((size_t)(le0 + i / NCOARSE) * tiles + blockIdx.x) * NCOARSE + (i % NCOARSE)] = at[k];
    }
  }
}
}  // namespace msm_recode
