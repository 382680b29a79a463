// The per-curve device kernels of the cuZK-style MSM pipeline for gfx950 (MI355X): everything that does field or group arithmetic, written once
// against the field interface and instantiated by every curve unit (curve_<name>.hip) with that curve's constants, in its own namespace
// MSM_KERNEL_NS.  The recode and the sort between stage 0 and the SMVP see no field: they are sort_kernels.h, compiled once by msm_hip.hip.
//
// Pipeline (reference: compute_msm, src/cuzk/msm.rs:75-417) and the HBM layout each stage reads/writes
// (W = windows handled by this GPU, stride = n rounded up to 4):
//
//                                                                                                            written by
//   bases      u32[n][16]            packed affine, Montgomery (R = 2^261), x || y, 64 B per point, resident     stage 0 (here: k_convert_points ...)
//                                    (+ phi(P_i) as records n .. 2n-1 with the endomorphism, + 15 more tables with fixed-base tables)
//   scalars    u32[n][8]             canonical little-endian (wire format)   (endomorphism: halves u32[2n][4], csrc/glv.h)  the caller (k_count<C, 4, Split>: the halves)
//   counts     u32[W][tiles][128]    per-tile coarse-bin histogram, then prefix over tiles                        sort (sort_kernels.h: k_count)
//   tmp_val    u32[W][stride]        point index | sign << 31, in coarse-bin order ; tmp_fine u8[W][stride] = slot & 255          sort (k_scatter_coarse)
//   val_idxs   u32[W][stride]        point index | sign << 31, grouped by bucket slot                             sort (k_sort_fine)
//   col_ptr    u32[W][32769]         start of every bucket slot in val_idxs                                      sort (k_sort_fine)
//   chunk_slot u32[W][chunks]        bucket slot of the first entry of every SMVP chunk                           sort (k_sort_fine)
//   buckets    u32[W][32768][40]     XYZZ records (160 B: 36 limbs + valid flag), Montgomery                      SMVP (here: k_smvp_chunks), stitch
//   heads/tails  [W][chunks][40]     partial sums of bucket runs that cross SMVP chunk boundaries                 SMVP
//   rows/cols/parts                  bucket-reduce scratch: 256 row sums, 128 column sums, 3 partial results per window  bucket reduce (here: k_bpr_*)
//   wsums      u8 [W][96]            window sums, Jacobian, canonical little-endian (the only data that leaves the device)  bucket reduce
//
// The reference keys its CSC rows by the biased digit (65536 rows per window, transpose.template.wgsl:47-73) and lets
// the SMVP thread visit rows h+k and h-k (smvp.template.wgsl:55-92).  Here the sort key is the bucket slot itself
// (|d| mod 2^15, 32768 rows) and the sign rides in bit 31 of the index, so one bucket is one contiguous run.
// Included by a curve unit after its field and group arithmetic (curve_unit.h; the G2 units: fq2.h in place of fq29.h).
#pragma once
#include "scalar_mul.h"
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "curve_ops.h"
#include "recode.h"

namespace MSM_KERNEL_NS {
using namespace MSM_FIELD_NS;
using namespace msm_layout;
using namespace msm_recode;  // ld8 / st8, block_excl_scan_256, k_count

// Sizes that follow the unit's field (FQ_WORDS packed 32-bit words per coordinate: 8 for the 254 / 255-bit fields, 12 for BLS12-381)
constexpr int CW = FQ_WORDS;        // words of a coordinate on the wire and in the resident bases
constexpr int PT_WORDS = 2 * CW;    // an affine point x || y: 64 B (96 B)
constexpr int JAC_WORDS = 3 * CW;   // a Jacobian record x || y || z: 96 B (144 B)

// (exponent tables live in constant memory; filled from the generated constexpr arrays)
template <int N>
struct cwords {
  uint32_t w[N];
};
template <int N>
constexpr cwords<N> make_cwords(const uint32_t (&src)[N]) {
  cwords<N> r{};
  for (int i = 0; i < N; i++) r.w[i] = src[i];
  return r;
}
// MSM_FQ2 (a G2 unit, csrc/fq2.h: the coordinate field is a quadratic extension): the prime-field point sampler (try-and-increment on x
// with a square root) is not built; a G2 unit samples multiples of the subgroup's generator instead (k_sample_points below).
#ifndef MSM_FQ2
__device__ __constant__ cwords<CW> c_pp1d4 = make_cwords(FQ_PP1D4_32);
#endif

// a coordinate's CW packed words (16-byte aligned: CW is a multiple of 4)
__device__ __forceinline__ void ld_coord(const uint32_t* p, uint32_t w[CW]) {
#pragma unroll
  for (int k = 0; k < CW / 4; k++) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[k];
    w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w;
  }
}
__device__ __forceinline__ void st_coord(uint32_t* p, const uint32_t w[CW]) {
#pragma unroll
  for (int k = 0; k < CW / 4; k++) reinterpret_cast<uint4*>(p)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
__device__ __forceinline__ fq ld_fq(const uint32_t* p) {  // packed -> limbs (no domain change)
  uint32_t w[CW];
  ld_coord(p, w);
  return fq_unpack(w);
}
__device__ __forceinline__ void st_fq(uint32_t* p, const fq& x) {  // x exact, < 2^(32 CW)
  uint32_t w[CW];
  fq_pack(w, x);
  st_coord(p, w);
}
// w >= modulus ?   MOD = 0: Fq modulus p (CW words; in an extension-field unit: ANY of the FQ_EXT components of CW / FQ_EXT words),
// MOD = 1: Fr modulus r (8 words)  (constants fold to immediates)
template <int MOD>
__device__ __forceinline__ bool geq_modulus(const uint32_t* w) {
  constexpr int NW = MOD == 0 ? CW / FQ_EXT : 8;
  bool any = false;
#pragma unroll
  for (int e = 0; e < (MOD == 0 ? FQ_EXT : 1); e++) {
    bool gt = false, lt = false;
#pragma unroll
    for (int i = NW - 1; i >= 0; i--) {
      const uint32_t m = MOD == 0 ? FQ_P32[i] : FR_R32[i];
      gt = gt || (!lt && w[e * NW + i] > m);
      lt = lt || (!gt && w[e * NW + i] < m);
    }
    any = any || !lt;
  }
  return any;
}
__device__ __forceinline__ bool fq_equal_exact(const fq& a, const fq& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) d |= a.v[i] ^ b.v[i];
  return d == 0;
}
__device__ __forceinline__ fq fq_curve_b() {  // the curve constant b (y^2 = x^3 + b), Montgomery form
  fq r;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) r.v[i] = FQ_B29[i];
  return r;
}

// Jacobian record, canonical non-Montgomery integers (the wire format of results)
__device__ __forceinline__ void st_jacobian_plain(uint32_t* p, const g1_xyzz& a) {
  fq X, Y, Z;
  g1_to_jacobian(a, X, Y, Z);
  st_fq(p, fq_from_mont(X));
  st_fq(p + CW, fq_from_mont(Y));
  st_fq(p + 2 * CW, fq_from_mont(Z));
}
__device__ __forceinline__ g1_xyzz ld_jacobian_plain(const uint32_t* p) {
  const fq X = fq_to_mont(ld_fq(p)), Y = fq_to_mont(ld_fq(p + CW)), Z = fq_to_mont(ld_fq(p + 2 * CW));
  return g1_from_jacobian(X, Y, Z);
}

// XYZZ record in scratch memory / LDS: 4 FQ_L limbs + identity flag (37 words with 9 limbs: an odd stride, no LDS bank conflicts)
constexpr int XYZZ_WORDS = 4 * FQ_L + 1;
template <typename PTR>
__device__ __forceinline__ void st_xyzz(PTR p, const g1_xyzz& a) {
#pragma unroll
  for (int i = 0; i < FQ_L; i++) {
    p[i] = a.x.v[i];
    p[FQ_L + i] = a.y.v[i];
    p[2 * FQ_L + i] = a.zz.v[i];
    p[3 * FQ_L + i] = a.zzz.v[i];
  }
  p[4 * FQ_L] = a.inf ? 1u : 0u;
}
template <typename PTR>
__device__ __forceinline__ g1_xyzz ld_xyzz(PTR p) {
  g1_xyzz a;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) {
    a.x.v[i] = p[i];
    a.y.v[i] = p[FQ_L + i];
    a.zz.v[i] = p[2 * FQ_L + i];
    a.zzz.v[i] = p[3 * FQ_L + i];
  }
  a.inf = p[4 * FQ_L] != 0;
  return a;
}

// ------------------------------------------------------------------------------------------------ stage 0: bases
// canonical wire bytes -> packed Montgomery affine (≙ decompose_scalars.template.wgsl:41-70, the point half)
__global__ void __launch_bounds__(256) k_convert_points(const uint32_t* in, uint32_t* out, size_t n,  // in may alias out (element-wise)
                                                        uint32_t flags, uint32_t* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wx[CW], wy[CW];
  ld_coord(in + i * PT_WORDS, wx);
  ld_coord(in + i * PT_WORDS + CW, wy);
  if (geq_modulus<0>(wx) || geq_modulus<0>(wy)) atomicOr(err, ERRBIT_NONCANONICAL);
  // flags bit 1 (MSM_HIP_BASES_MONT256): the words are x * 2^256 mod p, not x
  const bool m256 = (flags & 2u) != 0;
  const fq x = m256 ? fq_from_mont256(fq_unpack(wx)) : fq_to_mont(fq_unpack(wx));
  const fq y = m256 ? fq_from_mont256(fq_unpack(wy)) : fq_to_mont(fq_unpack(wy));
  if (flags & 1u) {
    const fq lhs = fq_canonical(fq_sqr(y));
    const fq rhs = fq_canonical(fq_tidy(fq_add(fq_mul(fq_sqr(x), x), fq_curve_b())));
    if (!fq_equal_exact(lhs, rhs)) atomicOr(err, ERRBIT_NOT_ON_CURVE);
  }
  st_fq(out + i * PT_WORDS, x);
  st_fq(out + i * PT_WORDS + CW, y);
}

// The same for a base set that may hold the point at infinity as an all-zero record (MSM_HIP_BASES_ZERO_IS_IDENTITY; (0, 0) is on none of the
// curves, b != 0).  Such a record is stored as the group's generator -- every resident record stays a point of order r, as k_precompute_tables and
// k_endo_points assume -- and marked in `id_bits` (bit i of word i / 64: one wave's ballot, stored by its first lane); id_count receives how many
// there are.  The launches zero the scalars of marked records (k_mask_identity) before anything reads them, so the placeholder is never summed.
__global__ void __launch_bounds__(256) k_convert_points_zero_id(const uint32_t* in, uint32_t* out, size_t n,  // in may alias out (element-wise)
                                                                uint32_t flags, uint32_t* __restrict__ err, uint64_t* __restrict__ id_bits,
                                                                uint32_t* __restrict__ id_count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  uint32_t wx[CW], wy[CW], any = 0;
  if (valid) {
    ld_coord(in + i * PT_WORDS, wx);
    ld_coord(in + i * PT_WORDS + CW, wy);
#pragma unroll
    for (int k = 0; k < CW; k++) any |= wx[k] | wy[k];
  }
  const bool zero = valid && any == 0;
  const unsigned long long ids = __ballot(zero);  // (a wave's 64 lanes are the records of one bitmap word)
  if ((threadIdx.x & 63) == 0 && valid) {
    id_bits[i >> 6] = ids;
    if (ids) atomicAdd(id_count, (uint32_t)__popcll(ids));
  }
  if (!valid) return;
  fq x, y;
  if (zero) {
#pragma unroll
    for (int k = 0; k < FQ_L; k++) {
      x.v[k] = FQ_GEN_X29[k];
      y.v[k] = FQ_GEN_Y29[k];
    }
  } else {
    if (geq_modulus<0>(wx) || geq_modulus<0>(wy)) atomicOr(err, ERRBIT_NONCANONICAL);
    const bool m256 = (flags & 2u) != 0;
    x = m256 ? fq_from_mont256(fq_unpack(wx)) : fq_to_mont(fq_unpack(wx));
    y = m256 ? fq_from_mont256(fq_unpack(wy)) : fq_to_mont(fq_unpack(wy));
    if (flags & 1u) {
      const fq lhs = fq_canonical(fq_sqr(y));
      const fq rhs = fq_canonical(fq_tidy(fq_add(fq_mul(fq_sqr(x), x), fq_curve_b())));
      if (!fq_equal_exact(lhs, rhs)) atomicOr(err, ERRBIT_NOT_ON_CURVE);
    }
  }
  st_fq(out + i * PT_WORDS, x);
  st_fq(out + i * PT_WORDS + CW, y);
}

// The endomorphism's point half (csrc/glv.h): record n + i = phi(P_i) = (beta x_i, y_i) behind the n plain bases
// (a G2 unit: beta is the element (beta, 0) of Fq2 -- the twist has j = 0 like the curve, tools/gen_constants.py emit_g2)
// (records first .. first + count - 1 of the n: the one-shot entry point converts the bases chunk by chunk as they arrive)
__global__ void __launch_bounds__(256) k_endo_points(uint32_t* __restrict__ bases, size_t n, size_t first, size_t count) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const size_t i = first + k;
  fq beta;
#pragma unroll
  for (int k = 0; k < FQ_L; k++) beta.v[k] = FQ_BETA29[k];
  st_fq(bases + (n + i) * PT_WORDS, fq_mul(ld_fq(bases + i * PT_WORDS), beta));
  const uint4* y = reinterpret_cast<const uint4*>(bases + i * PT_WORDS + CW);
  uint4* o = reinterpret_cast<uint4*>(bases + (n + i) * PT_WORDS + CW);
#pragma unroll
  for (int k = 0; k < CW / 4; k++) o[k] = y[k];
}

// Fixed-base tables (reference README.md "Future work": the Elastic-MSM precomputation trade-off): with
// T_w[i] = 2^(16 w) P_i stored for every window, sum_i s_i P_i = sum_i sum_w d_{i,w} T_w[i] needs ONE bucket set for all
// windows -- one stitch / bucket reduce instead of 16 and no window combine -- for 16 x the base memory.
// bases[(w * nb + i)][16]: table w behind table w - 1; table 0 is the plain converted base set (so every entry point that does
// not use the tables keeps working on the same buffer).  One thread per point: 16 doublings per table in XYZZ, then back to
// affine (one inversion by Fermat, a^(p-2)).
__device__ __constant__ cwords<CW / FQ_EXT> c_pm2 = make_cwords(FQ_PM2_32);  // p - 2 (the prime field's)
#ifndef MSM_FQ2
__device__ __forceinline__ fq fq_inv(const fq& a) {  // a exact, nonzero; result exact, < 2p
  fq acc = fq_one();
  for (int bit = 32 * CW - 1; bit >= 0; bit--) {  // (leading zero bits of p - 2 only square the initial one)
    acc = fq_sqr(acc);
    if ((c_pm2.w[bit >> 5] >> (bit & 31)) & 1u) acc = fq_mul(acc, a);
  }
  return acc;
}
#else
__device__ __forceinline__ fq fq_inv(const fq& a) {  // Fq2: 1 / (a0 + a1 u) = (a0 - a1 u) / (a0^2 + a1^2), one Fermat inversion in the prime field
  const fp a0 = f2_c0(a), a1 = f2_c1(a);
  const fp nrm = fpn::fq_mul2(a0, a0, a1, a1);  // the norm, exact, < 2p
  fp acc = fpn::fq_one();
  for (int bit = 32 * FP_WORDS - 1; bit >= 0; bit--) {
    acc = fpn::fq_sqr(acc);
    if ((c_pm2.w[bit >> 5] >> (bit & 31)) & 1u) acc = fpn::fq_mul(acc, nrm);
  }
  return f2_make(fpn::fq_mul(a0, acc), fpn::fq_mul(fpn::fq_sub<3>(fpn::fq_zero(), a1), acc));  // (3p - a1) / norm
}
#endif
// (step_bits: doublings between two tables -- 16, or 20 for the wide tables below, whose last table is only last_step_bits above the one before)
__global__ void __launch_bounds__(256) k_precompute_tables(uint32_t* __restrict__ bases, size_t n, size_t nb, int num_tables, int step_bits,
                                                           int last_step_bits) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const fq px = ld_fq(bases + i * PT_WORDS), py = ld_fq(bases + i * PT_WORDS + CW);
  g1_xyzz acc = g1_from_affine(px, py);
  for (int w = 1; w < num_tables; w++) {
    const int steps = w == num_tables - 1 ? last_step_bits : step_bits;
#pragma unroll 1
    for (int k = 0; k < steps; k++) acc = g1_double(acc);
    // affine again: x = X / ZZ, y = Y / ZZZ with one inversion of ZZ * ZZZ (a point of prime order never doubles to infinity)
    const fq t = fq_inv(fq_mul(acc.zz, acc.zzz));
    const fq x = fq_canonical(fq_mul(acc.x, fq_mul(t, acc.zzz)));
    const fq y = fq_canonical(fq_mul(acc.y, fq_mul(t, acc.zz)));
    st_fq(bases + ((size_t)w * nb + i) * PT_WORDS, x);
    st_fq(bases + ((size_t)w * nb + i) * PT_WORDS + CW, y);
    acc = g1_from_affine(x, y);
  }
}

// ------------------------------------------------------------------------------------------------ batch scalar multiplication
// msm_hip_mul_each / msm_hip_mul_base (csrc/scalar_mul.h has the arithmetic and the counts): out[i] = s_i * P_i over the plain records, or
// s_i * P_base with one base broadcast.  Two kernels per tile of outputs:
//   k_mul_each<ENDO>   one output per lane: the ladder, then the Jacobian record -- X' || Y' into the output record itself, Z into zbuf
//   k_mul_normalize    lane-serial chunks of SMUL_CHUNK results, 256 apart (consecutive lanes: consecutive records), one Fermat inversion per
//                      chunk: 1 / 16 inversion per output; the prefix products go to a scratch array laid out like zbuf
// A base marked in `id_bits` (MSM_HIP_BASES_ZERO_IS_IDENTITY; null: no such base) gives the identity whatever its scalar, which is not even
// compared with r; elsewhere a scalar >= r sets ERRBIT_NONCANONICAL (the host returns the error: nothing of the output is then meaningful).
template <bool ENDO>
__global__ void __launch_bounds__(256) k_mul_each(const uint32_t* __restrict__ bases, const uint32_t* __restrict__ scalars, size_t n, size_t base_first,
                                                  uint32_t broadcast, const uint64_t* __restrict__ id_bits, uint32_t* __restrict__ out_xy,
                                                  uint32_t* __restrict__ zbuf, uint32_t* __restrict__ err, uint32_t check_r) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t b = broadcast ? base_first : base_first + i;
  const bool ident = id_bits != nullptr && ((id_bits[b >> 6] >> (b & 63u)) & 1u) != 0;
  g1_xyzz r = g1_identity();
  if (!ident) {
    uint32_t k[8];
    ld8(scalars + i * 8, k);
    if (check_r && smul_geq_r(k)) {  // (check_r = 0: the table build, whose scalars j 2^(C w) are integers up to 2^256)
      atomicOr(err, ERRBIT_NONCANONICAL);
    } else {
      const fq px = ld_fq(bases + b * PT_WORDS), py = ld_fq(bases + b * PT_WORDS + CW);
      r = ENDO ? smul_endo(px, py, k) : smul_plain(px, py, k, check_r ? SMUL_R_BITS : SMUL_FULL_BITS);
    }
  }
  smul_store_jacobian(out_xy, zbuf, i, r);
}

// The fixed-base form of msm_hip_mul_base (csrc/scalar_mul.h, smul_fixed): the scalars of the table's entries, entry e = (w << (C - 1)) + j - 1 ...
// (entries first .. first + count - 1 into out[0 .. count - 1]: the build runs tile by tile)
__global__ void __launch_bounds__(256) k_mul_table_scalars(int c, size_t first, size_t count, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const size_t e = first + i;
  uint32_t k[8];
  smul_table_scalar(c, (int)(e >> (c - 1)), (uint32_t)(e & ((1u << (c - 1)) - 1u)) + 1u, k);
  st8(out + i * 8, k);
}
// ... and one output per lane from the finished table (packed Montgomery records, all-zero = identity): W gathered mixed additions, no doublings
__global__ void __launch_bounds__(256) k_mul_fixed(const uint32_t* __restrict__ table, int c, const uint32_t* __restrict__ scalars, size_t n,
                                                   uint32_t* __restrict__ out_xy, uint32_t* __restrict__ zbuf, uint32_t* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8];
  ld8(scalars + i * 8, k);
  g1_xyzz r = g1_identity();
  if (smul_geq_r(k)) atomicOr(err, ERRBIT_NONCANONICAL);
  else r = smul_fixed(table, c, k);
  smul_store_jacobian(out_xy, zbuf, i, r);
}

__global__ void __launch_bounds__(256) k_mul_normalize(uint32_t* __restrict__ xy, const uint32_t* __restrict__ zbuf, uint32_t* __restrict__ prefix, size_t n) {
  const size_t block_first = (size_t)blockIdx.x * (256 * SMUL_CHUNK);
  const size_t first = block_first + threadIdx.x;
  const size_t block_end = block_first + 256 * SMUL_CHUNK;
  const size_t end = block_end < n ? block_end : n;
  if (first >= end) return;
  const fq prod = smul_norm_forward(zbuf, prefix, first, 256, end);
  smul_norm_backward(xy, zbuf, prefix, first, 256, end, fq_inv(prod));
}

#ifndef MSM_FQ2
// ------------------------------------------------------------------------------------------------ group FFT over the resident bases
// msm_hip_bases_fft: out[i] = c * sum_j omega^(i j) P_j over the first n = 2^log_n plain records, a radix-2 decimation-in-time transform whose
// elements are curve points (csrc/scalar_mul.h, smul_butterfly).  log_n stages; between two stages the elements are packed Montgomery affine
// records like the resident bases, the identity as the all-zero record:
//   k_fft_stage<LADDER>  one butterfly per lane, n / 2 lanes.  Stage s pairs elements ia = (k >> s) 2^(s+1) + j and ib = ia + 2^s, j = k mod 2^s,
//                        with the twiddle omega^(j n / 2^(s+1)) (entry j << (log_n - 1 - s) of the table of the n / 2 powers of omega), and
//                        leaves a + w b and a - w b as Jacobian records at ia and ib: X' || Y' in the record, Z in zbuf (smul_store_jacobian).
//                        A lane reads and writes its own two elements only, so a stage may run in place (src == dst).  first != 0: element i is
//                        resident base bitrev(i), an identity if `id_bits` marks it; every twiddle of that stage is 1: LADDER = 0, additions only.
//   k_fft_normalize      k_mul_normalize's walk with the backward pass that keeps Montgomery records (smul_norm_backward<true>)
//   k_fft_scale<LADDER>  dst[i] = k * src[i] for one broadcast scalar (the 1 / n of MSM_HIP_FFT_SCALE_INV_N), again as Jacobian records
// The last pass of a call is normalised by k_mul_normalize, which writes wire records.
template <int LADDER>
__global__ void __launch_bounds__(256) k_fft_stage(const uint32_t* src, uint32_t* dst, uint32_t* zbuf, const uint32_t* __restrict__ twiddles, int log_n,
                                                   int stage, uint32_t first, const uint64_t* __restrict__ id_bits) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ((size_t)1 << (log_n - 1))) return;
  const size_t j = k & (((size_t)1 << stage) - 1);
  const size_t ia = ((k >> stage) << (stage + 1)) + j, ib = ia + ((size_t)1 << stage);
  size_t ra = ia, rb = ib;
  bool a_id = false, b_id = false;
  if (first) {
    ra = __brev((uint32_t)ia) >> (32 - log_n);
    rb = __brev((uint32_t)ib) >> (32 - log_n);
    if (id_bits != nullptr) {
      a_id = ((id_bits[ra >> 6] >> (ra & 63u)) & 1u) != 0;
      b_id = ((id_bits[rb >> 6] >> (rb & 63u)) & 1u) != 0;
    }
  }
  uint32_t w[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (LADDER != SMUL_LADDER_NONE) ld8(twiddles + (j << (log_n - 1 - stage)) * 8, w);
  g1_xyzz sum, diff;
  smul_butterfly<LADDER>(src + ra * PT_WORDS, a_id, src + rb * PT_WORDS, b_id, w, sum, diff);
  smul_store_jacobian(dst, zbuf, ia, sum);
  smul_store_jacobian(dst, zbuf, ib, diff);
}

__global__ void __launch_bounds__(256) k_fft_normalize(uint32_t* __restrict__ xy, const uint32_t* __restrict__ zbuf, uint32_t* __restrict__ prefix, size_t n) {
  const size_t block_first = (size_t)blockIdx.x * (256 * SMUL_CHUNK);
  const size_t first = block_first + threadIdx.x;
  const size_t block_end = block_first + 256 * SMUL_CHUNK;
  const size_t end = block_end < n ? block_end : n;
  if (first >= end) return;
  const fq prod = smul_norm_forward(zbuf, prefix, first, 256, end);
  smul_norm_backward<true>(xy, zbuf, prefix, first, 256, end, fq_inv(prod));
}

template <int LADDER>
__global__ void __launch_bounds__(256) k_fft_scale(const uint32_t* src, uint32_t* dst, uint32_t* zbuf, const uint32_t* __restrict__ scalar, size_t n) {  // src may alias dst (element-wise)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8];
  ld8(scalar, k);
  smul_store_jacobian(dst, zbuf, i, smul_twiddle<LADDER>(src + i * PT_WORDS, false, k));
}
#endif

// ------------------------------------------------------------------------------------------------ stage 1+2: what the recode takes from the curve
// The recode and the sort are curve-neutral (sort_kernels.h).  Two passes in front of them are not: the conversion of Montgomery scalars, which
// reduces modulo this curve's r, and the first pass of endomorphism launches, which splits every scalar with this curve's lattice (csrc/glv.h).
//
// Scalars handed over as s * 2^256 mod r (the in-memory limbs of a 4 x 64-bit Montgomery library with R = 2^256) are turned
// into the canonical wire format by one pre-pass: a 9-limb Montgomery reduction of (s_mont << 5), i.e. s_mont * 2^5 / 2^261.
#ifdef MSM_FQ2  // (a G2 unit: the container of a 256-bit scalar is an element of the PRIME field)
using sfe = fp;
constexpr int SF_L = FP_L, SF_WORDS = FP_WORDS;
__device__ __forceinline__ sfe sf_unpack(const uint32_t* w) { return fpn::fq_unpack(w); }
__device__ __forceinline__ void sf_pack(uint32_t* w, const sfe& x) { fpn::fq_pack(w, x); }
#else
using sfe = fq;
constexpr int SF_L = FQ_L, SF_WORDS = CW;
__device__ __forceinline__ sfe sf_unpack(const uint32_t* w) { return fq_unpack(w); }
__device__ __forceinline__ void sf_pack(uint32_t* w, const sfe& x) { fq_pack(w, x); }
#endif
__device__ __forceinline__ void fr_from_mont256(const uint32_t w[8], uint32_t out[8]) {
  // (the scalar field's 256-bit values in the unit's limb layout: SF_L limbs of FQ_W bits hold them with room to spare)
  constexpr int SH = FQ_W * SF_L - 256, SH_LIMBS = SH / FQ_W, SH_BITS = SH % FQ_W;  // s_mont * 2^SH / 2^(FQ_W SF_L) = s_mont / 2^256
  uint32_t wide[SF_WORDS];
#pragma unroll
  for (int k = 0; k < SF_WORDS; k++) wide[k] = k < 8 ? w[k] : 0u;
  const sfe x = sf_unpack(wide);
  uint64_t c[2 * SF_L + 1];
#pragma unroll
  for (int k = 0; k < 2 * SF_L + 1; k++) c[k] = 0;
#pragma unroll
  for (int k = 0; k < SF_L; k++) c[k + SH_LIMBS] = (uint64_t)x.v[k] << SH_BITS;
#pragma unroll
  for (int i = 0; i < SF_L; i++) {
    const uint32_t m = ((uint32_t)c[i] * FR_N0_29) & FQ_MASK;
#pragma unroll
    for (int j = 0; j < SF_L; j++) c[i + j] += (uint64_t)m * FR_R29[j];
    c[i + 1] += c[i] >> FQ_W;
  }
  sfe t;
#pragma unroll
  for (int k = SF_L; k < 2 * SF_L - 1; k++) {
    t.v[k - SF_L] = (uint32_t)c[k] & FQ_MASK;
    c[k + 1] += c[k] >> FQ_W;
  }
  t.v[SF_L - 1] = (uint32_t)c[2 * SF_L - 1];
  // t <= r: one conditional subtraction makes it canonical
  sfe d;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < SF_L; i++) {
    const uint32_t u = t.v[i] - FR_R29[i] - borrow;
    borrow = u >> 31;
    d.v[i] = (i < SF_L - 1) ? (u & FQ_MASK) : u;
  }
#pragma unroll
  for (int i = 0; i < SF_L; i++) t.v[i] = borrow ? t.v[i] : d.v[i];
  sf_pack(wide, t);
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = wide[k];
}

__global__ void __launch_bounds__(256) k_scalars_from_mont256(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t count,
                                                              uint32_t* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t w[8], o[8];
  ld8(in + i * 8, w);
  if (geq_modulus<1>(w)) atomicOr(err, ERRBIT_NONCANONICAL);
  fr_from_mont256(w, o);
  uint4* q = reinterpret_cast<uint4*>(out + i * 8);
  q[0] = make_uint4(o[0], o[1], o[2], o[3]);
  q[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// this unit's split as the functor k_count takes (recode.h): k_count<C, 4, glv_split_fn> is the first pass of endomorphism launches
struct glv_split_fn {
  __device__ __forceinline__ bool operator()(const uint32_t k[8], uint32_t h1[4], uint32_t h2[4]) const { return glv_split(k, h1, h2); }
};

// ------------------------------------------------------------------------------------------------ stage 3: SMVP
// Bucket accumulate (≙ smvp.template.wgsl:31-117, CPU model test/utils.rs:166-219):
//   B[w][k] = sum_{d=+k} P - sum_{d=-k} P  (k >= 1),   B[w][0] = -sum_{d=-2^15} P
// The reference gives one thread one bucket, so a wave runs as long as its fullest bucket.  Here every lane owns a
// fixed-length chunk of `chunk_len` consecutive entries of the slot-sorted list -- equal work per lane whatever the bucket
// sizes -- and flushes its accumulator whenever the slot changes.  The host picks a chunk length (in
// [SMVP_CHUNK_MIN, SMVP_CHUNK_MAX]; msm_plan.h: chunk_len_for) so that about SMVP_TARGET_LANES lanes exist for n entries per window (about three rounds of 3 waves
// per SIMD at 168 VGPRs, no scratch) and sizes the chunk arrays and grids with it; the length actually used is settled on the device
// from the entries the sort produced (sort_kernels.h, smvp_chunk_len: never longer than the host's).  Runs that cross a chunk boundary leave a "tail" piece
// (in the chunk where the run starts) and "head" pieces (in the chunks it continues into); k_smvp_stitch adds them.
// Buckets and pieces are stored as raw XYZZ records (no multiplication on the flush path).
constexpr int REC_WORDS = (XYZZ_WORDS + 3) / 4 * 4;  // 160 B record with 9 limbs: 36 limbs, valid flag, 3 pad words; 16-byte aligned (240 B with 14)
constexpr int REC_FLAG = 4 * FQ_L;                   // word index of the valid flag

// word I of a record: limbs of x, y, zz, zzz, then the valid flag, then padding (static indices only: an intermediate word array would
// not be promoted to registers and cost the stitch / row-column kernels a 148-byte scratch object each)
template <int I>
__device__ __forceinline__ uint32_t rec_get(const g1_xyzz& a) {
  if constexpr (I < FQ_L) return a.x.v[I];
  else if constexpr (I < 2 * FQ_L) return a.y.v[I - FQ_L];
  else if constexpr (I < 3 * FQ_L) return a.zz.v[I - 2 * FQ_L];
  else if constexpr (I < 4 * FQ_L) return a.zzz.v[I - 3 * FQ_L];
  else if constexpr (I == REC_FLAG) return a.inf ? 0u : 1u;
  else return 0u;
}
template <int I>
__device__ __forceinline__ void rec_set(g1_xyzz& a, uint32_t v) {
  if constexpr (I < FQ_L) a.x.v[I] = v;
  else if constexpr (I < 2 * FQ_L) a.y.v[I - FQ_L] = v;
  else if constexpr (I < 3 * FQ_L) a.zz.v[I - 2 * FQ_L] = v;
  else if constexpr (I < 4 * FQ_L) a.zzz.v[I - 3 * FQ_L] = v;
}
template <int... K>
__device__ __forceinline__ void st_rec_quads(uint4* q, const g1_xyzz& a, std::integer_sequence<int, K...>) {
  ((q[K] = make_uint4(rec_get<4 * K>(a), rec_get<4 * K + 1>(a), rec_get<4 * K + 2>(a), rec_get<4 * K + 3>(a))), ...);
}
template <int... K>
__device__ __forceinline__ void ld_rec_quads(const uint4* q, g1_xyzz& a, std::integer_sequence<int, K...>) {
  ((void)([&] {
     const uint4 v = q[K];
     rec_set<4 * K>(a, v.x);
     rec_set<4 * K + 1>(a, v.y);
     rec_set<4 * K + 2>(a, v.z);
     rec_set<4 * K + 3>(a, v.w);
   }()),
   ...);
}
__device__ __forceinline__ void st_rec(uint32_t* p, const g1_xyzz& a) {
  st_rec_quads(reinterpret_cast<uint4*>(p), a, std::make_integer_sequence<int, REC_WORDS / 4>{});
}
__device__ __forceinline__ g1_xyzz ld_rec(const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 fl = q[REC_FLAG / 4];
  const uint32_t flag = REC_FLAG % 4 == 0 ? fl.x : (REC_FLAG % 4 == 1 ? fl.y : (REC_FLAG % 4 == 2 ? fl.z : fl.w));
  if (flag == 0) return g1_identity();
  g1_xyzz a;
  ld_rec_quads(q, a, std::make_integer_sequence<int, REC_WORDS / 4>{});
  a.inf = false;
  return a;
}

// Assignments to the SMVP loop's accumulator from its rare paths (a run's first point; the repair after a doubling).  On the device they
// are written as moves INTO the accumulator's own registers (read-write operands): a plain assignment makes every coordinate a merge of
// two values at the end of the branch, and the register allocator then keeps the merged value in the rare path's registers -- the hot
// path, which updates the coordinates in place, pays a copy per limb and iteration to get there and back (measured: 36 + 18 v_mov).
__device__ __forceinline__ void smvp_set(fq& dst, const fq& src) {
#pragma unroll
  for (int i = 0; i < FQ_L; i++) asm("v_mov_b32 %0, %1" : "+v"(dst.v[i]) : "v"(src.v[i]));
}
__device__ __forceinline__ void smvp_set_one(fq& dst) {
#pragma unroll
  for (int i = 0; i < FQ_L; i++) asm("v_mov_b32 %0, %1" : "+v"(dst.v[i]) : "s"(FQ_ONE29[i]));
}
__device__ __forceinline__ void smvp_restart(g1_xyzz& acc, const fq& px, const fq& py) {
  smvp_set(acc.x, px);
  smvp_set(acc.y, py);
  smvp_set_one(acc.zz);
  smvp_set_one(acc.zzz);
  acc.inf = false;
}
__device__ __forceinline__ void smvp_assign(g1_xyzz& acc, const g1_xyzz& src) {
  smvp_set(acc.x, src.x);
  smvp_set(acc.y, src.y);
  smvp_set(acc.zz, src.zz);
  smvp_set(acc.zzz, src.zzz);
  acc.inf = src.inf;
}

// 168 VGPRs hold the 9-limb loop (3 waves per SIMD); 14 limbs take up to 256 (2 waves).  Fq2 on 9 limbs (BN254 G2) wants 278: capped at 256 -- 12 words
// of scratch -- because the second wave is worth 23 % of the kernel (4.29 -> 3.31 ms at 2^20, profiles/r03_g2_throughput.txt); Fq2 on 14 limbs: one wave
#ifndef MSM_SMVP_WAVES_WIDE
#define MSM_SMVP_WAVES_WIDE 1  // Fq2 on 14 limbs (BLS12-381 G2): 256 VGPRs + 130 AGPRs at one wave; two waves = a 256-register cap with scratch (A/B: profiles/r04_g2_two_waves.txt)
#endif
#ifndef MSM_SMVP_WAVES_9
#define MSM_SMVP_WAVES_9 3  // (2: experiment -- a third of the register file and of the wave slots left to the kernels of another launch, profiles/r05_two_context_overlap.txt)
#endif
constexpr int SMVP_WAVES_PER_SIMD = FQ_L <= 9 ? MSM_SMVP_WAVES_9 : FQ_L <= 18 ? 2 : MSM_SMVP_WAVES_WIDE;
// the stitch and the row / column sums (full additions: the widest kernels after the SMVP) in a unit with 18 limbs per coordinate: two waves per
// SIMD as well (256 VGPRs + 0.26 KB of scratch instead of 309 - 317 + AGPRs: -1.5 % per MSM)
#ifndef MSM_REDUCE_WAVES_FQ2
#define MSM_REDUCE_WAVES_FQ2 2
#endif
constexpr int REDUCE_WAVES_PER_SIMD = FQ_L == 18 ? MSM_REDUCE_WAVES_FQ2 : 1;  // (1: no constraint beyond the workgroup size)
__global__ void __launch_bounds__(256, SMVP_WAVES_PER_SIMD) k_smvp_chunks(const uint32_t* __restrict__ bases, const uint32_t* __restrict__ col_ptr,
                                                     const uint32_t* __restrict__ val_idxs, size_t stride, uint32_t chunks,
                                                     const uint32_t* __restrict__ chunk_len_dev, const uint32_t* __restrict__ chunk_slot,
                                                     uint32_t* __restrict__ buckets, uint32_t* __restrict__ heads,
                                                     uint32_t* __restrict__ tails, uint32_t half) {
  const uint32_t chunk_len = *chunk_len_dev;
#if defined(__HIP_DEVICE_COMPILE__) && MSM_SMVP_WAVES_9 == 2
  if constexpr (FQ_L <= 9) asm volatile("; two waves per SIMD" ::: "v175");  // 176 VGPRs allocated: 2 waves per SIMD whatever the loop needs
#endif
  const int lw = blockIdx.y;
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  const uint32_t* cp = col_ptr + (size_t)lw * (half + 1);
  const uint32_t nw = cp[half];
  const uint64_t begin64 = (uint64_t)c * chunk_len;
  if (c >= chunks || begin64 >= nw) return;
  const uint32_t begin = (uint32_t)begin64;
  const uint32_t end = (nw - begin > chunk_len) ? begin + chunk_len : nw;
  // slot containing entry `begin` (cp[s] <= begin < cp[s + 1]), tabulated by k_sort_fine
  uint32_t s = chunk_slot[(size_t)lw * chunks + c], run_begin = cp[s], run_end = cp[s + 1];
  const uint32_t* vi = val_idxs + (size_t)lw * stride;
  const size_t rec = ((size_t)lw * chunks + c) * REC_WORDS;
  g1_xyzz acc = g1_identity();
  bool wneg = false;  // sign carried by acc.y (g1_madd_w); applied when the accumulator is flushed
  // Two entries ahead: the index of entry t + 2 and the point of entry t + 1 are requested before the addition of entry t starts, so that
  // a gather that misses the Infinity Cache (bases beyond 256 MiB) is covered by ~4 us of arithmetic instead of stalling the wave.  Both
  // loads are unconditional (clamped to the chunk's last entry): a conditional load makes every prefetch register a merge of old and
  // new value, i.e. a copy per register and iteration.
  const uint32_t last = end - 1;
  uint32_t vnext = vi[begin];
  uint32_t vnn = vi[begin + 1 < end ? begin + 1 : last];
  uint32_t wx[CW], wy[CW];
  ld_coord(bases + (size_t)(vnext & 0x7fffffffu) * PT_WORDS, wx);
  ld_coord(bases + (size_t)(vnext & 0x7fffffffu) * PT_WORDS + CW, wy);
  for (uint32_t t = begin; t < end; t++) {
    const uint32_t v = vnext;
    fq px = fq_unpack(wx), py = fq_unpack(wy);
#if defined(__HIP_DEVICE_COMPILE__)
    // the loads below stay behind the unpacking (the limbs are pinned in front of this point): they can then reuse the registers of
    // wx / wy; hoisted above it they need a second set and 16 copies per iteration
#pragma unroll
    for (int i = 0; i < FQ_L; i++) asm volatile("" : "+v"(px.v[i]), "+v"(py.v[i]) : : "memory");
#endif
    vnext = vnn;
    vnn = vi[t + 2 < end ? t + 2 : last];
    {
      const uint32_t* pt = bases + (size_t)(vnext & 0x7fffffffu) * PT_WORDS;
      ld_coord(pt, wx);
      ld_coord(pt + CW, wy);
    }
    const bool sneg = (v >> 31) != 0u;  // bit 31: the digit is negative
    if (t == run_end) {  // the run of slot s ended inside this chunk
      if (run_begin >= begin) st_rec(buckets + ((size_t)lw * half + s) * REC_WORDS, g1_unsigned(acc, wneg));
      else st_rec(heads + rec, g1_unsigned(acc, wneg));
      acc.inf = true;  // (the coordinates of an empty accumulator are never read: no need to zero 36 registers)
      run_begin = run_end;
      // next non-empty slot (exists: t < nw).  Usually the very next one; after a few empty slots switch to a binary search of the
      // slot whose run contains entry t: a lane that walks thousands of empty slots with dependent loads (a few heavy buckets far
      // apart: few distinct scalars, or the two halves of equal scalars) would hold up the whole kernel for milliseconds
      int gap = 0;
      do { s++; run_end = cp[s + 1]; } while (run_end == run_begin && ++gap < 8);
      if (run_end == run_begin) {
        uint32_t lo = s + 1, hi = half - 1;  // cp[hi + 1] = nw > t = run_begin
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (cp[mid + 1] > run_begin) hi = mid;
          else lo = mid + 1;
        }
        s = lo;
        run_end = cp[s + 1];
      }
    }
    if (acc.inf) {  // the first point of a run: W = y with the digit's sign as the state -- no negation, no arithmetic
      smvp_restart(acc, px, py);
      wneg = sneg;
    } else {
      const int status = g1_madd_w_hot(acc, wneg, px, py, sneg);
      if (status) {  // the point met itself or its negative in the accumulator (duplicate bases): repair, from the point read again
        wneg = false;
        if (status == 1) {
          const uint32_t* pt = bases + (size_t)(v & 0x7fffffffu) * PT_WORDS;
          const fq qy = ld_fq(pt + CW);
          smvp_assign(acc, g1_double_affine(ld_fq(pt), sneg ? fq_neg_canonical(qy) : qy));
        } else {
          acc.inf = true;
        }
      }
    }
  }
  acc = g1_unsigned(acc, wneg);
  // last run of the chunk: complete only if it started here and ends exactly at or before `end`
  if (run_begin >= begin && run_end <= end) {
    st_rec(buckets + ((size_t)lw * half + s) * REC_WORDS, acc);
  } else if (run_begin < begin) {
    st_rec(heads + rec, acc);  // continuation of a run from an earlier chunk (it may continue further)
  } else {
    st_rec(tails + rec, acc);  // run starts here and continues into the next chunk(s)
  }
}

// x[dst] += x[src] for XYZZ records held in LDS
__device__ __forceinline__ void lds_add_pair(uint32_t* x, int dst, int src) {
  st_xyzz(x + dst * XYZZ_WORDS, g1_add(ld_xyzz(x + dst * XYZZ_WORDS), ld_xyzz(x + src * XYZZ_WORDS)));
}

// One lane per bucket slot: empty slots get the identity record (no memset of the bucket array is needed), runs that lie
// inside one chunk were already written by k_smvp_chunks, and a run that spans chunks c0 < ... < c1 is the tail piece of
// c0 plus the head pieces of c0+1 .. c1.  Buckets with more than STITCH_BIG pieces (heavily skewed scalars: one bucket
// may hold every entry of a window) are queued for k_smvp_stitch_big instead of being walked by one lane.
#ifndef MSM_STITCH_SORTED
#define MSM_STITCH_SORTED 1
#endif
constexpr uint32_t STITCH_BIG = 32;

__global__ void __launch_bounds__(256, REDUCE_WAVES_PER_SIMD) k_smvp_stitch(const uint32_t* __restrict__ col_ptr, uint32_t chunks, const uint32_t* __restrict__ chunk_len_dev,
                                                     const uint32_t* __restrict__ heads, const uint32_t* __restrict__ tails,
                                                     uint32_t* __restrict__ buckets, uint32_t* __restrict__ big_queue) {
  const int lw = blockIdx.y;
  const uint32_t half = gridDim.x * 256;              // bucket slots per window: one lane per slot
  const uint32_t chunk_len = *chunk_len_dev;
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;  // < half by grid construction
  const uint32_t* cp = col_ptr + (size_t)lw * (half + 1);
  const uint32_t b = cp[s], e = cp[s + 1];
  uint32_t c0 = 0, adds = 0;  // adds = c1 - c0 of a run this kernel walks, 0 for every other slot
  if (b == e) {
    st_rec(buckets + ((size_t)lw * half + s) * REC_WORDS, g1_identity());
  } else {
    c0 = b / chunk_len;
    const uint32_t c1 = (e - 1) / chunk_len;
    if (c0 != c1) {
      adds = c1 - c0;
      if (adds >= STITCH_BIG) {
        const uint32_t at = atomicAdd(&big_queue[0], 1u);
        if (at < STITCH_BIG_CAP) {
          big_queue[1 + at] = ((uint32_t)lw << 16) | s;
          adds = 0;
        }
      }
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  // The queue pointer above is a scalar load issued inside a branch; in the units whose group addition is large (Fq2) the branches below are far
  // ones, expanded through a scavenged SGPR pair -- which must not have that load still in flight (tools/check_long_branch_hazard.py)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
#if MSM_STITCH_SORTED
  // Round 5: a slot's run spans 1 .. 5 chunks (64 entries per bucket against ~28 per chunk), and a wave walks as long as its longest run -- about 4.5
  // additions for a mean of 2.3.  The workgroup's 256 slots are therefore handed to its lanes in DESCENDING order of their addition count (a
  // counting sort over 8 classes through LDS): every wave then holds runs of nearly equal length, and the lanes with nothing to add fill the
  // last wave(s), which leave at once.
  __shared__ uint32_t cls[4][8];
  __shared__ uint32_t perm_s[256], perm_c0[256], perm_adds[256];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const uint32_t k = adds < 7u ? adds : 7u;
  unsigned long long mine = 0;
#pragma unroll
  for (uint32_t v = 0; v < 8; v++) {
    const unsigned long long bal = __ballot(k == v);
    if (k == v) mine = bal;
    if (lane == 0) cls[wave][v] = (uint32_t)__popcll(bal);
  }
  __syncthreads();
  uint32_t pos = (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));  // same class, same wave, lower lane
#pragma unroll
  for (int w = 0; w < 4; w++) {
#pragma unroll
    for (uint32_t v = 0; v < 8; v++) {
      const uint32_t cnt = cls[w][v];
      if (v > k || (v == k && w < wave)) pos += cnt;  // longer runs first; same length: earlier waves first
    }
  }
  perm_s[pos] = s;
  perm_c0[pos] = c0;
  perm_adds[pos] = adds;
  __syncthreads();
  const uint32_t ms = perm_s[t], mc0 = perm_c0[t], madds = perm_adds[t];
#else
  const uint32_t ms = s, mc0 = c0, madds = adds;
#endif
  if (madds == 0) return;
  g1_xyzz acc = ld_rec(tails + ((size_t)lw * chunks + mc0) * REC_WORDS);
  for (uint32_t c = mc0 + 1; c <= mc0 + madds; c++) acc = g1_add(acc, ld_rec(heads + ((size_t)lw * chunks + c) * REC_WORDS));
  st_rec(buckets + ((size_t)lw * half + ms) * REC_WORDS, acc);
}

// Queued big buckets: one block per bucket (blocks stride over the queue); every thread adds a strided subset of the
// pieces, then an LDS tree.  The queue counter is reset for the slot's next launch by k_bpr_final, a later kernel of the same
// stream (a last-block hand-off here would cost a __threadfence per launch, queue empty or not).
// HUGE buckets (>= STITCH_HUGE pieces: one value shared by a large part of the scalars -- the ones and small constants of witness
// vectors, all-equal scalars) would keep their single workgroup busy for pieces / 256 dependent additions per thread while the rest
// of the GPU idles: when the queue is short (<= 256 items) the huge ones are shared by STITCH_BLOCKS / (their number) workgroups
// each; a workgroup leaves its partial sum in the slot's scratch records and the last one to arrive adds the partials
// (device-scope fences: only on this rare path).
// big_queue layout (words): [0] count, [1 .. CAP] items, [BIGQ_CHUNK_LEN] the launch's SMVP chunk length (smvp_chunk_len),
// [BIGQ_COUNTERS ..] 256 arrival counters (zero between launches), [BIGQ_SCRATCH ..] 256 XYZZ records.
constexpr uint32_t STITCH_HUGE = 1024;
constexpr size_t BIGQ_WORDS = BIGQ_SCRATCH + (size_t)STITCH_BLOCKS * REC_WORDS;

__global__ void __launch_bounds__(256) k_smvp_stitch_big(const uint32_t* __restrict__ col_ptr, uint32_t chunks,
                                                         const uint32_t* __restrict__ heads, const uint32_t* __restrict__ tails,
                                                         uint32_t* __restrict__ buckets, uint32_t* big_queue,
                                                         uint32_t half) {
  __shared__ uint32_t x[256 * XYZZ_WORDS];
  __shared__ uint32_t huge_flag[256], huge_list[256], wave_tot[4], s_nhuge, s_last;
  const int t = threadIdx.x;
  uint32_t count = big_queue[0];
  if (count > STITCH_BIG_CAP) count = STITCH_BIG_CAP;
  if (count == 0) return;
  const uint32_t chunk_len = big_queue[BIGQ_CHUNK_LEN];
  // the pieces of queue item `item`: chunks c0 .. c1 of local window lw, bucket slot s
  auto decode = [&](uint32_t item, uint32_t& lw, uint32_t& s, uint32_t& c0, uint32_t& c1) {
    const uint32_t code = big_queue[1 + item];
    lw = code >> 16;
    s = code & 0xffffu;
    const uint32_t* cp = col_ptr + (size_t)lw * (half + 1);
    c0 = cp[s] / chunk_len;
    c1 = (cp[s + 1] - 1) / chunk_len;
  };
  // block-wide sum of the per-thread accumulators -> x[0]
  auto block_sum = [&](const g1_xyzz& acc) {
    st_xyzz(x + t * XYZZ_WORDS, acc);
    __syncthreads();
    for (int sft = 128; sft >= 1; sft >>= 1) {
      if (t < sft) lds_add_pair(x, t, t + sft);
      __syncthreads();
    }
  };
  // which items are huge (every workgroup computes the same list, in queue order)
  const bool may_split = count <= 256 && gridDim.x == (unsigned)STITCH_BLOCKS;
  uint32_t nhuge = 0;
  if (may_split) {
    uint32_t f = 0;
    if ((uint32_t)t < count) {
      uint32_t lw, s, c0, c1;
      decode(t, lw, s, c0, c1);
      f = c1 - c0 + 1 >= STITCH_HUGE ? 1u : 0u;
    }
    huge_flag[t] = f;
    const uint32_t pos = block_excl_scan_256(f, wave_tot);
    if (f) huge_list[pos] = (uint32_t)t;
    if (t == 255) s_nhuge = pos + f;
    __syncthreads();
    nhuge = s_nhuge;
  }
  for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
    if (may_split && huge_flag[item]) continue;  // block-uniform
    uint32_t lw, s, c0, c1;
    decode(item, lw, s, c0, c1);
    g1_xyzz acc = g1_identity();
    for (uint32_t c = c0 + t; c <= c1; c += 256) {
      const uint32_t* piece = (c == c0 ? tails : heads) + ((size_t)lw * chunks + c) * REC_WORDS;
      acc = g1_add(acc, ld_rec(piece));
    }
    block_sum(acc);
    if (t == 0) st_rec(buckets + ((size_t)lw * half + s) * REC_WORDS, ld_xyzz(x));
    __syncthreads();
  }
  if (nhuge == 0) return;
  const uint32_t per = (uint32_t)STITCH_BLOCKS / nhuge;  // workgroups per huge bucket, >= 1
  const uint32_t hi = blockIdx.x / per, sub = blockIdx.x % per;
  if (hi >= nhuge) return;
  uint32_t lw, s, c0, c1;
  decode(huge_list[hi], lw, s, c0, c1);
  g1_xyzz acc = g1_identity();
  for (uint32_t c = c0 + sub * 256 + t; c <= c1; c += per * 256) {
    const uint32_t* piece = (c == c0 ? tails : heads) + ((size_t)lw * chunks + c) * REC_WORDS;
    acc = g1_add(acc, ld_rec(piece));
  }
  block_sum(acc);
  uint32_t* out = buckets + ((size_t)lw * half + s) * REC_WORDS;
  if (per == 1) {
    if (t == 0) st_rec(out, ld_xyzz(x));
    return;
  }
  uint32_t* counters = big_queue + BIGQ_COUNTERS;
  uint32_t* scratch = big_queue + BIGQ_SCRATCH;
  if (t == 0) {
    st_rec(scratch + (size_t)blockIdx.x * REC_WORDS, ld_xyzz(x));
    __threadfence();  // the partial is visible device-wide before this workgroup is counted
    s_last = atomicAdd(&counters[hi], 1u) == per - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();  // acquire: the other workgroups' partials
  block_sum((uint32_t)t < per ? ld_rec(scratch + ((size_t)hi * per + t) * REC_WORDS) : g1_identity());
  if (t == 0) {
    st_rec(out, ld_xyzz(x));
    counters[hi] = 0;  // ready for the slot's next launch
  }
}

// ------------------------------------------------------------------------------------------------ stage 4: bucket reduce
// S_w = sum_{k=1}^{h-1} k * B[k] + h * B[0]   (≙ bpr.template.wgsl:38-132, CPU models test/utils.rs:222-338).
//
// This stage is bound by the DEPTH of dependent group additions (a lone wave needs ~7.5 us per addition), not by bytes
// or work.  The reference's running sums (128 buckets per thread, then a 15-bit double-and-add, bpr.template.wgsl:66-75,
// 124-125) are ~270 additions deep; shortening the runs only trades depth for double-and-add work.  Instead the weighted
// sum is decomposed into PLAIN sums, which are shallow trees.  Slot 0 carries weight h = 2^15, so bucket position q
// (1..32768) reads slot q & 32767; write q - 1 = 128 * hi + lo:
//     S = sum_q q B_q = 128 * sum_hi hi * R_hi  +  sum_lo (lo + 1) * C_lo,   R_hi = sum_lo B[hi][lo],  C_lo = sum_hi B[hi][lo]
//   k_bpr_rowcol  the 256 row sums and 128 column sums of every window: 3 serial additions + a 5- or 6-level LDS tree
//   k_bpr_w256    W(X) = sum_{i<256} i * X_i by the same split applied twice more (16 x 16, then 4 x 4): ~16 additions deep
//   k_bpr_final   S = 128 * W(R) + W(C) + sum(C): 7 doublings + 2 additions, emits the window sum as canonical bytes
// Work: 2 additions per bucket (the minimum of the running-sum scheme) + O(1) per window; depth ~33 additions.

// tree-add `count` (power of two) records spaced `stride` records apart starting at x[base]; every thread of the block
// must call it (it contains barriers); on return x[base] holds the sum.  `id` enumerates jobs block-wide.

// LOG_R = log2 of the buckets each thread adds serially before the LDS tree.  The host picks 4 (16 buckets) when many
// windows are reduced at once -- fewer, better-filled wave-additions: the stage is then bound by the ~7 us a SIMD needs
// per wave-addition -- and 2 for few windows, where only the depth counts.
// LOG_ROWS = log2 of the rows of the window's bucket grid: 2^(C-1) buckets = 2^LOG_ROWS rows x 128 columns (8 / 6 / 4 for
// C = 16 / 14 / 12).  The row sums of window w land in rows[w][0 .. ROWS) (stride BPR_ROWS), the column sums in cols[w][0 .. 128).
template <int LOG_R, int LOG_ROWS>
__global__ void __launch_bounds__(256, REDUCE_WAVES_PER_SIMD) k_bpr_rowcol(const uint32_t* __restrict__ buckets, uint32_t* __restrict__ rows,
                                                    uint32_t* __restrict__ cols) {
  constexpr int R = 1 << LOG_R, ROWS = 1 << LOG_ROWS, NB = ROWS * BPR_COLS;
  static_assert(ROWS <= BPR_ROWS && R <= ROWS && R <= BPR_COLS, "bucket grid");
  constexpr int ROW_LANES = BPR_COLS / R, COL_LANES = ROWS / R;  // threads per row / per column
  constexpr int ROWS_PER_BLOCK = 256 / ROW_LANES, COLS_PER_BLOCK = 256 / COL_LANES;
  constexpr int ROW_BLOCKS = (ROWS + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  __shared__ uint32_t x[256 * XYZZ_WORDS];
  const int w = blockIdx.y, t = threadIdx.x;
  const uint32_t* bw = buckets + (size_t)w * NB * REC_WORDS;
  const bool row_block = (int)blockIdx.x < ROW_BLOCKS;
  // element e = q - 1 = 128 * hi + lo  ->  slot (e + 1) & (NB - 1)
  int e0, estep, group, lanes_per_group, out_index;
  bool live = true;  // a block may hold more row / column groups than the grid has left (small grids)
  if (row_block) {  // R consecutive lo per thread
    group = t / ROW_LANES;
    const int row = blockIdx.x * ROWS_PER_BLOCK + group, seg = t % ROW_LANES;
    live = row < ROWS;
    e0 = row * BPR_COLS + seg * R;
    estep = 1;
    lanes_per_group = ROW_LANES;
    out_index = row;
  } else {  // R consecutive hi per thread
    group = t / COL_LANES;
    const int col = ((int)blockIdx.x - ROW_BLOCKS) * COLS_PER_BLOCK + group, part = t % COL_LANES;
    live = col < BPR_COLS;
    e0 = part * R * BPR_COLS + col;
    estep = BPR_COLS;
    lanes_per_group = COL_LANES;
    out_index = col;
  }
  g1_xyzz acc = g1_identity();
  if (live) {
    acc = ld_rec(bw + (size_t)((e0 + 1) & (NB - 1)) * REC_WORDS);
#pragma unroll 1
    for (int i = 1; i < R; i++) acc = g1_add(acc, ld_rec(bw + (size_t)((e0 + i * estep + 1) & (NB - 1)) * REC_WORDS));
  }
  st_xyzz(x + t * XYZZ_WORDS, acc);
  __syncthreads();
  const int k = t & (lanes_per_group - 1);
  for (int sft = lanes_per_group >> 1; sft >= 1; sft >>= 1) {
    if (k < sft) lds_add_pair(x, t, t + sft);
    __syncthreads();
  }
  if (k == 0 && live) {
    uint32_t* out = (row_block ? rows + (size_t)w * BPR_ROWS * XYZZ_WORDS : cols + (size_t)w * 256 * XYZZ_WORDS) + (size_t)out_index * XYZZ_WORDS;
    for (int i = 0; i < XYZZ_WORDS; i++) out[i] = x[t * XYZZ_WORDS + i];
  }
}

// ---- cooperative group operations: 8 lanes share ONE addition / doubling -------------------------------------------
// In the narrow tail of the reduction only a few additions are independent, so most lanes of a wave idle while a lone wave
// needs ~12 us per XYZZ addition (14 dependent field multiplications).  The multiplications of one addition are mostly
// independent of each other (critical path 4), so an octet of lanes computes them side by side: lane role r = lane & 7
// takes one product per stage, operands and intermediate results travel through LDS, stages are separated by block
// barriers.  An addition then costs 4 multiplication latencies + 5 barriers, a doubling 3 + 4.
// Every thread of the block must call these functions (they contain __syncthreads); octet o = threadIdx.x >> 3 works on
// its own operands `pa`, `pb` -> `pout` (LDS pointers to XYZZ_WORDS records; pout may alias pa or pb) when `active`.
constexpr int COOP_WORDS = 16 * FQ_L;  // scratch words per octet

__device__ __forceinline__ fq ldf(const uint32_t* p) {
  fq r;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void stf(uint32_t* p, const fq& a) {
#pragma unroll
  for (int i = 0; i < FQ_L; i++) p[i] = a.v[i];
}
__device__ __forceinline__ void coop_copy(uint32_t* dst, const uint32_t* src, int r) {  // 8 lanes copy one record
  if (dst != src)
    for (int i = r; i < XYZZ_WORDS; i += 8) dst[i] = src[i];
}

__device__ __noinline__ void coop_add(uint32_t* sc_all, const uint32_t* pa, const uint32_t* pb, uint32_t* pout, bool active) {
  const int r = threadIdx.x & 7;
  uint32_t* sc = sc_all + (threadIdx.x >> 3) * COOP_WORDS;
  // mode 0: full addition; 1: result = a (b is the identity); 2: result = b; 3: inactive
  int mode = 3;
  if (active) mode = pa[4 * FQ_L] != 0 ? 2 : (pb[4 * FQ_L] != 0 ? 1 : 0);
  fq keep = fq_zero();  // r0 keeps P, r1 keeps R across stages
  // stage 1: U1 = ax*bzz, U2 = bx*azz, S1 = ay*bzzz, S2 = by*azzz, ZZ12 = azz*bzz, ZZZ12 = azzz*bzzz  -> sc[0..5]
  if (mode == 0 && r < 6) {
    const uint32_t *fa, *fb;
    if (r < 4) {
      const uint32_t* first = (r & 1) ? pb : pa;
      const uint32_t* second = (r & 1) ? pa : pb;
      fa = first + ((r & 2) ? FQ_L : 0);
      fb = second + ((r & 2) ? 3 * FQ_L : 2 * FQ_L);
    } else {
      fa = pa + (r == 4 ? 2 * FQ_L : 3 * FQ_L);
      fb = pb + (r == 4 ? 2 * FQ_L : 3 * FQ_L);
    }
    stf(sc + r * FQ_L, fq_mul(ldf(fa), ldf(fb)));
  }
  __syncthreads();
  // stage 2: r0: P = U2 - U1, PP = P^2 -> sc[6] ; r1: R = S2 - S1 -> sc[9], RR = R^2 -> sc[7]
  if (mode == 0 && r < 2) {
    keep = fq_sub<3>(ldf(sc + (r == 0 ? 1 : 3) * FQ_L), ldf(sc + (r == 0 ? 0 : 2) * FQ_L));
    stf(sc + (6 + r) * FQ_L, fq_sqr(keep));
    if (r == 1) stf(sc + 9 * FQ_L, keep);
  }
  __syncthreads();
  bool special = false;  // equal x coordinates: doubling or cancellation, done serially by lane 0 at the end
  if (mode == 0) special = fq_is_zero_exact(ldf(sc + 6 * FQ_L));
  // stage 3: PPP = P*PP -> sc[10], Q = U1*PP -> sc[11], ZZ3 = ZZ12*PP -> sc[12]
  if (mode == 0 && !special && r < 3) {
    const fq PP = ldf(sc + 6 * FQ_L);
    const fq other = r == 0 ? keep : ldf(sc + (r == 1 ? 0 : 4) * FQ_L);
    stf(sc + (10 + r) * FQ_L, fq_mul(other, PP));
  }
  __syncthreads();
  // stage 4: r0: X3 = RR - PPP - 2Q -> sc[13], Y3 = R*(Q - X3) - S1*PPP -> sc[14] ; r1: ZZZ3 = ZZZ12*PPP -> sc[15]
  if (mode == 0 && !special && r < 2) {
    const fq PPP = ldf(sc + 10 * FQ_L);
    if (r == 0) {
      const fq Q = ldf(sc + 11 * FQ_L);
      const fq X3 = fq_sub<7>(ldf(sc + 7 * FQ_L), fq_add(PPP, fq_dbl(Q)));
      const fq T = fq_sub<10>(Q, X3);
      const fq nS1 = fq_sub<3>(fq_zero(), ldf(sc + 2 * FQ_L));
      stf(sc + 13 * FQ_L, X3);
      stf(sc + 14 * FQ_L, fq_mul2(ldf(sc + 9 * FQ_L), T, nS1, PPP));
    } else {
      stf(sc + 15 * FQ_L, fq_mul(ldf(sc + 5 * FQ_L), PPP));
    }
  }
  __syncthreads();
  if (mode == 0) {
    if (special) {
      if (r == 0) st_xyzz(pout, g1_add(ld_xyzz(pa), ld_xyzz(pb)));
    } else if (r < 4) {
      const int src = r == 0 ? 13 : (r == 1 ? 14 : (r == 2 ? 12 : 15));
      stf(pout + r * FQ_L, ldf(sc + src * FQ_L));
    } else if (r == 4) {
      pout[4 * FQ_L] = 0;
    }
  } else if (mode == 1) {
    coop_copy(pout, pa, r);
  } else if (mode == 2) {
    coop_copy(pout, pb, r);
  }
  __syncthreads();
}

__device__ __noinline__ void coop_double(uint32_t* sc_all, const uint32_t* pa, uint32_t* pout, bool active) {
  const int r = threadIdx.x & 7;
  uint32_t* sc = sc_all + (threadIdx.x >> 3) * COOP_WORDS;
  const bool work = active && pa[4 * FQ_L] == 0;  // doubling the identity leaves it unchanged
  fq keep = fq_zero();                      // r0 keeps U = 2Y
  // stage 1: r0: V = U^2 -> sc[0] ; r1: XX = X^2 -> sc[1]
  if (work && r < 2) {
    if (r == 0) {
      keep = fq_dbl(ldf(pa + FQ_L));
      stf(sc + 0 * FQ_L, fq_sqr(keep));
    } else {
      stf(sc + 1 * FQ_L, fq_sqr(ldf(pa)));
    }
  }
  __syncthreads();
  // stage 2: r0: W = U*V -> sc[2] ; r1: S = X*V -> sc[3] ; r2: M = 3*XX -> sc[5], MM = M^2 -> sc[4] ; r3: ZZ3 = V*ZZ -> sc[6]
  if (work && r < 4) {
    if (r == 2) {
      const fq XX = ldf(sc + 1 * FQ_L);
      const fq M = fq_norm(fq_add(fq_dbl(XX), XX));
      stf(sc + 5 * FQ_L, M);
      stf(sc + 4 * FQ_L, fq_sqr(M));
    } else {
      const fq V = ldf(sc + 0 * FQ_L);
      const fq other = r == 0 ? keep : ldf(pa + (r == 1 ? 0 : 2 * FQ_L));
      stf(sc + (r == 0 ? 2 : (r == 1 ? 3 : 6)) * FQ_L, fq_mul(other, V));
    }
  }
  __syncthreads();
  // stage 3: r0: X3 = MM - 2S -> sc[7], Y3 = M*(S - X3) - W*Y -> sc[8] ; r1: ZZZ3 = W*ZZZ -> sc[9]
  if (work && r < 2) {
    const fq W = ldf(sc + 2 * FQ_L);
    if (r == 0) {
      const fq S = ldf(sc + 3 * FQ_L);
      const fq X3 = fq_sub<5>(ldf(sc + 4 * FQ_L), fq_dbl(S));
      const fq T = fq_sub<8>(S, X3);
      const fq nY = fq_sub<6>(fq_zero(), ldf(pa + FQ_L));
      stf(sc + 7 * FQ_L, X3);
      stf(sc + 8 * FQ_L, fq_mul2(ldf(sc + 5 * FQ_L), T, nY, W));
    } else {
      stf(sc + 9 * FQ_L, fq_mul(W, ldf(pa + 3 * FQ_L)));
    }
  }
  __syncthreads();
  if (work) {
    if (r < 4) {
      const int src = r == 0 ? 7 : (r == 1 ? 8 : (r == 2 ? 6 : 9));
      stf(pout + r * FQ_L, ldf(sc + src * FQ_L));
    } else if (r == 4) {
      pout[4 * FQ_L] = 0;
    }
  } else if (active) {
    coop_copy(pout, pa, r);
  }
  __syncthreads();
}

// W(X) = sum_{i<256} i * X_i for X = rows (blockIdx.x == 0) or the columns padded to 256 with identities (blockIdx.x == 1);
// out[w][blockIdx.x] = W(X); for the columns additionally out[w][2] = sum(X).
// 16 x 16 split (RR_a = row sums, CC_b = column sums of the 16 x 16 arrangement of X): W = 16 * W16(RR) + W16(CC);
// W16(V) by a 4 x 4 split: W16 = 4 * W4(r) + W4(c); W4(u) = u1 + 2 u2 + 3 u3 = (u1 + u3) + 2 (u2 + u3).
// Levels with at most 32 independent operations use the cooperative octet operations above.
// (needs 256 records + 32 octets of scratch in LDS: 50 KB with 9 limbs; with 14 limbs it would pass the 64 KB a workgroup may declare, so
//  a unit of that size finishes its window sums from the bit-plane sums instead: k_bpr_planes<true> + k_bpr_final_planes below)
constexpr bool BPR_USE_W256 = (256 * XYZZ_WORDS + 32 * COOP_WORDS) * 4 <= 65536;
__global__ void __launch_bounds__(256) k_bpr_w256(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cols,
                                                  uint32_t* __restrict__ out, int nrows) {
  __shared__ uint32_t x[BPR_USE_W256 ? 256 * XYZZ_WORDS : 1];
  __shared__ uint32_t sc[BPR_USE_W256 ? 32 * COOP_WORDS : 1];
  if constexpr (!BPR_USE_W256) return;
  const int w = blockIdx.y, which_in = blockIdx.x, t = threadIdx.x;
  const int a = t >> 4, b = t & 15, o = t >> 3;  // o: octet index, 0..31
  auto X = [&](int i) { return x + i * XYZZ_WORDS; };
  // after the trees only records 8g of x stay live; the free ones hold the small intermediate vectors
  auto Y = [&](int j) { return x + (8 * (j >> 1) + 1 + (j & 1)) * XYZZ_WORDS; };  // j < 64
  auto Z = [&](int j) { return x + (8 * j + 3) * XYZZ_WORDS; };                   // j < 16
  auto U = [&](int j) { return x + (8 * j + 4) * XYZZ_WORDS; };                   // j < 8
  auto T = [&](int j) { return x + (8 * j + 5) * XYZZ_WORDS; };                   // j < 8 (total of the row sums)
  auto Q = [&](int j) { return x + (8 * j + 6) * XYZZ_WORDS; };                   // j < 8 (W4 temporaries)
  g1_xyzz xi;
  if (which_in == 0) xi = t < nrows ? ld_xyzz(rows + ((size_t)w * BPR_ROWS + t) * XYZZ_WORDS) : g1_identity();  // rows padded to 256
  else xi = t < BPR_COLS ? ld_xyzz(cols + ((size_t)w * 256 + t) * XYZZ_WORDS) : g1_identity();
  st_xyzz(X(t), xi);
  __syncthreads();
  // level 1 (256 additions, all lanes busy): threads with b < 8 add row pairs, the others add column pairs
  g1_xyzz l1;
  int l1_dst;
  if (b < 8) {
    l1 = g1_add(xi, ld_xyzz(X(16 * a + b + 8)));
    l1_dst = a * 8 + b;  // row partials: [0, 128)
  } else {
    const int job = a * 8 + (b - 8), c = job & 15, pr = job >> 4;
    l1 = g1_add(ld_xyzz(X(16 * pr + c)), ld_xyzz(X(16 * (pr + 8) + c)));
    l1_dst = 128 + c * 8 + pr;  // column partials: [128, 256)
  }
  __syncthreads();
  st_xyzz(X(l1_dst), l1);
  __syncthreads();
  for (int sft = 4; sft >= 2; sft >>= 1) {  // 32 groups of 8 -> 2 (128 and 64 additions)
    if (t < 32 * sft) {
      const int g = t / sft, k = t % sft;
      lds_add_pair(x, g * 8 + k, g * 8 + k + sft);
    }
    __syncthreads();
  }
  coop_add(sc, X(o * 8), X(o * 8 + 1), X(o * 8), true);  // 32 groups: 2 -> 1
  // V0[i] = X(8 i) (16 row sums RR), V1[i] = X(128 + 8 i) (16 column sums CC)
  auto V = [&](int v, int i) { return X(v * 128 + 8 * i); };
  {  // 4 x 4 split, level 1: 32 jobs -> Y(v*16 + job)
    const int v = o >> 4, job = o & 15;
    const uint32_t *pa, *pb;
    if (job < 8) {  // row pair (i, j): V[4i + j] + V[4i + j + 2]
      const int i = job >> 1, j = job & 1;
      pa = V(v, 4 * i + j);
      pb = V(v, 4 * i + j + 2);
    } else {  // column pair (j, pr): V[4 pr + j] + V[4 (pr + 2) + j]
      const int j = (job - 8) >> 1, pr = job & 1;
      pa = V(v, 4 * pr + j);
      pb = V(v, 4 * (pr + 2) + j);
    }
    coop_add(sc, pa, pb, Y(v * 16 + job), true);
  }
  {  // level 2: r_i, c_j (16 jobs) -> Z(v*8 + q) ; total of V0, level 1 (8 jobs) -> T(k)
    const uint32_t *pa = x, *pb = x;
    uint32_t* po = x;
    const bool act = o < 24;
    if (o < 16) {
      const int v = o >> 3, q = o & 7;  // q < 4: r_q ; q >= 4: c_{q-4}
      const int base = v * 16 + (q < 4 ? 2 * q : 8 + 2 * (q - 4));
      pa = Y(base);
      pb = Y(base + 1);
      po = Z(v * 8 + q);
    } else if (o < 24) {
      const int k = o - 16;
      pa = V(0, k);
      pb = V(0, k + 8);
      po = T(k);
    }
    coop_add(sc, pa, pb, po, act);
  }
  {  // W4 step A: p = u1 + u3 -> U(j), q = u2 + u3 -> Q(j) for the 4 vectors j = v*2 + which ; total 8 -> 4
    const uint32_t *pa = x, *pb = x;
    uint32_t* po = x;
    const bool act = o < 12;
    if (o < 8) {
      const int j = o >> 1;
      const uint32_t* q4 = Z(j * 4) - 0;  // u_i = Z(j*4 + i)
      (void)q4;
      pa = Z(j * 4 + ((o & 1) ? 2 : 1));
      pb = Z(j * 4 + 3);
      po = (o & 1) ? Q(j) : U(j);
    } else if (o < 12) {
      const int k = o - 8;
      pa = T(k);
      pb = T(k + 4);
      po = T(k);
    }
    coop_add(sc, pa, pb, po, act);
  }
  coop_double(sc, Q(o & 3), Q(o & 3), o < 4);  // W4 step B: q <- 2 q
  {  // W4 step C: W4 = p + 2q -> U(j) ; total 4 -> 2
    const uint32_t *pa = x, *pb = x;
    uint32_t* po = x;
    const bool act = o < 6;
    if (o < 4) {
      pa = U(o);
      pb = Q(o);
      po = U(o);
    } else if (o < 6) {
      const int k = o - 4;
      pa = T(k);
      pb = T(k + 2);
      po = T(k);
    }
    coop_add(sc, pa, pb, po, act);
  }
  // W16(v) = 4 * W4(r_v) + W4(c_v): U(2v) <- 4 U(2v), then U(4 + v) = U(2v) + U(2v + 1) ; total 2 -> 1
  coop_double(sc, U(2 * (o & 1)), U(2 * (o & 1)), o < 2);
  coop_double(sc, U(2 * (o & 1)), U(2 * (o & 1)), o < 2);
  {
    const uint32_t *pa = x, *pb = x;
    uint32_t* po = x;
    const bool act = o < 3;
    if (o < 2) {
      pa = U(2 * o);
      pb = U(2 * o + 1);
      po = U(4 + o);
    } else if (o == 2) {
      pa = T(0);
      pb = T(1);
      po = T(0);
    }
    coop_add(sc, pa, pb, po, act);
  }
  // W256 = 16 * W16(RR) + W16(CC)
  for (int i = 0; i < 4; i++) coop_double(sc, U(4), U(4), o == 0);
  coop_add(sc, U(4), U(5), U(4), o == 0);
  if (t < XYZZ_WORDS) out[((size_t)w * 3 + which_in) * XYZZ_WORDS + t] = U(4)[t];
  if (which_in == 1 && t >= 64 && t < 64 + XYZZ_WORDS) out[((size_t)w * 3 + 2) * XYZZ_WORDS + (t - 64)] = T(0)[t - 64];
}

// one lane per window: S = 128 * W(R) + W(C) + sum(C), emitted as canonical Jacobian bytes.  (Operands stay in registers
// here, which measured faster than the cooperative LDS form: 52 vs 71 us.)
// (every kernel that ends a launch's reduce chain also hands the launch's error word to the host -- err_host is the slot's pinned word, written
//  directly -- and clears it for the slot's next occupant: two copies and a fill less at the end of every chain)
__device__ __forceinline__ void finish_error_word(uint32_t* __restrict__ err_dev, uint32_t* __restrict__ err_host) {
  *err_host = *err_dev;
  *err_dev = 0;
}
// (emit_total: shares of the wide tables' virtual windows -- record 2 w is the window sum, record 2 w + 1 the window's PLAIN total
//  TC_w = sum_slot B[w][slot], which the finish needs beside it: host_g1.h, combine_wide_pairs)
__global__ void __launch_bounds__(64) k_bpr_final(const uint32_t* __restrict__ parts, int w_count, uint32_t* __restrict__ wsums,
                                                  uint32_t* __restrict__ big_queue, uint32_t* __restrict__ err_dev, uint32_t* __restrict__ err_host,
                                                  int emit_total) {
  const int w = threadIdx.x;
  if (w == 0) {
    big_queue[0] = 0;  // the stitch's queue of big buckets, consumed earlier on this stream: empty for the next launch
    finish_error_word(err_dev, err_host);
  }
  if (w >= w_count) return;
  g1_xyzz acc = ld_xyzz(parts + ((size_t)w * 3 + 0) * XYZZ_WORDS);
  for (int i = 0; i < 7; i++) acc = g1_double(acc);
  const g1_xyzz total = ld_xyzz(parts + ((size_t)w * 3 + 2) * XYZZ_WORDS);
  acc = g1_add(acc, g1_add(ld_xyzz(parts + ((size_t)w * 3 + 1) * XYZZ_WORDS), total));
  st_jacobian_plain(wsums + (size_t)(emit_total ? 2 * w : w) * JAC_WORDS, acc);
  if (emit_total) st_jacobian_plain(wsums + (size_t)(2 * w + 1) * JAC_WORDS, total);
}

// ... or, for a launch whose sums go to the host anyway (one MSM per launch: its LATENCY is what counts): the narrow end of the reduction
// is not done here at all.  W(X) = sum_i i X_i = sum_b 2^b P_b with the PLAIN bit-plane sums P_b = sum_{i: bit b of i set} X_i -- eight
// (rows) + seven (columns) + the column total = PLANES_PER_WINDOW masked tree sums per window, all independent and 8 additions deep,
// instead of k_bpr_w256's ~16 dependent levels and k_bpr_final's 9 operations in a lone wave (~200 us together); the positional
// combination S_w = sum_b 2^(b+7) PR_b + sum_b 2^b PC_b + TC is 29 group operations per window on the host (host_g1.h:
// window_sum_from_planes, ~8 us; the windows side by side on the host pool).
// Grid (PLANES_PER_WINDOW, windows); plane 0 .. 7: row bit b, 8 .. 14: column bit b - 8, 15: column total.  out[w][plane] x 96 B Jacobian.
// XYZZ_OUT: the plane sums stay on the device as XYZZ records (k_bpr_final_planes finishes the window sums there).
template <bool XYZZ_OUT>
__global__ void __launch_bounds__(256) k_bpr_planes(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cols, uint32_t* __restrict__ out,
                                                    int nrows, uint32_t* __restrict__ big_queue, uint32_t* __restrict__ err_dev,
                                                    uint32_t* __restrict__ err_host) {
  __shared__ uint32_t x[256 * XYZZ_WORDS];
  const int w = blockIdx.y, plane = blockIdx.x, t = threadIdx.x;
  if (!XYZZ_OUT && w == 0 && plane == 0 && t == 0) {  // as k_bpr_final: this kernel ends the chain (`out` may be the slot's pinned host buffer itself)
    big_queue[0] = 0;
    finish_error_word(err_dev, err_host);
  }
  const bool is_row = plane < 8;
  const int bit = is_row ? plane : plane - 8;  // 7 for the column total: bit 7 of a column index is never set -> handled by `all`
  const bool all = plane == PLANES_PER_WINDOW - 1;
  const int count = is_row ? nrows : BPR_COLS;
  const bool take = t < count && (all || ((t >> bit) & 1));
  const uint32_t* src = is_row ? rows + ((size_t)w * BPR_ROWS + t) * XYZZ_WORDS : cols + ((size_t)w * 256 + t) * XYZZ_WORDS;
  // first level straight from memory: thread t < 128 adds elements t and t + 128 (both masked)
  g1_xyzz acc = g1_identity();
  if (t < 128) {
    if (take) acc = ld_xyzz(src);
    const int u = t + 128;
    if (u < count && (all || ((u >> bit) & 1))) acc = g1_add(acc, ld_xyzz(src + (size_t)128 * XYZZ_WORDS));
    st_xyzz(x + t * XYZZ_WORDS, acc);
  }
  __syncthreads();
  for (int sft = 64; sft >= 1; sft >>= 1) {
    if (t < sft) lds_add_pair(x, t, t + sft);
    __syncthreads();
  }
  if constexpr (XYZZ_OUT) {
    if (t < XYZZ_WORDS) out[((size_t)w * PLANES_PER_WINDOW + plane) * XYZZ_WORDS + t] = x[t];
  } else {
    if (t == 0) st_jacobian_plain(out + ((size_t)w * PLANES_PER_WINDOW + plane) * JAC_WORDS, ld_xyzz(x));
  }
}
// one lane per window: S_w = sum_b 2^(b+7) PR_b + sum_b 2^b PC_b + TC from the plane sums (XYZZ records), as canonical Jacobian bytes --
// the device-side counterpart of host_g1.h: window_sum_from_planes, for sums that stay on the device
__global__ void __launch_bounds__(64) k_bpr_final_planes(const uint32_t* __restrict__ planes, int w_count, uint32_t* __restrict__ wsums,
                                                         uint32_t* __restrict__ big_queue, uint32_t* __restrict__ err_dev, uint32_t* __restrict__ err_host,
                                                         int emit_total) {
  const int w = threadIdx.x;
  if (w == 0) {
    big_queue[0] = 0;
    finish_error_word(err_dev, err_host);
  }
  if (w >= w_count) return;
  const uint32_t* pw = planes + (size_t)w * PLANES_PER_WINDOW * XYZZ_WORDS;
  g1_xyzz acc = g1_identity();
#pragma unroll 1
  for (int pos = 14; pos >= 0; pos--) {
    acc = g1_double(acc);
    acc = g1_add(acc, ld_xyzz(pw + (size_t)(pos >= 7 ? pos - 7 : 8 + pos) * XYZZ_WORDS));
  }
  const g1_xyzz total = ld_xyzz(pw + (size_t)(PLANES_PER_WINDOW - 1) * XYZZ_WORDS);
  acc = g1_add(acc, total);
  st_jacobian_plain(wsums + (size_t)(emit_total ? 2 * w : w) * JAC_WORDS, acc);
  if (emit_total) st_jacobian_plain(wsums + (size_t)(2 * w + 1) * JAC_WORDS, total);
}

// bucket records -> Jacobian wire records (stage read-back for the parity tests)
__global__ void __launch_bounds__(256) k_export_buckets(const uint32_t* __restrict__ buckets, uint32_t* __restrict__ out, size_t count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  st_jacobian_plain(out + i * JAC_WORDS, ld_rec(buckets + i * REC_WORDS));
}

// ------------------------------------------------------------------------------------------------ samplers
// deterministic synthetic inputs (≙ sample_scalars / sample_points, src/lib.rs:20-42, but seeded)
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// NW 32-bit words (8: a scalar or a coordinate of the 254 / 255-bit fields, masked to 254 bits; 12: a BLS12-381 coordinate, 381 bits)
template <int NW>
__device__ __forceinline__ void draw_words(uint64_t seed, uint64_t index, uint64_t attempt, uint64_t domain, uint32_t w[NW]) {
  uint64_t base = splitmix64(seed ^ ((domain & 0xFF) << 56)) ^ (index * 0xD1342543DE82EF95ull);
  base = splitmix64(base ^ (attempt * 0xA0761D6478BD642Full));
  uint64_t s = base;
#pragma unroll
  for (int i = 0; i < NW / 2; i++) {
    s = splitmix64(s);
    w[2 * i] = (uint32_t)s;
    w[2 * i + 1] = (uint32_t)(s >> 32);
  }
  if constexpr (NW == 8) w[7] &= 0x3FFFFFFFu;        // 254 bits
  else w[NW - 1] &= (1u << (FQ_BITS - 32 * (NW - 1))) - 1u;  // as many bits as p has
}
__device__ __forceinline__ void draw256(uint64_t seed, uint64_t index, uint64_t attempt, uint64_t domain, uint32_t w[8]) {
  draw_words<8>(seed, index, attempt, domain, w);
}

__global__ void __launch_bounds__(256) k_sample_scalars(uint64_t seed, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (uint64_t attempt = 0;; attempt++) {
    draw256(seed, i, attempt, 1, w);
    if (!geq_modulus<1>(w)) break;
  }
  st8(out + i * 8, w);
}

#ifndef MSM_FQ2
__device__ __constant__ cwords<CW> c_sqrt_t = make_cwords(FQ_SQRT_T_32);
__device__ __constant__ cwords<CW> c_sqrt_tp1h = make_cwords(FQ_SQRT_TP1H_32);
__device__ __forceinline__ fq fq_pow254(const fq& a, const uint32_t* e) {  // a^e, e < 2^(32 CW - 2) (constant memory), a exact
  fq acc = fq_one();
  for (int bit = 32 * CW - 3; bit >= 0; bit--) {
    acc = fq_sqr(acc);
    if ((e[bit >> 5] >> (bit & 31)) & 1u) acc = fq_mul(acc, a);
  }
  return acc;
}
// a candidate square root of a (the caller checks y^2 == a).  p = 3 mod 4 (BN254 Fq): a^((p+1)/4).  Otherwise (Grumpkin's base
// field, p - 1 = 2^28 t): Tonelli-Shanks with every loop bounded by the 2-adicity, so a non-residue just yields a wrong candidate.
__device__ __forceinline__ fq fq_sqrt_candidate(const fq& a) {  // a exact
  if constexpr (FQ_SQRT_S == 0) {
    return fq_pow254(a, c_pp1d4.w);
  } else {
    fq x = fq_pow254(a, c_sqrt_tp1h.w), b = fq_pow254(a, c_sqrt_t.w), c;
#pragma unroll
    for (int i = 0; i < FQ_L; i++) c.v[i] = FQ_SQRT_C0_29[i];
    const fq one = fq_canonical(fq_one());
    int m = FQ_SQRT_S;
    for (int round = 0; round < FQ_SQRT_S; round++) {
      if (fq_equal_exact(fq_canonical(b), one)) break;
      int i = 0;  // least i with b^(2^i) == 1
      fq q = b;
      while (i < m && !fq_equal_exact(fq_canonical(q), one)) {
        q = fq_sqr(q);
        i++;
      }
      if (i >= m) break;  // not a square
      fq bb = c;
      for (int k = 0; k < m - i - 1; k++) bb = fq_sqr(bb);
      x = fq_mul(x, bb);
      c = fq_sqr(bb);
      b = fq_mul(b, c);
      m = i;
    }
    return x;
  }
}

__global__ void __launch_bounds__(256) k_sample_points(uint64_t seed, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wx[CW];
  for (uint64_t attempt = 0;; attempt++) {
    draw_words<CW>(seed, i, attempt, 2, wx);
    if (geq_modulus<0>(wx)) continue;
    const fq x = fq_to_mont(fq_unpack(wx));
    const fq rhs = fq_canonical(fq_tidy(fq_add(fq_mul(fq_sqr(x), x), fq_curve_b())));
    const fq y = fq_sqrt_candidate(rhs);
    if (!fq_equal_exact(fq_canonical(fq_sqr(y)), rhs)) continue;
    fq yp = fq_from_mont(y);  // canonical integer
    if ((yp.v[0] & 1u) != ((wx[0] >> 1) & 1u)) yp = fq_neg_canonical(yp);
    st_coord(out + i * PT_WORDS, wx);
    st_fq(out + i * PT_WORDS + CW, yp);
    break;
  }
}
#else  // MSM_FQ2
// G2: P_i = (a + i b) G for seeded odd a, b < r and the standard generator G of the order-r subgroup -- byte for byte what the oracle's
// sample_points(n, seed) produces (oracle/bn254_g2_ref.py; its sample_multipliers gives every MSM over these points a closed form).  Points
// of G2 proper, unlike try-and-increment on the twist (whose cofactor is huge): fit for the endomorphism mode.  One lane per point: a
// double-and-add over the 288-bit integer a + i b (not reduced: G has order r), then one inversion in Fq2.
__global__ void __launch_bounds__(256) k_sample_points(uint64_t seed, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t ab[2][8];
  for (int which = 0; which < 2; which++) {  // a, b = sample_scalar(seed ^ 0x6732, 0 / 1) | 1
    for (uint64_t attempt = 0;; attempt++) {
      draw256(seed ^ 0x6732ull, (uint64_t)which, attempt, 1, ab[which]);
      if (!geq_modulus<1>(ab[which])) break;
    }
    ab[which][0] |= 1u;
  }
  uint32_t m[10];  // a + i b < 2^254 + 2^28 2^254
  {
    const uint64_t lo = (uint32_t)i, hi = (uint64_t)i >> 32;  // (i < 2^28: hi = 0; kept general)
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < 10; k++) {
      uint64_t t = c + (k < 8 ? ab[0][k] : 0u);
      uint64_t carry = t >> 32;
      t &= 0xffffffffull;
      if (k < 8) {
        const uint64_t p0 = lo * ab[1][k];
        t += p0 & 0xffffffffull;
        carry += p0 >> 32;
      }
      if (k >= 1 && k < 9) {
        const uint64_t p1 = hi * ab[1][k - 1];
        t += p1 & 0xffffffffull;
        carry += p1 >> 32;
      }
      m[k] = (uint32_t)t;
      c = carry + (t >> 32);
    }
  }
  fq gx, gy;
#pragma unroll
  for (int k = 0; k < FQ_L; k++) {
    gx.v[k] = FQ_GEN_X29[k];
    gy.v[k] = FQ_GEN_Y29[k];
  }
  const g1_xyzz g = g1_from_affine(gx, gy);
  g1_xyzz acc = g1_identity();
#pragma unroll 1
  for (int bit = 32 * 10 - 1; bit >= 0; bit--) {
    acc = g1_double(acc);
    if ((m[bit >> 5] >> (bit & 31)) & 1u) acc = g1_add(acc, g);
  }
  // a + i b is not a multiple of r for the sizes that fit a context (a, b odd, i < 2^28): acc is a point
  const fq t = fq_inv(fq_mul(acc.zz, acc.zzz));
  st_fq(out + i * PT_WORDS, fq_from_mont(fq_mul(acc.x, fq_mul(t, acc.zzz))));
  st_fq(out + i * PT_WORDS + CW, fq_from_mont(fq_mul(acc.y, fq_mul(t, acc.zz))));
}
#endif  // MSM_FQ2

// ------------------------------------------------------------------------------------------------ op hooks for tests
// (≙ src/cuzk/wgsl/test/test_field.wgsl:13-62, test_point.wgsl:18-88)
__global__ void __launch_bounds__(256) k_test_fq(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                 uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const fq x = fq_to_mont(ld_fq(a + i * CW));
  const fq y = b ? fq_to_mont(ld_fq(b + i * CW)) : fq_zero();
  fq z;
  switch (op) {
    case 0: z = fq_add(x, y); break;
    case 1: z = fq_sub<2>(x, y); break;
    case 2: z = fq_mul(x, y); break;
    case 3: z = fq_sqr(x); break;
    case 4: z = fq_neg_canonical(x); break;
    // the SMVP's multipliers (inline assembly on the device, fq29_asm.h), called directly; 8 and 9 feed them lazy limbs
    case 5: z = fq_mul_fast(x, y); break;
    case 6: z = fq_sqr_fast(x); break;
    case 7: z = fq_mul2_fast(x, y, y, x); break;                    // x y + y x
    case 8: z = fq_mul_fast(fq_add(x, y), fq_dbl(x)); break;        // (x + y) * 2x, limbs up to 2^30
    default: z = fq_sqr_fast(fq_add(x, y)); break;                  // (x + y)^2
  }
  st_fq(out + i * CW, fq_from_mont(z));
}

__global__ void __launch_bounds__(256) k_test_g1(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                 uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1_xyzz p = ld_jacobian_plain(a + i * JAC_WORDS);
  g1_xyzz r;
  if (op == 0) {
    r = g1_add(p, ld_jacobian_plain(b + i * JAC_WORDS));
  } else if (op == 1) {
    r = g1_double(p);
  } else if (op == 2) {
    const fq qx = fq_to_mont(ld_fq(b + i * PT_WORDS)), qy = fq_to_mont(ld_fq(b + i * PT_WORDS + CW));
    g1_madd(p, qx, qy);
    r = p;
  } else {  // the SMVP's signed-state form (g1_madd_w): 3: p + q - q + q ; 4: p - q - q  (every sign state, both digit signs)
    const fq qx = fq_to_mont(ld_fq(b + i * PT_WORDS)), qy = fq_to_mont(ld_fq(b + i * PT_WORDS + CW));
    bool wneg = false;
    if (op == 3) {
      g1_madd_w(p, wneg, qx, qy, false);
      g1_madd_w(p, wneg, qx, qy, true);
      g1_madd_w(p, wneg, qx, qy, false);
    } else {
      g1_madd_w(p, wneg, qx, qy, true);
      g1_madd_w(p, wneg, qx, qy, true);
    }
    r = g1_unsigned(p, wneg);
  }
  st_jacobian_plain(out + i * JAC_WORDS, r);
}

__global__ void __launch_bounds__(256) k_test_g1_mul_u32(const uint32_t* __restrict__ a, const uint32_t* __restrict__ k,
                                                         uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_jacobian_plain(out + i * JAC_WORDS, g1_mul_u32(ld_jacobian_plain(a + i * JAC_WORDS), k[i]));
}

// ------------------------------------------------------------------------------------------------ the unit's table
// What the host code reaches of this unit (curve_ops.h), every entry assigned by name.  A G2 unit offers no group FFT: its entries stay null.
static CurveOps curve_ops_table() {
  CurveOps o{};
  o.convert_points = k_convert_points;
  o.convert_points_zero_id = k_convert_points_zero_id;
  o.precompute_tables = k_precompute_tables;
  o.endo_points = k_endo_points;
  o.mul_each[0] = k_mul_each<false>;
  o.mul_each[1] = k_mul_each<true>;
  o.mul_normalize = k_mul_normalize;
  o.mul_chunk = SMUL_CHUNK;
  o.mul_table_scalars = k_mul_table_scalars;
  o.mul_fixed = k_mul_fixed;
  o.r_bits = SMUL_R_BITS;
  o.count_split[0] = k_count<12, 4, glv_split_fn>;
  o.count_split[1] = k_count<14, 4, glv_split_fn>;
  o.count_split[2] = k_count<16, 4, glv_split_fn>;
  o.count_split_sparse[0] = k_count<12, 4, glv_split_fn, 0, SparseIdx>;
  o.count_split_sparse[1] = k_count<14, 4, glv_split_fn, 0, SparseIdx>;
  o.count_split_sparse[2] = k_count<16, 4, glv_split_fn, 0, SparseIdx>;
  o.scalars_from_mont256 = k_scalars_from_mont256;
  o.smvp_chunks = k_smvp_chunks;
  o.smvp_stitch = k_smvp_stitch;
  o.smvp_stitch_big = k_smvp_stitch_big;
  o.rowcol_4_8 = k_bpr_rowcol<4, 8>;
  o.rowcol_2_8 = k_bpr_rowcol<2, 8>;
  o.rowcol_3_8 = k_bpr_rowcol<3, 8>;
  o.rowcol_4_6 = k_bpr_rowcol<4, 6>;
  o.rowcol_2_6 = k_bpr_rowcol<2, 6>;
  o.rowcol_2_4 = k_bpr_rowcol<2, 4>;
  o.bpr_w256 = k_bpr_w256;
  o.bpr_final = k_bpr_final;
  o.bpr_planes = k_bpr_planes<false>;
  o.bpr_planes_xyzz = k_bpr_planes<true>;
  o.bpr_final_planes = k_bpr_final_planes;
  o.use_w256 = BPR_USE_W256;
  o.coord_words = CW;
  o.rec_words = REC_WORDS;
  o.xyzz_words = XYZZ_WORDS;
  o.glv = GLV_SUPPORTED;
  o.sample_scalars = k_sample_scalars;
  o.sample_points = k_sample_points;
  o.export_buckets = k_export_buckets;
  o.test_fq = k_test_fq;
  o.test_g1 = k_test_g1;
  o.test_g1_mul_u32 = k_test_g1_mul_u32;
  o.combine_windows = host::combine_windows;
  o.window_from_planes = host::window_from_planes;
  o.combine_wide = host::combine_wide;
  o.combine_wide_pairs = host::combine_wide_pairs;
  o.to_affine64 = host::to_affine64;
#ifndef MSM_FQ2
  o.fft_stage[0] = k_fft_stage<0>;
  o.fft_stage[1] = k_fft_stage<1>;
  o.fft_stage[2] = k_fft_stage<2>;
  o.fft_normalize = k_fft_normalize;
  o.fft_scale[0] = k_fft_scale<1>;
  o.fft_scale[1] = k_fft_scale<2>;
#endif
  o.fr_r = FR_R32;
  return o;
}
}  // namespace MSM_KERNEL_NS
