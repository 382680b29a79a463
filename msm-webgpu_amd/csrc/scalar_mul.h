// Batch scalar multiplication, the per-lane arithmetic: Q = k P for one (scalar, base) pair, and the shared-inversion normalisation of a
// batch of results (msm_hip_mul_each / msm_hip_mul_base; kernels: msm_kernels.h, k_mul_each and k_mul_normalize).
//
// Endomorphism ladder (smul_endo).  k = k1 + k2 lambda (csrc/glv.h: |k1|, |k2| < 2^127, signs s1, s2), so k P = |k1| T1 + |k2| T2 with
// T1 = s1 P and T2 = s2 phi(P) = (beta x, s2 y): one joint (Shamir) double-and-add ladder over 127 bits with the table {T1, T2, T1 + T2}.
// T3 = T1 + T2 comes out of one mixed addition in XYZZ form (X3, Y3, ZZ, ZZZ).  Instead of an inversion to make it affine, the whole ladder
// moves to the isomorphic curve y^2 = x^3 + b ZZ^3 under (x, y) -> (x ZZ, y ZZZ): there T3 = (X3, Y3) IS affine, T1 and T2 cost two
// products each, and the group formulas of g1.h (a = 0: none of them reads b) run unchanged, so every step of the ladder is one doubling and
// at most one MIXED addition whichever way the signs fall.  The result comes back by multiplying its ZZ, ZZZ with the isomorphism's.
// Counted from g1.h: 127 (9 + 10 * 3 / 4) + ~30 for the table ~ 2.1 k field multiplications per product; a wave issues the addition in every
// step (some lane needs it), 127 * 19 ~ 2.4 k.
//
// Plain ladder (smul_plain): one step per bit of r (256 for the table build's integer scalars) over the table {P} -- k P as the integer multiple, for any point of the curve (the library's
// convention for base sets of a curve with a cofactor, where phi(P) = lambda P holds only on the subgroup of order r).  Leading zero bits
// double the identity, which g1_double returns at once.
//
// The accumulator meets every special case through the branches of g1_madd: acc = +-T (k1 = +-k2 steps, bases of small order) and the identity.
//
// Normalisation (smul_norm_forward / smul_norm_backward).  A result leaves the ladder as a Jacobian record (X', Y', Z) = (X ZZ, Y ZZZ, ZZ),
// x = X' / Z^2, y = Y' / Z^3, Z = 0 for the identity.  SMUL_CHUNK results share ONE field inversion (Montgomery's trick): the forward pass
// stores the running product of the nonzero Z of a chunk behind every element, the caller inverts the chunk's product, the backward pass peels
// one inverse per element off it.  Identities contribute the factor 1 and are written as all-zero records (the MSM_HIP_BASES_ZERO_IS_IDENTITY
// encoding).  Per result: 1 product forward, 8 backward (two of them the conversions out of Montgomery form), and 1 / SMUL_CHUNK of an inversion.
// A chunk is the elements first, first + stride, ... below `end`: with stride = the workgroup size, consecutive lanes touch consecutive records.
//
// Host + device code: tests/host_harness/scalar_mul_harness.cpp builds it with g++ -DFQ_CHECK (every limb bound asserted) against the oracle.
#ifndef MSM_CURVE_UNIT
#pragma once
#include "g1.h"
#include "glv.h"
#endif
#include <cstddef>
#include <cstdint>

// In a unit that asks for calls instead of inlined group operations (MSM_G1_OUTLINE: BLS12-381 G2, csrc/g1.h) the ladders' mixed addition and
// their few field products are calls too: the kernel then stays far below the reach of a short branch (no expanded long branches for the
// code-generation gate to examine, tools/check_long_branch_hazard.py) and the unit's compile time stays where it was.
#if defined(MSM_G1_OUTLINE) && defined(__HIPCC__)
#define SMUL_HD __host__ __device__ __noinline__
#else
#define SMUL_HD FQ_HD
#endif

namespace MSM_FIELD_NS {

SMUL_HD void smul_madd(g1_xyzz& a, const fq& px, const fq& py) { g1_madd(a, px, py); }
SMUL_HD fq smul_mul(const fq& a, const fq& b) { return fq_mul(a, b); }

constexpr int SMUL_CHUNK = 16;        // results that share one inversion
constexpr int SMUL_HALF_BITS = 127;   // steps of the endomorphism ladder (glv.h: |k1|, |k2| < 2^127)
constexpr int SMUL_FULL_BITS = 256;   // steps of the plain ladder for any 32-byte scalar (the table build); SMUL_R_BITS for a scalar below r
constexpr int smul_r_bits() {
  int b = 256;
  while (b > 0 && !((FR_R32[(b - 1) >> 5] >> ((b - 1) & 31)) & 1u)) b--;
  return b;
}
constexpr int SMUL_R_BITS = smul_r_bits();  // bit length of r: 254 (BN254, Grumpkin) or 255
constexpr int SMUL_FIXED_MIN_BITS = 4, SMUL_FIXED_MAX_BITS = 16;  // digit widths of the fixed-base table (smul_table_scalar: why not below 4)

FQ_HD uint32_t smul_bit(const uint32_t* k, int bit) { return (k[bit >> 5] >> (bit & 31)) & 1u; }

// k >= r ?  (8 words each)
FQ_HD bool smul_geq_r(const uint32_t k[8]) {
  bool gt = false, lt = false;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    gt = gt || (!lt && k[i] > FR_R32[i]);
    lt = lt || (!gt && k[i] < FR_R32[i]);
  }
  return !lt;
}

// packed words <-> limbs (no domain change; x exact and below 2^(32 FQ_WORDS) for the store)
FQ_HD fq smul_ld(const uint32_t* p) {
  uint32_t w[FQ_WORDS];
#pragma unroll
  for (int i = 0; i < FQ_WORDS; i++) w[i] = p[i];
  return fq_unpack(w);
}
FQ_HD void smul_st(uint32_t* p, const fq& x) {
  uint32_t w[FQ_WORDS];
  fq_pack(w, x);
#pragma unroll
  for (int i = 0; i < FQ_WORDS; i++) p[i] = w[i];
}
FQ_HD bool smul_all_zero(const fq& x) {
  uint32_t z = 0;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) z |= x.v[i];
  return z == 0;
}

// k (px, py) for any 32-byte k: the integer multiple.  (px, py) Montgomery, canonical.
FQ_HD g1_xyzz smul_plain(const fq& px, const fq& py, const uint32_t k[8], int nbits = SMUL_FULL_BITS) {  // k < 2^nbits
  g1_xyzz acc = g1_identity();
#pragma unroll 1
  for (int bit = nbits - 1; bit >= 0; bit--) {
    acc = g1_double(acc);
    if (smul_bit(k, bit)) smul_madd(acc, px, py);
  }
  return acc;
}

// k (px, py) for a point of order r, through the endomorphism.  (px, py) Montgomery, canonical; any 32-byte k (the split reduces it mod r).
FQ_HD g1_xyzz smul_endo(const fq& px, const fq& py, const uint32_t k[8]) {
  uint32_t h1[4], h2[4];
  glv_split(k, h1, h2);
  const bool s1 = (h1[3] >> 31) != 0, s2 = (h2[3] >> 31) != 0;
  h1[3] &= 0x7fffffffu;
  h2[3] &= 0x7fffffffu;
  fq beta;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) beta.v[i] = FQ_BETA29[i];
  const fq x2 = fq_canonical(smul_mul(px, beta));
  const fq ny = fq_neg_canonical(py);
  fq y1, y2;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) {
    y1.v[i] = s1 ? ny.v[i] : py.v[i];
    y2.v[i] = s2 ? ny.v[i] : py.v[i];
  }
  // T3 = T1 + T2 in XYZZ; the isomorphism (x, y) -> (x ZZ, y ZZZ) makes it affine
  g1_xyzz t3 = g1_from_affine(px, y1);
  smul_madd(t3, x2, y2);
  const bool inf3 = t3.inf;  // T1 = -T2: only for a base outside the subgroup of order r; the entry is then never added
  if (inf3) {
    t3.zz = fq_one();
    t3.zzz = fq_one();
  }
  const fq t1x = smul_mul(px, t3.zz), t1y = smul_mul(y1, t3.zzz);  // exact, < 2p: operands of g1_madd like the resident bases
  const fq t2x = smul_mul(x2, t3.zz), t2y = smul_mul(y2, t3.zzz);
  const fq t3x = fq_tidy(t3.x), t3y = fq_tidy(t3.y);

  g1_xyzz acc = g1_identity();
#pragma unroll 1
  for (int bit = SMUL_HALF_BITS - 1; bit >= 0; bit--) {
    acc = g1_double(acc);
    const uint32_t b1 = smul_bit(h1, bit), b2 = smul_bit(h2, bit);
    if ((b1 | b2) != 0u && !(inf3 && (b1 & b2) != 0u)) {
      fq tx, ty;
#pragma unroll
      for (int i = 0; i < FQ_L; i++) {
        tx.v[i] = b1 ? (b2 ? t3x.v[i] : t1x.v[i]) : t2x.v[i];
        ty.v[i] = b1 ? (b2 ? t3y.v[i] : t1y.v[i]) : t2y.v[i];
      }
      smul_madd(acc, tx, ty);
    }
  }
  if (!acc.inf) {  // back from the isomorphic curve
    acc.zz = smul_mul(acc.zz, t3.zz);
    acc.zzz = smul_mul(acc.zzz, t3.zzz);
  }
  return acc;
}

// ---- fixed base: k P from a table of multiples, no doublings
// T_w[j] = j 2^(C w) P for j = 1 .. 2^(C-1) and w < W = (SMUL_R_BITS + 1 + C) / C windows, record (w << (C - 1)) + j - 1 of `table`: packed Montgomery
// affine records like the resident bases, an all-zero record for a multiple that is the identity (a base of small order).  k < r is recoded into
// W signed C-bit digits d_w in [-2^(C-1), 2^(C-1)) with the bias trick of the MSM's recode (recode.h, bias_scalar): digit w of k + bias,
// bias = sum_w 2^(C w + C - 1), is d_w + 2^(C-1), and C W >= SMUL_R_BITS + 2 keeps k + bias below 2^(C W) for every C: no carry is lost.  k P = sum_w d_w 2^(C w) P: W gathered
// mixed additions (10 products each).
FQ_HD int smul_fixed_windows(int c) { return (SMUL_R_BITS + 1 + c) / c; }
// the scalar of table entry (w, j), j 2^(C w), as 8 words; 0 where it does not fit 256 bits.  That happens only in a top window at bit 256 (r of 255 bits), whose digit is nonzero only if
// k + (the bias below bit 256, < 2^255 / (1 - 2^-C)) reaches 2^256: k > 0.934 2^255 at C = 4, more for wider digits -- above every supported r
// (BLS12-381: 0.906 2^255).  At C < 4 it could be reached: SMUL_FIXED_MIN_BITS.
FQ_HD void smul_table_scalar(int c, int w, uint32_t j, uint32_t k[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = 0;
  const int bit = c * w;
  if (bit + 32 - __builtin_clz(j) > 256) return;
  const uint64_t v = (uint64_t)j << (bit & 31);
  k[bit >> 5] = (uint32_t)v;
  if ((bit >> 5) + 1 < 8) k[(bit >> 5) + 1] = (uint32_t)(v >> 32);
}
FQ_HD g1_xyzz smul_fixed(const uint32_t* table, int c, const uint32_t k[8]) {
  const int W = smul_fixed_windows(c);
  uint32_t t[10];
  {  // t = k + bias
    uint32_t bias[10];
#pragma unroll
    for (int i = 0; i < 10; i++) bias[i] = 0;
    for (int w = 0; w < W; w++) {
      const int b = c * w + c - 1;
      bias[b >> 5] |= 1u << (b & 31);
    }
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      carry += (uint64_t)(i < 8 ? k[i] : 0u) + bias[i];
      t[i] = (uint32_t)carry;
      carry >>= 32;
    }
  }
  g1_xyzz acc = g1_identity();
  const int32_t half = 1 << (c - 1);
#pragma unroll 1
  for (int w = 0; w < W; w++) {
    const int bit = c * w;
    const uint64_t two = (uint64_t)t[bit >> 5] | ((uint64_t)t[(bit >> 5) + 1] << 32);
    const int32_t d = (int32_t)((uint32_t)(two >> (bit & 31)) & ((1u << c) - 1u)) - half;
    if (d == 0) continue;
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    const uint32_t* rec = table + (((size_t)w << (c - 1)) + mag - 1) * 2 * FQ_WORDS;
    const fq px = smul_ld(rec), py = smul_ld(rec + FQ_WORDS);
    if (smul_all_zero(px) && smul_all_zero(py)) continue;  // the identity
    const fq ny = fq_neg_canonical(py);
    fq ty;
#pragma unroll
    for (int i = 0; i < FQ_L; i++) ty.v[i] = d < 0 ? ny.v[i] : py.v[i];
    smul_madd(acc, px, ty);
  }
  return acc;
}

// One result into the batch's arrays: record i of `xy` gets X' || Y' (Montgomery, canonical), z[i] gets Z (0 for the identity)
FQ_HD void smul_store_jacobian(uint32_t* xy, uint32_t* z, size_t i, const g1_xyzz& a) {
  fq X, Y, Z;
  g1_to_jacobian(a, X, Y, Z);
  smul_st(xy + i * 2 * FQ_WORDS, X);
  smul_st(xy + i * 2 * FQ_WORDS + FQ_WORDS, Y);
  smul_st(z + i * FQ_WORDS, Z);
}

// Forward pass over one chunk: prefix[i] = product of the nonzero z of the chunk up to and including element i (exact, < 2p).
// Returns the chunk's product (1 if every element is the identity): the caller inverts it.
FQ_HD fq smul_norm_forward(const uint32_t* z, uint32_t* prefix, size_t first, size_t stride, size_t end) {
  fq acc = fq_one();
#pragma unroll 1
  for (int j = 0; j < SMUL_CHUNK; j++) {
    const size_t i = first + (size_t)j * stride;
    if (i >= end) break;
    const fq zj = smul_ld(z + i * FQ_WORDS);
    if (!smul_all_zero(zj)) acc = fq_mul(acc, zj);
    smul_st(prefix + i * FQ_WORDS, acc);
  }
  return acc;
}

// Backward pass: `inv` = 1 / (the chunk's product).  Record i of `xy` (X' || Y') becomes the affine point x || y as canonical integers,
// or the all-zero record for the identity.  MONT (the stages of msm_hip_bases_fft): x || y stay in Montgomery form, canonical -- a packed record
// like the resident bases, the identity still the all-zero record -- and the two conversions are saved: 6 products backward.
template <bool MONT = false>
FQ_HD void smul_norm_backward(uint32_t* xy, const uint32_t* z, const uint32_t* prefix, size_t first, size_t stride, size_t end, fq inv) {
  int count = 0;
  while (count < SMUL_CHUNK && first + (size_t)count * stride < end) count++;
#pragma unroll 1
  for (int j = count - 1; j >= 0; j--) {
    const size_t i = first + (size_t)j * stride;
    uint32_t* rec = xy + i * 2 * FQ_WORDS;
    const fq zj = smul_ld(z + i * FQ_WORDS);
    if (smul_all_zero(zj)) {
#pragma unroll
      for (int w = 0; w < 2 * FQ_WORDS; w++) rec[w] = 0u;
      continue;
    }
    const fq zi = j > 0 ? fq_mul(inv, smul_ld(prefix + (i - stride) * FQ_WORDS)) : inv;  // 1 / z_j
    inv = fq_mul(inv, zj);
    const fq zi2 = fq_sqr(zi);
    const fq zi3 = fq_mul(zi2, zi);
    const fq x = fq_mul(smul_ld(rec), zi2), y = fq_mul(smul_ld(rec + FQ_WORDS), zi3);
    smul_st(rec, MONT ? fq_canonical(x) : fq_from_mont(x));
    smul_st(rec + FQ_WORDS, MONT ? fq_canonical(y) : fq_from_mont(y));
  }
}

// ---- the butterfly of the group FFT over the resident bases (msm_hip_bases_fft; kernels: msm_kernels.h, k_fft_stage)
// Operands are packed Montgomery affine records (x || y, canonical) in which the ALL-ZERO record is the identity ((0, 0) is on none of the curves);
// `*_identity` marks an operand as the identity whatever its record holds (a resident base flagged in the identity bitmap).
// LADDER: 0 none (the twiddle is 1: the first stage), 1 smul_plain over the bits of r, 2 smul_endo -- chosen per call as msm_hip_mul_each chooses.
constexpr int SMUL_LADDER_NONE = 0, SMUL_LADDER_PLAIN = 1, SMUL_LADDER_ENDO = 2;

// t = w * (the point of record b), w < r.  An identity operand runs no ladder.
template <int LADDER>
FQ_HD g1_xyzz smul_twiddle(const uint32_t* b, bool b_identity, const uint32_t w[8]) {
  if (b_identity) return g1_identity();
  const fq px = smul_ld(b), py = smul_ld(b + FQ_WORDS);
  if (smul_all_zero(px) && smul_all_zero(py)) return g1_identity();
  if (LADDER == SMUL_LADDER_NONE) return g1_from_affine(px, py);
  return LADDER == SMUL_LADDER_ENDO ? smul_endo(px, py, w) : smul_plain(px, py, w, SMUL_R_BITS);
}

// sum = a + w b, diff = a - w b.  Record a is loaded only after the ladder has returned, so the ladder's live state and the butterfly's never
// overlap.  Both results come from mixed additions INTO t = w b: sum = t + a, diff = -(t + (-a)), so that a == t (a doubling and the identity),
// a == -t (the identity and a doubling) and t the identity (a and a, from g1_madd's empty accumulator) are the branches g1_madd already has;
// a the identity is met here: sum = t, diff = -t.
template <int LADDER>
FQ_HD void smul_butterfly(const uint32_t* a, bool a_identity, const uint32_t* b, bool b_identity, const uint32_t w[8], g1_xyzz& sum, g1_xyzz& diff) {
  sum = smul_twiddle<LADDER>(b, b_identity, w);
  diff = sum;
  if (!a_identity) {
    const fq ax = smul_ld(a), ay = smul_ld(a + FQ_WORDS);
    if (!(smul_all_zero(ax) && smul_all_zero(ay))) {
      smul_madd(sum, ax, ay);
      smul_madd(diff, ax, fq_neg_canonical(ay));
    }
  }
  if (!diff.inf) diff.y = fq_sub<3>(fq_zero(), fq_tidy(diff.y));  // Y < 5p -> exact, < 2p -> -Y < 3p, normal
}

}  // namespace MSM_FIELD_NS
#undef SMUL_HD
