// Poseidon and Poseidon2 over the scalar field (libmsm_frhash.so, include/msm_frhash.h), written once and instantiated per field: a unit
// (csrc/frhash_<name>.hip) includes csrc/fq29.h over the field's constants (fr_<name>_constants.h) and then this file, inside its own MSM_FIELD_NS.
// Everything a lane does is an FQ_HD function, which the kernels at the bottom call and which the host program of tests/test_frhash_host.py runs
// serially on the CPU with every bound of csrc/fq29.h asserted.
//
//   round k:  u[i] = s[i] + rc[k t + i];  u[i] = u[i]^5 for all i (full round) or for i = 0 (partial round);  s'[i] = sum_j M[i][j] u[j]
//
// Representation.  The data are x F: F = 1 (canonical) or F = 2^256 (MSM_FRHASH_MONT256).  Inside, a value x is x R, R = 2^261 (fq_mul(a, b)
// = a b / R).  The table the host writes (csrc/frhash_plan.h) starts with two constants for each form: `in` = R^2 / F, so that fq_mul(x F, in)
// = x R, and `out` = F, so that fq_mul(x R, out) = x F.  Behind them the round constants and the matrix, each as c R, canonical.  The table's address
// does not depend on the lane: the compiler reads it with scalar loads.
//
// The lane.  One permutation per lane, 64 lanes (one wave) to a workgroup.  A state of t <= 12 elements is up to 108 registers and, read
// with a round's loop counter, would have to live in scratch memory; it lives in LDS instead -- a slab per lane, word w of element e at
// ((e FQ_L + w) 64 + lane), so that the 64 lanes of an access meet 64 different banks -- in two copies, s and s', that change places after every
// round: 2 t FQ_L 256 bytes a workgroup (13.5 KiB at t = 3, 54 KiB at t = 12), given with the launch.  A lane touches its own slab alone:
// nothing is synchronised.  Live in registers are one accumulator, one element of u and one of M.  One code path serves every t.
//
// The matrix step pairs its products: fq_mul2(u[j], M[i][j], M[i][j+1], u[j+1]) is two products with ONE Montgomery reduction (243
// multiply-adds instead of 324); an odd t starts with a single product.
//
// The bounds, for the tightest field (BLS12-381: FQ_HEADROOM = 70; a product needs value(a) value(b) <= FQ_HEADROOM r^2):
//   s       an element of the state between two rounds is "normal" (fq_norm after every lazy addition) with value < (t + 3) r: a converted input
//           (exact, < 2r); or a sum of ceil(t / 2) products and paired products of < 2r each -- < (t + 1) r -- to which the sponge adds one
//           converted input (< 2r).
//   u       s + rc, rc canonical: normal, value < (t + 4) r <= 16 r.
//   x^5     where (t + 4)^2 <= FQ_HEADROOM (t <= 4 for BLS12-381, t <= 7 for Pallas and Vesta, t <= 9 for BN254 and Grumpkin) u goes into the
//           squaring as it is; a wider state is tidied first (fq_tidy: exact, < 2r; needs value <= FQ_HEADROOM r).  x^2, x^4: exact, < 2r;
//           x^4 u: 2 (t + 4) r^2.
//   M u     one pair: 2 (t + 4) r^2 <= 32 r^2, the static_assert below.  M and u are normal or exact, as fq_mul2 wants of its last three operands.
//   store   fq_mul(s, out), out < r: (t + 3) r^2.
// The host program runs the pattern that reaches them (state, constants and matrix all r - 1, t = 12) under FQ_CHECK.
//
// The slack of these bounds.  They are sufficient, not tight: "< 2r" for a product is the multiplier's contract, but a Montgomery product of
// value T is < T / R + r, and T / R <= 2 (t + 4) r^2 / R <= 2 (t + 4) / FQ_HEADROOM r is a fraction of r, so a sum of ceil(t / 2) pairs stays near
// ceil(t / 2) r instead of (t + 1) r.  Measured in the host program (tests/test_frhash_host.py: constants, matrix, capacity and state all r - 1,
// the standard parameters, sponges), the largest S-box input before fq_tidy was 4.9 r at t = 8 (Pallas; the bound says 12 r), 6.4 r at t = 10
// (BN254, Grumpkin; 14 r), 5.7 r at t = 10 and 6.6 r at t = 12 for BLS12-381 (14 r, 16 r), 6.9 r at t = 12 overall (Grumpkin): its square is
// below FQ_HEADROOM for every field at every width.  So with `tidy` forced to false at t = 8 alone, or at t = 10 alone, every FQ_CHECK run and
// every comparison with the model still passes: the tests at each field's boundary widths (t = 4 | 5, 7 | 8, 9 | 10) check that both code
// paths compute the permutation, they cannot show that the tidy is needed where the rule above asks for it.  The rule stays: it is what
// the stated bounds prove.
//
// Poseidon2 (FrhashArgs::kind = FRHASH_KIND_POSEIDON2; include/msm_frhash.h has the definition): the same lane, the same slab layout, ONE copy
// of the state -- t FQ_L 256 bytes a workgroup, 27 KiB at t = 12 --, both linear layers in place, `cur` always 0.  frh_permute takes this path
// on the uniform kind: a scalar branch, no lane diverges (the kernels at the bottom take it once, before the lane's function).  The table holds R_F t + R_P round constants in the order of their use, then mu (t).
//   external layer (M_E), t = 2, 3: one pass sums the slab, a second adds the sum to every element.  t = 4, 8, 12: pass 1 takes a block of
//           four into registers, runs the paper's chain of eight additions and doublings (a carry-save pass after each: a limb holds at most
//           five addends) and writes it back; pass 2, position p = 0 .. 3 after the other, tidies the elements at p of every block and sums
//           them in one register set, then (t > 4) adds that sum to each of them.  The slab is indexed by loop counters, the registers never.
//   internal round: u = s[0] + rc, u^5, a running sum of u^5 and s[1 ..]; then s[i] = fq_mul2(s[i], mu[i], one, sum) = mu[i] s[i] + sum under
//           ONE Montgomery reduction (`one` = R mod r): exact and < 2r, so nothing grows from round to round and nothing is tidied behind it.
// Its bounds (H = FQ_HEADROOM; a product needs value(a) value(b) <= H r^2, fq_tidy value <= H r; the constexpr functions and the static_assert
// below state them per width):
//   in      what the first layer reads is tidied first (t products): a converted input is exact already, but the sponge has added one (< 2r) to
//           what a permutation left (< E r), and M4 multiplies a bound by 16.  From there on every input of an external layer is exact and < 2r:
//           a tidied element, an S-box output or an fq_mul2 result.
//   M4      rows sum to 16: an output < 32 r.  At t = 12 the final element would be 2 x that plus two more blocks', 128 r: more than BLS12-381's
//           H = 70 lets into fq_tidy or a product, and more than nine 29-bit limbs hold for that r.  So the block outputs are made exact
//           HERE, before anything is summed across blocks: fq_tidy of a value < 32 r <= H r (t products a layer; at t = 4, where M_E = M4,
//           they replace the tidy the S-box input would need at 33 r).
//   sums    a position sum of t / 4 tidied outputs: < (t / 2) r; an element of the result < E r with E = t / 2 + 2 (6 at t = 8, 8 at t = 12).
//           Where (E + 1)^2 > H or t E + 2 > H (the S-box input and the first internal round, below) -- t = 12 on BLS12-381 -- the four
//           position sums are tidied as well (4 products a layer) and E = 4.  t = 4: E = 2.  t = 2, 3: E = 2 t + 2 (6, 8), nothing tidied.
//   x^5     u = s + rc < (E + 1) r, normal; tidied first where (E + 1)^2 > H -- the rule of the Poseidon path; with the above, t = 3 on
//           BLS12-381 alone.  In an internal round behind the first, u < 3 r.
//   M_I     sum < (2 + (t - 1) E) r in the first internal round (s[1 ..] are an external layer's), < 2 t r later; fq_mul2's value is
//           s[i] mu[i] + one sum < (E + 2 + (t - 1) E) r^2 = (t E + 2) r^2 <= 50 r^2.  The sum is normal (a carry-save pass after every
//           addition) and below 2^261, as fq_mul2 wants of its last operand.
//   store   fq_mul(s, out): E r^2.
// Products a permutation, S the 3 of an S-box (4 where tidied), L the layer's (0 at t < 4, t, or t + 4), a pair of fq_mul2 counted as 2:
//   t + (R_F / 2 + R_F / 2) (t S + L) + L + R_P (S + 2 t).
//
// frg_load / frg_store of csrc/frgate_kernels.h are restated here (frh_load ..): including that file would instantiate libmsm_frgate.so's kernel in
// every unit of this library.
//
// No kernel waits for another workgroup.
#pragma once
#include <cstddef>
#include <cstdint>

#define FRHASH_THREADS 64          // lanes of a workgroup: one wave
#define FRHASH_MAX_WIDTH 12
#define FRHASH_MAX_FULL_ROUNDS 16
#define FRHASH_MAX_PARTIAL_ROUNDS 128
#define FRHASH_TAB_IN 0            // the table: R^2 / F
#define FRHASH_TAB_OUT 8           // F
#define FRHASH_TAB_MONT 16         // the same two for F = 2^256 (FrhashArgs::form)
#define FRHASH_TAB_RC 32           // the round constants, then the matrix
#define FRHASH_RESULT_HEAD 8       // the result buffer: the error word and seven words of padding
#define FRHASH_KIND_POSEIDON 0u    // FrhashArgs::kind: a dense matrix in every round
#define FRHASH_KIND_ANY (-1)       // (a template argument only: read FrhashArgs::kind)
#define FRHASH_KIND_POSEIDON2 1u   // an external and an internal linear layer (MSM_FRHASH_POSEIDON2); behind the round constants: mu

// what the host plans (csrc/frhash_plan.h) -- plain data, the same for every field's unit
struct FrhashArgs {
  uint32_t t, full_rounds, partial_rounds;
  uint32_t n;            // permutations, or rows of a sponge
  uint32_t len, stride;  // the sponge: elements of a row, and from one row to the next
  uint32_t capacity_at, out_at;
  uint32_t form;         // where the data form's two constants start: 0, or FRHASH_TAB_MONT
  uint32_t tile;         // the lanes of a workgroup that take a permutation (FRHASH_THREADS; fewer under msm_frhash_test_tile)
  uint32_t kind;         // FRHASH_KIND_*: which permutation the handle's table describes
  uint32_t capacity[8];  // capacity R, canonical
};

#define FRHASH_LDS_WORDS(t) (2u * (t) * FQ_LIMBS * FRHASH_THREADS)
#define FRHASH2_LDS_WORDS(t) ((t) * FQ_LIMBS * FRHASH_THREADS)  // Poseidon2: one copy of the state

#if defined(__HIPCC__)
// what the host code (csrc/frhash_host.h) knows of a field's unit
struct FrhashOps {
  const uint32_t* r32;
  void (*permute)(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* state, const uint32_t* table, const FrhashArgs* g, uint32_t* err);
  void (*hash)(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* a, const uint32_t* table, const FrhashArgs* g, uint32_t* err);
};
#endif

namespace MSM_FIELD_NS {

// the LDS a launch asks for
inline uint32_t frhash_lds_bytes(const FrhashArgs& g) { return 4u * (g.kind == FRHASH_KIND_POSEIDON2 ? FRHASH2_LDS_WORDS(g.t) : FRHASH_LDS_WORDS(g.t)); }

static_assert(2 * (FRHASH_MAX_WIDTH + 4) <= FQ_HEADROOM, "a pair of the matrix step (two products of an entry < r and an element < (t + 4) r) does not fit fq_mul2");

FQ_HD bool frh_words_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}
FQ_HD void frh_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FQ_HD void frh_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
// element `at` of a vector, exact and below r; false (and zero) where the stored value is not below r
FQ_HD bool frh_load(fq& x, const uint32_t* src, size_t at) {
  uint32_t w[8];
  frh_load_words(w, src, at);
  const bool ok = frh_words_below_r(w);
  x = ok ? fq_unpack(w) : fq_zero();
  return ok;
}
FQ_HD fq frh_trusted(const uint32_t* src) {  // eight words the host code wrote: below r
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = src[i];
  return fq_unpack(w);
}
// a lazy sum: a normal (limbs < 2^29 + 8), b normal or exact; out normal.  The value is the caller's to bound.
FQ_HD fq frh_acc(const fq& a, const fq& b) { return fq_norm(fq_add(a, b)); }

// the lane's slab (w: the workgroup's LDS from the lane's own word on; on the host, an array of the same shape): element e of it
FQ_HD fq frh_get(const uint32_t* w, uint32_t e) {
  fq x;
#pragma unroll
  for (int l = 0; l < FQ_L; l++) x.v[l] = w[(e * FQ_L + l) * FRHASH_THREADS];
  return x;
}
FQ_HD void frh_put(uint32_t* w, uint32_t e, const fq& x) {
#pragma unroll
  for (int l = 0; l < FQ_L; l++) w[(e * FQ_L + l) * FRHASH_THREADS] = x.v[l];
}

// u^5 for u normal with value < (t + 4) r (tidy: that is too much to square).  Out: exact, < 2r.
FQ_HD fq frh_sbox(const fq& u, bool tidy) {
  const fq b = tidy ? fq_tidy(u) : u;
  return fq_mul(fq_sqr(fq_sqr(b)), b);
}

// ---- Poseidon2 ----------------------------------------------------------------------------------------------------------------------------------
// the bounds of the header, in units of r: E (an element behind an external layer), whether the position sums and the S-box input are tidied
constexpr bool frh2_tidy_sums(uint32_t t) { return t >= 8 && ((t / 2 + 3) * (t / 2 + 3) > (uint32_t)FQ_HEADROOM || t * (t / 2 + 2) + 2 > (uint32_t)FQ_HEADROOM); }
constexpr uint32_t frh2_bound(uint32_t t) { return t < 4 ? 2 * t + 2 : t == 4 ? 2 : frh2_tidy_sums(t) ? 4 : t / 2 + 2; }
constexpr bool frh2_tidy_sbox(uint32_t t) { return (frh2_bound(t) + 1) * (frh2_bound(t) + 1) > (uint32_t)FQ_HEADROOM; }
constexpr bool frh2_fits(uint32_t t) {
  return frh2_bound(t) + 2 <= (uint32_t)FQ_HEADROOM                                      // the first layer's tidy: a permutation's output and an absorbed input
         && 16 * 2 <= FQ_HEADROOM                                                        // the tidy of an M4 output
         && t / 2 <= (uint32_t)FQ_HEADROOM                                               // the tidy of a position sum
         && (frh2_tidy_sbox(t) ? frh2_bound(t) + 1 : (frh2_bound(t) + 1) * (frh2_bound(t) + 1)) <= (uint32_t)FQ_HEADROOM  // the S-box input
         && t * frh2_bound(t) + 2 <= (uint32_t)FQ_HEADROOM && 2 * t + 2 <= (uint32_t)FQ_HEADROOM;                         // fq_mul2 of the first internal round, of the later ones
}
static_assert(frh2_fits(2) && frh2_fits(3) && frh2_fits(4) && frh2_fits(8) && frh2_fits(12), "a Poseidon2 width does not fit the multiplier's headroom");

// M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]] over four normal elements, by eight additions and doublings; out: normal, < 16 x the inputs' bound
FQ_HD void frh2_m4(fq& x0, fq& x1, fq& x2, fq& x3) {
  const fq t0 = frh_acc(x0, x1), t1 = frh_acc(x2, x3);
  const fq t2 = frh_acc(fq_dbl(x1), t1), t3 = frh_acc(fq_dbl(x3), t0);
  const fq t4 = frh_acc(fq_dbl(fq_dbl(t1)), t3), t5 = frh_acc(fq_dbl(fq_dbl(t0)), t2);
  x0 = frh_acc(t3, t5), x1 = t5, x2 = frh_acc(t2, t4), x3 = t4;
}

// s = M_E s in the lane's slab.  In: every element exact and < 2r (first: normal and < (E + 2) r, tidied here).  Out: normal, < E r.
FQ_HD void frh2_external(uint32_t t, uint32_t* w, bool first) {
  if (first) {
#pragma unroll 1
    for (uint32_t e = 0; e < t; e++) frh_put(w, e, fq_tidy(frh_get(w, e)));
  }
  if (t < 4) {  // out[i] = s[i] + sum_j s[j]
    fq sum = frh_get(w, 0);
#pragma unroll 1
    for (uint32_t e = 1; e < t; e++) sum = frh_acc(sum, frh_get(w, e));
#pragma unroll 1
    for (uint32_t e = 0; e < t; e++) frh_put(w, e, frh_acc(sum, frh_get(w, e)));
    return;
  }
#pragma unroll 1
  for (uint32_t e = 0; e < t; e += 4) {  // M4 on every block of four
    fq x0 = frh_get(w, e), x1 = frh_get(w, e + 1), x2 = frh_get(w, e + 2), x3 = frh_get(w, e + 3);
    frh2_m4(x0, x1, x2, x3);
    frh_put(w, e, x0), frh_put(w, e + 1, x1), frh_put(w, e + 2, x2), frh_put(w, e + 3, x3);
  }
  const bool tidy_sums = frh2_tidy_sums(t);  // (uniform)
#pragma unroll 1
  for (uint32_t p = 0; p < 4; p++) {  // the block outputs made exact; across the blocks, the sum of those at position p added to each of them
    fq sum = fq_zero();
#pragma unroll 1
    for (uint32_t e = p; e < t; e += 4) {
      const fq y = fq_tidy(frh_get(w, e));
      frh_put(w, e, y);
      sum = frh_acc(sum, y);
    }
    if (t == 4) continue;  // M_E = M4
    if (tidy_sums) sum = fq_tidy(sum);
#pragma unroll 1
    for (uint32_t e = p; e < t; e += 4) frh_put(w, e, frh_acc(sum, frh_get(w, e)));
  }
}

// The Poseidon2 permutation of the t elements of the lane's slab, in place: every element normal and < (E + 2) r -> normal and < E r, E = frh2_bound(t)
FQ_HD void frh2_permute(const FrhashArgs& g, const uint32_t* table, uint32_t* w) {
  const uint32_t t = g.t, half = g.full_rounds / 2, rounds = g.full_rounds + g.partial_rounds;
  const bool tidy = frh2_tidy_sbox(t);  // (uniform)
  const uint32_t* rc = table + FRHASH_TAB_RC;
  const uint32_t* mu = rc + (size_t)8 * (g.full_rounds * t + g.partial_rounds);
  const fq one = fq_one();
  uint32_t used = 0;  // round constants used so far: an index from the kernel's argument, never a pointer carried round the loop -- scalar loads
#pragma unroll 1
  for (uint32_t k = 0; k <= rounds; k++) {  // k = 0: the initial layer; k >= 1: round k - 1
    if (k > half && k <= half + g.partial_rounds) {  // an internal round
      const fq u = frh_sbox(frh_acc(frh_get(w, 0), frh_trusted(rc + 8 * used)), tidy);
      used += 1;
      frh_put(w, 0, u);
      fq sum = u;
#pragma unroll 1
      for (uint32_t i = 1; i < t; i++) sum = frh_acc(sum, frh_get(w, i));
#pragma unroll 1
      for (uint32_t i = 0; i < t; i++) frh_put(w, i, fq_mul2(frh_get(w, i), frh_trusted(mu + 8 * i), one, sum));  // mu[i] s[i] + sum
      continue;
    }
    if (k) {
#pragma unroll 1
      for (uint32_t i = 0; i < t; i++) frh_put(w, i, frh_sbox(frh_acc(frh_get(w, i), frh_trusted(rc + 8 * (used + i))), tidy));
      used += t;
    }
    frh2_external(t, w, k == 0);
  }
}

// The permutation of the state in copy `cur` (0 or 1: elements cur t ..) of the lane's slab, every element normal and < (t + 3) r.
// -> the copy that holds the result, every element normal and < (t + 1) r.  (A Poseidon2 handle: in place, copy 0; its bounds are frh2_permute's.)
// KIND: FRHASH_KIND_* where the caller has settled it (the kernels), FRHASH_KIND_ANY where the arguments say (the host programs).
template <int KIND = FRHASH_KIND_ANY>
FQ_HD uint32_t frh_permute(const FrhashArgs& g, const uint32_t* table, uint32_t* w, uint32_t cur) {
  if ((KIND == FRHASH_KIND_ANY ? g.kind : (uint32_t)KIND) == FRHASH_KIND_POSEIDON2) {  // (uniform: a scalar branch, or none)
    frh2_permute(g, table, w);
    return 0;
  }
  const uint32_t t = g.t, half = g.full_rounds / 2, rounds = g.full_rounds + g.partial_rounds;
  const bool tidy = (t + 4) * (t + 4) > (uint32_t)FQ_HEADROOM;  // (uniform)
  const uint32_t* rc = table + FRHASH_TAB_RC;
  const uint32_t* m = rc + (size_t)8 * rounds * t;
#pragma unroll 1
  for (uint32_t k = 0; k < rounds; k++) {
    const uint32_t boxes = (k < half || k >= half + g.partial_rounds) ? t : 1;
    const uint32_t from = cur * t, to = (cur ^ 1) * t;
#pragma unroll 1
    for (uint32_t i = 0; i < t; i++) {  // u, over s
      fq u = frh_acc(frh_get(w, from + i), frh_trusted(rc + 8 * (k * t + i)));
      if (i < boxes) u = frh_sbox(u, tidy);
      frh_put(w, from + i, u);
    }
#pragma unroll 1
    for (uint32_t i = 0; i < t; i++) {  // s'[i] = sum_j M[i][j] u[j]
      const uint32_t* row = m + 8 * i * t;
      uint32_t j = t & 1;
      fq acc = j ? fq_mul(frh_get(w, from), frh_trusted(row)) : fq_zero();
#pragma unroll 1
      for (; j < t; j += 2)
        acc = frh_acc(acc, fq_mul2(frh_get(w, from + j), frh_trusted(row + 8 * j), frh_trusted(row + 8 * (j + 1)), frh_get(w, from + j + 1)));
      frh_put(w, to + i, acc);
    }
    cur ^= 1;
  }
  return cur;
}

// state i < n of a batch: t elements in, t elements out (the same t elements where the call is in place)
template <int KIND = FRHASH_KIND_ANY>
FQ_HD bool frh_permute_lane(const FrhashArgs& g, uint32_t i, const uint32_t* state, const uint32_t* table, uint32_t* out, uint32_t* w) {
  const fq in = frh_trusted(table + g.form + FRHASH_TAB_IN);
  bool ok = true;
#pragma unroll 1
  for (uint32_t e = 0; e < g.t; e++) {
    fq x;
    ok &= frh_load(x, state, (size_t)i * g.t + e);  // (n t <= 2^26)
    frh_put(w, e, fq_mul(x, in));
  }
  const uint32_t at = frh_permute<KIND>(g, table, w, 0) * g.t;
  const fq back = frh_trusted(table + g.form + FRHASH_TAB_OUT);
#pragma unroll 1
  for (uint32_t e = 0; e < g.t; e++) {
    uint32_t words[8];
    fq_pack(words, fq_canonical(fq_mul(frh_get(w, at + e), back)));
    frh_store_words(out, (size_t)i * g.t + e, words);
  }
  return ok;
}

// row i < n of a sponge: len elements in, one out
template <int KIND = FRHASH_KIND_ANY>
FQ_HD bool frh_hash_lane(const FrhashArgs& g, uint32_t i, const uint32_t* a, const uint32_t* table, uint32_t* out, uint32_t* w) {
  const fq in = frh_trusted(table + g.form + FRHASH_TAB_IN);
  const uint32_t t = g.t, rate = t - 1;
  bool ok = true;
#pragma unroll 1
  for (uint32_t e = 0; e < t; e++) frh_put(w, e, e == g.capacity_at ? frh_trusted(g.capacity) : fq_zero());
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t first = 0; first < g.len; first += rate) {
    const uint32_t some = g.len - first < rate ? g.len - first : rate;
#pragma unroll 1
    for (uint32_t p = 0; p < some; p++) {
      const uint32_t e = cur * t + p + (p >= g.capacity_at ? 1 : 0);
      fq x;
      ok &= frh_load(x, a, (size_t)i * g.stride + first + p);  // ((n - 1) stride + len <= 2^26)
      frh_put(w, e, frh_acc(frh_get(w, e), fq_mul(x, in)));
    }
    cur = frh_permute<KIND>(g, table, w, cur);
  }
  uint32_t words[8];
  fq_pack(words, fq_canonical(fq_mul(frh_get(w, cur * t + g.out_at), frh_trusted(table + g.form + FRHASH_TAB_OUT))));
  frh_store_words(out, i, words);
  return ok;
}

#if defined(__HIPCC__)
// Each kernel tests the kind ONCE, up front, and instantiates the lane's function for it on either side of that scalar branch: within an
// instance the kind is a compile-time constant, so each side is laid out as a whole, the Poseidon side as the kernel it is without a second
// kind.  This is deliberate, not tidiness: the Poseidon loops are sensitive to it where LDS leaves a SIMD one wave at most (DESIGN.md section
// 4.24.1 has the measurement), and tests/test_frhash2_codegen.py checks that both instances are there.
__global__ void __launch_bounds__(FRHASH_THREADS) k_frhash_permute(uint32_t* out, const uint32_t* state, const uint32_t* __restrict__ table, const FrhashArgs g,
                                                                   uint32_t* err) {
  extern __shared__ uint32_t frh_lds[];
  const uint32_t i = blockIdx.x * g.tile + threadIdx.x;
  if (threadIdx.x >= g.tile || i >= g.n) return;
  bool ok;
  if (g.kind == FRHASH_KIND_POSEIDON2) ok = frh_permute_lane<FRHASH_KIND_POSEIDON2>(g, i, state, table, out, frh_lds + threadIdx.x);
  else ok = frh_permute_lane<FRHASH_KIND_POSEIDON>(g, i, state, table, out, frh_lds + threadIdx.x);
  if (!ok) atomicOr(err, 1u);
}
__global__ void __launch_bounds__(FRHASH_THREADS) k_frhash_hash(uint32_t* __restrict__ out, const uint32_t* __restrict__ a, const uint32_t* __restrict__ table,
                                                                const FrhashArgs g, uint32_t* err) {
  extern __shared__ uint32_t frh_lds[];
  const uint32_t i = blockIdx.x * g.tile + threadIdx.x;
  if (threadIdx.x >= g.tile || i >= g.n) return;
  bool ok;
  if (g.kind == FRHASH_KIND_POSEIDON2) ok = frh_hash_lane<FRHASH_KIND_POSEIDON2>(g, i, a, table, out, frh_lds + threadIdx.x);
  else ok = frh_hash_lane<FRHASH_KIND_POSEIDON>(g, i, a, table, out, frh_lds + threadIdx.x);
  if (!ok) atomicOr(err, 1u);
}

inline void frhash_launch_permute(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* state, const uint32_t* table, const FrhashArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frhash_permute, dim3(blocks), dim3(FRHASH_THREADS), frhash_lds_bytes(*g), st, out, state, table, *g, err);
}
inline void frhash_launch_hash(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* a, const uint32_t* table, const FrhashArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frhash_hash, dim3(blocks), dim3(FRHASH_THREADS), frhash_lds_bytes(*g), st, out, a, table, *g, err);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS
