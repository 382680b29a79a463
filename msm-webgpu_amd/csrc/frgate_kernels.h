// Constraint evaluation over rows of the scalar field (libmsm_frgate.so, include/msm_frgate.h), written once and instantiated per field: a unit
// (csrc/frgate_<name>.hip) includes csrc/fq29.h over the field's constants (fr_<name>_constants.h) and then this file, inside its own MSM_FIELD_NS.
// Everything a lane does is an FQ_HD function, which the kernel at the bottom calls and which the host program of tests/test_frgate_host.py runs
// serially on the CPU with every bound of csrc/fq29.h asserted.
//
//   out[i] = (ACCUMULATE ? out[i] : 0) + scale[i mod scale_len] sum_t coeff_t prod_f a[rows[f]][(i + off_f) mod n],   off_f = rots[f] step mod n
//
// Representation.  The data are x F: F = 1 (canonical) or F = 2^256 (MSM_FRGATE_MONT256).  fq_mul(a, b) = a b / R, R = 2^261: a chain of d
// stored factors carries F^d / R^(d-1), and one more product, by the term's constant coeff R^d / F^(d-1), leaves coeff F prod -- a stored
// value.  With a scale the host hands the constant a further R / F: the sum is then E R, and its product with a stored scale element s F is
// E s F.  The host (csrc/frgate_plan.h) writes one record per term: the constant, the degree and, per factor, the first element of its row
// (rows[f] stride) and its offset.
//
// The lane.  One element per lane, 256 lanes to a workgroup, one launch.  Consecutive lanes read consecutive elements of a row, rotated or not
// (a wave's 64 elements are 2 KiB in a line, in two pieces where the rotation wraps inside them).  The term records are read at an address
// that does not depend on the lane.  The terms run one after the other and a term's factors one after the other: what is live is the running
// product, the factor on its way in and the lane's sum -- three field elements, fewer than k_frmle_round keeps.
//
// The bounds, for the tightest field (BLS12-381: FQ_HEADROOM = 70; a product needs value(a) value(b) <= FQ_HEADROOM r^2):
//   the chain     every factor is canonical (< r, checked by the lane).  p = fq_mul(p, v) takes an exact p < 2r and a canonical v: 2 r^2; the last
//                 product, by the term's constant (< r): 2 r^2.  Result exact, < 2r.
//   the lane sum  term values (< 2r each) are added lazily, with fq_norm after every addition; after every FRGATE_TIDY_EVERY = 32 terms the sum
//                 is tidied (fq_tidy: exact, < 2r, the same value mod r).  So a tidy, and the final product by the scale (canonical) or by one,
//                 meets at most 2r + 32 x 2r = 66r <= 70r.  That is the static_assert below; the host program runs the pattern that reaches it (64
//                 terms of degree 8, every element, coefficient and scale r - 1, accumulated onto r - 1) under FQ_CHECK.
//
// frm_load / frm_store / frm_add of csrc/frmle_kernels.h are restated here (frg_load ..): including that file would instantiate
// libmsm_frmle.so's kernels in every unit of this library.
//
// LDS: none.  No kernel waits for another workgroup.
#pragma once
#include <cstddef>
#include <cstdint>

#define FRGATE_THREADS 256
#define FRGATE_MAX_DEGREE 8
#define FRGATE_MAX_TERMS 64
#define FRGATE_MAX_ROWS 32
#define FRGATE_TIDY_EVERY 32  // terms between two tidies of the lane's sum
// a term on the device: the constant (8 words), the degree, the first element of each factor's row (8), each factor's offset (8), 3 words of padding
#define FRGATE_TERM_WORDS 28
#define FRGATE_TERM_DEGREE 8
#define FRGATE_TERM_BASE 9
#define FRGATE_TERM_OFF 17
#define FRGATE_RESULT_HEAD 8  // the result buffer: the error word and seven words of padding

// what the host plans (csrc/frgate_plan.h) -- plain data, the same for every field's unit
struct FrgateArgs {
  uint32_t n;           // elements, a power of two
  uint32_t num_terms;   // 1 .. FRGATE_MAX_TERMS
  uint32_t scale_mask;  // scale_len - 1
  uint32_t has_scale;
  uint32_t accumulate;
};

#if defined(__HIPCC__)
// what the host code (csrc/frgate_host.h) knows of a field's unit
struct FrgateOps {
  const uint32_t* r32;
  void (*apply)(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* a, const uint32_t* terms, const uint32_t* scale, const FrgateArgs* g, uint32_t* err);
};
#endif

namespace MSM_FIELD_NS {

static_assert(2 * (FRGATE_TIDY_EVERY + 1) <= FQ_HEADROOM, "apply: a lane's lazy sum (a tidied sum and FRGATE_TIDY_EVERY terms of < 2r) does not fit fq_tidy");

FQ_HD bool frg_words_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}
FQ_HD void frg_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FQ_HD void frg_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
// element `at` of a vector, exact and below r; false (and zero) where the stored value is not below r
FQ_HD bool frg_load(fq& x, const uint32_t* src, size_t at) {
  uint32_t w[8];
  frg_load_words(w, src, at);
  const bool ok = frg_words_below_r(w);
  x = ok ? fq_unpack(w) : fq_zero();
  return ok;
}
FQ_HD fq frg_trusted(const uint32_t* src) {  // eight words the host code wrote: below r
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = src[i];
  return fq_unpack(w);
}
FQ_HD void frg_store(uint32_t* dst, size_t at, const fq& x) {  // x canonical
  uint32_t w[8];
  fq_pack(w, x);
  frg_store_words(dst, at, w);
}
// a + b mod r for canonical a, b: one carry chain, one conditional subtraction.  Out: canonical.
FQ_HD fq frg_add(const fq& a, const fq& b) {
  fq t;
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) {
    const uint32_t s = a.v[i] + b.v[i] + carry;
    t.v[i] = i < FQ_L - 1 ? (s & FQ_MASK) : s;
    carry = s >> FQ_W;
  }
  return fq_canonical(t);
}
// a lazy sum: a normal (limbs < 2^29 + 8), b exact; out normal.  The value is the caller's to bound.
FQ_HD fq frg_acc(const fq& a, const fq& b) { return fq_norm(fq_add(a, b)); }

// term record tw at element i: coeff F prod_f a[base_f + ((i + off_f) mod n)] (coeff R prod with a scale), exact, < 2r
FQ_HD bool frg_term(const FrgateArgs& g, uint32_t i, const uint32_t* a, const uint32_t* tw, fq& value) {
  const uint32_t mask = g.n - 1, degree = tw[FRGATE_TERM_DEGREE];
  fq p;
  bool ok = frg_load(p, a, tw[FRGATE_TERM_BASE] + ((i + tw[FRGATE_TERM_OFF]) & mask));  // (batch stride <= 2^26: element numbers fit 32 bits)
#pragma unroll 1
  for (uint32_t f = 1; f < degree; f++) {
    fq v;
    ok &= frg_load(v, a, tw[FRGATE_TERM_BASE + f] + ((i + tw[FRGATE_TERM_OFF + f]) & mask));
    p = fq_mul(p, v);
  }
  value = fq_mul(p, frg_trusted(tw));
  return ok;
}
// element i < n of the call
FQ_HD bool frg_lane(const FrgateArgs& g, uint32_t i, const uint32_t* a, const uint32_t* terms, const uint32_t* scale, uint32_t* out) {
  bool ok = true;
  fq sum = fq_zero();
#pragma unroll 1
  for (uint32_t term = 0; term < g.num_terms; term++) {
    fq value;
    ok &= frg_term(g, i, a, terms + (size_t)FRGATE_TERM_WORDS * term, value);
    sum = frg_acc(sum, value);
    if ((term + 1) % FRGATE_TIDY_EVERY == 0) sum = fq_tidy(sum);  // (uniform)
  }
  fq by = fq_one();  // without a scale: a tidy
  if (g.has_scale) ok &= frg_load(by, scale, i & g.scale_mask);
  fq res = fq_canonical(fq_mul(sum, by));
  if (g.accumulate) {
    fq old;
    ok &= frg_load(old, out, i);
    res = frg_add(res, old);
  }
  frg_store(out, i, res);
  return ok;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(FRGATE_THREADS) k_frgate_apply(uint32_t* out, const uint32_t* __restrict__ a, const uint32_t* __restrict__ terms,
                                                                 const uint32_t* __restrict__ scale, const FrgateArgs g, uint32_t* err) {
  const uint32_t i = blockIdx.x * FRGATE_THREADS + threadIdx.x;
  if (i >= g.n) return;
  if (!frg_lane(g, i, a, terms, scale, out)) atomicOr(err, 1u);
}

inline void frgate_launch_apply(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* a, const uint32_t* terms, const uint32_t* scale, const FrgateArgs* g,
                                uint32_t* err) {
  hipLaunchKernelGGL(k_frgate_apply, dim3(blocks), dim3(FRGATE_THREADS), 0, st, out, a, terms, scale, *g, err);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS
