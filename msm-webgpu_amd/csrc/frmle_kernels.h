// Sumcheck over multilinear tables of the scalar field (libmsm_frmle.so, include/msm_frmle.h), written once and instantiated per field: a unit
// (csrc/frmle_<name>.hip) includes csrc/fq29.h over the field's constants (fr_<name>_constants.h) and then this file, inside its own MSM_FIELD_NS.
// Everything a lane does is an FQ_HD function, which the kernels at the bottom call and which the host program of tests/test_frmle_host.py runs
// serially on the CPU with every bound of csrc/fq29.h asserted.
//
// Representation.  The data are x F: F = 1 (canonical) or F = 2^256 (MSM_FRMLE_MONT256).  fq_mul(a, b) = a b / R, R = 2^261, so a challenge c that
// arrives as c R multiplies a stored value into a stored value: fq_mul(h F, c R) = h c F.  The host (csrc/frmle_plan.h) hands every kernel its
// constants in that shape.  A table is n = 2^k elements and the FIRST variable is the TOP bit of the index: binding it pairs i with i + n / 2.
//   bind     lo + c (hi - lo) for canonical lo, hi: d = hi - lo + 2r limb by limb (fq_sub<2>: normal, < 3r), one product d (c R) -- 3r r <= 70 r^2,
//            exact and < 2r --, its canonical form added to lo with one carry chain: canonical.  fold, eval and the fused round are made of it.
//   fold     one lane per pair, one launch; a lane reads its two elements before it writes one, and no other lane touches them: in place is safe.
//   eval     a tile of 2^v <= 1024 consecutive elements holds the last v variables of its level: a lane binds the two lowest over its four
//            consecutive elements (three binds), the 2^(v-2) lane values are bound by a tree in LDS -- slot[x] = bind(slot[x], slot[x + width]),
//            width = 2^(v-3) .. 1, one product each -- and the tile's value is one word of the level above, which binds the next ten variables.
//            A level's z_j R travel in the kernel arguments.  A tile with v < 10 variables (the test hook, the top level) runs exactly v binds deep:
//            the lanes and slots beyond 2^v elements are never read -- a hole is not a zero under a bind.
//   eq       out[i] = c prod_j (bit_(k-1-j)(i) ? p_j : 1 - p_j), one lane per four elements: the lane's factor from tables of 16 entries per 4 bits
//            of the lane's number (built by the host; table 0 carries c F, the others R), the four in-lane factors from a 4-entry table.
//   round    g(t) = sum_i sum_terms coeff prod_f (lo_f + t (hi_f - lo_f)), t = 0 .. D.  A lane owns up to four pairs of a tile of 1024 pairs,
//            pair j of lane l at the in-tile offset 256 j + l (consecutive lanes read consecutive elements).  With fold_by the lane first binds
//            the top variable of every row at its pairs and stores both halves -- positions i and i + n/4, which no other lane reads or writes --
//            then reads its own stores back term by term.  Per-tile sums, one word per point, go to plain-sum levels above (k_frmle_sum).
//            The kernel is instantiated per number of points D + 1 = 2 .. 5.
//
// The bounds of round, for the tightest field (BLS12-381: FQ_HEADROOM = 70; a product needs value(a) value(b) <= FQ_HEADROOM r^2):
//   values at t   lo canonical (< r), the difference hi - lo CANONICAL (< r: two carry chains -- the limb-wise difference + 2r would be < 3r and the
//                 value at t = 4 then < 13r, whose square, 169 r^2, is beyond every field but BN254's), so value(t) = value(t - 1) + diff, a lazy
//                 sum renormalised by fq_norm (limbs < 2^29 + 8), is < (t + 1) r <= 5r.
//   the chain     the first product takes two such values: 25 r^2 <= 70 r^2; every further one an exact value < 2r and one < 5r: 10 r^2; the last
//                 one, by the term's constant coeff R^d / F^(d-1) < r, 2 r^2 (degree 1: 5 r^2).  The chain carries F^d / R^(d-1), the constant
//                 restores F and applies the coefficient.  Result exact, < 2r.
//   the lane sum  at most FRMLE_E pairs x FRMLE_MAX_TERMS terms of < 2r each, added lazily with fq_norm after every addition: < 64r <= 70r, which
//                 fq_tidy takes (value x (R mod r) <= FQ_HEADROOM r^2).  Both bounds are static_asserts below; the host program runs the
//                 patterns that reach them (lo = 0, hi = r - 1 at degree 4) under FQ_CHECK.
//
// LOW FIRST (MSM_FRMLE_LOW_FIRST: the first variable is bit 0 of the index, arkworks' order).  Binding pairs 2 i with 2 i + 1, and the SAME lane
// functions and kernels do it: the mode travels in FrmleFoldArgs / FrmleRoundArgs and only selects addresses -- a pair's two elements are 1 apart
// instead of `half`, a fused pair's four elements are 4 i .. 4 i + 3 --, uniformly for the launch; the arithmetic and its bounds are those above.
// A lane then reads 64 contiguous bytes per row (128 in the fused round) as 16-byte loads; a wave's loads together cover whole lines.  eval and eq
// need no mode: the host reverses the point.  What the mode does change is WHERE a result may be stored: output i of an in-place bind lands on
// slot i, an input of lane i / 2 (fused: the outputs 2 i, 2 i + 1 of lane i are inputs of lane i / 2), which may run in another workgroup at any
// time.  No kernel waits for one, so the host never launches such a pair of lanes together (csrc/frmle_plan.h: the schedule); to the lanes here
// that is a range of outputs (first, count) and an output row stride.
//
// frp_load / frp_store / frp_add of csrc/frpoly_kernels.h are restated here (frm_load ..): including that file would instantiate libmsm_frpoly.so's
// four kernels in every unit of this library.
//
// LDS: k_frmle_eval, k_frmle_round and k_frmle_sum 9216 bytes each (256 slots of nine limbs); k_frmle_fold and k_frmle_eq none.  No kernel waits
// for another workgroup: the levels are launches of their own (csrc/frmle_host.h).
#pragma once
#include <cstddef>
#include <cstdint>

#define FRMLE_THREADS 256
#define FRMLE_E 4
#define FRMLE_TILE (FRMLE_THREADS * FRMLE_E)
#define FRMLE_STEPS 8       // log2(FRMLE_THREADS): the steps of the trees
#define FRMLE_TILE_VARS 10  // log2(FRMLE_TILE): the variables of a full tile

#define FRMLE_MAX_DEGREE 4
#define FRMLE_MAX_TERMS 8
#define FRMLE_MAX_ROWS 16
#define FRMLE_POINTS (FRMLE_MAX_DEGREE + 1)
#define FRMLE_TERM_WORDS 16   // a term on the device: the constant (8 words), the degree, the four rows, three words of padding
#define FRMLE_WINDOW_BITS 4   // eq: a table per 4 bits of the lane's number ...
#define FRMLE_WINDOW_SIZE 16  // ... of 16 entries
#define FRMLE_MAX_WINDOWS 6   // 2^26 elements are 2^24 lanes
#define FRMLE_RESULT_HEAD 8   // the result buffer: the error word and seven words of padding, then the values of the call

// what the host plans (csrc/frmle_plan.h) -- plain data, the same for every field's unit; every constant is 8 words, canonical
struct FrmleFoldArgs {
  uint32_t c[8];        // c R
  uint32_t low;         // MSM_FRMLE_LOW_FIRST: output i binds the elements 2 i and 2 i + 1; what follows is read under it only
  uint32_t first;       // the launch computes the outputs first .. first + half - 1 of every row (`half`: the kernel's count of outputs per row)
  uint32_t out_stride;  // the rows of out are this many elements apart (the scratch rows of the in-place schedule are not `stride` apart)
};
struct FrmleEvalArgs {
  uint32_t tile;  // elements per tile in use (the test hook shrinks it), a power of two <= FRMLE_TILE
  uint32_t vars;  // variables a tile of this level binds: log2(tile), or fewer at the top level
  uint32_t z[FRMLE_TILE_VARS][8];  // z[j] R: the variable at bit j of the in-tile offset
};
struct FrmleEqArgs {
  uint32_t windows;  // tables in use
  uint32_t q[FRMLE_E][8];  // the factor of the element's two lowest bits, times R
};
struct FrmleRoundArgs {
  uint32_t tile;       // pairs per tile in use, a power of two <= FRMLE_TILE
  uint32_t num_terms;  // 1 .. FRMLE_MAX_TERMS
  uint32_t points;     // D + 1, D the largest degree
  uint32_t fold;       // bind the top variable of every row first
  uint32_t batch;      // rows (<= FRMLE_MAX_ROWS): all of them are folded
  uint32_t c[8];       // fold_by R
  uint32_t low;        // MSM_FRMLE_LOW_FIRST: pair i is the elements 2 i and 2 i + 1, and FRMLE_LOW_WORDS words behind the terms say the rest
};
// Low first, what a launch of k_frmle_round needs beyond FrmleRoundArgs sits behind its terms in device memory, at word FRMLE_TERM_WORDS num_terms:
// the kernel has no scalar register left for more arguments (they would be live from its first instruction to its last), while a word behind
// `terms` is loaded where it is used.  The lane functions read them low first only; the kernel reads FRMLE_LOW_TILES in both orders.  Offsets:
#define FRMLE_LOW_WORDS 8
#define FRMLE_LOW_FIRST_PAIR 0  // the launch's pairs are first .. end - 1; tile k of the launch begins at first + k tile
#define FRMLE_LOW_END_PAIR 1
#define FRMLE_LOW_TILES 2       // the tiles of all launches of the round: partial[t * tiles + block], `partial` moved on by the launches before
#define FRMLE_LOW_TO_SCRATCH 3  // with fold: the folded rows go to the scratch rows (1) or stay in a (0) ...
#define FRMLE_LOW_OUT_AT 4      // ... which begin this many words behind `partial` (the same allocation) ...
#define FRMLE_LOW_OUT_STRIDE 5  // ... and are this many elements apart

#if defined(__HIPCC__)
// what the host code (csrc/frmle_host.h) knows of a field's unit
struct FrmleOps {
  const uint32_t* r32;
  void (*fold)(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* a, size_t half, size_t batch, size_t stride, const FrmleFoldArgs* g, uint32_t* err);
  void (*eval)(unsigned blocks, hipStream_t st, const uint32_t* a, uint32_t* totals, size_t stride, uint32_t tiles, const FrmleEvalArgs* g, uint32_t* err);
  void (*eq)(unsigned blocks, hipStream_t st, uint32_t* out, size_t n, const uint32_t* tables, const FrmleEqArgs* p);
  void (*round)(unsigned blocks, hipStream_t st, uint32_t* a, uint32_t half, uint32_t stride, const uint32_t* terms, uint32_t* partial, const FrmleRoundArgs* g, uint32_t* err);
  void (*sum)(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, size_t len, uint32_t tiles, uint32_t tile);
};
#endif

namespace MSM_FIELD_NS {

static_assert(FRMLE_POINTS * FRMLE_POINTS <= FQ_HEADROOM, "round: two values at t = FRMLE_MAX_DEGREE (< (t + 1) r each) do not fit one product");
static_assert(2 * FRMLE_E * FRMLE_MAX_TERMS <= FQ_HEADROOM, "round: a lane's lazy sum (pairs x terms x 2r) does not fit fq_tidy");

FQ_HD bool frm_words_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}
FQ_HD void frm_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FQ_HD void frm_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
// element `at` of a vector, exact and below r; false (and zero) where the stored value is not below r
FQ_HD bool frm_load(fq& x, const uint32_t* src, size_t at) {
  uint32_t w[8];
  frm_load_words(w, src, at);
  const bool ok = frm_words_below_r(w);
  x = ok ? fq_unpack(w) : fq_zero();
  return ok;
}
FQ_HD fq frm_trusted(const uint32_t* src, size_t at) {  // a word this library or its host code wrote: below r
  uint32_t w[8];
  frm_load_words(w, src, at);
  return fq_unpack(w);
}
FQ_HD void frm_store(uint32_t* dst, size_t at, const fq& x) {  // x exact, < 2r
  uint32_t w[8];
  fq_pack(w, fq_canonical(x));
  frm_store_words(dst, at, w);
}
FQ_HD fq frm_const(const uint32_t w[8]) { return fq_unpack(w); }
// the same for all lanes, but held in vector registers: k_frmle_round keeps more uniform values alive than there are scalar registers, and a
// constant that only ever meets vector operands is the one to move (device code; an empty assembly statement that the compiler cannot see through)
FQ_HD fq frm_in_vgprs(fq x) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int i = 0; i < FQ_L; i++) asm volatile("" : "+v"(x.v[i]));
#endif
  return x;
}

// a + b mod r for canonical a, b: one carry chain, one conditional subtraction.  Out: canonical.
FQ_HD fq frm_add(const fq& a, const fq& b) {
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
// lo + c (hi - lo) for canonical lo, hi and c R canonical: canonical (the bounds are at the top of the file)
FQ_HD fq frm_bind(const fq& lo, const fq& hi, const fq& c) { return frm_add(lo, fq_canonical(fq_mul(fq_sub<2>(hi, lo), c))); }
// a lazy sum: a normal (limbs < 2^29 + 8), b exact or normal; out normal.  The value is the caller's to bound.
FQ_HD fq frm_acc(const fq& a, const fq& b) { return fq_norm(fq_add(a, b)); }
FQ_HD fq frm_exact(const fq& x) { return fq_canonical(fq_tidy(x)); }  // normal, <= FQ_HEADROOM r  ->  canonical

// ---- 1. fold ------------------------------------------------------------------------------------------------------------------------------------
// pair i of row `row`: out[row][i] = bind(a[row][i], a[row][i + half]); low first, output o = g.first + i: out[row][o] = bind(a[row][2 o],
// a[row][2 o + 1]), the rows of out g.out_stride apart.  One uniform branch: the top-first side is the code it was before there was a choice
// (selects on the 64-bit offsets cost the top-first fold 3 % at 2^20: DESIGN.md section 4.20.1).
FQ_HD bool frm_fold_pair(const FrmleFoldArgs& g, size_t row, size_t i, size_t half, size_t stride, const uint32_t* a, uint32_t* out) {
  fq lo, hi;
  if (!g.low) {
    bool ok = frm_load(lo, a, row * stride + i);
    ok &= frm_load(hi, a, row * stride + i + half);
    frm_store(out, row * stride + i, frm_bind(lo, hi, frm_const(g.c)));
    return ok;
  }
  const size_t o = g.first + i, from = row * stride + 2 * o;
  bool ok = frm_load(lo, a, from);
  ok &= frm_load(hi, a, from + 1);
  frm_store(out, row * g.out_stride + o, frm_bind(lo, hi, frm_const(g.c)));
  return ok;
}

// ---- 2. eval ------------------------------------------------------------------------------------------------------------------------------------
// Workgroup (row, k) owns the elements [k tile, (k + 1) tile) of its row, of which 2^vars exist (tile = 2^vars but at the top level, which has
// one tile).  The lane's value -- canonical -- goes to slot[lane] where the lane has elements.
FQ_HD bool frm_eval_load(const FrmleEvalArgs& g, size_t stride, size_t row, size_t k, uint32_t lane, const uint32_t* a, fq* slot) {
  const uint32_t first = lane * FRMLE_E;
  if (first >= (1u << g.vars)) return true;
  const size_t at = row * stride + k * g.tile + first;
  fq e0, e1, e2, e3;
  bool ok = frm_load(e0, a, at);
  if (g.vars >= 1) {
    ok &= frm_load(e1, a, at + 1);
    e0 = frm_bind(e0, e1, frm_const(g.z[0]));
  }
  if (g.vars >= 2) {
    ok &= frm_load(e2, a, at + 2);
    ok &= frm_load(e3, a, at + 3);
    e2 = frm_bind(e2, e3, frm_const(g.z[0]));
    e0 = frm_bind(e0, e2, frm_const(g.z[1]));
  }
  slot[lane] = e0;
  return ok;
}
// step < FRMLE_STEPS binds the variable at bit step + 2 of the in-tile offset, where the tile has it: slot[x] with slot[x + 2^step], x < 2^step
FQ_HD bool frm_eval_has_step(const FrmleEvalArgs& g, uint32_t step) { return step + 2 < g.vars; }
FQ_HD void frm_eval_step(const FrmleEvalArgs& g, fq* slot, uint32_t step, uint32_t x) { slot[x] = frm_bind(slot[x], slot[x + (1u << step)], frm_const(g.z[step + 2])); }
FQ_HD void frm_eval_store(const fq* slot, uint32_t* totals, size_t at) { frm_store(totals, at, slot[0]); }

// ---- 3. eq --------------------------------------------------------------------------------------------------------------------------------------
// lane: out[4 lane + j] = tables[0][d_0] tables[1][d_1] .. q[j], d_w the w-th 4 bits of the lane's number.  tables[16 w + d]: 8 words each.
FQ_HD void frm_eq_lane(const FrmleEqArgs& p, size_t lane, size_t n, const uint32_t* tables, uint32_t* out) {
  const size_t first = lane * FRMLE_E;
  if (first >= n) return;
  fq acc = frm_trusted(tables, lane & (FRMLE_WINDOW_SIZE - 1));
  for (uint32_t w = 1; w < p.windows; w++) {
    const uint32_t d = (uint32_t)(lane >> (FRMLE_WINDOW_BITS * w)) & (FRMLE_WINDOW_SIZE - 1);
    acc = fq_mul(acc, frm_trusted(tables, FRMLE_WINDOW_SIZE * w + d));
  }
#pragma unroll
  for (int j = 0; j < FRMLE_E; j++)
    if (first + j < n) frm_store(out, first + j, fq_mul(acc, frm_const(p.q[j])));
}

// ---- 4. round -----------------------------------------------------------------------------------------------------------------------------------
// Where a launch's lanes find their pairs, the same for all of them.  Top first, pair i of a table is the elements i and i + half, and the fused
// fold takes i, i + half, i + 2 half, i + 3 half and stores the folded i and i + half in place.  Low first, pair i is 2 i and 2 i + 1, the fused
// fold takes 4 i .. 4 i + 3 and stores the folded 2 i and 2 i + 1 in `rows` -- a, or the scratch rows behind `partial` --, and the launch's pairs
// are those the words behind the terms name (FRMLE_LOW_*).  The two orders differ in these few offsets and in nothing else, and k_frmle_round
// has very few scalar registers to spare: the offsets are made once per lane, and the order is not looked at again.
struct FrmRoundWhere {
  uint32_t shift;  // pair i begins at element i << shift of its row (the fused fold's four at i << 2 shift)
  uint32_t apart;  // a pair's two elements are this far apart, and so are the fused fold's two results.  The fused fold binds elements
                   // apart << (1 - shift) apart -- 2 half, or 1 -- and its second bind begins apart << shift behind its first -- half, or 2
  uint32_t first;  // the launch's pairs are first .. end - 1
  uint32_t end;
  uint32_t rows_at;  // the folded rows: 0: a itself; otherwise they begin this many words behind `partial` (never 0: the partials lie between)
  uint32_t rows_stride;  // ... and are this many elements apart
};
FQ_HD FrmRoundWhere frm_round_where(const FrmleRoundArgs& g, uint32_t half, uint32_t stride, const uint32_t* terms) {
  FrmRoundWhere w;
  w.rows_at = 0, w.rows_stride = stride;
  if (g.low) {  // (uniform)
    const uint32_t* const lw = terms + FRMLE_TERM_WORDS * g.num_terms;
    w.shift = 1, w.apart = 1, w.first = lw[FRMLE_LOW_FIRST_PAIR], w.end = lw[FRMLE_LOW_END_PAIR];
    if (g.fold && lw[FRMLE_LOW_TO_SCRATCH]) w.rows_at = lw[FRMLE_LOW_OUT_AT], w.rows_stride = lw[FRMLE_LOW_OUT_STRIDE];
  } else {
    w.shift = 0, w.apart = half, w.first = 0, w.end = half;
  }
  return w;
}
FQ_HD uint32_t* frm_round_rows(const FrmRoundWhere& w, uint32_t* a, uint32_t* partial) { return w.rows_at ? partial + w.rows_at : a; }
// the fused fold: pair i of the FOLDED tables, for every row
FQ_HD bool frm_round_fold_pair(const FrmleRoundArgs& g, const FrmRoundWhere& w, uint32_t* a, uint32_t stride, uint32_t i, uint32_t* rows) {
  bool ok = true;
  const fq c = frm_in_vgprs(frm_const(g.c));
  const uint32_t bound = w.apart << (1 - w.shift), second = w.apart << w.shift;
  for (uint32_t row = 0; row < g.batch; row++) {
    const uint32_t at = row * stride + (i << (2 * w.shift)), to = row * w.rows_stride + (i << w.shift);  // (batch stride <= 2^26: element numbers fit 32 bits)
    fq x0, x1, x2, x3;
    ok &= frm_load(x0, a, at);
    ok &= frm_load(x1, a, at + second);
    ok &= frm_load(x2, a, at + bound);
    ok &= frm_load(x3, a, at + second + bound);
    frm_store(rows, to, frm_bind(x0, x2, c));
    frm_store(rows, to + w.apart, frm_bind(x1, x3, c));
  }
  return ok;
}
FQ_HD bool frm_round_fold_pair(const FrmleRoundArgs& g, uint32_t* a, uint32_t stride, uint32_t i, uint32_t half) {
  return frm_round_fold_pair(g, frm_round_where(g, half, stride, nullptr), a, stride, i, a);  // (top first: no word behind the terms is read)
}
// pair i: every term's product at t = 0 .. points - 1, times the term's constant, added to acc[t] (normal; the lane's bound is at the top)
template <int POINTS>
FQ_HD bool frm_round_pair(const FrmleRoundArgs& g, const FrmRoundWhere& w, const uint32_t* rows, uint32_t i, const uint32_t* terms, fq acc[POINTS]) {
  bool ok = true;
  const uint32_t from = i << w.shift;
#pragma unroll 1
  for (uint32_t term = 0; term < g.num_terms; term++) {
    const uint32_t* tw = terms + (size_t)FRMLE_TERM_WORDS * term;
    const fq restore = frm_in_vgprs(frm_trusted(tw, 0));
    const uint32_t degree = tw[8];
    fq val[POINTS - 1], diff[POINTS - 1];  // (no term has more factors than the largest degree, POINTS - 1)
#pragma unroll
    for (int f = 0; f < POINTS - 1; f++) {
      if ((uint32_t)f < degree) {
        const uint32_t at = tw[9 + f] * w.rows_stride + from;
        fq hi;
        ok &= frm_load(val[f], rows, at);
        ok &= frm_load(hi, rows, at + w.apart);
        diff[f] = frm_add(hi, fq_neg_canonical(val[f]));
      }
    }
#pragma unroll
    for (int t = 0; t < POINTS; t++) {
      if (t) {
#pragma unroll
        for (int f = 0; f < POINTS - 1; f++)
          if ((uint32_t)f < degree) val[f] = frm_acc(val[f], diff[f]);
      }
      fq p = val[0];
#pragma unroll
      for (int f = 1; f < POINTS - 1; f++)
        if ((uint32_t)f < degree) p = fq_mul(p, val[f]);
      acc[t] = frm_acc(acc[t], fq_mul(p, restore));
    }
  }
  return ok;
}
// the lane's pairs of tile k: in-tile offsets lane, 256 + lane, ..; acc (normal, < 64r) receives their sums.  With fold_by the lane folds and
// stores all its pairs first and reads its own stores back afterwards: what only the fold needs is dead by then.  (`partial` is read low first
// only: the scratch rows lie behind it.)
template <int POINTS>
FQ_HD bool frm_round_lane(const FrmleRoundArgs& g, uint32_t* a, uint32_t half, uint32_t stride, uint32_t k, uint32_t lane, const uint32_t* terms, fq acc[POINTS],
                          uint32_t* partial = nullptr) {
  bool ok = true;
#pragma unroll
  for (int t = 0; t < POINTS; t++) acc[t] = fq_zero();
  const FrmRoundWhere w = frm_round_where(g, half, stride, terms);
  if (g.fold) {
#pragma unroll 1
    for (uint32_t j = 0; j < FRMLE_E; j++) {
      const uint32_t off = j * FRMLE_THREADS + lane, i = w.first + k * g.tile + off;
      if (off >= g.tile || i >= w.end) break;
      ok &= frm_round_fold_pair(g, w, a, stride, i, frm_round_rows(w, a, partial));
    }
  }
#pragma unroll 1
  for (uint32_t j = 0; j < FRMLE_E; j++) {
    const uint32_t off = j * FRMLE_THREADS + lane, i = w.first + k * g.tile + off;
    if (off >= g.tile || i >= w.end) break;
    ok &= frm_round_pair<POINTS>(g, w, frm_round_rows(w, a, partial), i, terms, acc);
  }
  return ok;
}
// plain sums of canonical slots: slot[x] += slot[x + 2^step], x < 2^step
FQ_HD void frm_sum_step(fq* slot, uint32_t step, uint32_t x) { slot[x] = frm_add(slot[x], slot[x + (1u << step)]); }

// ---- 5. sum: the levels above round's tiles -----------------------------------------------------------------------------------------------------
// rows of len canonical words this library wrote; workgroup (row, k) sums [k tile, (k + 1) tile).  A hole is 0.
FQ_HD void frm_sum_load(uint32_t tile, size_t len, size_t row, size_t k, uint32_t lane, const uint32_t* in, fq* slot) {
  fq s = fq_zero();
#pragma unroll
  for (int j = 0; j < FRMLE_E; j++) {
    const uint32_t off = lane * FRMLE_E + (uint32_t)j;
    const size_t at = k * tile + off;
    if (off < tile && at < len) s = frm_add(s, frm_trusted(in, row * len + at));
  }
  slot[lane] = s;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(FRMLE_THREADS) k_frmle_fold(uint32_t* out, const uint32_t* a, size_t half, size_t batch, size_t stride, const FrmleFoldArgs g, uint32_t* err) {
  const size_t idx = (size_t)blockIdx.x * FRMLE_THREADS + threadIdx.x;
  if (idx >= batch * half) return;
  if (!frm_fold_pair(g, idx / half, idx % half, half, stride, a, out)) atomicOr(err, 1u);
}

// block = row * tiles + k
__global__ void __launch_bounds__(FRMLE_THREADS) k_frmle_eval(const uint32_t* a, uint32_t* totals, size_t stride, uint32_t tiles, const FrmleEvalArgs g, uint32_t* err) {
  __shared__ uint32_t lds[FQ_LIMBS * FRMLE_THREADS];
  fq* slot = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  if (!frm_eval_load(g, stride, blockIdx.x / tiles, blockIdx.x % tiles, lane, a, slot)) atomicOr(err, 1u);
#pragma unroll
  for (uint32_t step = FRMLE_STEPS; step-- > 0;) {
    if (frm_eval_has_step(g, step)) {  // (uniform)
      __syncthreads();
      if (lane < (1u << step)) frm_eval_step(g, slot, step, lane);
    }
  }
  if (lane == 0) frm_eval_store(slot, totals, blockIdx.x);  // (lane 0 wrote slot[0] itself)
}

__global__ void __launch_bounds__(FRMLE_THREADS) k_frmle_eq(uint32_t* out, size_t n, const uint32_t* tables, const FrmleEqArgs p) {
  frm_eq_lane(p, (size_t)blockIdx.x * FRMLE_THREADS + threadIdx.x, n, tables, out);
}

// block = tile k; partial[t * tiles + k] = the tile's sum at point t, tiles = the word FRMLE_LOW_TILES behind the terms, which the host code writes in
// both orders (read here, at the end, not kept from the start).  One kernel per number of points, 2 .. 5 (g.points says which one runs): a
// round of degree 2 does not carry the registers of one of degree 4.
template <int POINTS>
__global__ void __launch_bounds__(FRMLE_THREADS) k_frmle_round(uint32_t* a, uint32_t half, uint32_t stride, const uint32_t* terms, uint32_t* partial, const FrmleRoundArgs g,
                                                               uint32_t* err) {
  __shared__ uint32_t lds[FQ_LIMBS * FRMLE_THREADS];
  fq* slot = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  fq acc[POINTS];
  if (!frm_round_lane<POINTS>(g, a, half, stride, blockIdx.x, lane, terms, acc, partial)) atomicOr(err, 1u);
#pragma unroll
  for (int t = 0; t < POINTS; t++) {
    __syncthreads();
    slot[lane] = frm_exact(acc[t]);
    for (uint32_t step = FRMLE_STEPS; step-- > 0;) {
      __syncthreads();
      if (lane < (1u << step)) frm_sum_step(slot, step, lane);
    }
    if (lane == 0) frm_store(partial, (size_t)t * terms[FRMLE_TERM_WORDS * g.num_terms + FRMLE_LOW_TILES] + blockIdx.x, slot[0]);
  }
}

// block = row * tiles + k
__global__ void __launch_bounds__(FRMLE_THREADS) k_frmle_sum(const uint32_t* in, uint32_t* out, size_t len, uint32_t tiles, uint32_t tile) {
  __shared__ uint32_t lds[FQ_LIMBS * FRMLE_THREADS];
  fq* slot = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  frm_sum_load(tile, len, blockIdx.x / tiles, blockIdx.x % tiles, lane, in, slot);
  for (uint32_t step = FRMLE_STEPS; step-- > 0;) {
    __syncthreads();
    if (lane < (1u << step)) frm_sum_step(slot, step, lane);
  }
  if (lane == 0) frm_store(out, blockIdx.x, slot[0]);
}

inline void frmle_launch_fold(unsigned blocks, hipStream_t st, uint32_t* out, const uint32_t* a, size_t half, size_t batch, size_t stride, const FrmleFoldArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frmle_fold, dim3(blocks), dim3(FRMLE_THREADS), 0, st, out, a, half, batch, stride, *g, err);
}
inline void frmle_launch_eval(unsigned blocks, hipStream_t st, const uint32_t* a, uint32_t* totals, size_t stride, uint32_t tiles, const FrmleEvalArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frmle_eval, dim3(blocks), dim3(FRMLE_THREADS), 0, st, a, totals, stride, tiles, *g, err);
}
inline void frmle_launch_eq(unsigned blocks, hipStream_t st, uint32_t* out, size_t n, const uint32_t* tables, const FrmleEqArgs* p) {
  hipLaunchKernelGGL(k_frmle_eq, dim3(blocks), dim3(FRMLE_THREADS), 0, st, out, n, tables, *p);
}
inline void frmle_launch_round(unsigned blocks, hipStream_t st, uint32_t* a, uint32_t half, uint32_t stride, const uint32_t* terms, uint32_t* partial, const FrmleRoundArgs* g,
                               uint32_t* err) {
  switch (g->points) {
    case 2: hipLaunchKernelGGL(k_frmle_round<2>, dim3(blocks), dim3(FRMLE_THREADS), 0, st, a, half, stride, terms, partial, *g, err); break;
    case 3: hipLaunchKernelGGL(k_frmle_round<3>, dim3(blocks), dim3(FRMLE_THREADS), 0, st, a, half, stride, terms, partial, *g, err); break;
    case 4: hipLaunchKernelGGL(k_frmle_round<4>, dim3(blocks), dim3(FRMLE_THREADS), 0, st, a, half, stride, terms, partial, *g, err); break;
    default: hipLaunchKernelGGL(k_frmle_round<5>, dim3(blocks), dim3(FRMLE_THREADS), 0, st, a, half, stride, terms, partial, *g, err); break;
  }
}
inline void frmle_launch_sum(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, size_t len, uint32_t tiles, uint32_t tile) {
  hipLaunchKernelGGL(k_frmle_sum, dim3(blocks), dim3(FRMLE_THREADS), 0, st, in, out, len, tiles, tile);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS
