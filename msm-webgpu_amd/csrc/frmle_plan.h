// The constants and the level structure of libmsm_frmle.so's calls: pure host code, no HIP (csrc/frmle_host.h launches what this plans; the host
// program of tests/test_frmle_host.py runs the same plan through the same per-lane code on the CPU).  Needs the Frmle*Args of csrc/frmle_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "host_fr.h"

namespace msm_frmle {

using host_fr::Field;
using host_fr::Fr;

inline Fr pow2(const Field& f, int k) {  // 2^k mod r
  Fr x = {{1, 0, 0, 0}};
  for (int i = 0; i < k; i++) x = f.add(x, x);
  return x;
}
inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }
inline bool power_of_two(size_t n) { return n && !(n & (n - 1)); }
inline int log2_of(size_t n) {  // n a power of two
  int k = 0;
  while (((size_t)1 << k) < n) k++;
  return k;
}

// the device's Montgomery radix is R = 2^261 (csrc/fq29.h); F = 2^256 for mont256 data, 1 otherwise.  Below, values with an m are in the HOST's
// Montgomery form (csrc/host_fr.h: 2^256), whatever the data's form is.
inline Fr form(const Field& f, bool mont) { return mont ? pow2(f, 256) : Fr{{1, 0, 0, 0}}; }
// xm times the plain value k, as a plain value: what the device reads
inline void store_scaled(const Field& f, const Fr& xm, const Fr& k, uint32_t w[8]) { host_fr::store_words(f.mul(xm, k), w); }
inline Fr one_minus_m(const Field& f, const Fr& xm) {  // (1 - x) in the host's form, from x in it
  const Fr neg = Field::sub_raw(f.modulus(), xm);      // r - x in (0, r]: add() reduces the sum
  return f.add(neg, f.one());
}

// rows of n values: level l has len[l] values per row in ceil(len[l] / tile) tiles; the last level has one tile per row (as csrc/frpoly_plan.h)
inline std::vector<size_t> plan_levels(size_t n, uint32_t tile) {
  std::vector<size_t> len(1, n);
  while ((len.back() + tile - 1) / tile > 1) len.push_back((len.back() + tile - 1) / tile);
  return len;
}

inline FrmleFoldArgs plan_fold(const Field& f, const uint8_t c[32]) {
  FrmleFoldArgs g;
  memset(&g, 0, sizeof g);
  store_scaled(f, f.to_mont(host_fr::load32(c)), pow2(f, 261), g.c);
  return g;
}

// ---- low first (MSM_FRMLE_LOW_FIRST): the schedules ----------------------------------------------------------------------------------------------
// Output i of a bind is a function of the elements 2 i and 2 i + 1 and, in place, is stored on slot i: an input of output i / 2.  Lanes of one
// launch run in any order, across workgroups that do not wait for each other; launches on one stream run one after the other.  So within a
// launch no lane may store where another lane of that launch reads.  Of the n / 2 outputs of a row,
//   the upper half, [n / 4, n / 2), reads [n / 2, n) and stores to [n / 4, n / 2): apart, safe in place in one launch;
//   the lower half, [0, n / 4), reads [0, n / 2) and would store to [0, n / 4): it goes to the scratch buffer instead, rows n / 4 apart.
// The lower half runs FIRST -- it reads [n / 4, n / 2) as the row was --, the upper half second, and one device-to-device copy on the same stream
// (not a kernel: hipMemcpy2DAsync) brings the scratch rows home.  n = 2 has one output, whose slot only its own lane reads: one launch in place.
// The alternative, all n / 2 outputs to scratch and all copied back, moves n more elements per row where this moves n / 2.
struct LowLaunch {
  uint32_t first, count;  // the outputs first .. first + count - 1 of every row
  bool to_scratch;        // stored to the scratch rows (`copy` elements apart) instead of the rows themselves
};
struct LowSchedule {
  std::vector<LowLaunch> launches;  // in stream order
  size_t copy = 0;                  // elements at the head of every row that come home from scratch afterwards
};
// the in-place bind of a table of n >= 2 elements to n / 2 outputs
inline LowSchedule plan_low_in_place(size_t n) {
  LowSchedule s;
  const uint32_t outputs = (uint32_t)(n / 2), lower = outputs / 2;
  if (lower) {
    s.launches.push_back(LowLaunch{0, lower, true});
    s.copy = lower;
  }
  s.launches.push_back(LowLaunch{lower, outputs - lower, false});
  return s;
}
inline FrmleFoldArgs plan_fold_low(const Field& f, const uint8_t c[32], const LowLaunch& l, size_t out_stride) {
  FrmleFoldArgs g = plan_fold(f, c);
  g.low = 1, g.first = l.first, g.out_stride = (uint32_t)out_stride;
  return g;
}
// The fused round over a table of n >= 4 elements is the same schedule over the PAIRS of the folded table: pair i (< n / 4) reads 4 i .. 4 i + 3
// and stores the folded 2 i and 2 i + 1, so the pairs [0, n / 8) go to scratch (rows n / 4 apart) and [n / 8, n / 4) stay in place; n = 4 has one
// pair.  Each launch has its own tiles, numbered one after the other: partials = the tiles of both.  A launch has half the round's pairs, and the
// two run one after the other: with tiles of HALF the size (low_fused_tile) each of them has the workgroups the one top-first launch has --
// at 2^20 and the design's tile 256, one per compute unit, where 128 would leave half the chip idle twice over.
inline uint32_t low_fused_tile(uint32_t tile) { return tile / 2; }  // (tile >= 2)
inline LowSchedule plan_low_fused(size_t n) {
  LowSchedule s = plan_low_in_place(n / 2);  // (as many pairs as a table of n / 2 has outputs, split the same way)
  s.copy *= 2;
  return s;
}
inline uint32_t low_tiles(const LowLaunch& l, uint32_t tile) { return (l.count + tile - 1) / tile; }
// the levels of a low-first fused round: the pairs, the partials of the schedule's launches (tiles of launch_tile pairs), and plain sums over
// tiles of `tile` above them as plan_levels has them
inline std::vector<size_t> plan_levels_low_fused(const LowSchedule& s, size_t pairs, uint32_t launch_tile, uint32_t tile) {
  size_t partials = 0;
  for (const LowLaunch& l : s.launches) partials += low_tiles(l, launch_tile);
  std::vector<size_t> len(1, pairs);
  if (partials > 1) {
    const std::vector<size_t> above = plan_levels(partials, tile);
    len.insert(len.end(), above.begin(), above.end());
  }
  return len;
}
// the point of eval and eq with point[j] at bit j: the top-first calls take it reversed
inline std::vector<uint8_t> reversed_point(const uint8_t* point, int k) {
  std::vector<uint8_t> out((size_t)k * 32);
  for (int j = 0; j < k; j++) memcpy(out.data() + 32 * (size_t)j, point + 32 * (size_t)(k - 1 - j), 32);
  return out;
}

// eval of a table of 2^k elements at point (k x 32 bytes; point[0] is the TOP bit's variable): level l binds the bits [l t, l t + vars) of the
// index, t = log2(tile); bit b is the variable point[k - 1 - b]
inline std::vector<FrmleEvalArgs> plan_eval(const Field& f, uint32_t tile, int k, const uint8_t* point) {
  const int t = log2_of(tile);
  const size_t levels = k ? (size_t)(k + t - 1) / t : 1;
  std::vector<FrmleEvalArgs> out(levels);
  const Fr radix = pow2(f, 261);
  for (size_t l = 0; l < levels; l++) {
    FrmleEvalArgs& g = out[l];
    memset(&g, 0, sizeof g);
    g.tile = tile;
    const int left = k - (int)l * t;
    g.vars = (uint32_t)(left < t ? left : t);
    for (uint32_t j = 0; j < g.vars; j++) store_scaled(f, f.to_mont(host_fr::load32(point + 32 * (k - 1 - ((int)l * t + (int)j)))), radix, g.z[j]);
  }
  return out;
}

// eq over n = 2^k elements: the tables -- words[8 (16 w + d) ..] = the product of the factors of the bits 2 + 4 w .. 5 + 4 w of the index as the
// bits of d say, times c F for w = 0 and R above, as many windows as the lane numbers of n elements have digits -- and the four factors of the
// bits 0 and 1, times R.  A bit the index does not have has the factors 1 (clear) and 0 (set).
inline FrmleEqArgs plan_eq(const Field& f, size_t n, const uint8_t* point, const uint8_t c[32], bool mont, std::vector<uint32_t>& words) {
  FrmleEqArgs p;
  memset(&p, 0, sizeof p);
  const int k = log2_of(n);
  const size_t lanes = (n + FRMLE_E - 1) / FRMLE_E;
  p.windows = 1;
  while (p.windows < FRMLE_MAX_WINDOWS && ((lanes - 1) >> (FRMLE_WINDOW_BITS * p.windows))) p.windows++;
  const Fr radix = pow2(f, 261);
  const Fr zero = {{0, 0, 0, 0}};
  auto factor = [&](int bit, uint32_t set) -> Fr {
    if (bit >= k) return set ? zero : f.one();
    const Fr pm = f.to_mont(host_fr::load32(point + 32 * (k - 1 - bit)));
    return set ? pm : one_minus_m(f, pm);
  };
  for (uint32_t j = 0; j < FRMLE_E; j++) store_scaled(f, f.mul(factor(1, j >> 1), factor(0, j & 1u)), radix, p.q[j]);
  words.assign((size_t)p.windows * FRMLE_WINDOW_SIZE * 8, 0);
  const Fr first = f.from_mont(f.mul(f.to_mont(host_fr::load32(c)), f.to_mont(form(f, mont))));  // c F
  for (uint32_t w = 0; w < p.windows; w++) {
    for (uint32_t d = 0; d < FRMLE_WINDOW_SIZE; d++) {
      Fr xm = f.one();
      for (int u = 0; u < FRMLE_WINDOW_BITS; u++) xm = f.mul(xm, factor(2 + FRMLE_WINDOW_BITS * (int)w + u, (d >> u) & 1u));
      store_scaled(f, xm, w ? radix : first, words.data() + 8 * (FRMLE_WINDOW_SIZE * w + d));
    }
  }
  return p;
}

// a term as the caller gives it (include/msm_frmle.h: msm_frmle_term), field by field
struct Term {
  const uint8_t* coeff;
  uint32_t degree;
  const uint32_t* rows;
};
// round: the kernel's arguments and words[16 term ..] = the term's constant coeff R^d / F^(d-1) -- the product chain of d factors carries
// F^d / R^(d-1), one product by the constant leaves coeff F prod --, its degree and its rows
inline FrmleRoundArgs plan_round(const Field& f, uint32_t tile, const Term* terms, size_t num_terms, size_t batch, const uint8_t* fold_by, bool mont,
                                 std::vector<uint32_t>& words) {
  FrmleRoundArgs g;
  memset(&g, 0, sizeof g);
  g.tile = tile, g.num_terms = (uint32_t)num_terms, g.batch = (uint32_t)batch, g.fold = fold_by != nullptr;
  if (fold_by) store_scaled(f, f.to_mont(host_fr::load32(fold_by)), pow2(f, 261), g.c);
  words.assign(num_terms * FRMLE_TERM_WORDS, 0);
  uint32_t top = 0;
  for (size_t k = 0; k < num_terms; k++) {
    const int d = (int)terms[k].degree;
    if (terms[k].degree > top) top = terms[k].degree;
    uint32_t* w = words.data() + FRMLE_TERM_WORDS * k;
    store_scaled(f, f.to_mont(host_fr::load32(terms[k].coeff)), pow2(f, mont ? 5 * d + 256 : 261 * d), w);
    w[8] = terms[k].degree;
    for (int j = 0; j < d; j++) w[9 + j] = terms[k].rows[j];
  }
  g.points = top + 1;
  return g;
}
// The constants of a round as k_frmle_round takes them, in either order (top first: the one launch of all pairs): for every launch of the schedule the terms (`words` as plan_round left them) and behind them the
// FRMLE_LOW_WORDS of that launch (csrc/frmle_kernels.h) -- launch l takes its terms at word l * low_block_words(num_terms).  tiles: of all
// launches; out_at: where the scratch rows begin, in words behind the FIRST launch's `partial` (a later launch's is moved on by 8 words per tile
// before it, which is taken off here); the scratch rows are s.copy elements apart.
inline size_t low_block_words(size_t num_terms) { return num_terms * FRMLE_TERM_WORDS + FRMLE_LOW_WORDS; }
inline void plan_round_launches(FrmleRoundArgs& g, bool low, const LowSchedule& s, uint32_t tile, size_t out_at, std::vector<uint32_t>& words) {
  g.low = low, g.tile = tile;  // (tile: of the launches -- low_fused_tile of the call's for the low-first fused round)
  const std::vector<uint32_t> terms = words;
  const size_t block = low_block_words(g.num_terms);
  words.assign(block * s.launches.size(), 0);
  uint32_t tiles = 0, before = 0;
  for (const LowLaunch& l : s.launches) tiles += low_tiles(l, tile);
  for (size_t k = 0; k < s.launches.size(); k++) {
    const LowLaunch& l = s.launches[k];
    uint32_t* w = words.data() + block * k;
    memcpy(w, terms.data(), terms.size() * 4);
    w += terms.size();
    w[FRMLE_LOW_FIRST_PAIR] = l.first, w[FRMLE_LOW_END_PAIR] = l.first + l.count, w[FRMLE_LOW_TILES] = tiles;
    w[FRMLE_LOW_TO_SCRATCH] = l.to_scratch, w[FRMLE_LOW_OUT_AT] = (uint32_t)(out_at - 8 * (size_t)before), w[FRMLE_LOW_OUT_STRIDE] = (uint32_t)s.copy;
    before += low_tiles(l, tile);
  }
}

}  // namespace msm_frmle
