// Launch planning of libmsm_hip.so: what a launch request is (LaunchMode, LaunchRequest), what is decided once from it (LaunchPlan, plan_launch), the
// shape a whole MSM takes on a context (whole_msm_request, batch_group) and the policies behind them -- window bits, the wide tables' digit width and
// top digit, SMVP chunk lengths, digit planes, upload parts -- with the environment readers those policies consult.
// HIP-free: no HIP include and no HIP call, so tests/host_harness/msm_plan_harness.cpp runs it on the CPU (tests/test_msm_plan_host.py).  Of a
// context it reads the fields of PlanInputs alone, and of the device one number, num_cus(), which it only declares: msm_ctx.h defines it for the
// library, the harness for itself.  Assumes nothing included before it.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/msm_hip.h"
#include "msm_layout.h"

using namespace msm_layout;

// What planning reads of a context: msm_hip_ctx (msm_ctx.h) derives from it, the CPU harness fills one in by hand
struct PlanInputs {
  int curve = MSM_HIP_CURVE_BN254_G1;
  size_t n_bases = 0;                 // points per table
  bool precomputed = false;           // d_bases holds the 16 tables 2^(16 w) P_i (MSM_HIP_BASES_PRECOMPUTE)
  int wide_bits_choice = 0;           // msm_hip_set_wide_bits: the digit width the next wide base set gets (0: by the number of bases)
  int wide_bits = 0;                  // != 0: d_bases holds the wide tables 2^(C w) P_i for C-bit digits (MSM_HIP_BASES_PRECOMPUTE_WIDE; pick_wide_bits)
  bool endo = false;                  // d_bases holds phi(P_i) behind the n bases (MSM_HIP_BASES_ENDOMORPHISM)
  size_t n_identity = 0;              // identity records among the resident bases: nonzero -> every launch masks its scalars (k_mask_identity)
  uint32_t scalar_format = 0;         // MSM_HIP_SCALARS_CANONICAL / MONT256 / U8 .. U64 / MSM_HIP_SCALAR_U128 [| MSM_HIP_SCALAR_SIGNED] (read by each launch)
  int window_bits = 0;                // 0: chosen from n for whole-MSM launches (pick_window_bits); else 12 / 14 / 16
  bool debug = false;
};

namespace {
// What a launch's local windows are made of
enum LaunchMode {
  MODE_PLAIN = 0,   // windows [w_begin, w_end) of 254-bit scalars over the n bases
  MODE_TABLES = 1,  // fixed-base tables: all windows of a vector feed one bucket set (MSM_HIP_BASES_PRECOMPUTE)
  MODE_HALVES = 2,  // endomorphism: 127-bit halves k1, k2 over the 2n points P_i, phi(P_i) (MSM_HIP_BASES_ENDOMORPHISM, csrc/glv.h)
  MODE_WIDE = 3,    // wide fixed-base tables: ceil(255 / C) digits of C = 16 .. 20 bits per scalar, one bucket set of 2^(C-1) slots run as 2^(C-16) virtual windows of 2^15
                    // (MSM_HIP_BASES_PRECOMPUTE_WIDE; sort_kernels.h: k_count_wide)
  MODE_NARROW = 4,  // narrow scalars (MSM_HIP_SCALARS_U8 .. U64, MSM_HIP_SCALAR_U128, and their MSM_HIP_SCALAR_SIGNED forms): the
                    // narrow_windows(C, bytes) windows of n x 1 .. 16 B integers over the plain records 0 .. n-1, which every base mode keeps
                    // (recode.h: k_count<C, SW, void, NB>)
};

// bytes of a narrow scalar format (MSM_HIP_SCALARS_U8 .. U64, MSM_HIP_SCALAR_U128, each with or without MSM_HIP_SCALAR_SIGNED); 0 for the
// 32-byte formats and for every value that is no format at all (the flag alone or on a 32-byte format, unused numbers)
inline int narrow_bytes(uint32_t format) {
  switch (format & ~MSM_HIP_SCALAR_SIGNED) {
    case MSM_HIP_SCALARS_U8: return 1;
    case MSM_HIP_SCALARS_U16: return 2;
    case MSM_HIP_SCALARS_U32: return 4;
    case MSM_HIP_SCALARS_U64: return 8;
    case MSM_HIP_SCALAR_U128: return 16;
    default: return 0;
  }
}
inline bool narrow_signed(uint32_t format) { return narrow_bytes(format) && (format & MSM_HIP_SCALAR_SIGNED); }  // two's-complement values
// U8 / U16 (I8 / I16) run as byte windows (one per byte of the magnitude, digits 1 .. 255, a one-level counting sort: sort_kernels.h, k_byte_count
// ...) on the 12-bit bucket grid -- the smallest the reduce kernels have, 2^11 slots of which 255 can fill; the wider formats as truncated signed
// C-bit windows (C from n) through the two-level sort
inline bool byte_windows(int nb) { return nb == 1 || nb == 2; }
constexpr int BYTE_WBITS = 12;
inline int narrow_windows(int wbits, int nb) { return byte_windows(nb) ? nb : narrow_nwin_of(wbits, nb); }
inline int narrow_max_windows(int nb) { return byte_windows(nb) ? BYTE_MAXLW : MAXLW; }  // local windows per launch (byte windows: 256 bins each)

constexpr uint32_t MAX_TILES = 1024;
constexpr int NSLOT = MSM_HIP_NUM_SLOTS;  // result slots

// What a caller asks of one launch.  The defaults are one plain whole MSM of 16-bit windows over the first n bases into slot 0, its sums to the
// host, so a call site names only what differs.  plan_launch checks it and makes the LaunchPlan.
struct LaunchRequest {
  const void* scalars = nullptr;      // device: nvec contiguous vectors of n scalars in the context's scalar format
  size_t n = 0;
  int slot = 0;
  int nvec = 1;
  void* sums_dev = nullptr;           // device memory for the window sums; null: the slot's own buffer, and from there the host
  LaunchMode mode = MODE_PLAIN;
  int w_begin = 0, w_end = NWIN;      // windows [w_begin, w_end) of every vector, in units of `wbits`-bit windows (MODE_WIDE: all T digits)
  int wbits = WBITS;                  // (MODE_WIDE: the tables' digit width)
  int v_begin = 0, v_count = 0;       // MODE_WIDE, v_count != 0: a SHARE of the virtual windows -- [v_begin, v_begin + v_count) of every vector, whose sums are
                                      // (window sum, plain total) pairs, 2 records per local window.  0: whole MSMs, all 2^(C-16) virtual windows
  bool sparse = false;                // a sparse launch: input j is (scalar j, base indices[j]) and n counts entries (SparseIdx) -- one whole MSM, into
  const uint32_t* indices = nullptr;  // the slot, over the resident bases from record 0; not on wide tables.  The n indices are device memory
  size_t base_off = 0;                // point i of the launch is base base_off + i (the parts of msm_hip_run)
  bool sync = false;                  // a synchronous call (run = launch + finish at once): nothing will be pipelined behind this launch

  LaunchRequest(const void* scalars_ = nullptr, size_t n_ = 0, int slot_ = 0, int nvec_ = 1, void* sums_dev_ = nullptr)
      : scalars(scalars_), n(n_), slot(slot_), nvec(nvec_), sums_dev(sums_dev_) {}
  LaunchRequest& windows(LaunchMode mode_, int begin, int end, int bits = WBITS) {
    mode = mode_, w_begin = begin, w_end = end, wbits = bits;
    return *this;
  }
  LaunchRequest& wide(int bits, int vbegin, int vcount) {  // all digits of `bits`-bit wide tables
    v_begin = vbegin, v_count = vcount;
    return windows(MODE_WIDE, 0, wide_tables_of(bits), bits);
  }
};

// What a launch is made of: its request as plan_launch settled it, and everything decided once from that -- read by the launch's buffer sizing
// (ensure_work), both stages of its enqueue (enqueue_sort, enqueue_reduce), the host finish and the stage read-back hooks
struct LaunchPlan : LaunchRequest {   // (settled: wbits = the window bits of everything behind the recode, 16 for MODE_WIDE; v_count = the virtual windows run)
  int nb = 0;                         // MODE_NARROW: bytes per scalar ...
  bool nb_signed = false;             // ... and whether they are two's-complement (MSM_HIP_SCALAR_SIGNED)
  int nb_kernel() const { return nb_signed ? -nb : nb; }  // the format as the scalar-loading kernels name it (msm_layout.h: narrow_width)
  int w_count_vec = 0;                // windows [w_begin, w_begin + w_count_vec) of every vector, in the request's window bits (MODE_WIDE: the T digits)
  int wide_bits = 0;                  // MODE_WIDE: the tables' digit width
  bool pairs = false;                 // MODE_WIDE, a share of the virtual windows: the launch leaves (window sum, plain total) record pairs
  uint32_t half = 0, ncoarse = 0;     // bucket slots per window; coarse bins that can hold entries
  int w_count = 0;                    // local windows (bucket sets) of the launch
  int nwin = 0, combine_bits = 0;     // host finish: window sums per MSM, and the bits between consecutive windows
  bool whole = false;                 // every vector's windows make a whole MSM that the host finish can combine
  size_t n_sc = 0, n_entries = 0;     // inputs of the recode; entries one local window may receive
  int full_windows = 0;               // local windows of one whole MSM in this mode: the sort arrays are sized for at least that many
  bool digits = false;                // the first pass keeps the digit planes for the debug read-back
  bool planes = false, share_shape = false, list_path = false;  // use_planes; the share kernels of the wide tables (k_scatter_wide<C, true>, k_scatter_list)
  uint32_t tiles = 0, tile_len = 0, subtiles = 0;  // tiles of scalars of the two global sort passes; LIST_SUB sub-tiles
  uint32_t chunks = 0, chunk_len = 0;              // SMVP chunks per local window and their (longest) length
  size_t stride = 0;                               // per-window stride of the entry arrays
  bool mask = false;                               // the bases hold identity records: the scalars are first copied with theirs zeroed (k_mask_identity)
  bool fine_hist = false;                          // written by the sort stage: it ran k_fine_hist
};

// Part policy of the upload-bound call shapes (msm_hip_msm_curve: bases + scalars from the host; msm_hip_run: scalars from the host): 0 = the default
// (MSM_HIP_ONESHOT_PARTS, else 2 parts from 2^19 points on); set by the test hook msm_hip_test_oneshot_parts
std::atomic<int> g_oneshot_parts{0};
std::atomic<size_t> g_oneshot_parts_min_n{0};
// `two_from`, `three_from`: log2 of the point counts from which the call shape runs 2 / 3 parts (measured: profiles/r05_oneshot.txt)
inline int env_oneshot_parts() {
  static const int v = [] { const char* e = getenv("MSM_HIP_ONESHOT_PARTS"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= 4 ? v : 0; }();
  return v;
}
// what the last upload-bound call ran as (test hook msm_hip_test_env_report): its parts, and the most upload chunks of one part (the one-shot call's
// overlapped upload; 0 for msm_hip_run)
std::atomic<int> g_probe_upload_parts{0}, g_probe_upload_chunks{0};
inline int upload_parts(size_t n, int cap, int two_from, int three_from) {
  const int env_parts = env_oneshot_parts();
  const int hook = g_oneshot_parts.load();
  const size_t hook_n = g_oneshot_parts_min_n.load();
  int want = hook ? hook : env_parts;
  if (!want) want = n >= ((size_t)1 << three_from) ? 3 : 2;
  if (want > cap) want = cap;
  const size_t min_n = hook_n ? hook_n : ((size_t)1 << two_from);
  return n >= min_n && n >= (size_t)want ? want : 1;
}

// entries per SMVP lane: about SMVP_TARGET_LANES lanes over all windows of the run, within the kernel's limits
inline size_t target_lanes() {  // MSM_HIP_TARGET_LANES overrides the default for tuning experiments
  static const size_t v = [] {
    const char* e = getenv("MSM_HIP_TARGET_LANES");
    const long x = e ? atol(e) : 0;
    return x >= 1024 ? (size_t)x : (size_t)SMVP_TARGET_LANES;
  }();
  return v;
}
inline size_t num_cus();  // compute units of the current device (defined by msm_ctx.h, or by the CPU harness)
// The SMVP is bound by the multiplier, so a SIMD needs time proportional to (waves it is given) x (chunk length) however many of them are
// resident at once, and a workgroup puts one wave on each SIMD of its CU: the kernel takes  ceil(workgroups / CUs) x chunk length  (round 3
// sweep of the length at 2^20, profiles/r03_chunk_len_sweep.txt: a sawtooth of 6.5 % that this expression reproduces within 1 - 2 %).  Around the
// length that gives about SMVP_TARGET_LANES lanes (+- 25 %: the stitch's work follows the lane count) a length whose product is more than 1 % lower
// than the plain quotient's replaces it (2^20 with 8 or 16 windows: 32, exact, instead of 29: 1.5 % per MSM).  (What the shares of an 8-rank run gained this round -- 3.5 % per MSM at 7 x 2 windows per launch -- came
// from the quotient itself, 25, no longer being rounded up to a multiple of 4, 28.)  MSM_HIP_CHUNK_SEARCH=0: the plain quotient.
inline bool chunk_search() {
  static const bool v = [] { const char* e = getenv("MSM_HIP_CHUNK_SEARCH"); return !e || atoi(e) != 0; }();
  return v;
}
inline uint32_t chunk_len_for(size_t n, int w_count) {
  const bool search = chunk_search();
  size_t base = (n * (size_t)w_count + target_lanes() - 1) / target_lanes();
  if (base < (size_t)SMVP_CHUNK_MIN) base = SMVP_CHUNK_MIN;
  if (base > (size_t)SMVP_CHUNK_MAX) base = SMVP_CHUNK_MAX;
  if (!search || base <= (size_t)SMVP_CHUNK_MIN) return (uint32_t)base;
  const size_t cus = num_cus();
  auto cost = [&](size_t c) {
    const size_t groups = (size_t)w_count * (((n + c - 1) / c + 255) / 256);
    return (groups + cus - 1) / cus * c;
  };
  size_t lo = base - base / 4, hi = base + base / 4 + 1;
  if (lo < (size_t)SMVP_CHUNK_MIN) lo = SMVP_CHUNK_MIN;
  if (hi > (size_t)SMVP_CHUNK_MAX) hi = SMVP_CHUNK_MAX;
  // (only a length that is more than 1 % better than the plain quotient replaces it: the expression is a model, and a different lane count
  //  moves work between the SMVP and the stitch -- at 2^24, 512 instead of 456 is 0.2 % better by the model and 1.5 % slower measured)
  const size_t base_cost = cost(base);
  size_t best = base, best_cost = base_cost - base_cost / 100;
  for (size_t c = lo; c <= hi; c++) {
    const size_t k = cost(c);
    const size_t d = c > base ? c - base : base - c, bd = best > base ? best - base : base - best;
    if (k < best_cost || (best != base && k == best_cost && d < bd)) {
      best = c;
      best_cost = k;
    }
  }
  return (uint32_t)best;
}
inline uint32_t chunks_for(size_t n, uint32_t chunk_len) { return (uint32_t)((n + chunk_len - 1) / chunk_len); }
// head/tail piece records needed for any run over at most n points: w_count * chunks is largest at w_count = NWIN
inline size_t piece_records_for(size_t n) {
  size_t worst = 0;
  for (int w = 1; w <= NWIN; w++) {
    const size_t r = (size_t)w * chunks_for(n, chunk_len_for(n, w));
    if (r > worst) worst = r;
  }
  return worst;
}

inline size_t stride_for(size_t n) { return (n + 3) & ~(size_t)3; }

// The top digit of the wide tables' recode (sort_kernels.h: wide_digit), from the scalar field's modulus r (its top 64 bits, r >> 192):
// its largest value over the scalars below r -- (r - 1 + the recode's bias below the digit) >> P, P = the digit's position -- decides the shift
// (the largest that keeps the shifted digit within 2^(C-1)), and r / 2^P, the range of a uniform scalar's top digit, how many virtual windows
// the shifted digit spreads over.  A top digit that does not fit after all is rejected by the kernel, never mis-added.
inline uint64_t scalar_modulus_top64(int curve) {
  switch (curve) {
    case MSM_HIP_CURVE_BLS12_381:
    case MSM_HIP_CURVE_BLS12_381_G2: return 0x73eda753299d7d48ull;
    case MSM_HIP_CURVE_PALLAS:
    case MSM_HIP_CURVE_VESTA: return 0x4000000000000000ull;  // both moduli: 2^254 + (a 126-bit number)
    default: return 0x30644e72e131a029ull;                   // BN254's r, and its p (Grumpkin's scalar field): the same top 64 bits
  }
}
inline int wide_top_pos(int bits) { return bits * (wide_tables_of(bits) - 1); }  // bit position of the top digit: 240 / 238 / 252 / 247 / 240 at 16 .. 20 bits (>= 192)
inline uint32_t wide_top_max(int curve, int bits) {
  const uint64_t top = scalar_modulus_top64(curve);
  const int fb = wide_top_pos(bits) - 192;                   // fraction bits of `top` below the digit
  const uint64_t frac = top << (64 - fb);                    // (r mod 2^P) / 2^P as a 64-bit fraction, truncated
  // the bias below the digit / 2^P = 1/2 + 2^(-C-1) + 2^(-2C-1) + ... as a 64-bit fraction: every term of the series that has a bit there, + 2 units
  // for its tail and for the truncation of `frac` -- an UPPER bound (round 4 stopped after two terms + 2^20, which the third term, 2^(63-2C),
  // exceeds: right for the five moduli of this library, not a bound), so a width is at worst refused for a modulus on a carry boundary, never
  // accepted wrongly; tests/test_abi.py compares with the exact big-integer value for every curve and width
  uint64_t bias = 2;
  for (int sh = 63; sh >= 0; sh -= bits) bias += 1ull << sh;
  return (uint32_t)(top >> fb) + (frac + bias < frac ? 1u : 0u);               // + the carry into the digit
}
// Round 5: with INTERLEAVED virtual windows (sort_kernels.h: wide_key) the narrow top digit spreads over the windows by itself and is used as it
// is -- no shift.  (Round 4 shifted it by the largest amount that kept it within 2^(C-1), to spread it over contiguous magnitude ranges;
// MSM_HIP_WIDE_TOP_SHIFT still forces a shift for A/B runs: the kernels and the tables' last step honour it.)
inline int env_wide_top_shift() {  // tuning aid
  static const int v = [] { const char* e = getenv("MSM_HIP_WIDE_TOP_SHIFT"); return e ? atoi(e) : -1; }();
  return v;
}
inline int wide_top_shift(int curve, int bits) {
  const int forced = env_wide_top_shift();
  if (forced < 0) return 0;
  const uint32_t dmax = wide_top_max(curve, bits), half = 1u << (bits - 1);
  int s = 0;
  while (s + 1 < bits && s < forced && ((uint64_t)dmax << (s + 1)) <= half) s++;
  return s;
}
// Can the curve's scalars be recoded into C-bit digits at all?  The top digit is never negative and becomes a bucket magnitude, so it must not
// pass 2^(C-1): with 17-bit digits (15 x 17 = 255 bits) that holds for BN254, Grumpkin and -- just: their moduli are 2^254 + a 126-bit number, the
// top digit of their largest scalars is exactly 2^16 -- Pallas and Vesta, not for BLS12-381's modulus of 1.8 x 2^254.
inline bool wide_bits_fit(int curve, int bits) { return wide_top_max(curve, bits) <= (1u << (bits - 1)); }
// Digit width of the wide tables for a base set of n points (profiles/r04_wide_tables.txt, same-box A/Bs against the endomorphism mode).  What an
// MSM costs in the pipeline is sort + SMVP + the stitch / reduce work that runs beside the next launch, and the last grows with the bucket sets:
// 16 bits (16 additions per point like every other mode, but ONE bucket set: the 16-bit tables' shape behind these kernels' all-digits-at-once
// scatter) wins up to 2^16 points, where grouped launches and latencies are all stitch / reduce; 17 bits (15 additions per point, 2 bucket sets)
// up to 2^20 points (+4 % at 2^20), 20 bits (13 additions, 16 bucket sets) beyond (2^21: 372 - 380 against 366 - 369 MSM/s with 17 bits; +11 % over the
// endomorphism mode at 2^22, +18 % at 2^24), where the additions are
// all that counts.  19 bits (14 additions, 8 bucket sets; the 7-bit top digit makes <= 128
// giant buckets) lies between them at every size and serves the curve 17 bits cannot (BLS12-381); 18 bits (a 2-bit top digit: 3 giant buckets) loses everywhere.
// msm_hip_set_wide_bits / MSM_HIP_WIDE_BITS = 16 .. 20 override.  -1: the chosen width cannot hold the curve's scalars.
inline int env_wide_bits() {
  static const int v = [] { const char* e = getenv("MSM_HIP_WIDE_BITS"); const int v = e ? atoi(e) : 0; return v >= 16 && v <= 20 ? v : 0; }();
  return v;
}
inline int pick_wide_bits(const PlanInputs* ctx, size_t n) {
  const int forced = env_wide_bits();
  const int asked = ctx->wide_bits_choice ? ctx->wide_bits_choice : forced;  // msm_hip_set_wide_bits, then the environment
  if (asked) return wide_bits_fit(ctx->curve, asked) ? asked : -1;
  const int bits = n <= ((size_t)1 << 16) ? 16 : n <= ((size_t)1 << 20) ? 17 : 20;
  return wide_bits_fit(ctx->curve, bits) ? bits : 19;
}
// SMVP lanes and lengths of a wide fixed-base launch over n points (sort_kernels.h: k_count_wide).  For uniform scalars every virtual window
// receives (T - 1) n / VWIN entries from the T - 1 full digits, and the windows the shifted top digit reaches their share of its n more: the fullest
// window's expected count F sets the device's chunk length (smvp_chunk_len), so the lanes are planned for F (+ 0.4 % + 64 entries: its
// fluctuation is 0.07 % at 2^20) -- planned for the mean, the length the device settles on would be one entry more than the one the host
// searched for, 4 % at 2^20.  Skewed scalars spread any other way: the arrays' per-window stride (`worst`) and the longest chunk the
// device may pick (`host_len`) cover one window that holds everything.
struct WideShape {
  size_t worst;
  uint32_t chunk_len, chunks, host_len;
};
inline double wide_slack() {  // tuning aid
  static const double v = [] { const char* e = getenv("MSM_HIP_WIDE_SLACK_PCT"); return e ? atof(e) / 100.0 : 0.004; }();
  return v;
}
inline WideShape wide_shape(size_t n, int curve, int bits, int lwin) {  // (lwin local windows share the lanes: nvec whole MSMs x VWIN, or nvec shares x their virtual windows)
  const int WIDE_TABLES = wide_tables_of(bits), WIDE_VWIN = wide_vwin_of(bits);
  WideShape w;
  w.worst = n * (size_t)WIDE_TABLES;
  // interleaved virtual windows (sort_kernels.h: wide_key): consecutive magnitudes go to consecutive windows, so every digit -- the narrow top one
  // included -- spreads evenly: each window expects T n / VWIN entries (a forced top shift of s puts the top digit's n entries into every 2^s-th
  // window only)
  const int shift = wide_top_shift(curve, bits);
  const int top_windows = WIDE_VWIN >> (shift < bits - WBITS ? shift : bits - WBITS);
  const double slack = wide_slack();
  const double fullest = (double)n * (WIDE_TABLES - 1) / WIDE_VWIN + (double)n / (top_windows > 0 ? top_windows : 1);
  const size_t typ = (size_t)(fullest * (1.0 + slack)) + 64;
  w.chunk_len = chunk_len_for(typ, lwin);
  w.chunks = chunks_for(typ, w.chunk_len);
  w.host_len = (uint32_t)((w.worst + w.chunks - 1) / w.chunks);
  if (w.host_len < w.chunk_len) w.host_len = w.chunk_len;
  return w;
}

// Window size of a WHOLE-MSM launch (the reference hard-codes c = 16 for n >= 2^16, src/cuzk/msm.rs:79).
// Measured on MI355X (profiles/r02_window_bits_latency.txt): what a small MSM costs is the DEPTH of the bucket reduce (~50
// dependent group additions at ~7 us each), which does not shrink with the bucket count -- so smaller windows, which need more
// windows (19 at 14 bits, 22 at 12), only win while the accumulation itself is negligible: 12 bits up to 2^12 points
// (0.70 vs 0.80 ms latency, 0.34 vs 0.40 ms pipelined), 16 bits from 2^13 up; 14 bits never wins and is kept as an explicit
// choice for ONE MSM per launch (msm_hip_set_window_bits).
// Several whole MSMs per launch (the batch entry points; nvec > 1) are a different regime: 4 - 8 MSMs' bucket sets are stitched and
// reduced side by side, so the work per bucket counts, not the depth of one reduce -- 14 bits (a quarter of the buckets for a
// quarter more additions) wins up to 2^16 points, in both base modes (profiles/r02_window_bits_grouped.txt: 2^12 +41 %, 2^14 +29 %,
// 2^16 +6 % with the endomorphism; +45 % / +50 % / +27 % plain; 16 bits from 2^17 up).
// `nvec` whole MSMs must fit MAXLW local windows.  The window-sharding entry points always use 16-bit windows: their w_begin / w_end
// index the reference's 16 windows.
// (`nb`: narrow scalars of nb bytes -- the same choice, with their own window count)
inline int env_window_bits() {  // tuning aid
  static const int v = [] { const char* e = getenv("MSM_HIP_WINDOW_BITS"); return e ? atoi(e) : 0; }();
  return v;
}
inline int pick_window_bits(const PlanInputs* ctx, size_t n, int nvec, bool halves = false, int nb = 0) {
  const int forced = env_window_bits();
  int bits = ctx->window_bits ? ctx->window_bits : (forced == 12 || forced == 14 || forced == 16 ? forced : 0);
  if (!bits) bits = nvec > 1 ? (n <= ((size_t)1 << 16) ? 14 : 16) : (n <= ((size_t)1 << 12) ? 12 : 16);
  while (bits < 16 && nvec * (nb ? narrow_nwin_of(bits, nb) : nwin_of(bits, halves)) > MAXLW) bits += 2;
  return bits;
}

// Does a launch's second sort pass read digit planes left by the first (k_scatter_planes) instead of the scalars again?  Yes for window
// shares -- at most PLANES_MAX_W of a vector's windows (8 GPUs: 2 of 16, or 1 of 8 half-length windows): 2 B per (input, window) instead
// of 32 B per scalar, and no scalars held in registers.  Not for fixed-base tables (one bucket set per vector) and not while the debug
// read-back wants the planes in its own format.  MSM_HIP_PLANES_MAX_W overrides the limit (0: never; tuning aid).  Never for sparse launches
// (k_scatter_planes writes positions, not the entries' base indices), whatever the tuning aids say.
inline int planes_max_w() {
  static const int v = [] { const char* e = getenv("MSM_HIP_PLANES_MAX_W"); return e ? atoi(e) : 8; }();
  return v;
}
inline bool planes_whole() {  // A/B aid: whole MSMs too
  static const bool v = [] { const char* e = getenv("MSM_HIP_PLANES_WHOLE"); return e && e[0] == '1'; }();
  return v;
}
inline bool use_planes(const PlanInputs* ctx, LaunchMode mode, int w_count_vec, int wbits, bool sparse) {
  const int max_w = planes_max_w();
  const bool whole = planes_whole();
  if (sparse || mode == MODE_TABLES || mode == MODE_WIDE || mode == MODE_NARROW || ctx->debug) return false;
  if (whole) return true;
  return w_count_vec <= max_w && w_count_vec < nwin_of(wbits, mode == MODE_HALVES);
}

inline bool wide_share_lists() {  // MSM_HIP_WIDE_SHARE_LISTS=0: the two-pass shape of the wide tables' shares (A/B aid)
  static const bool v = [] { const char* e = getenv("MSM_HIP_WIDE_SHARE_LISTS"); return !e || atoi(e) != 0; }();
  return v;
}

constexpr size_t MAX_POINTS = (size_t)1 << 28;  // point indices carry the digit sign in bit 31; 2^28 keeps every per-window offset in u32

// (sparse: n entries, which may outnumber the bases -- their indices repeat)
int check_run_args(const PlanInputs* ctx, const void* scalars, size_t n, bool sparse = false) {
  if (!ctx || (!scalars && n) || n > MAX_POINTS) return MSM_HIP_ERR_INVALID_ARG;
  if (ctx->n_bases == 0 && n) return MSM_HIP_ERR_NO_BASES;
  if (n > ctx->n_bases && !sparse) return MSM_HIP_ERR_INVALID_ARG;
  return MSM_HIP_OK;
}

// The one place a launch request is checked and shaped
int plan_launch(const PlanInputs* ctx, const LaunchRequest& r, LaunchPlan& p) {
  const LaunchMode mode = r.mode;
  const size_t n = r.n;
  const int nvec = r.nvec, w_begin = r.w_begin, w_end = r.w_end, wbits = r.wbits;
  const bool merge = mode == MODE_TABLES, halves = mode == MODE_HALVES, wide = mode == MODE_WIDE;
  const bool pairs = wide && r.v_count != 0;
  const int nb = ctx && mode == MODE_NARROW ? narrow_bytes(ctx->scalar_format) : 0;
  if (const int rc = check_run_args(ctx, r.scalars, n, r.sparse)) return rc;
  // windows of one whole MSM in this mode, in the request's units (fixed-base tables: the 16, or wide_tables_of(C) = nwin_of(C), digits of a scalar)
  const int whole_windows = nb ? narrow_windows(wbits, nb) : merge ? NWIN : nwin_of(wbits, halves);
  if (r.sparse && (wide || (!r.indices && n) || nvec != 1 || r.sums_dev || r.base_off || w_begin != 0 || w_end != whole_windows)) return MSM_HIP_ERR_INVALID_ARG;
  if (!r.sparse && r.base_off + n > ctx->n_bases) return MSM_HIP_ERR_INVALID_ARG;
  if (r.slot < 0 || r.slot >= NSLOT || w_begin < 0 || w_end > whole_windows || w_begin >= w_end) return MSM_HIP_ERR_INVALID_ARG;
  // narrow scalars: whole MSMs only, over the plain records, from a pointer aligned to the scalar's size
  if (mode == MODE_NARROW && (!nb || w_begin != 0 || w_end != whole_windows || r.sums_dev || r.base_off || nvec * w_end > narrow_max_windows(nb) ||
                              (byte_windows(nb) && wbits != BYTE_WBITS) ||
                              reinterpret_cast<uintptr_t>(r.scalars) % (uintptr_t)nb)) return MSM_HIP_ERR_INVALID_ARG;
  if (wide && (nvec < 1 || w_begin != 0 || wbits != ctx->wide_bits || w_end != whole_windows)) return MSM_HIP_ERR_INVALID_ARG;
  if (wide && !pairs && (nvec * wide_vwin_of(ctx->wide_bits) > 24 || r.sums_dev)) return MSM_HIP_ERR_INVALID_ARG;
  if (pairs && (r.v_begin < 0 || r.v_count < 0 || r.v_begin + r.v_count > wide_vwin_of(ctx->wide_bits))) return MSM_HIP_ERR_INVALID_ARG;
  if (!wide && r.v_count) return MSM_HIP_ERR_INVALID_ARG;
  const int v_count = wide && !pairs ? wide_vwin_of(ctx->wide_bits) : r.v_count;
  const int w_count_vec = w_end - w_begin;
  // fixed-base tables (`merge`): the w_count_vec windows of a vector feed one bucket set -- one local window of up to n * w_count_vec entries per
  // vector -- whose entries index the tables (window w of point i = record w * n_bases + i).  Wide tables: the same indexing; each vector's bucket
  // set of 2^(C-1) slots is run as 2^(C-16) local ("virtual") windows of 2^15, into which the entries fall by the top bits of their digit's
  // magnitude (sort_kernels.h: k_count_wide).  Otherwise local window lw = v * w_count_vec + (w - w_begin).
  const int w_count = merge ? nvec : wide ? nvec * v_count : nvec * w_count_vec;
  if (nvec < 1 || w_count > MAXLW) return MSM_HIP_ERR_INVALID_ARG;

  p = LaunchPlan{};
  static_cast<LaunchRequest&>(p) = r;
  p.nb = nb;
  p.nb_signed = nb && narrow_signed(ctx->scalar_format);
  p.w_count_vec = w_count_vec;
  p.wide_bits = wide ? ctx->wide_bits : 0;
  p.v_count = v_count;
  p.pairs = pairs;
  p.wbits = wide ? WBITS : wbits;  // (everything behind the recode sees local windows of 16 bits)
  p.half = 1u << (p.wbits - 1);
  p.ncoarse = p.half / FINE;
  p.w_count = w_count;
  // fixed-base launches leave ONE sum per vector (every table already carries its power of two): nothing to combine but the copy
  p.nwin = merge ? 1 : wide ? v_count : whole_windows;
  p.combine_bits = byte_windows(nb) ? 8 : p.wbits;  // (byte windows: window j weighs 2^(8 j))
  p.whole = !pairs && w_count_vec == whole_windows;
  // endomorphism (`halves`): the recode runs over 2n halves of 16 B (the first pass splits the scalars) against 2n points -- P_i and, n_bases records
  // further on, phi(P_i) -- in half as many windows
  p.n_sc = halves ? 2 * n : n;
  p.n_entries = merge || wide ? n * (size_t)w_count_vec : p.n_sc;  // (wide: what ONE virtual window may receive)
  p.full_windows = wide ? wide_vwin_of(ctx->wide_bits) : merge ? 1 : whole_windows;  // local windows
  p.digits = ctx->debug && !merge && !wide && !byte_windows(nb);
  // window shares (a few of a scalar's windows per vector): the first pass leaves digit planes, the second reads them (k_scatter_planes)
  p.planes = use_planes(ctx, mode, w_count_vec, p.wbits, r.sparse);
  // shares of at most WIDE_SHARE_VWIN_MAX virtual windows of wide tables: the first pass leaves compact lists of the share's entries per sub-tile of
  // LIST_SUB scalars (k_count_wide_list / k_scatter_list); tiles are then whole sub-tiles.  MSM_HIP_WIDE_SHARE_LISTS=0: the two-pass shape (A/B aid)
  p.share_shape = pairs && v_count <= WIDE_SHARE_VWIN_MAX;
  p.list_path = p.share_shape && wide_share_lists();
  // tiles of scalars for the two global sort passes: >= 2048 scalars each, at most MAX_TILES of them
  const uint32_t tile_unit = p.list_path ? (uint32_t)LIST_SUB : 256u;
  p.tile_len = 2048;
  if ((p.n_sc + p.tile_len - 1) / p.tile_len > MAX_TILES) p.tile_len = (uint32_t)((((p.n_sc + MAX_TILES - 1) / MAX_TILES) + tile_unit - 1) / tile_unit * tile_unit);
  p.tiles = (uint32_t)((p.n_sc + p.tile_len - 1) / p.tile_len);
  p.subtiles = (uint32_t)((p.n_sc + LIST_SUB - 1) / LIST_SUB);
  if (wide) {
    const WideShape ws = wide_shape(n, ctx->curve, ctx->wide_bits, w_count);
    p.chunk_len = ws.host_len;  // (the longest the device may pick: smvp_chunk_len)
    p.chunks = ws.chunks;
  } else {
    p.chunk_len = chunk_len_for(p.n_entries, w_count);
    p.chunks = chunks_for(p.n_entries, p.chunk_len);
  }
  p.stride = stride_for(p.n_entries);
  p.mask = ctx->n_identity != 0;
  return MSM_HIP_OK;
}

// `r` (its n and nvec) as a WHOLE MSM on this context: the mode, window bits and windows that the scalar format, then the mode the bases are held in,
// give it -- narrow scalars, wide tables, 16-bit tables, the endomorphism, plain windows.  The one place that rule lives: the dense and the sparse
// entry points, the batch runners' group size (batch_group) and the one-shot call all ask here.
// Nothing to compute (n == 0: identity sums) is the plain 16-bit request whatever the format and the bases, and so is a request no mode has room
// for (nvec x 16 windows beyond MAXLW), which plan_launch then rejects -- as it rejects narrow and wide windows beyond their limits.
LaunchRequest whole_msm_request(const PlanInputs* ctx, LaunchRequest r) {
  if (r.n == 0) return r.windows(MODE_PLAIN, 0, NWIN);
  if (const int nb = narrow_bytes(ctx->scalar_format)) {  // over the plain records, which every base mode keeps
    const int wbits = byte_windows(nb) ? BYTE_WBITS : pick_window_bits(ctx, r.n, r.nvec, false, nb);
    return r.windows(MODE_NARROW, 0, narrow_windows(wbits, nb), wbits);
  }
  if (ctx->wide_bits) return r.wide(ctx->wide_bits, 0, 0);             // an MSM is 2^(C-16) local windows, of which a launch holds at most 24
  if (ctx->precomputed) return r.windows(MODE_TABLES, 0, NWIN);         // one bucket set per vector
  if (ctx->endo && r.nvec * nwin_of(16, true) <= MAXLW) {  // half-length scalars over 2n points
    const int wbits = pick_window_bits(ctx, r.n, r.nvec, true);
    return r.windows(MODE_HALVES, 0, nwin_of(wbits, true), wbits);
  }
  const int wbits = r.nvec * NWIN <= MAXLW ? pick_window_bits(ctx, r.n, r.nvec) : WBITS;
  return r.windows(MODE_PLAIN, 0, nwin_of(wbits), wbits);
}

// MSMs per launch of the batch runners: small MSMs cannot fill the GPU one at a time (kernel latencies dominate below
// ~2^19 points), so up to MAXLW / NWIN = 4 of them -- at most about 2^20 points together -- share one kernel sequence
size_t batch_group(const PlanInputs* ctx, size_t n, size_t batch) {
  // 4 at 16 bits, 3 at 14, 2 at 12 (8 / 6 / 5 with the endomorphism's half-length scalars); with fixed-base tables every MSM is one local window
  // (window size of a grouped launch: pick_window_bits with nvec > 1)
  // (wide tables: an MSM is 2^(C-16) local windows, and its launch leaves bit-plane sums for at most 24 of them: 24 / 12 / 3 / 1 MSMs at 16 / 17 / 19 / 20 bits)
  // (narrow scalars: their own windows, over the plain records whatever the base mode)
  const LaunchRequest w = whole_msm_request(ctx, LaunchRequest(nullptr, n, 0, 2));  // (grouped: the window bits of nvec > 1)
  const int per_msm = w.mode == MODE_TABLES ? 1 : w.mode == MODE_WIDE ? wide_vwin_of(w.wbits) : w.w_end;  // local windows
  const int room = w.mode == MODE_NARROW ? narrow_max_windows(narrow_bytes(ctx->scalar_format)) : w.mode == MODE_WIDE ? 24 : MAXLW;
  const size_t fit = (size_t)(room / per_msm);
  size_t g = n ? ((size_t)1 << 20) / n : 1;
  if (g > fit) g = fit;
  if (g > batch) g = batch;
  return g ? g : 1;
}
}  // namespace
