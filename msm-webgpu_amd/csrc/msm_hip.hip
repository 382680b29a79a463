// libmsm_hip.so -- host side of the MI355X BN254 MSM engine behind the C ABI of include/msm_hip.h.
//
// Replaces, for the hot path only, the reference's orchestrator compute_msm (src/cuzk/msm.rs:75-417) and its wgpu
// wrappers (src/cuzk/gpu.rs): one persistent context = three HIP streams, pooled device buffers, bases resident in HBM
// in device Montgomery form; no per-call device creation, shader generation or pipeline compilation
// (cf. src/cuzk/msm.rs:88-94, src/cuzk/shader_manager.rs:74-100).
//
// Execution model.  Every launch (one MSM, or several scalar vectors sharing one kernel sequence: up to MAXLW local
// windows) runs in one of MSM_HIP_NUM_SLOTS result slots (own bucket, piece, col_ptr and window-sum buffers):
//   stream "main"   : recode + sort + SMVP accumulate                               -> event smvp_done[slot]
//   stream "reduce" : (waits smvp_done) stitch + bucket reduce -> window sums -> D2H -> event done[slot]
// The stitch and the bucket reduce are bound by the depth of dependent group additions and occupy few waves; putting them
// on their own stream lets the sort + SMVP of the NEXT launch (other slot) run meanwhile.  The host window combine of a
// slot (src/cuzk/msm.rs:411-416) runs in the caller's thread inside msm_hip_finish / msm_hip_finish_batch.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>

#define MSM_HIP_TEST_HOOKS 1
#include "../../include/msm_hip.h"
#include "curve_ops.h"
#include "host_fr.h"
#include "host_pool.h"
// the curve-neutral recode and sort, compiled here once for every curve; each curve's own kernels are a translation unit of their own (curve_ops.h)
#include "sort_kernels.h"

using namespace msm_layout;
using namespace msm_sort;

namespace {
// curve id (MSM_HIP_CURVE_*) -> its table
inline const CurveOps* curve_ops(int curve) {
  switch (curve) {
    case MSM_HIP_CURVE_BN254_G1: return msm_hip_curve_ops_bn254();
    case MSM_HIP_CURVE_GRUMPKIN: return msm_hip_curve_ops_grumpkin();
    case MSM_HIP_CURVE_PALLAS: return msm_hip_curve_ops_pallas();
    case MSM_HIP_CURVE_VESTA: return msm_hip_curve_ops_vesta();
    case MSM_HIP_CURVE_BLS12_381: return msm_hip_curve_ops_bls12_381();
    case MSM_HIP_CURVE_BN254_G2: return msm_hip_curve_ops_bn254_g2();
    case MSM_HIP_CURVE_BLS12_381_G2: return msm_hip_curve_ops_bls12_381_g2();
    default: return nullptr;  // (every entry point checks the curve id first)
  }
}

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

constexpr int N_MAIN_EVENTS = 7;  // boundaries of the 6 timed stages on the main stream
constexpr uint32_t MAX_TILES = 1024;
constexpr size_t MAX_JB = 288;  // the largest Jacobian record of any curve (BLS12-381 G2: 3 x 96 B; BN254 G2: 3 x 64 B; BLS12-381 G1: 3 x 48 B; the 254 / 255-bit G1 curves: 96 B)
constexpr size_t WSUM_BYTES = (size_t)24 * PLANES_PER_WINDOW * MAX_JB;  // MAXLW window sums or, for one host-combined MSM, the bit-plane sums (k_bpr_planes) of its <= 22 windows
static_assert(WSUM_BYTES >= (size_t)2 * MAXLW * MAX_JB, "window-sum buffer (pairs of records for shares of the wide tables' virtual windows)");
constexpr int NSLOT = MSM_HIP_NUM_SLOTS;  // result slots
constexpr int NREDUCE = 2;  // reduce streams (slot k uses stream k % NREDUCE): two bucket reduces may be in flight when the
                            // main-stream work of one MSM is shorter than its bucket reduce (few windows per GPU).  The context
                            // then owns 3 streams; streams beyond the process's hardware queues (GPU_MAX_HW_QUEUES) share
                            // them: correct, with less overlap.

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

struct Slot {
  uint8_t* h_wsums = nullptr;      // pinned: MAXLW x 96 B window sums + 4 B error word
  uint8_t* d_wsums = nullptr;      // device: MAXLW x 96 B window sums + 4 B error word
  uint32_t* d_buckets = nullptr;   // [cap_lw][32768] XYZZ records
  size_t cap_buckets = 0;          // bucket records d_buckets holds (local windows x slots per window of the largest launch seen)
  uint32_t* d_partials = nullptr;  // bucket-reduce scratch: [W][256] row sums, [W][256] column sums, [W][3] parts (XYZZ)
  uint32_t* d_col_ptr = nullptr;   // [W][32769] start of every bucket slot's run in the sorted entry list
  uint32_t* d_heads = nullptr;     // [W][chunks] XYZZ records: SMVP pieces of runs that cross chunk boundaries
  uint32_t* d_tails = nullptr;     // [W][chunks] XYZZ records
  uint32_t* d_big_queue = nullptr;    // buckets with many pieces (skewed scalars): [0] = count, items, arrival counters, scratch records (BIGQ_*)
  hipEvent_t ev[N_MAIN_EVENTS] = {};
  hipEvent_t red0 = nullptr, red1 = nullptr;  // bucket reduce begin / end on the reduce stream
  hipEvent_t smvp_done = nullptr;             // main -> reduce hand-off
  hipEvent_t done = nullptr;                  // everything of this slot finished (recorded on the reduce stream)
  hipEvent_t staged = nullptr;                // host scalars of this slot have landed in d_host_scalars (copy stream)
  uint32_t* d_host_scalars = nullptr;         // staging of msm_hip_launch's host scalars (this slot's own: no launch of
  size_t cap_host_scalars = 0;                // another slot can still be reading it), in scalars; allocated on first use
  size_t cap_recs = 0;                        // capacity (records) of d_heads / d_tails
  bool ready = false;                         // small buffers + events exist (slots are set up on first use)
  bool timed = false, pending = false, to_host = false;
  bool parts = false;                         // h_wsums holds the bit-plane sums of every window (k_bpr_planes): the host finishes the window sums
  int timing_level = 0;
  LaunchPlan plan;                            // the launch in this slot
};

}  // namespace

namespace {
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
}  // namespace

struct msm_hip_ctx {
  int device = 0;
  int curve = MSM_HIP_CURVE_BN254_G1;
  const CurveOps* ops = nullptr;
  size_t cb = 32, pb = 64, jb = 96;     // bytes of a coordinate, an affine point and a Jacobian record on this curve's wire (48 / 96 / 144: BLS12-381)
  hipStream_t stream = nullptr;         // main
  hipStream_t reduce_stream[NREDUCE] = {};  // bucket reduce + result copies
  int last_hip_error = 0;

  uint32_t* d_bases = nullptr;  // n_bases x 16 words
  size_t n_bases = 0, cap_bases = 0;  // points per table; capacity in point records (16 x n_bases with fixed-base tables)
  bool precomputed = false;           // d_bases holds the 16 tables 2^(16 w) P_i (MSM_HIP_BASES_PRECOMPUTE)
  int wide_bits_choice = 0;           // msm_hip_set_wide_bits: the digit width the next wide base set gets (0: by the number of bases)
  int wide_bits = 0;                  // != 0: d_bases holds the wide tables 2^(C w) P_i for C-bit digits (MSM_HIP_BASES_PRECOMPUTE_WIDE; pick_wide_bits)
  bool endo = false;                  // d_bases holds phi(P_i) behind the n bases (MSM_HIP_BASES_ENDOMORPHISM)
  uint64_t* d_id_bits = nullptr;      // MSM_HIP_BASES_ZERO_IS_IDENTITY: bit i = base i is the identity (ceil(n / 64) words; k_convert_points_zero_id)
  size_t cap_id_bits = 0;             // in words
  size_t n_identity = 0;              // identity records among the resident bases: nonzero -> every launch masks its scalars (k_mask_identity)
  uint32_t* d_halves = nullptr;       // the split scalars of one launch (main stream only): [vector][2n] x 4 words
  size_t cap_halves = 0;              // in scalars

  hipStream_t copy_stream = nullptr;    // H2D of host scalars (created on first use by msm_hip_launch)
  hipEvent_t input_ready = nullptr;     // a caller's producer stream -> main stream (msm_hip_wait_stream)
  hipEvent_t bases_ready = nullptr;     // the one-shot entry point: the last chunk of the bases has been converted (conversion stream -> main stream)
  hipEvent_t chunk_landed[8] = {};      // ... and chunk k of the wire bytes has landed (copy stream -> conversion stream)
  size_t cap_entries = 0;  // capacity of the entry arrays (tmp_val, tmp_fine, val): local windows x per-window stride
  size_t cap_chunk_slot = 0;  // capacity (records) of d_chunk_slot
  uint8_t* d_batch_stage = nullptr;   // staging ring (NSLOT vectors) of msm_hip_run_batch, allocated on first use
  size_t cap_batch_stage = 0;
  uint16_t* d_digits = nullptr;  // digit-code planes [local window][n]: debug read-back, or the input of the second sort pass (k_scatter_planes)
  uint64_t* d_negbits = nullptr; // with the planes of a launch: one sign bit per input of every vector
  size_t cap_planes = 0;         // capacity (u16 entries) of d_digits; d_negbits holds cap_planes / 64 + 2 MAXLW words
  bool debug = false;
  int timing_level = 2;  // 0: no stage events, 1: only around the SMVP kernel, 2: every stage boundary
  uint32_t* d_counts = nullptr;      // [W][tiles][128]
  uint32_t* d_bin_total = nullptr;   // [W][128]
  uint32_t* d_bin_fill = nullptr;    // [W][128] the same for launches whose first pass is k_count, which fills it with atomics: zero between launches (k_sort_fine)
  bool bin_fill_dirty = true;        // ... unless a launch was abandoned between the two: the next one clears it first
  uint32_t* d_coarse_ptr = nullptr;  // [W][129]
  uint32_t* d_tmp_val = nullptr;     // [W][stride] coarse-bin order
  uint8_t* d_tmp_fine = nullptr;     // [W][stride]
  uint32_t* d_val = nullptr;         // [W][stride] slot order
  uint32_t* d_chunk_slot = nullptr;  // [W][chunks] bucket slot of every SMVP chunk's first entry
  uint32_t* d_list_len = nullptr;    // shares of the wide tables' virtual windows: [W][sub-tiles] lengths of the first pass's compact entry lists (k_count_wide_list)
  size_t cap_list_len = 0;
  uint32_t* d_scalar_conv = nullptr;  // canonical copies of scalars handed over in R = 2^256 Montgomery form (one launch's worth); behind them, a
                                      // masked launch's copy of its scalars with those of identity bases zeroed (k_mask_identity)
  size_t cap_scalar_conv = 0;         // in 32-byte scalars
  uint32_t scalar_format = 0;         // MSM_HIP_SCALARS_CANONICAL / MONT256 / U8 .. U64 / MSM_HIP_SCALAR_U128 [| MSM_HIP_SCALAR_SIGNED] (read by each launch)
  int window_bits = 0;                // 0: chosen from n for whole-MSM launches (pick_window_bits); else 12 / 14 / 16
  uint32_t* d_part_hist = nullptr;  // [MAXLW][128][FINE_SPLIT][256] sub-range histograms of huge coarse bins (k_fine_hist), on first use
  size_t fine_hist_min_n = FINE_BIG + 1;  // any n that can produce a coarse bin beyond FINE_BIG: run k_fine_hist (3 us when none does)
  int skew_credit = 0;  // launches left for which k_fine_hist runs although uniform scalars could not fill a bin: set when a launch met a huge bin (wait_slot)
  uint32_t* d_err = nullptr;
  uint8_t* d_stage = nullptr;  // staging for host byte inputs of set_bases / test hooks
  size_t cap_stage = 0;
  uint32_t* d_mul = nullptr;   // batch scalar multiplication (msm_hip_mul_each / msm_hip_mul_base): one tile's Z values, prefix products, converted and
  size_t cap_mul = 0;          // masked scalars and, for the host entry points, staged scalars and output; in words
  uint32_t* d_mul_table = nullptr;  // msm_hip_mul_base's fixed-base table T_w[j] = j 2^(C w) P_base (packed Montgomery records); in words
  size_t cap_mul_table = 0;
  int mul_table_bits = 0;      // C of the table held (0: none), of base mul_table_base, built by the ladder mul_table_endo: the cache key.  set_bases drops it
  size_t mul_table_base = 0;
  bool mul_table_endo = false;
  size_t mul_policy_min_n = 0; // test hook msm_hip_test_mul_policy: != 0: the table runs exactly when n >= this (SIZE_MAX: never) ...
  int mul_policy_bits = 0;     // ... != 0: with this digit width
  int mul_last_bits = 0;       // the last call's table digit width (0: a ladder)
  int mul_force_ladder = 0;    // test hook msm_hip_test_mul_ladder: 0 the policy, 1 always the plain ladder, 2 the endomorphism's wherever the curve has one
  int mul_last_path = 0;       // what the last such call ran (test hook msm_hip_test_mul_last): 0 nothing, 1 the plain ladder, 2 the endomorphism ladder, 3 the table as cached, 4 the table, built by this call
  uint32_t* d_fft = nullptr;   // group FFT over the resident bases (msm_hip_bases_fft): n Montgomery point records, their Z values and prefix products, the
  size_t cap_fft = 0;          // broadcast scalar and, for the host entry point, the staged output; in words
  uint32_t* d_fft_tw = nullptr;  // ... its twiddles omega^j, j < n / 2 (canonical, 8 words each), cached under the key (fft_tw_log_n, fft_tw_omega): they do
  size_t cap_fft_tw = 0;         // not depend on the bases.  In words
  int fft_tw_log_n = 0;          // (0: no table held)
  uint8_t fft_tw_omega[32] = {};
  int fft_last_stages = 0;     // the last such call (test hook msm_hip_test_fft_last): butterfly stages run, and the ladder of its twiddled stages and of the
  int fft_last_ladder = 0;     // scale pass: 0 none ran, 1 the plain ladder, 2 the endomorphism's

  Slot slot[NSLOT];
  LaunchPlan last;  // the last launch that enqueued kernels, and its slot (for the stage read-back hooks)
  int last_slot = 0;
  int last_logr = 0;                // ... the LOG_R of its k_bpr_rowcol variant (pick_rowcol), and whether its stitch + reduce ran on the main stream
  bool last_inline_reduce = false;  //     (test hook msm_hip_test_env_report)
  float stage_ms[10] = {};
};

namespace {

#define HIP_TRY(ctx, expr)                                                             \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      if (ctx) (ctx)->last_hip_error = (int)e_;                                        \
      return e_ == hipErrorOutOfMemory ? MSM_HIP_ERR_OUT_OF_MEMORY : MSM_HIP_ERR_HIP; \
    }                                                                                  \
  } while (0)

template <typename T>
int dev_alloc(msm_hip_ctx* ctx, T*& p, size_t count) {
  if (p) {
    (void)hipFree(p);
    p = nullptr;
  }
  HIP_TRY(ctx, hipMalloc((void**)&p, count * sizeof(T)));
  return MSM_HIP_OK;
}

// Grow a pooled buffer set of capacity `cap` (in the caller's unit) to `size`: `alloc(size)` (re)allocates every buffer of the set, and `cap` reads 0
// until all of them exist.  `sync`: a context-wide set that the main stream may still be using -- wait for it first.
template <typename Alloc>
int grow(msm_hip_ctx* ctx, size_t& cap, size_t size, bool sync, Alloc alloc) {
  if (size <= cap) return MSM_HIP_OK;
  if (sync) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  cap = 0;
  if (const int rc = alloc(size)) return rc;
  cap = size;
  return MSM_HIP_OK;
}

int ensure_stage(msm_hip_ctx* ctx, size_t bytes) {
  return grow(ctx, ctx->cap_stage, bytes, false, [&](size_t c) { return dev_alloc(ctx, ctx->d_stage, c); });
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
// compute units of the current device (the devices of a node are alike: asked once)
inline size_t num_cus() {
  static const size_t v = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) return (size_t)cus;
    return (size_t)256;
  }();
  return v;
}
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
inline int pick_wide_bits(const msm_hip_ctx* ctx, size_t n) {
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

// RAII: every ABI entry point runs on its context's device and leaves the caller's current device as it found it
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = prev == device || hipSetDevice(device) == hipSuccess;
    if (prev == device) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(ctx)                     \
  DeviceGuard device_guard_((ctx)->device); \
  if (!device_guard_.ok) return MSM_HIP_ERR_NO_DEVICE

// first use of a result slot: its events and small buffers (the big ones -- buckets, pieces -- follow in ensure_work).
// Slots are set up lazily so that a context that only ever runs one MSM at a time (the reference's call shape,
// src/cuzk/msm.rs:75-94: create, run once, destroy) allocates one slot's worth of memory, not four.
int setup_slot(msm_hip_ctx* ctx, Slot& s) {
  if (s.ready) return MSM_HIP_OK;
  int rc;
  if (!s.h_wsums) {
    HIP_TRY(ctx, hipHostMalloc((void**)&s.h_wsums, WSUM_BYTES + 4, hipHostMallocDefault));
    memset(s.h_wsums, 0, WSUM_BYTES + 4);
  }
  if ((rc = dev_alloc(ctx, s.d_wsums, WSUM_BYTES + 4))) return rc;
  if ((rc = dev_alloc(ctx, s.d_partials, (size_t)MAXLW * (256 + 256 + PLANES_PER_WINDOW) * ctx->ops->xyzz_words))) return rc;
  if ((rc = dev_alloc(ctx, s.d_col_ptr, (size_t)MAXLW * (HALF + 1)))) return rc;
  if ((rc = dev_alloc(ctx, s.d_big_queue, BIGQ_SCRATCH + (size_t)STITCH_BLOCKS * ctx->ops->rec_words))) return rc;
  // zeroed on the stream that first reads them (the slot's reduce stream; the error word is first written on the main
  // stream, which waits for `done` below) -- not on the null stream, which the non-blocking streams do not order with
  hipStream_t rs = ctx->reduce_stream[(&s - ctx->slot) % NREDUCE];
  HIP_TRY(ctx, hipMemsetAsync(s.d_wsums, 0, WSUM_BYTES + 4, rs));
  HIP_TRY(ctx, hipMemsetAsync(s.d_big_queue, 0, 4, rs));
  HIP_TRY(ctx, hipMemsetAsync(s.d_big_queue + BIGQ_COUNTERS, 0, (size_t)STITCH_BLOCKS * 4, rs));
  if (!s.done) HIP_TRY(ctx, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  if (!s.smvp_done) HIP_TRY(ctx, hipEventCreateWithFlags(&s.smvp_done, hipEventDisableTiming));
  if (!s.staged) HIP_TRY(ctx, hipEventCreateWithFlags(&s.staged, hipEventDisableTiming));
  if (!s.red0) HIP_TRY(ctx, hipEventCreate(&s.red0));
  if (!s.red1) HIP_TRY(ctx, hipEventCreate(&s.red1));
  for (int i = 0; i < N_MAIN_EVENTS; i++)
    if (!s.ev[i]) HIP_TRY(ctx, hipEventCreate(&s.ev[i]));
  HIP_TRY(ctx, hipEventRecord(s.done, rs));  // the first launch into the slot waits for the memsets through this event
  s.ready = true;
  return MSM_HIP_OK;
}

// make the pools fit launch `p` into slot `s` (set up, not pending).  The sort arrays are sized for at least one whole MSM in the launch's mode
// (p.full_windows) over up to p.n_entries entries per window.
int ensure_work(msm_hip_ctx* ctx, const LaunchPlan& p, Slot& s) {
  int rc;
  const size_t n = p.n_entries;
  const size_t need_recs = (size_t)p.w_count * p.chunks;
  const size_t need_entries = p.stride * (size_t)p.w_count;
  const size_t entries = std::max(p.stride * (size_t)p.full_windows, need_entries);  // any single MSM over up to n entries per window
  if ((p.planes || ctx->debug) && need_entries > ctx->cap_planes &&  // digit planes (main stream only, like the sort arrays)
      (rc = grow(ctx, ctx->cap_planes, std::max(entries, ctx->cap_entries), true, [&](size_t c) {
         const int r = dev_alloc(ctx, ctx->d_digits, c);
         return r ? r : dev_alloc(ctx, ctx->d_negbits, c / 64 + 2 * MAXLW);
       })))
    return rc;
  if (need_entries > ctx->cap_entries || need_recs > ctx->cap_chunk_slot) {
    // growing the context-wide sort arrays (main stream only): nothing may still be running on them
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = grow(ctx, ctx->cap_entries, entries, false, [&](size_t c) {
           int r = dev_alloc(ctx, ctx->d_tmp_val, c);
           if (!r) r = dev_alloc(ctx, ctx->d_tmp_fine, c);
           return r ? r : dev_alloc(ctx, ctx->d_val, c);
         })))
      return rc;
    if ((rc = grow(ctx, ctx->cap_chunk_slot, std::max(piece_records_for(n), need_recs), false, [&](size_t c) { return dev_alloc(ctx, ctx->d_chunk_slot, c); })))
      return rc;
  }
  if (need_recs > s.cap_recs &&  // this slot's piece arrays (the slot is idle: its previous occupant was collected)
      (rc = grow(ctx, s.cap_recs, std::max(piece_records_for(n), need_recs), false, [&](size_t c) {
         const int r = dev_alloc(ctx, s.d_heads, c * ctx->ops->rec_words);
         return r ? r : dev_alloc(ctx, s.d_tails, c * ctx->ops->rec_words);
       })))
    return rc;
  const size_t need_buckets = (size_t)p.w_count << (p.wbits - 1);
  if (need_buckets > s.cap_buckets &&  // one MSM's worth (16 x 2^15 at 16 bits) at least; larger launches grow it
      (rc = grow(ctx, s.cap_buckets, std::max((size_t)NWIN * HALF, need_buckets), false, [&](size_t c) { return dev_alloc(ctx, s.d_buckets, c * ctx->ops->rec_words); })))
    return rc;
  if (n >= ctx->fine_hist_min_n && !ctx->d_part_hist) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = dev_alloc(ctx, ctx->d_part_hist, (size_t)MAXLW * NCOARSE * FINE_SPLIT * FINE))) return rc;
  }
  const size_t scalars = (size_t)p.nvec * p.n;
  if (p.pairs &&  // the list lengths of a share's first pass
      (rc = grow(ctx, ctx->cap_list_len, (size_t)p.w_count * p.subtiles, true, [&](size_t c) { return dev_alloc(ctx, ctx->d_list_len, c); })))
    return rc;
  if (p.mode == MODE_HALVES && !p.planes &&  // (the halves as an array: only when the second pass reads them)
      (rc = grow(ctx, ctx->cap_halves, scalars, true, [&](size_t c) { return dev_alloc(ctx, ctx->d_halves, c * 8); })))
    return rc;
  // canonical copies of MONT256 scalars, and behind them a masked launch's copy of its scalars (any width: nb bytes each, 32 for the 32-byte formats)
  const size_t conv = (ctx->scalar_format == MSM_HIP_SCALARS_MONT256 && !p.nb ? scalars : 0) + (p.mask ? (scalars * (p.nb ? p.nb : 32) + 31) / 32 : 0);
  if (conv && (rc = grow(ctx, ctx->cap_scalar_conv, conv, true, [&](size_t c) { return dev_alloc(ctx, ctx->d_scalar_conv, c * 8); })))
    return rc;
  return MSM_HIP_OK;
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
inline int pick_window_bits(const msm_hip_ctx* ctx, size_t n, int nvec, bool halves = false, int nb = 0) {
  const int forced = env_window_bits();
  int bits = ctx->window_bits ? ctx->window_bits : (forced == 12 || forced == 14 || forced == 16 ? forced : 0);
  if (!bits) bits = nvec > 1 ? (n <= ((size_t)1 << 16) ? 14 : 16) : (n <= ((size_t)1 << 12) ? 12 : 16);
  while (bits < 16 && nvec * (nb ? narrow_nwin_of(bits, nb) : nwin_of(bits, halves)) > MAXLW) bits += 2;
  return bits;
}

// MSM_HIP_DEBUG_SYNC=1 (diagnostic): wait after every kernel of a launch and name it on stderr, so that a device fault is
// pinned to a kernel.  Destroys all overlap; never set for measurements.
inline bool debug_sync() {
  static const bool v = [] { const char* e = getenv("MSM_HIP_DEBUG_SYNC"); return e && e[0] == '1'; }();
  return v;
}
#define AFTER_KERNEL(ctx, name, stream)                                   \
  do {                                                                    \
    if (debug_sync()) {                                                   \
      fprintf(stderr, "[msm_hip] %s ...", name);                          \
      fflush(stderr);                                                     \
      hipError_t e_ = hipStreamSynchronize(stream);                       \
      fprintf(stderr, " %s\n", e_ == hipSuccess ? "ok" : hipGetErrorString(e_)); \
      fflush(stderr);                                                     \
      if (e_ != hipSuccess) {                                             \
        (ctx)->last_hip_error = (int)e_;                                  \
        return MSM_HIP_ERR_HIP;                                           \
      }                                                                   \
    }                                                                     \
  } while (0)

inline unsigned blocks_for(size_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

int err_from_bits(uint32_t bits) {
  if (bits & ERRBIT_NOT_ON_CURVE) return MSM_HIP_ERR_NOT_ON_CURVE;
  if (bits & (ERRBIT_NONCANONICAL | ERRBIT_SCALAR_CARRY)) return MSM_HIP_ERR_NONCANONICAL;
  if (bits & ERRBIT_BAD_INDEX) return MSM_HIP_ERR_INVALID_ARG;  // a sparse launch's device index was out of range (it counted as a zero scalar)
  return MSM_HIP_OK;
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
inline bool use_planes(const msm_hip_ctx* ctx, LaunchMode mode, int w_count_vec, int wbits, bool sparse) {
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
int check_run_args(msm_hip_ctx* ctx, const void* scalars, size_t n, bool sparse = false) {
  if (!ctx || (!scalars && n) || n > MAX_POINTS) return MSM_HIP_ERR_INVALID_ARG;
  if (ctx->n_bases == 0 && n) return MSM_HIP_ERR_NO_BASES;
  if (n > ctx->n_bases && !sparse) return MSM_HIP_ERR_INVALID_ARG;
  return MSM_HIP_OK;
}

// The one place a launch request is checked and shaped
int plan_launch(msm_hip_ctx* ctx, const LaunchRequest& r, LaunchPlan& p) {
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
LaunchRequest whole_msm_request(const msm_hip_ctx* ctx, LaunchRequest r) {
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

// f(std::integral_constant<decltype(V), V>{}) for the V among V0, Vs... that equals the runtime value `v` -- the last one for any other value:
// a kernel template is instantiated for exactly the values listed
template <auto V0, auto... Vs, typename F>
void dispatch(decltype(V0) v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<decltype(V0), V0>{});
  else if (v == V0) f(std::integral_constant<decltype(V0), V0>{});
  else dispatch<Vs...>(v, f);
}

// The launch's first stage, on the main stream: everything that needs the scalars alone -- recode, the two sort passes and the fine sort (+ the
// debug read-back's ordering).  The slot's previous occupant (bucket reduce + copies on the reduce stream) must have drained; its error word was
// re-zeroed at the end of that chain.  Stage events cost a few microseconds of queue time each, so only the ones the current timing level asks
// for are recorded.
int enqueue_sort(msm_hip_ctx* ctx, LaunchPlan& p, Slot& s, const uint32_t* d_scalars) {
  const bool merge = p.mode == MODE_TABLES, halves = p.mode == MODE_HALVES, wide = p.mode == MODE_WIDE;
  const bool bytes = byte_windows(p.nb);  // U8 / U16, I8 / I16: byte windows with their own one-level sort (sort_kernels.h: k_byte_count ...)
  const size_t merge_nb = merge || wide ? ctx->n_bases : 0;
  hipStream_t st = ctx->stream;
  const dim3 grid(p.tiles, p.nvec), block(256);
  uint32_t* d_err = reinterpret_cast<uint32_t*>(s.d_wsums + WSUM_BYTES);
  // the SMVP chunk length the device settles on for this launch (k_scatter_coarse -> fine sort, SMVP, stitch): a word of the slot
  uint32_t* d_chunk_len = s.d_big_queue + BIGQ_CHUNK_LEN;
  const int tl = ctx->timing_level;
  auto mark = [&](int i) { return tl >= 2 ? hipEventRecord(s.ev[i], st) : hipSuccess; };
  HIP_TRY(ctx, hipStreamWaitEvent(st, s.done, 0));
  HIP_TRY(ctx, mark(0));
  const bool mont = ctx->scalar_format == MSM_HIP_SCALARS_MONT256 && !p.nb;
  if (p.mask) {  // identity records among the bases: a copy of the scalars with theirs zeroed, before anything validates or converts them (stage 0)
    uint8_t* masked = reinterpret_cast<uint8_t*>(ctx->d_scalar_conv) + (mont ? (size_t)p.nvec * p.n * 32 : 0);  // (behind the canonical copies)
    dispatch<32, 16, 8, 4, 2, 1>(p.nb ? p.nb : 32, [&](auto w) {  // (by width: zeroing does not ask about the sign)
      hipLaunchKernelGGL(k_mask_identity<decltype(w)::value>, dim3(blocks_for(p.n, 256), p.nvec), dim3(256), 0, st, (const uint8_t*)d_scalars, masked, p.n,
                         p.base_off, (const uint64_t*)ctx->d_id_bits, (uint32_t)ctx->n_bases, p.sparse ? p.indices : (const uint32_t*)nullptr);
    });
    AFTER_KERNEL(ctx, "k_mask_identity", st);
    d_scalars = reinterpret_cast<const uint32_t*>(masked);
  }
  if (mont) {  // Montgomery-form scalars: canonical copies first (part of stage 0)
    const size_t count = (size_t)p.nvec * p.n;
    hipLaunchKernelGGL(ctx->ops->scalars_from_mont256, dim3(blocks_for(count, 256)), dim3(256), 0, st, d_scalars, ctx->d_scalar_conv, count, d_err);
    AFTER_KERNEL(ctx, "k_scalars_from_mont256", st);
    d_scalars = ctx->d_scalar_conv;
  }
  const unsigned gpos_bytes = (unsigned)(merge ? p.nvec : p.nvec * p.w_count_vec) * NCOARSE * 4;  // k_scatter_coarse's run cursors (dynamic LDS)
  const int top_shift = wide ? wide_top_shift(ctx->curve, p.wide_bits) : 0;
  // inputs of the two-level sort: 32-byte scalars (8 words) or the endomorphism's halves (4), or narrow scalars of 4 / 8 / 16 bytes (1 / 2 / 4
  // words), unsigned or signed.  f(C, SW, NB) for the kernel parameters of this launch.
  const int sw = halves ? 4 : 8;
  auto sort_input = [&](auto f) {
    dispatch<16, 14, 12>(p.wbits, [&](auto c) {
      dispatch<4, 8, 16, -4, -8, -16, 0>(p.nb_kernel(), [&](auto b) {
        constexpr int NB = decltype(b)::value;
        if constexpr (NB != 0) f(c, std::integral_constant<int, (narrow_width(NB) + 3) / 4>{}, b);
        else dispatch<8, 4>(sw, [&](auto w) { f(c, w, b); });
      });
    });
  };
  // first pass: recode + coarse histogram (+ digit planes: 1 = debug read-back, 2 = the second pass reads them).  Endomorphism launches:
  // the same kernel splits every scalar k = k1 + k2 lambda itself and leaves the halves (interleaved: input 2 j = k1 of scalar j, 2 j + 1 =
  // k2; a vector's 2n halves take the room of its n scalars, vector stride n * 8 words either way) for a scalar-reading second pass.
  uint16_t* digits = p.digits ? ctx->d_digits : nullptr;
  uint16_t* plane_out = p.planes ? ctx->d_digits : digits;
  const int plane_mode = p.planes ? 2 : (digits ? 1 : 0);
  // sparse launches: the same passes instantiated with one more argument (msm_layout.h: SparseIdx) -- the count passes guard the indices, the
  // scatter passes write them in place of the positions
  const SparseIdx sp{p.indices, (uint32_t)ctx->n_bases, d_err};
  // k_count leaves the prefix over tiles and the bin totals itself (bin_fill); the other first passes are followed by a scan kernel
  const bool fused_scan = !wide && !bytes;
  const uint32_t* bin_total = fused_scan ? ctx->d_bin_fill : ctx->d_bin_total;
  if (fused_scan) {
    if (ctx->bin_fill_dirty) HIP_TRY(ctx, hipMemsetAsync(ctx->d_bin_fill, 0, (size_t)MAXLW * NCOARSE * 4, st));
    ctx->bin_fill_dirty = true;  // (until this launch's k_sort_fine is in the stream)
  }
  if (wide) {
    dispatch<16, 17, 18, 19, 20>(p.wide_bits, [&](auto c) {
      constexpr int C = decltype(c)::value;
      if (p.list_path)
        hipLaunchKernelGGL(k_count_wide_list<C>, grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.nvec, p.n * 8, ctx->d_counts, d_err, top_shift,
                           p.v_begin, p.v_count, ctx->d_val, ctx->d_list_len, p.stride, p.subtiles);
      else
        hipLaunchKernelGGL(k_count_wide<C>, grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.nvec, p.n * 8, ctx->d_counts, d_err, top_shift,
                           p.v_begin, p.v_count);
    });
  } else if (bytes) {
    dispatch<1, 2, -1, -2>(p.nb_kernel(), [&](auto b) {
      if (p.sparse)
        hipLaunchKernelGGL((k_byte_count<decltype(b)::value, SparseIdx>), grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.tile_len, p.tiles, ctx->d_counts, sp);
      else
        hipLaunchKernelGGL(k_byte_count<decltype(b)::value>, grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.tile_len, p.tiles, ctx->d_counts);
    });
  } else if (halves) {
    const int k = p.wbits == 16 ? 2 : p.wbits == 14 ? 1 : 0;
    if (p.sparse)
      hipLaunchKernelGGL(ctx->ops->count_split_sparse[k], grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin, p.w_count_vec, p.nvec, p.n * 8,
                         ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, (uint64_t*)nullptr, ctx->d_halves, d_err, merge_nb, sp);
    else
      hipLaunchKernelGGL(ctx->ops->count_split[k], grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin,
                         p.w_count_vec, p.nvec, p.n * 8, ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, p.planes ? ctx->d_negbits : nullptr,
                         p.planes ? nullptr : ctx->d_halves, d_err, merge_nb);
    d_scalars = ctx->d_halves;
  } else {
    sort_input([&](auto c, auto w, auto b) {
      constexpr int C = decltype(c)::value, SW = decltype(w)::value, NB = decltype(b)::value;
      if constexpr (NB != 0 || SW == 8) {  // (the halves were counted above, by the pass that splits them)
        const size_t vec_stride = p.n * (NB ? narrow_width(NB) : 8);
        if (p.sparse)
          hipLaunchKernelGGL((k_count<C, SW, void, NB, SparseIdx>), grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin, p.w_count_vec,
                             p.nvec, vec_stride, ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, (uint64_t*)nullptr, (uint32_t*)nullptr, d_err, merge_nb, sp);
        else
          hipLaunchKernelGGL((k_count<C, SW, void, NB>), grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin, p.w_count_vec, p.nvec,
                             vec_stride, ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, (uint64_t*)nullptr, (uint32_t*)nullptr, d_err, merge_nb);
      }
    });
  }
  AFTER_KERNEL(ctx, "k_count", st);
  HIP_TRY(ctx, mark(1));
  if (bytes) hipLaunchKernelGGL(k_byte_scan, dim3(BYTE_BINS / 4, p.w_count), dim3(256), 0, st, ctx->d_counts, p.tiles, ctx->d_bin_total);
  else if (!fused_scan) hipLaunchKernelGGL(k_scan_tiles, dim3(NCOARSE / 4, p.w_count), dim3(256), 0, st, ctx->d_counts, p.tiles, ctx->d_bin_total);  // all 128 bins: the scatter scans them
  if (!fused_scan) AFTER_KERNEL(ctx, "k_scan_tiles", st);
  HIP_TRY(ctx, mark(2));
  if (p.list_path) {  // shares of at most WIDE_SHARE_VWIN_MAX virtual windows: from the first pass's lists
    hipLaunchKernelGGL(k_scatter_list, dim3(p.tiles, p.w_count), dim3(256), 0, st, (const uint32_t*)ctx->d_val, (const uint32_t*)ctx->d_list_len, p.stride,
                       (uint32_t)(LIST_SUB * wide_tables_of(p.wide_bits)), p.subtiles, p.n_sc, p.tile_len, p.tiles, p.w_count, ctx->d_counts, ctx->d_bin_total,
                       ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine, merge_nb, p.chunks, p.chunk_len, d_chunk_len);
  } else if (wide) {  // (... or, MSM_HIP_WIDE_SHARE_LISTS=0, the small shape of the two-pass kernel: four workgroups per CU instead of one)
    dispatch<16, 17, 18, 19, 20>(p.wide_bits, [&](auto c) {
      dispatch<true, false>(p.share_shape, [&](auto share) {
        constexpr int C = decltype(c)::value;
        constexpr bool SHARE = decltype(share)::value;
        hipLaunchKernelGGL((k_scatter_wide<C, SHARE>), grid, dim3(WideScatterShape<C, SHARE>::THREADS), 0, st, d_scalars, p.n_sc, p.stride, p.tile_len, p.tiles,
                           p.nvec, p.n * 8, ctx->d_counts, ctx->d_bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine, merge_nb, p.chunks, p.chunk_len,
                           d_chunk_len, top_shift, p.v_begin, p.v_count);
      });
    });
  } else if (p.planes) {
    hipLaunchKernelGGL(k_scatter_planes, dim3(p.tiles), dim3(256), 0, st, ctx->d_digits, halves ? ctx->d_negbits : (const uint64_t*)nullptr, p.n_sc, p.stride,
                       p.tile_len, p.tiles, p.w_count, p.w_count_vec, ctx->d_counts, bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine,
                       (uint32_t)ctx->n_bases, p.chunks, p.chunk_len, d_chunk_len);
  } else if (bytes) {
    dispatch<1, 2, -1, -2>(p.nb_kernel(), [&](auto b) {
      if (p.sparse)
        hipLaunchKernelGGL((k_byte_scatter<decltype(b)::value, SparseIdx>), grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.stride, p.tile_len, p.tiles,
                           p.w_count, ctx->d_counts, ctx->d_bin_total, s.d_col_ptr, p.half, ctx->d_val, p.chunks, p.chunk_len, d_chunk_len, sp);
      else
        hipLaunchKernelGGL(k_byte_scatter<decltype(b)::value>, grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.stride, p.tile_len, p.tiles, p.w_count,
                           ctx->d_counts, ctx->d_bin_total, s.d_col_ptr, p.half, ctx->d_val, p.chunks, p.chunk_len, d_chunk_len);
    });
  } else {
    sort_input([&](auto c, auto w, auto b) {
      constexpr int C = decltype(c)::value, SW = decltype(w)::value, NB = decltype(b)::value;
      const size_t vec_stride = p.n * (NB ? narrow_width(NB) : 8);
      if (p.sparse)
        hipLaunchKernelGGL((k_scatter_coarse<C, SW, NB, SparseIdx>), grid, block, gpos_bytes, st, d_scalars, p.n_sc, p.stride, p.tile_len, p.tiles, p.w_begin,
                           p.w_count_vec, p.nvec, vec_stride, ctx->d_counts, bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine,
                           merge_nb, (uint32_t)p.n, halves ? (uint32_t)ctx->n_bases : 0u, p.chunks, p.chunk_len, d_chunk_len, sp);
      else
        hipLaunchKernelGGL((k_scatter_coarse<C, SW, NB>), grid, block, gpos_bytes, st, d_scalars, p.n_sc, p.stride, p.tile_len, p.tiles, p.w_begin,
                           p.w_count_vec, p.nvec, vec_stride, ctx->d_counts, bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine,
                           merge_nb, (uint32_t)p.n, halves ? (uint32_t)ctx->n_bases : 0u, p.chunks, p.chunk_len, d_chunk_len);
    });
  }
  AFTER_KERNEL(ctx, "k_scatter_coarse", st);
  HIP_TRY(ctx, mark(3));
  // large n: the sub-range histograms of huge coarse bins are made once, not by every sharer.  (round 5) Not launched at all while uniform scalars
  // cannot fill a coarse bin to three quarters of FINE_BIG -- 2^20 points and below: its 8192 workgroups found nothing to do and took 19 us of every
  // launch's main stream; skewed scalars that make such a bin after all take the sharers' own histograms (k_sort_fine's fallback path)
  // ... ADAPTIVELY (later in round 5): few distinct / small / equal scalars (witness vectors) fill huge bins at any size, and the fallback costs their
  // fine sort 2 - 2.5 x (profiles/r05_skew_hist.txt): k_sort_fine reports a huge bin in the slot's status word, and the 64 launches after such a
  // report run k_fine_hist (a prover's MSMs come in series of like inputs; the first of a series pays the fallback once).  The report means SKEW:
  // a bin of more than HUGE_BIN_MEANS mean bins -- the top window of endomorphism halves reaches two means, which at 2^20 is FINE_BIG, and used to
  // keep the kernel in every launch of uniform scalars; such bins are shared without histograms at no measurable cost (sort_kernels.h: k_sort_fine)
  // Narrow scalars always run it and leave the credit alone: their top window holds only the recode's carry (U8: all entries) -- one huge bin by
  // construction, which says nothing about the context's later 32-byte launches
  if (bytes) {  // byte windows: the scatter has grouped the entries by slot already; only the SMVP's chunk table is left
    hipLaunchKernelGGL(k_byte_chunks, dim3(blocks_for(p.chunks, 256), p.w_count), dim3(256), 0, st, (const uint32_t*)s.d_col_ptr, p.half, p.chunks,
                       (const uint32_t*)d_chunk_len, ctx->d_chunk_slot);
    AFTER_KERNEL(ctx, "k_byte_chunks", st);
  } else {
    const uint32_t* part_hist = nullptr;
    const bool hist_useful = p.nb || ctx->fine_hist_min_n != FINE_BIG + 1 || p.n_entries / p.ncoarse * 4 > (size_t)FINE_BIG * 3 || ctx->skew_credit > 0;
    if (ctx->skew_credit > 0 && !p.nb) ctx->skew_credit--;
    p.fine_hist = p.n_entries >= ctx->fine_hist_min_n && hist_useful;
    if (p.fine_hist) {
      hipLaunchKernelGGL(k_fine_hist, dim3(p.ncoarse, p.w_count, FINE_SPLIT), dim3(256), 0, st, ctx->d_tmp_fine, p.stride, ctx->d_coarse_ptr,
                         ctx->d_part_hist);
      AFTER_KERNEL(ctx, "k_fine_hist", st);
      part_hist = ctx->d_part_hist;
    }
    hipLaunchKernelGGL(k_sort_fine, dim3(p.ncoarse, p.w_count, FINE_SPLIT), dim3(256), 0, st, ctx->d_tmp_val, ctx->d_tmp_fine, p.stride, ctx->d_coarse_ptr,
                       s.d_col_ptr, ctx->d_val, p.chunks, d_chunk_len, ctx->d_chunk_slot, part_hist, d_err, fused_scan ? ctx->d_bin_fill : (uint32_t*)nullptr);
    AFTER_KERNEL(ctx, "k_sort_fine", st);
    if (fused_scan) ctx->bin_fill_dirty = false;
  }
  if (ctx->debug) {  // deterministic transpose for the stage read-back: every slot's run in ascending order
    hipLaunchKernelGGL(k_order_runs, dim3(blocks_for(p.n_entries, 256), p.w_count), dim3(256), 0, st, s.d_col_ptr, ctx->d_val, ctx->d_tmp_val, p.stride, p.half);
    hipLaunchKernelGGL(k_copy_runs, dim3(blocks_for(p.n_entries, 256), p.w_count), dim3(256), 0, st, s.d_col_ptr, ctx->d_tmp_val, ctx->d_val, p.stride, p.half);
    AFTER_KERNEL(ctx, "k_order_runs", st);
  }
  return MSM_HIP_OK;
}

// The bucket reduce's row / column pass: the curve's k_bpr_rowcol<LOG_R, LOG_ROWS> and its workgroups per window.  Serial run per thread before
// the LDS tree: 16 buckets when many windows are reduced at once (fewest wave-additions), 4 for a few windows (shallowest); measured optimum for 16
// and for 2 windows respectively
struct RowCol {
  void (*kernel)(const uint32_t*, uint32_t*, uint32_t*);
  int blocks;
  int logr;  // LOG_R of the variant (test hook msm_hip_test_env_report)
};
inline int bpr_force_logr() {  // tuning aid
  static const int v = [] { const char* e = getenv("MSM_HIP_BPR_LOGR"); return e ? atoi(e) : 0; }();
  return v;
}
RowCol pick_rowcol(const msm_hip_ctx* ctx, const LaunchPlan& p, const Slot& s) {
  const int force_logr = bpr_force_logr();
  const CurveOps* o = ctx->ops;
  if (p.wbits == 16) {
    // one small MSM alone in its launch (8 half-length windows, up to 2^18 points): 8 buckets per thread -- its latency is what counts
    // (-4 % at 2^16, -2.6 % at 2^18; the same setting costs grouped launches 3 - 16 % and a pipelined 2^20 MSM 0.5 %)
    // ... and so is a larger one that has the GPU to itself: no other result slot of the context is in flight when it is launched
    // (latency 1.81 -> 1.77 ms at 2^20; in a pipeline only the very first launch is alone: throughput unchanged)
    bool alone = p.nvec == 1 && p.w_count == 8;
    for (const Slot& q : ctx->slot) alone = alone && (&q == &s || !q.pending);
    const bool small_single = p.nvec == 1 && p.w_count == 8 && (p.n_entries <= ((size_t)1 << 19) || alone);
    if (force_logr == 4 || (force_logr == 0 && p.w_count >= 8 && !small_single)) return {o->rowcol_4_8, bpr_rowcol_blocks<4, 8>(), 4};
    if (force_logr == 3 || (force_logr == 0 && small_single)) return {o->rowcol_3_8, bpr_rowcol_blocks<3, 8>(), 3};
    return {o->rowcol_2_8, bpr_rowcol_blocks<2, 8>(), 2};
  }
  if (p.wbits == 14) {  // 64 rows x 128 columns
    if (force_logr == 4 || (force_logr == 0 && p.w_count > 2 * nwin_of(14))) return {o->rowcol_4_6, bpr_rowcol_blocks<4, 6>(), 4};
    return {o->rowcol_2_6, bpr_rowcol_blocks<2, 6>(), 2};
  }
  return {o->rowcol_2_4, bpr_rowcol_blocks<2, 4>(), 2};  // 16 rows x 128 columns
}

// The launch's second stage: the SMVP (it reads the bases) on the main stream, then stitch + bucket reduce on the slot's reduce stream, few waves
// of long dependent chains; the error word and, for the host, the window sums go to the slot's pinned buffer.  Returns without waiting.
inline bool inline_reduce_on() {  // MSM_HIP_INLINE_REDUCE=0: the stitch and the bucket reduce always on the reduce stream
  static const bool v = [] { const char* e = getenv("MSM_HIP_INLINE_REDUCE"); return !e || atoi(e) != 0; }();
  return v;
}
inline unsigned smvp_lds_pad() {  // A/B aid: dynamic LDS added to the SMVP's workgroups
  static const unsigned v = [] { const char* e = getenv("MSM_HIP_SMVP_LDS_PAD"); const long v = e ? atol(e) : 0; return v > 0 && v <= 65536 ? (unsigned)v : 0u; }();
  return v;
}
int enqueue_reduce(msm_hip_ctx* ctx, const LaunchPlan& p, Slot& s) {
  hipStream_t st = ctx->stream, rs = ctx->reduce_stream[(&s - ctx->slot) % NREDUCE];
  // a synchronous call with nothing else in flight (msm_hip_run_*: the caller waits for this launch before it issues another): the stitch and
  // the bucket reduce follow the SMVP on the MAIN stream -- no cross-stream hand-off (an event wait costs ~10 us more than an in-stream kernel
  // boundary), and no next launch exists whose sort the separate stream would let overlap.  MSM_HIP_INLINE_REDUCE=0: always the reduce stream.
  if (inline_reduce_on() && p.sync) {
    bool others = false;
    for (const Slot& o : ctx->slot) others = others || (&o != &s && o.pending);
    if (!others) rs = st;
  }
  const bool to_host = !p.sums_dev;
  uint32_t* wsums_out = static_cast<uint32_t*>(to_host ? s.d_wsums : p.sums_dev);
  uint32_t* d_err = reinterpret_cast<uint32_t*>(s.d_wsums + WSUM_BYTES);
  uint32_t* d_chunk_len = s.d_big_queue + BIGQ_CHUNK_LEN;
  const int tl = ctx->timing_level;
  // the SMVP's own begin / end timestamps: attached to its dispatch (hipExtLaunchKernelGGL) instead of two event packets around it -- a
  // packet between two kernels costs a few microseconds of queue time, and these two sat between every launch's sort and its SMVP and
  // between the SMVP and the next launch (bench.py times every launch's SMVP for the roofline figure).  Level 2 keeps the packets: its
  // stage boundaries are read as differences of consecutive events.
  HIP_TRY(ctx, tl >= 2 ? hipEventRecord(s.ev[4], st) : hipSuccess);
  hipExtLaunchKernelGGL(ctx->ops->smvp_chunks, dim3((p.chunks + 255) / 256, p.w_count), dim3(256), smvp_lds_pad(), st, tl == 1 ? s.ev[4] : nullptr,
                        tl == 1 ? s.ev[5] : nullptr, 0, (const uint32_t*)(ctx->d_bases + p.base_off * 2 * (size_t)ctx->ops->coord_words), (const uint32_t*)s.d_col_ptr,
                        (const uint32_t*)ctx->d_val, p.stride, p.chunks, (const uint32_t*)d_chunk_len, (const uint32_t*)ctx->d_chunk_slot, s.d_buckets, s.d_heads,
                        s.d_tails, p.half);
  AFTER_KERNEL(ctx, "k_smvp_chunks", st);
  HIP_TRY(ctx, tl >= 2 ? hipEventRecord(s.ev[5], st) : hipSuccess);
  if (rs != st) HIP_TRY(ctx, hipEventRecord(s.smvp_done, st));

  if (rs != st) HIP_TRY(ctx, hipStreamWaitEvent(rs, s.smvp_done, 0));
  hipLaunchKernelGGL(ctx->ops->smvp_stitch, dim3(p.half / 256, p.w_count), dim3(256), 0, rs, s.d_col_ptr, p.chunks, d_chunk_len, s.d_heads, s.d_tails,
                     s.d_buckets, s.d_big_queue);
  AFTER_KERNEL(ctx, "k_smvp_stitch", rs);
  hipLaunchKernelGGL(ctx->ops->smvp_stitch_big, dim3(STITCH_BLOCKS), dim3(256), 0, rs, s.d_col_ptr, p.chunks, s.d_heads, s.d_tails, s.d_buckets,
                     s.d_big_queue, p.half);
  AFTER_KERNEL(ctx, "k_smvp_stitch_big", rs);
  if (tl >= 2) {
    HIP_TRY(ctx, hipEventRecord(s.ev[6], rs));
    HIP_TRY(ctx, hipEventRecord(s.red0, rs));
  }
  uint32_t* d_rows = s.d_partials;
  uint32_t* d_cols = d_rows + (size_t)MAXLW * 256 * ctx->ops->xyzz_words;
  uint32_t* d_parts = d_cols + (size_t)MAXLW * 256 * ctx->ops->xyzz_words;
  const RowCol rowcol = pick_rowcol(ctx, p, s);
  hipLaunchKernelGGL(rowcol.kernel, dim3(rowcol.blocks, p.w_count), dim3(256), 0, rs, s.d_buckets, d_rows, d_cols);
  AFTER_KERNEL(ctx, "k_bpr_rowcol", rs);
  // A launch that carries ONE MSM whose sums the host combines anyway (finish): the narrow end of the reduction -- ~25 dependent group
  // operations at ~7 us each in k_bpr_w256 / k_bpr_final -- is replaced by 16 independent masked tree sums per window (k_bpr_planes, 8 deep)
  // and 29 operations per window on the host (0.3 us each).  Sums that stay on the device (window shards for the gather), grouped launches
  // (their host thread is on the critical path: several MSMs' worth of host work per launch) and debug read-backs get finished sums.
  // (a wide fixed-base launch always leaves the plane sums -- its finish needs every virtual window's plain total, which is one of them --: plan_launch
  //  admits it only as whole MSMs whose sums go to the host, at most 24 virtual windows together)
  const bool wide = p.mode == MODE_WIDE;
  const bool parts_mode = to_host && !p.pairs && (p.nvec == 1 || wide) && (!ctx->debug || wide) && p.w_count <= 24;
  // the kernel that ends the chain writes the launch's error word into the slot's pinned buffer itself and clears it (no copy, no fill); a
  // single MSM's bit-plane sums go to the pinned buffer directly as well (12 KB of stores over the host link instead of a copy behind the kernel)
  uint32_t* h_err = reinterpret_cast<uint32_t*>(s.h_wsums + WSUM_BYTES);
  const int bpr_cols = (int)(p.half / BPR_COLS);
  if (parts_mode) {
    hipLaunchKernelGGL(ctx->ops->bpr_planes, dim3(PLANES_PER_WINDOW, p.w_count), dim3(256), 0, rs, d_rows, d_cols, reinterpret_cast<uint32_t*>(s.h_wsums),
                       bpr_cols, s.d_big_queue, d_err, h_err);
    AFTER_KERNEL(ctx, "k_bpr_planes", rs);
  } else if (ctx->ops->use_w256) {
    hipLaunchKernelGGL(ctx->ops->bpr_w256, dim3(2, p.w_count), dim3(256), 0, rs, d_rows, d_cols, d_parts, bpr_cols);
    AFTER_KERNEL(ctx, "k_bpr_w256", rs);
    hipLaunchKernelGGL(ctx->ops->bpr_final, dim3(1), dim3(64), 0, rs, d_parts, p.w_count, wsums_out, s.d_big_queue, d_err, h_err, p.pairs ? 1 : 0);
    AFTER_KERNEL(ctx, "k_bpr_final", rs);
  } else {  // a field too wide for k_bpr_w256's LDS footprint (BLS12-381): the same bit-plane sums, finished on the device
    hipLaunchKernelGGL(ctx->ops->bpr_planes_xyzz, dim3(PLANES_PER_WINDOW, p.w_count), dim3(256), 0, rs, d_rows, d_cols, d_parts, bpr_cols, s.d_big_queue,
                       d_err, h_err);
    AFTER_KERNEL(ctx, "k_bpr_planes<xyzz>", rs);
    hipLaunchKernelGGL(ctx->ops->bpr_final_planes, dim3(1), dim3(64), 0, rs, d_parts, p.w_count, wsums_out, s.d_big_queue, d_err, h_err, p.pairs ? 1 : 0);
    AFTER_KERNEL(ctx, "k_bpr_final_planes", rs);
  }
  if (tl >= 2) HIP_TRY(ctx, hipEventRecord(s.red1, rs));
  if (to_host && !parts_mode) HIP_TRY(ctx, hipMemcpyAsync(s.h_wsums, wsums_out, (size_t)p.w_count * (p.pairs ? 2 : 1) * ctx->jb, hipMemcpyDeviceToHost, rs));
  HIP_TRY(ctx, hipEventRecord(s.done, rs));
  HIP_TRY(ctx, hipGetLastError());

  s.plan = p;
  s.parts = parts_mode;
  s.timed = tl >= 1;
  s.timing_level = tl;
  s.pending = true;
  s.to_host = to_host;
  ctx->last = p;
  ctx->last_slot = (int)(&s - ctx->slot);
  ctx->last_logr = rowcol.logr;
  ctx->last_inline_reduce = rs == st;
  return MSM_HIP_OK;
}

// wait for slot `s`, fetch its error word and stage times
int wait_slot(msm_hip_ctx* ctx, Slot& s) {
  HIP_TRY(ctx, hipEventSynchronize(s.done));
  s.pending = false;
  if (s.timed) {
    s.timed = false;
    for (int i = 0; i < 8; i++) ctx->stage_ms[i] = 0.0f;
    if (s.timing_level >= 2) {
      for (int i = 0; i < 6; i++) HIP_TRY(ctx, hipEventElapsedTime(&ctx->stage_ms[i], s.ev[i], s.ev[i + 1]));
      HIP_TRY(ctx, hipEventElapsedTime(&ctx->stage_ms[6], s.red0, s.red1));
      HIP_TRY(ctx, hipEventElapsedTime(&ctx->stage_ms[7], s.ev[0], s.red1));
    } else {
      HIP_TRY(ctx, hipEventElapsedTime(&ctx->stage_ms[4], s.ev[4], s.ev[5]));
    }
  }
  uint32_t bits;
  memcpy(&bits, s.h_wsums + WSUM_BYTES, 4);
  if ((bits & INFOBIT_HUGE_BIN) && !s.plan.nb) ctx->skew_credit = 64;  // (see the launch of k_fine_hist; a narrow launch's huge bins are its own)
  return err_from_bits(bits);
}

// after a failed batch: collect every slot that is still pending so that the context stays usable
void drain_slots(msm_hip_ctx* ctx) {
  for (Slot& s : ctx->slot)
    if (s.pending) (void)wait_slot(ctx, s);
}

// room for n bases; no run may still be reading the old ones (the SMVP on the main stream)
constexpr size_t MAX_PRECOMPUTE_POINTS = (size_t)1 << 24;  // 16 tables: 16 GiB, and table indices stay below 2^28

// The mode a base set is held in.  Asked for explicitly (tables, endomorphism images, or MSM_HIP_BASES_PLAIN: the reference's 16 windows
// over n points), or -- none of the three -- the fastest the curve has: the drop-in call shape (flags = 0; msm_hip_msm_bn254_g1 ≙ compute_msm,
// src/cuzk/msm.rs:75-94) runs the mode the headline figure is measured in (656 vs 701 - 714 MSM/s at 2^20 in round 3, when it did not).
constexpr uint32_t BASE_FLAGS_ALL = MSM_HIP_CHECK_ON_CURVE | MSM_HIP_BASES_MONT256 | MSM_HIP_BASES_PRECOMPUTE | MSM_HIP_BASES_ENDOMORPHISM | MSM_HIP_BASES_PLAIN |
                                    MSM_HIP_BASES_PRECOMPUTE_WIDE | MSM_HIP_BASES_ZERO_IS_IDENTITY;
constexpr size_t MAX_WIDE_POINTS = (size_t)1 << 24;  // 13 tables of 20-bit digits: 13 GiB; sort arrays of 16 x 13 n entries: 31 GiB
inline bool reduce_priority_on() {  // MSM_HIP_REDUCE_PRIORITY=0: plain reduce streams (msm_hip_ctx_create_curve)
  static const bool v = [] { const char* e = getenv("MSM_HIP_REDUCE_PRIORITY"); return !e || atoi(e) != 0; }();
  return v;
}
inline bool bases_auto() {  // MSM_HIP_BASES_AUTO=0: flags = 0 means plain (rounds 1 - 3)
  static const bool v = [] { const char* e = getenv("MSM_HIP_BASES_AUTO"); return !e || atoi(e) != 0; }();
  return v;
}
inline uint32_t resolve_base_flags(const msm_hip_ctx* ctx, size_t n, uint32_t flags) {
  const bool auto_endo = bases_auto();
  if (flags & (MSM_HIP_BASES_PRECOMPUTE | MSM_HIP_BASES_PRECOMPUTE_WIDE | MSM_HIP_BASES_ENDOMORPHISM | MSM_HIP_BASES_PLAIN)) return flags;
  // ... on the curves of prime order only: phi(P) = lambda P holds on the subgroup of order r, and a base set of a curve with a cofactor
  // (BLS12-381, the G2 twists) may hold points outside it, for which the plain MSM is still defined -- there the mode stays an opt-in
  const bool prime_order = ctx->curve == MSM_HIP_CURVE_BN254_G1 || ctx->curve == MSM_HIP_CURVE_GRUMPKIN || ctx->curve == MSM_HIP_CURVE_PALLAS ||
                           ctx->curve == MSM_HIP_CURVE_VESTA;
  if (auto_endo && prime_order && ctx->ops->glv && n <= MAX_POINTS / 2) return flags | MSM_HIP_BASES_ENDOMORPHISM;
  return flags;
}

int reserve_bases(msm_hip_ctx* ctx, size_t n, uint32_t flags) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const bool wide = (flags & MSM_HIP_BASES_PRECOMPUTE_WIDE) != 0;
  const bool tables = (flags & MSM_HIP_BASES_PRECOMPUTE) != 0 || wide, endo = (flags & MSM_HIP_BASES_ENDOMORPHISM) != 0;
  if (n > MAX_POINTS || (tables && n > MAX_PRECOMPUTE_POINTS) || (wide && n > MAX_WIDE_POINTS) || (endo && n > MAX_POINTS / 2) || (tables && endo))
    return MSM_HIP_ERR_INVALID_ARG;
  if ((flags & ~BASE_FLAGS_ALL) || ((flags & MSM_HIP_BASES_PLAIN) && (tables || endo)) || (wide && (flags & MSM_HIP_BASES_PRECOMPUTE)))
    return MSM_HIP_ERR_INVALID_ARG;
  if ((endo && !ctx->ops->glv) || (tables && !ctx->ops->precompute_tables)) return MSM_HIP_ERR_INVALID_ARG;
  if (wide && pick_wide_bits(ctx, n) < 0) return MSM_HIP_ERR_INVALID_ARG;  // (msm_hip_set_wide_bits asked for a width that cannot hold this curve's scalars)
  ctx->n_bases = 0;
  ctx->precomputed = false;
  ctx->wide_bits = 0;
  ctx->endo = false;
  ctx->n_identity = 0;
  ctx->mul_table_bits = 0;  // (msm_hip_mul_base's table belongs to the old set)
  const size_t records = wide ? n * (size_t)wide_tables_of(pick_wide_bits(ctx, n)) : tables ? n * NWIN : endo ? 2 * n : n;
  return grow(ctx, ctx->cap_bases, records, false, [&](size_t c) { return dev_alloc(ctx, ctx->d_bases, c * 2 * (size_t)ctx->ops->coord_words); });
}

// wire bytes at d_xy (may be ctx->d_bases itself: the conversion is element-wise) -> resident Montgomery bases
// (MSM_HIP_BASES_ZERO_IS_IDENTITY: all-zero records are the identity -- marked in d_id_bits, counted in the error word's neighbour d_err[1])
int set_bases_from_device(msm_hip_ctx* ctx, const uint32_t* d_xy, size_t n, uint32_t flags) {
  if (n == 0) return MSM_HIP_OK;
  const bool zero_id = (flags & MSM_HIP_BASES_ZERO_IS_IDENTITY) != 0;
  int rc;
  if (zero_id && (rc = grow(ctx, ctx->cap_id_bits, (n + 63) / 64, false, [&](size_t c) { return dev_alloc(ctx, ctx->d_id_bits, c); }))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, zero_id ? 8 : 4, ctx->stream));
  if (zero_id)
    hipLaunchKernelGGL(ctx->ops->convert_points_zero_id, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, d_xy, ctx->d_bases, n, flags, ctx->d_err,
                       ctx->d_id_bits, ctx->d_err + 1);
  else
    hipLaunchKernelGGL(ctx->ops->convert_points, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, d_xy, ctx->d_bases, n, flags, ctx->d_err);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t bits[2] = {0u, 0u};
  HIP_TRY(ctx, hipMemcpyAsync(bits, ctx->d_err, zero_id ? 8 : 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = err_from_bits(bits[0]))) return rc;
  if (flags & (MSM_HIP_BASES_PRECOMPUTE | MSM_HIP_BASES_PRECOMPUTE_WIDE)) {  // tables 1 .. 15 behind the plain set: T_w[i] = 2^(16 w) P_i (wide: 1 .. 13, 2^(19 w) P_i, the last one top_shift doublings short)
    const bool wide = (flags & MSM_HIP_BASES_PRECOMPUTE_WIDE) != 0;
    const int wb = wide ? pick_wide_bits(ctx, n) : 0;
    hipLaunchKernelGGL(ctx->ops->precompute_tables, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_bases, n, n, wide ? wide_tables_of(wb) : (int)NWIN,
                       wide ? wb : (int)WBITS, wide ? wb - wide_top_shift(ctx->curve, wb) : (int)WBITS);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->precomputed = !wide;
    ctx->wide_bits = wb;
  }
  if (flags & MSM_HIP_BASES_ENDOMORPHISM) {  // phi(P_i) = (beta x_i, y_i) behind the plain set
    hipLaunchKernelGGL(ctx->ops->endo_points, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_bases, n, (size_t)0, n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->endo = true;
  }
  ctx->n_identity = bits[1];
  ctx->n_bases = n;
  return MSM_HIP_OK;
}

}  // namespace

namespace {
// MSMs per launch of the batch runners: small MSMs cannot fill the GPU one at a time (kernel latencies dominate below
// ~2^19 points), so up to MAXLW / NWIN = 4 of them -- at most about 2^20 points together -- share one kernel sequence
size_t batch_group(msm_hip_ctx* ctx, size_t n, size_t batch) {
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

// software pipeline over the result slots: the host combine of group j overlaps the device work of groups j+1 .. j+2.
// `stage` (may be null) copies group j's scalars to the device and returns their device address.
template <typename Stage>
int run_batch_groups(msm_hip_ctx* ctx, size_t n, size_t batch, uint8_t* out_xyz, Stage stage) {
  const size_t g = batch_group(ctx, n, batch);
  const size_t groups = (batch + g - 1) / g;
  constexpr size_t DEPTH = NSLOT - 1;
  int rc = MSM_HIP_OK;
  for (size_t j = 0; j < groups + DEPTH; j++) {
    if (j >= DEPTH) {
      const size_t k = j - DEPTH;
      if ((rc = msm_hip_finish_batch(ctx, (int)(k % NSLOT), out_xyz + ctx->jb * k * g))) break;
    }
    if (j < groups) {
      const size_t first = j * g, count = first + g <= batch ? g : batch - first;
      const void* dev = nullptr;
      if ((rc = stage(j, first, count, &dev))) break;
      if ((rc = msm_hip_launch_windows_batch_device(ctx, dev, n, (int)count, 0, NWIN, (int)(j % NSLOT), nullptr))) break;
    }
  }
  if (rc) drain_slots(ctx);
  return rc;
}
}  // namespace

extern "C" {

int msm_hip_abi_version(void) { return 7; }  // 7 (round 5): curve-neutral names, virtual-window launches + pair combine, msm_hip_msm_curve, msm_hip_mgpu_set_wide_bits; the sparse calls (msm_hip_run_sparse ...) arrived within 7

const char* msm_hip_strerror(int code) {
  switch (code) {
    case MSM_HIP_OK: return "ok";
    case MSM_HIP_ERR_NO_DEVICE: return "no usable HIP device";
    case MSM_HIP_ERR_INVALID_ARG: return "invalid argument";
    case MSM_HIP_ERR_OUT_OF_MEMORY: return "out of device memory";
    case MSM_HIP_ERR_NONCANONICAL: return "non-canonical field element in input";
    case MSM_HIP_ERR_NOT_ON_CURVE: return "base point not on the curve";
    case MSM_HIP_ERR_NO_BASES: return "bases not set";
    case MSM_HIP_ERR_HIP: return "HIP runtime error";
    case MSM_HIP_ERR_SLOT_BUSY: return "result slot still holds an unfinished MSM";
    default: return "unknown error";
  }
}

int msm_hip_last_hip_error(msm_hip_ctx* ctx) { return ctx ? ctx->last_hip_error : 0; }
void* msm_hip_stream(msm_hip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int msm_hip_ctx_create(msm_hip_ctx** out, int device_id) { return msm_hip_ctx_create_curve(out, device_id, MSM_HIP_CURVE_BN254_G1); }

int msm_hip_ctx_curve(const msm_hip_ctx* ctx) { return ctx ? ctx->curve : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_ctx_create_curve(msm_hip_ctx** out, int device_id, int curve) {
  if (!out) return MSM_HIP_ERR_INVALID_ARG;
  *out = nullptr;
  if (curve < 0 || curve >= MSM_HIP_NUM_CURVES) return MSM_HIP_ERR_INVALID_ARG;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return MSM_HIP_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= count) return MSM_HIP_ERR_INVALID_ARG;
  DeviceGuard guard(device_id);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  msm_hip_ctx* ctx = new (std::nothrow) msm_hip_ctx();
  if (!ctx) return MSM_HIP_ERR_OUT_OF_MEMORY;
  ctx->device = device_id;
  ctx->curve = curve;
  ctx->ops = curve_ops(curve);
  ctx->cb = 4 * (size_t)ctx->ops->coord_words;
  ctx->pb = 2 * ctx->cb;
  ctx->jb = 3 * ctx->cb;
  if (const char* e = getenv("MSM_HIP_FINE_HIST_MIN_LOGN")) {  // tuning aid
    const int l = atoi(e);
    if (l >= 0 && l < 40) ctx->fine_hist_min_n = (size_t)1 << l;
  }
  int rc = MSM_HIP_OK;
  auto fail = [&](int code) {
    msm_hip_ctx_destroy(ctx);
    return code;
  };
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return fail(MSM_HIP_ERR_NO_DEVICE);
  // The reduce streams run at the device's highest stream priority: the previous launch's stitch and bucket reduce then finish beside the
  // next launch's sort (latency-bound kernels that leave the multiplier idle) instead of trailing into its SMVP, which they slow down
  // (2^20, one GPU, five same-box pairs: 1.4025 vs 1.4231 ms per MSM, SMVP 0.976 vs 0.989 ms; a rank's window shares and 2^16: within the
  // noise; the opposite assignment -- main stream high, reduce low -- costs 3 %).  MSM_HIP_REDUCE_PRIORITY=0: plain streams.
  const bool reduce_high = reduce_priority_on();
  int prio_least = 0, prio_greatest = 0;
  if (reduce_high && hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = prio_least = 0;
  for (int k = 0; k < NREDUCE; k++) {
    if (reduce_high && prio_greatest != prio_least &&
        hipStreamCreateWithPriority(&ctx->reduce_stream[k], hipStreamNonBlocking, prio_greatest) == hipSuccess)
      continue;
    (void)hipGetLastError();
    ctx->reduce_stream[k] = nullptr;
    if (hipStreamCreateWithFlags(&ctx->reduce_stream[k], hipStreamNonBlocking) != hipSuccess) return fail(MSM_HIP_ERR_NO_DEVICE);
  }
  if (hipEventCreateWithFlags(&ctx->input_ready, hipEventDisableTiming) != hipSuccess) return fail(MSM_HIP_ERR_HIP);
  if ((rc = dev_alloc(ctx, ctx->d_counts, (size_t)MAXLW * MAX_TILES * NCOARSE))) return fail(rc);
  if ((rc = dev_alloc(ctx, ctx->d_bin_total, (size_t)MAXLW * NCOARSE))) return fail(rc);
  if ((rc = dev_alloc(ctx, ctx->d_bin_fill, (size_t)MAXLW * NCOARSE))) return fail(rc);
  if ((rc = dev_alloc(ctx, ctx->d_coarse_ptr, (size_t)MAXLW * (NCOARSE + 1)))) return fail(rc);
  if ((rc = dev_alloc(ctx, ctx->d_err, 2))) return fail(rc);  // the error word, and the identity count of a base conversion
  // result slots (buckets, piece arrays, events) are set up by the first launch that uses them: setup_slot / ensure_work
  *out = ctx;
  return MSM_HIP_OK;
}

void msm_hip_ctx_destroy(msm_hip_ctx* ctx) {
  if (!ctx) return;
  DeviceGuard guard(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
  for (hipStream_t r : ctx->reduce_stream)
    if (r) (void)hipStreamSynchronize(r);
  void* bufs[] = {ctx->d_list_len, ctx->d_bases,   ctx->d_halves, ctx->d_batch_stage, ctx->d_scalar_conv, ctx->d_part_hist, ctx->d_digits, ctx->d_negbits, ctx->d_counts,     ctx->d_bin_total, ctx->d_bin_fill, ctx->d_coarse_ptr,
                  ctx->d_tmp_val, ctx->d_tmp_fine, ctx->d_val,    ctx->d_chunk_slot, ctx->d_err,       ctx->d_stage, ctx->d_id_bits, ctx->d_mul, ctx->d_mul_table, ctx->d_fft, ctx->d_fft_tw};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (int k = 0; k < NSLOT; k++) {
    Slot& s = ctx->slot[k];
    if (s.h_wsums) (void)hipHostFree(s.h_wsums);
    void* sbufs[] = {s.d_wsums, s.d_buckets, s.d_partials, s.d_col_ptr, s.d_heads, s.d_tails, s.d_big_queue, s.d_host_scalars};
    for (void* b : sbufs)
      if (b) (void)hipFree(b);
    hipEvent_t evs[] = {s.done, s.smvp_done, s.staged, s.red0, s.red1};
    for (hipEvent_t e : evs)
      if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < N_MAIN_EVENTS; i++)
      if (s.ev[i]) (void)hipEventDestroy(s.ev[i]);
  }
  if (ctx->input_ready) (void)hipEventDestroy(ctx->input_ready);
  if (ctx->bases_ready) (void)hipEventDestroy(ctx->bases_ready);
  for (hipEvent_t e : ctx->chunk_landed)
    if (e) (void)hipEventDestroy(e);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  for (hipStream_t r : ctx->reduce_stream)
    if (r) (void)hipStreamDestroy(r);
  delete ctx;
}

int msm_hip_wait_stream(msm_hip_ctx* ctx, void* producer_stream) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  HIP_TRY(ctx, hipEventRecord(ctx->input_ready, static_cast<hipStream_t>(producer_stream)));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->input_ready, 0));
  return MSM_HIP_OK;
}

int msm_hip_set_bases_device(msm_hip_ctx* ctx, const void* xy_dev, size_t n, uint32_t flags) {
  if (!ctx || (!xy_dev && n)) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  flags = resolve_base_flags(ctx, n, flags);
  int rc = reserve_bases(ctx, n, flags);
  if (rc) return rc;
  return set_bases_from_device(ctx, static_cast<const uint32_t*>(xy_dev), n, flags);
}

int msm_hip_set_bases(msm_hip_ctx* ctx, const uint8_t* xy_host, size_t n, uint32_t flags) {
  if (!ctx || (!xy_host && n)) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  flags = resolve_base_flags(ctx, n, flags);
  int rc = reserve_bases(ctx, n, flags);
  if (rc) return rc;
  // the wire bytes land in the bases array itself and are converted in place (same 64 B per point): no staging buffer
  if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bases, xy_host, n * ctx->pb, hipMemcpyHostToDevice, ctx->stream));
  return set_bases_from_device(ctx, ctx->d_bases, n, flags);
}

}  // extern "C"

namespace {
// what a sparse entry point returns for a null context: NO_DEVICE when the process has no usable device (no context can exist), else INVALID_ARG
int no_context_code() {
  int count = 0;
  return hipGetDeviceCount(&count) != hipSuccess || count <= 0 ? MSM_HIP_ERR_NO_DEVICE : MSM_HIP_ERR_INVALID_ARG;
}

// one launch into the request's slot: plan, buffers, sort, reduce
int launch_impl(msm_hip_ctx* ctx, const LaunchRequest& r) {
  LaunchPlan p;
  int rc = plan_launch(ctx, r, p);
  if (rc) return rc;
  ON_DEVICE(ctx);
  Slot& s = ctx->slot[r.slot];
  if (s.pending) return MSM_HIP_ERR_SLOT_BUSY;  // its result was never collected (msm_hip_finish / msm_hip_slot_sync)
  if ((rc = setup_slot(ctx, s))) return rc;
  s.plan = p;
  s.parts = false;
  s.to_host = r.sums_dev == nullptr;
  if (r.n == 0) {  // identity window sums, nothing to compute
    s.pending = true;
    s.timed = false;
    memset(s.h_wsums, 0, WSUM_BYTES + 4);
    if (r.sums_dev) {
      HIP_TRY(ctx, hipMemsetAsync(r.sums_dev, 0, (size_t)p.w_count * (p.pairs ? 2 : 1) * ctx->jb, ctx->reduce_stream[r.slot % NREDUCE]));
      HIP_TRY(ctx, hipEventRecord(s.done, ctx->reduce_stream[r.slot % NREDUCE]));
    }
    return MSM_HIP_OK;
  }
  if ((rc = ensure_work(ctx, p, s)) || (rc = enqueue_sort(ctx, p, s, static_cast<const uint32_t*>(r.scalars)))) return rc;
  return enqueue_reduce(ctx, p, s);
}

// A dense request in the reference's 16 windows: whole MSMs whose sums stay in the slot (finish / finish_batch combines them) take the shape
// whole_msm_request gives them -- the window size follows n --, everything else runs as the plain 16-bit windows asked for
// (not with narrow scalars, the format of this launch: the window-sharding calls index the 16 windows of 32-byte scalars)
int launch_dense(msm_hip_ctx* ctx, LaunchRequest r) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const bool whole = r.w_begin == 0 && r.w_end == NWIN && !r.sums_dev && r.nvec >= 1;
  if (!whole && narrow_bytes(ctx->scalar_format)) return MSM_HIP_ERR_INVALID_ARG;
  return launch_impl(ctx, whole ? whole_msm_request(ctx, r) : r);
}

// Sparse: one whole MSM of r.n entries in the mode the resident bases and the scalar format call for, as launch_dense picks it for as many points
// (not on wide tables: out of scope)
int launch_sparse(msm_hip_ctx* ctx, LaunchRequest r) {
  if (!ctx) return no_context_code();
  if (ctx->wide_bits) return MSM_HIP_ERR_INVALID_ARG;
  r.sparse = true;
  return launch_impl(ctx, whole_msm_request(ctx, r));
}

// a synchronous call: `launch` (launch_dense, launch_sparse, launch_host) of `r` into slot 0 with nothing pipelined behind it, and its finish at once
int run_sync(msm_hip_ctx* ctx, int (*launch)(msm_hip_ctx*, LaunchRequest), LaunchRequest r, uint8_t* out_xyz) {
  r.slot = 0;
  r.sync = true;
  const int rc = launch(ctx, r);
  return rc ? rc : msm_hip_finish(ctx, 0, out_xyz);
}
}  // namespace

extern "C" {

int msm_hip_launch_windows_batch_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int nvec, int w_begin, int w_end,
                                              int slot, void* window_sums_dev) {
  return launch_dense(ctx, LaunchRequest(scalars_dev, n, slot, nvec, window_sums_dev).windows(MODE_PLAIN, w_begin, w_end));
}

int msm_hip_launch_half_windows_batch_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int nvec, int hw_begin, int hw_end,
                                                   int slot, void* window_sums_dev) {
  if (!ctx || narrow_bytes(ctx->scalar_format)) return MSM_HIP_ERR_INVALID_ARG;
  if (!ctx->endo && ctx->n_bases) return MSM_HIP_ERR_INVALID_ARG;  // needs bases set with MSM_HIP_BASES_ENDOMORPHISM
  return launch_impl(ctx, LaunchRequest(scalars_dev, n, slot, nvec, window_sums_dev).windows(MODE_HALVES, hw_begin, hw_end));
}

int msm_hip_launch_vwindows_batch_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int nvec, int v_begin, int v_end, int slot,
                                         void* sums_dev) {
  if (!ctx || narrow_bytes(ctx->scalar_format)) return MSM_HIP_ERR_INVALID_ARG;
  if (!ctx->wide_bits) return ctx->n_bases || !n ? MSM_HIP_ERR_INVALID_ARG : MSM_HIP_ERR_NO_BASES;  // needs bases set with MSM_HIP_BASES_PRECOMPUTE_WIDE
  if (v_begin < 0 || v_end <= v_begin) return MSM_HIP_ERR_INVALID_ARG;
  return launch_impl(ctx, LaunchRequest(scalars_dev, n, slot, nvec, sums_dev).wide(ctx->wide_bits, v_begin, v_end - v_begin));
}

int msm_hip_launch_windows_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int w_begin, int w_end, int slot,
                                        void* window_sums_dev) {
  return msm_hip_launch_windows_batch_device(ctx, scalars_dev, n, 1, w_begin, w_end, slot, window_sums_dev);
}

int msm_hip_launch_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int slot) { return launch_dense(ctx, LaunchRequest(scalars_dev, n, slot)); }

int msm_hip_launch_sparse_device(msm_hip_ctx* ctx, const uint32_t* indices_dev, const void* scalars_dev, size_t nnz, int slot) {
  LaunchRequest r(scalars_dev, nnz, slot);
  r.indices = indices_dev;
  return launch_sparse(ctx, r);
}

int msm_hip_run_sparse_device(msm_hip_ctx* ctx, const uint32_t* indices_dev, const void* scalars_dev, size_t nnz, uint8_t out_xyz[96]) {
  if (ctx && !out_xyz) return MSM_HIP_ERR_INVALID_ARG;
  LaunchRequest r(scalars_dev, nnz);
  r.indices = indices_dev;
  return run_sync(ctx, launch_sparse, r, out_xyz);
}

int msm_hip_slot_wait_stream(msm_hip_ctx* ctx, int slot, void* foreign_stream) {
  if (!ctx || slot < 0 || slot >= NSLOT) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  HIP_TRY(ctx, hipStreamWaitEvent(static_cast<hipStream_t>(foreign_stream), ctx->slot[slot].done, 0));
  return MSM_HIP_OK;
}

int msm_hip_slot_sync(msm_hip_ctx* ctx, int slot) {
  if (!ctx || slot < 0 || slot >= NSLOT) return MSM_HIP_ERR_INVALID_ARG;
  Slot& s = ctx->slot[slot];
  if (!s.pending) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  return wait_slot(ctx, s);
}

int msm_hip_finish_batch(msm_hip_ctx* ctx, int slot, uint8_t* out_xyz) {
  if (!ctx || !out_xyz || slot < 0 || slot >= NSLOT) return MSM_HIP_ERR_INVALID_ARG;
  Slot& s = ctx->slot[slot];
  const LaunchPlan& p = s.plan;
  const int nwin = p.nwin;
  if (!s.pending || !s.to_host || !p.whole) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  int rc = wait_slot(ctx, s);
  if (rc) return rc;
  auto t0 = std::chrono::steady_clock::now();
  std::atomic<bool> all_ok{true};
  if (s.parts) {  // one MSM (wide tables: up to 12), its windows as bit-plane sums: the windows' positional sums side by side, then the chain over them
    uint8_t sums[24 * MAX_JB];
    const size_t jb = ctx->jb;
    const int total = p.wide_bits ? p.nvec * nwin : nwin;
    combine_pool().run(total, [&](int w) {
      if (!ctx->ops->window_from_planes(s.h_wsums + (size_t)w * PLANES_PER_WINDOW * jb, sums + jb * (size_t)w)) all_ok = false;
    });
    if (p.wide_bits) {  // V virtual windows: V sum_vw W_vw - sum_{j=0}^{V-2} (TC_0 + ... + TC_j) (host_g1.h: combine_wide_strided), one chain per MSM
      combine_pool().run(p.nvec, [&](int v) {
        if (!ctx->ops->combine_wide(sums + jb * (size_t)v * nwin, s.h_wsums + (size_t)v * nwin * PLANES_PER_WINDOW * jb, nwin, out_xyz + jb * (size_t)v)) all_ok = false;
      });
    } else if (!ctx->ops->combine_windows(sums, nwin, p.combine_bits, out_xyz)) all_ok = false;
  } else {
    combine_pool().run(p.nvec, [&](int v) {  // one independent Horner chain per MSM of the launch: side by side when there are several
      if (!ctx->ops->combine_windows(s.h_wsums + (size_t)v * nwin * ctx->jb, nwin, p.combine_bits, out_xyz + ctx->jb * (size_t)v)) all_ok = false;
    });
  }
  if (!all_ok) return MSM_HIP_ERR_HIP;
  ctx->stage_ms[8] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return MSM_HIP_OK;
}

int msm_hip_finish(msm_hip_ctx* ctx, int slot, uint8_t out_xyz[96]) {
  if (!ctx || slot < 0 || slot >= NSLOT || ctx->slot[slot].plan.nvec != 1) return MSM_HIP_ERR_INVALID_ARG;
  return msm_hip_finish_batch(ctx, slot, out_xyz);
}

int msm_hip_run_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, uint8_t out_xyz[96]) {
  if (!out_xyz || !ctx) return MSM_HIP_ERR_INVALID_ARG;
  return run_sync(ctx, launch_dense, LaunchRequest(scalars_dev, n), out_xyz);
}

}  // extern "C"

namespace {
// The host inputs of a launch -> slot `s`'s own staging buffer (the slot must be idle, so nothing is reading it; set up here on first use; its
// capacity counts 32-byte scalars) on copy stream `cs` (null: the context's own, created on first use), so that the copy overlaps whatever the main
// and reduce streams still hold of earlier launches (a caller that alternates two slots gets the copy of MSM i+1 under the device work of MSM i);
// the main stream waits for it on the device.  From pageable memory the call returns when the bytes have left the caller's buffer; from pinned
// memory (hipHostMalloc / hipHostRegister) at once -- the buffer must then stay untouched until finish / slot_sync.
// `sbytes` bytes of scalars to s.d_host_scalars and, for a sparse launch, its nnz indices behind them (256-byte aligned), to *d_idx.
int stage_host(msm_hip_ctx* ctx, Slot& s, const void* scalars_host, size_t sbytes, hipStream_t cs = nullptr, const uint32_t* indices_host = nullptr,
               size_t nnz = 0, const uint32_t** d_idx = nullptr) {
  if (s.pending) return MSM_HIP_ERR_SLOT_BUSY;
  int rc = setup_slot(ctx, s);
  if (rc) return rc;
  if (!cs) {
    if (!ctx->copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    cs = ctx->copy_stream;
  }
  const size_t off = (sbytes + 255) & ~(size_t)255, total = indices_host ? off + nnz * 4 : sbytes;
  if ((rc = grow(ctx, s.cap_host_scalars, (total + 31) / 32, false, [&](size_t c) { return dev_alloc(ctx, s.d_host_scalars, c * 8); }))) return rc;
  uint8_t* base = reinterpret_cast<uint8_t*>(s.d_host_scalars);
  HIP_TRY(ctx, hipMemcpyAsync(base, scalars_host, sbytes, hipMemcpyHostToDevice, cs));
  if (indices_host) {
    HIP_TRY(ctx, hipMemcpyAsync(base + off, indices_host, nnz * 4, hipMemcpyHostToDevice, cs));
    *d_idx = reinterpret_cast<const uint32_t*>(base + off);
  }
  HIP_TRY(ctx, hipEventRecord(s.staged, cs));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s.staged, 0));
  return MSM_HIP_OK;
}

// one whole MSM from host scalars (r.scalars; narrow formats cross the link as they are, never widened on the host): staged, then as launch_dense
int launch_host(msm_hip_ctx* ctx, LaunchRequest r) {
  int rc = check_run_args(ctx, r.scalars, r.n);
  if (rc) return rc;
  if (r.slot < 0 || r.slot >= NSLOT) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  Slot& s = ctx->slot[r.slot];
  if (r.n) {
    const int nb = narrow_bytes(ctx->scalar_format);
    if ((rc = stage_host(ctx, s, r.scalars, r.n * (nb ? (size_t)nb : 32)))) return rc;
    r.scalars = s.d_host_scalars;
  }
  return launch_dense(ctx, r);
}

// first point of part k of n points split into `parts` ranges (the first n % parts ranges take one more)
inline size_t part_first(size_t n, int parts, int k) { return n / parts * k + std::min(n % parts, (size_t)k); }
}  // namespace

extern "C" {

int msm_hip_launch(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, int slot) { return launch_host(ctx, LaunchRequest(scalars_host, n, slot)); }

int msm_hip_run(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, uint8_t out_xyz[96]) {
  if (!out_xyz || !ctx) return MSM_HIP_ERR_INVALID_ARG;
  // Parts (round 5): 32 n bytes over the host link come before anything can run.  From 2^19 points on the call is the sum of sub-MSMs over
  // ranges of the points, one result slot each: part k + 1's scalars arrive while part k is sorted and accumulated, and the results are added
  // on the host.  (Not with fixed-base tables: their launches are shaped by the table count.)
  // (Nor with narrow scalars: 1 - 16 bytes per point leave no upload worth hiding, and the parts below step through 32-byte scalars.)
  int parts = ctx->precomputed || ctx->wide_bits || narrow_bytes(ctx->scalar_format) || !scalars_host ? 1 : upload_parts(n, NSLOT, 20, 22);  // (2^20: 2.44 -> 2.38 ms, 2^22: 8.61 -> 6.91; 2^19: slower)
  for (int k = 0; k < parts; k++)
    if (ctx->slot[k].pending) parts = 1;  // the caller has launches of its own in flight: the plain path (which reports a busy slot 0)
  g_probe_upload_parts.store(parts > 1 && n <= ctx->n_bases ? parts : 1);
  g_probe_upload_chunks.store(0);
  if (parts > 1 && n <= ctx->n_bases) {
    uint8_t sums[NSLOT * MAX_JB];
    int rc = MSM_HIP_OK, launched = 0;
    for (int k = 0; k < parts && !rc; k++) {
      const size_t first = part_first(n, parts, k), next = part_first(n, parts, k + 1);
      LaunchRequest r(scalars_host + first * 32, next - first, k);
      r.base_off = first;
      rc = launch_host(ctx, r);
      if (!rc) launched++;
    }
    for (int k = 0; k < launched; k++) {
      const int frc = msm_hip_finish(ctx, k, sums + (size_t)k * ctx->jb);
      if (!rc) rc = frc;
    }
    if (!rc && !ctx->ops->combine_windows(sums, parts, 0, out_xyz)) rc = MSM_HIP_ERR_NONCANONICAL;  // (window_bits = 0: the plain sum)
    return rc;
  }
  return run_sync(ctx, launch_host, LaunchRequest(scalars_host, n), out_xyz);
}

// Host inputs of a sparse MSM: the indices are checked here, before anything is enqueued; one upload of both arrays into slot 0's staging buffer
// and one launch (the part-splitting of msm_hip_run splits base ranges: not for sparse entries)
int msm_hip_run_sparse(msm_hip_ctx* ctx, const uint32_t* indices_host, const uint8_t* scalars_host, size_t nnz, uint8_t out_xyz[96]) {
  if (!ctx) return no_context_code();
  if (!out_xyz || (nnz && (!indices_host || !scalars_host)) || nnz > MAX_POINTS || ctx->wide_bits) return MSM_HIP_ERR_INVALID_ARG;
  if (nnz == 0) return msm_hip_run_sparse_device(ctx, nullptr, nullptr, 0, out_xyz);
  if (ctx->n_bases == 0) return MSM_HIP_ERR_NO_BASES;
  for (size_t j = 0; j < nnz; j++)
    if (indices_host[j] >= ctx->n_bases) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  Slot& s = ctx->slot[0];
  const int nb = narrow_bytes(ctx->scalar_format);
  const uint32_t* d_idx = nullptr;
  if (const int rc = stage_host(ctx, s, scalars_host, nnz * (nb ? (size_t)nb : 32), nullptr, indices_host, nnz, &d_idx)) return rc;
  return msm_hip_run_sparse_device(ctx, d_idx, s.d_host_scalars, nnz, out_xyz);
}

int msm_hip_run_batch_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, size_t batch, uint8_t* out_xyz) {
  if (!out_xyz && batch) return MSM_HIP_ERR_INVALID_ARG;
  int rc = check_run_args(ctx, scalars_dev, n);
  if (rc) return rc;
  const uint8_t* sc = static_cast<const uint8_t*>(scalars_dev);
  const size_t sbytes = narrow_bytes(ctx->scalar_format) ? (size_t)narrow_bytes(ctx->scalar_format) : 32;  // (a vector: n x sbytes)
  return run_batch_groups(ctx, n, batch, out_xyz, [&](size_t, size_t first, size_t, const void** dev) {
    *dev = sc + first * n * sbytes;
    return (int)MSM_HIP_OK;
  });
}

int msm_hip_run_batch(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, size_t batch, uint8_t* out_xyz) {
  if (!out_xyz && batch) return MSM_HIP_ERR_INVALID_ARG;
  int rc = check_run_args(ctx, scalars_host, n);
  if (rc) return rc;
  if (n == 0) {
    if (batch) memset(out_xyz, 0, ctx->jb * batch);
    return MSM_HIP_OK;
  }
  ON_DEVICE(ctx);
  const size_t vec = n * (narrow_bytes(ctx->scalar_format) ? (size_t)narrow_bytes(ctx->scalar_format) : 32), entry = vec * batch_group(ctx, n, batch);
  if ((rc = grow(ctx, ctx->cap_batch_stage, entry * NSLOT, true, [&](size_t c) { return dev_alloc(ctx, ctx->d_batch_stage, c); }))) return rc;
  // group j is staged in ring entry j % NSLOT on the main stream just ahead of its own sort (the entry's previous
  // reader, group j - NSLOT, was finished DEPTH + 1 iterations ago)
  return run_batch_groups(ctx, n, batch, out_xyz, [&](size_t j, size_t first, size_t count, const void** dev) {
    uint8_t* stage = ctx->d_batch_stage + (j % NSLOT) * entry;
    if (hipMemcpyAsync(stage, scalars_host + first * vec, count * vec, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      return (int)MSM_HIP_ERR_HIP;
    *dev = stage;
    return (int)MSM_HIP_OK;
  });
}

int msm_hip_run_windows_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int w_begin, int w_end,
                                     void* window_sums_dev) {
  if (!window_sums_dev) return MSM_HIP_ERR_INVALID_ARG;
  int rc = msm_hip_launch_windows_device(ctx, scalars_dev, n, w_begin, w_end, 0, window_sums_dev);
  if (rc) return rc;
  return msm_hip_slot_sync(ctx, 0);
}

int msm_hip_combine_windows_bn254(const uint8_t* window_sums_host, int num_windows, uint8_t out_xyz[96]) {
  if (!window_sums_host || !out_xyz || num_windows < 1 || num_windows > NWIN) return MSM_HIP_ERR_INVALID_ARG;
  if (!curve_ops(MSM_HIP_CURVE_BN254_G1)->combine_windows(window_sums_host, num_windows, WBITS, out_xyz)) return MSM_HIP_ERR_NONCANONICAL;
  return MSM_HIP_OK;
}

int msm_hip_combine_windows_batch_curve(int curve, const uint8_t* window_sums_host, int num_windows, int nvec, uint8_t* out_xyz) {
  if (curve < 0 || curve >= MSM_HIP_NUM_CURVES) return MSM_HIP_ERR_INVALID_ARG;
  if (!window_sums_host || !out_xyz || num_windows < 1 || num_windows > NWIN || nvec < 0) return MSM_HIP_ERR_INVALID_ARG;
  const CurveOps* ops = curve_ops(curve);
  const size_t jb = 12 * (size_t)ops->coord_words;
  std::atomic<bool> ok{true};
  // independent Horner chains (47 us each on one core): side by side on the combine pool when there are several
  combine_pool().run(nvec, [&](int v) {
    if (!ops->combine_windows(window_sums_host + (size_t)v * num_windows * jb, num_windows, WBITS, out_xyz + (size_t)v * jb)) ok = false;
  });
  return ok ? MSM_HIP_OK : MSM_HIP_ERR_NONCANONICAL;
}

int msm_hip_combine_vwindows_batch_curve(int curve, const uint8_t* pairs_host, int num_vwindows, int nvec, uint8_t* out_xyz) {
  if (curve < 0 || curve >= MSM_HIP_NUM_CURVES) return MSM_HIP_ERR_INVALID_ARG;
  if (!pairs_host || !out_xyz || num_vwindows < 1 || num_vwindows > 16 || nvec < 0) return MSM_HIP_ERR_INVALID_ARG;
  const CurveOps* ops = curve_ops(curve);
  const size_t jb = 12 * (size_t)ops->coord_words;
  std::atomic<bool> ok{true};
  combine_pool().run(nvec, [&](int v) {  // one short chain per MSM (2 additions per virtual window + 15 doublings), side by side
    if (!ops->combine_wide_pairs(pairs_host + (size_t)v * num_vwindows * 2 * jb, num_vwindows, out_xyz + (size_t)v * jb)) ok = false;
  });
  return ok ? MSM_HIP_OK : MSM_HIP_ERR_NONCANONICAL;
}

int msm_hip_g1_to_affine_bn254(const uint8_t xyz[96], uint8_t out_xy[64]) {
  if (!xyz || !out_xy) return MSM_HIP_ERR_INVALID_ARG;
  const int r = curve_ops(MSM_HIP_CURVE_BN254_G1)->to_affine64(xyz, out_xy);
  return r < 0 ? MSM_HIP_ERR_NONCANONICAL : r;
}

int msm_hip_combine_windows_curve(int curve, const uint8_t* window_sums_host, int num_windows, uint8_t out_xyz[96]) {
  if (curve < 0 || curve >= MSM_HIP_NUM_CURVES) return MSM_HIP_ERR_INVALID_ARG;
  if (!window_sums_host || !out_xyz || num_windows < 1 || num_windows > NWIN) return MSM_HIP_ERR_INVALID_ARG;
  if (!curve_ops(curve)->combine_windows(window_sums_host, num_windows, WBITS, out_xyz)) return MSM_HIP_ERR_NONCANONICAL;
  return MSM_HIP_OK;
}

int msm_hip_g1_to_affine_curve(int curve, const uint8_t xyz[96], uint8_t out_xy[64]) {
  if (curve < 0 || curve >= MSM_HIP_NUM_CURVES) return MSM_HIP_ERR_INVALID_ARG;
  if (!xyz || !out_xy) return MSM_HIP_ERR_INVALID_ARG;
  const int r = curve_ops(curve)->to_affine64(xyz, out_xy);
  return r < 0 ? MSM_HIP_ERR_NONCANONICAL : r;
}

// The one-shot keeps ONE context per device alive between calls (the reference creates and drops its wgpu device on every call,
// src/cuzk/msm.rs:88-94; here that costs 0.3 ms of creation, ~1 ms of first-use allocations and 3.4 ms of hipFree per call --
// more than the MSM).  Process-wide, mutex-protected (one-shot calls on one device are serialised, as a context requires);
// msm_hip_oneshot_release() drops the kept contexts; MSM_HIP_ONESHOT_KEEP=0 restores create / destroy per call.
namespace {
constexpr int ONESHOT_MAX_DEVICES = 64;
constexpr int ONESHOT_MAX_PARTS = 4;  // contexts per (curve, device): a large one-shot MSM runs as up to this many sub-MSMs over ranges of the points (below)
std::mutex g_oneshot_mutex;
msm_hip_ctx* g_oneshot_ctx[MSM_HIP_NUM_CURVES][ONESHOT_MAX_DEVICES][ONESHOT_MAX_PARTS] = {};
inline bool oneshot_keep() {
  static const bool v = [] { const char* e = getenv("MSM_HIP_ONESHOT_KEEP"); return !(e && e[0] == '0'); }();
  return v;
}
inline bool oneshot_overlap() {
  static const bool v = [] { const char* e = getenv("MSM_HIP_ONESHOT_OVERLAP"); return !e || atoi(e) != 0; }();
  return v;
}
inline size_t oneshot_chunk() {  // points per upload chunk of the overlapped one-shot call (MSM_HIP_ONESHOT_CHUNK_LOG: tuning aid)
  static const size_t v = [] {
    const char* e = getenv("MSM_HIP_ONESHOT_CHUNK_LOG");
    const int l = e ? atoi(e) : 18;
    return (size_t)1 << (l >= 10 && l <= 28 ? l : 18);
  }();
  return v;
}
}  // namespace

}  // extern "C"

namespace {
// The one-shot call on a kept (or fresh) context, OVERLAPPED (round 5): the reference uploads everything, then dispatches (src/cuzk/msm.rs:84-94,
// 441-480); here the 32 n bytes of scalars go first and their recode + sort (everything that needs the scalars alone: enqueue_sort) runs while
// the 64 n bytes of points are still arriving -- in chunks on the copy stream, each converted to the device form (and its endomorphism image
// made) as soon as it has landed --, and only the SMVP (enqueue_reduce) waits for the last chunk.  Hidden: the sort (~0.26 ms at 2^20), the
// conversion kernels (~0.1 ms) and one host synchronisation.  MSM_HIP_ONESHOT_OVERLAP=0: upload, convert, then run (rounds 1 - 4).
// Two halves: oneshot_enqueue queues everything (copies on `cs` -- the copy stream of the call's FIRST part, so that the parts' uploads follow each
// other instead of sharing the link -- and both launch stages), oneshot_collect waits for the result.  `he_out`: the first HIP error of the
// chunk loop (the launch is completed regardless, its result discarded).
int oneshot_enqueue(msm_hip_ctx* ctx, hipStream_t cs, const uint8_t* xy_host, const uint8_t* scalars_host, size_t n, hipError_t* he_out, bool* queued) {
  ON_DEVICE(ctx);
  *he_out = hipSuccess;
  *queued = false;  // true: the launch was taken to its reduce stage -- oneshot_collect has to follow, whatever this function returns
  const uint32_t flags = resolve_base_flags(ctx, n, 0);
  const bool endo = (flags & MSM_HIP_BASES_ENDOMORPHISM) != 0;
  int rc = reserve_bases(ctx, n, flags);  // (waits for the main stream: nothing is reading the old bases)
  if (rc) return rc;
  Slot& s = ctx->slot[0];
  if (!ctx->bases_ready) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->bases_ready, hipEventDisableTiming));
  // 1. the scalars, and their sort
  if ((rc = stage_host(ctx, s, scalars_host, n * 32, cs))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, 4, cs));  // (ahead of every chunk's copy, hence of every conversion)
  ctx->n_bases = n;  // (what the launch checks n against, and with `endo` what shapes it; the records themselves follow below)
  ctx->endo = endo;
  LaunchRequest req = whole_msm_request(ctx, LaunchRequest(s.d_host_scalars, n));
  req.sync = true;
  LaunchPlan p;
  auto sort = [&]() -> int {
    int r = plan_launch(ctx, req, p);
    if (!r) r = ensure_work(ctx, p, s);
    if (!r) r = enqueue_sort(ctx, p, s, s.d_host_scalars);
    if (!r) HIP_TRY(ctx, hipGetLastError());
    return r;
  };
  if ((rc = sort())) {
    ctx->n_bases = 0;
    return rc;
  }
  // 2. the points behind the scalars on the copy stream, in a few chunks (2^18 points = 16 MiB: smaller ones cost the pageable copy path more
  //    than they hide, profiles/r05_oneshot.txt); every chunk is converted on ANOTHER stream (the second reduce stream, idle in this call shape)
  //    as soon as it has landed, so the copies follow each other without waiting for kernels
  const size_t chunk = oneshot_chunk();
  hipStream_t conv = ctx->reduce_stream[NREDUCE - 1];
  hipError_t he = hipSuccess;
  int k = 0;
  for (size_t first = 0; first < n && he == hipSuccess; first += chunk, k++) {
    const size_t count = n - first < chunk ? n - first : chunk;
    uint32_t* dst = ctx->d_bases + first * 2 * (size_t)ctx->ops->coord_words;
    hipEvent_t& landed = ctx->chunk_landed[k & 7];
    if (!landed && (he = hipEventCreateWithFlags(&landed, hipEventDisableTiming)) != hipSuccess) break;
    if ((he = hipMemcpyAsync(dst, xy_host + first * ctx->pb, count * ctx->pb, hipMemcpyHostToDevice, cs)) != hipSuccess) break;
    if ((he = hipEventRecord(landed, cs)) != hipSuccess) break;
    if ((he = hipStreamWaitEvent(conv, landed, 0)) != hipSuccess) break;
    hipLaunchKernelGGL(ctx->ops->convert_points, dim3(blocks_for(count, 256)), dim3(256), 0, conv, dst, dst, count, flags, ctx->d_err);
    if (endo) hipLaunchKernelGGL(ctx->ops->endo_points, dim3(blocks_for(count, 256)), dim3(256), 0, conv, ctx->d_bases, n, first, count);
    he = hipGetLastError();
  }
  if (k > g_probe_upload_chunks.load()) g_probe_upload_chunks.store(k);
  if (he == hipSuccess) he = hipEventRecord(ctx->bases_ready, conv);
  if (he == hipSuccess) he = hipStreamWaitEvent(ctx->stream, ctx->bases_ready, 0);
  // 3. the rest of the launch (on failure above too: the sort left the slot's streams mid-launch -- the bases it then reads are whatever arrived,
  //    and the result is discarded)
  *queued = true;
  rc = enqueue_reduce(ctx, p, s);
  *he_out = he;
  return rc;
}

// ... and the wait: the result of the part (discarded after a failure of its enqueue half), then the conversion's error word
int oneshot_collect(msm_hip_ctx* ctx, int rc, hipError_t he, uint8_t* out_xyz) {
  ON_DEVICE(ctx);
  hipStream_t conv = ctx->reduce_stream[NREDUCE - 1];
  uint8_t scratch[MAX_JB];
  const int frc = rc ? rc : msm_hip_finish(ctx, 0, he == hipSuccess ? out_xyz : scratch);
  uint32_t base_bits = 0;  // the conversion's error word (read last: the launch was queued behind the copy stream before the host waits for anything)
  if (he == hipSuccess) he = hipStreamSynchronize(conv);
  if (he == hipSuccess) he = hipMemcpy(&base_bits, ctx->d_err, 4, hipMemcpyDeviceToHost);
  if (he != hipSuccess) {
    ctx->last_hip_error = (int)he;
    ctx->n_bases = 0;
    return MSM_HIP_ERR_HIP;
  }
  if (const int brc = err_from_bits(base_bits)) {  // a non-canonical coordinate: the bases are not usable (as msm_hip_set_bases_* reports it)
    ctx->n_bases = 0;
    return brc;
  }
  return frc;
}
}  // namespace

extern "C" {

int msm_hip_msm_curve(int curve, const uint8_t* xy_host, const uint8_t* scalars_host, size_t n, uint8_t* out_xyz) {
  int dev = 0;
  if (curve < 0 || curve >= MSM_HIP_NUM_CURVES) return MSM_HIP_ERR_INVALID_ARG;
  if (hipGetDevice(&dev) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;  // the caller's current device (0 unless it chose another)
  if (!out_xyz || ((!xy_host || !scalars_host) && n)) return MSM_HIP_ERR_INVALID_ARG;
  const bool keep = oneshot_keep() && dev >= 0 && dev < ONESHOT_MAX_DEVICES;
  std::lock_guard<std::mutex> lock(g_oneshot_mutex);  // (also without `keep`: the part policy below is process-wide state)
  const bool overlap = oneshot_overlap();
  // Parts (round 5): a large one-shot MSM is upload-bound -- 96 n bytes over the host link against ~1 ms of SMVP at 2^20 --, and the SMVP cannot start
  // before the last point has arrived.  Sum over the points is sum over RANGES of the points: the call runs as `parts` sub-MSMs, each on a context
  // of its own, their uploads queued one behind the other on one copy stream, so that part k accumulates its buckets while part k + 1 is still
  // arriving and only the LAST part's SMVP (n / parts points) follows the upload.  The results are added on the host (parts - 1 additions).
  // 2 parts from 2^19 points on (MSM_HIP_ONESHOT_PARTS: tuning aid; more parts pay more per-part sorting, stitching and bucket reducing).
  const bool overlapped = overlap && n > 0 && n <= MAX_POINTS / 2;
  const int parts = overlapped ? upload_parts(n, ONESHOT_MAX_PARTS, 19, 30) : 1;  // (2^19: 2.00 -> 1.93 ms, 2^20: 3.55 -> 3.08, 2^22: 13.2 -> 11.1; three parts never better)
  g_probe_upload_parts.store(parts);
  g_probe_upload_chunks.store(0);  // (oneshot_enqueue: the most chunks of one part)
  msm_hip_ctx* ctxs[ONESHOT_MAX_PARTS] = {};
  int rc = MSM_HIP_OK;
  for (int k = 0; k < parts && !rc; k++) {
    if (keep) ctxs[k] = g_oneshot_ctx[curve][dev][k];
    if (!ctxs[k]) {
      rc = msm_hip_ctx_create_curve(&ctxs[k], dev, curve);
      if (!rc && keep) g_oneshot_ctx[curve][dev][k] = ctxs[k];
    }
  }
  if (!rc && !overlapped) {
    rc = msm_hip_set_bases(ctxs[0], xy_host, n, 0);
    if (!rc) rc = msm_hip_run(ctxs[0], scalars_host, n, out_xyz);
  } else if (!rc) {
    msm_hip_ctx* c0 = ctxs[0];
    if (!c0->copy_stream) {
      DeviceGuard guard(c0->device);
      if (hipStreamCreateWithFlags(&c0->copy_stream, hipStreamNonBlocking) != hipSuccess) rc = MSM_HIP_ERR_HIP;
    }
    int prc[ONESHOT_MAX_PARTS] = {};
    hipError_t phe[ONESHOT_MAX_PARTS] = {};
    bool queued[ONESHOT_MAX_PARTS] = {};
    uint8_t sums[ONESHOT_MAX_PARTS * MAX_JB];
    const size_t pb = c0->pb, jb = c0->jb;
    size_t first[ONESHOT_MAX_PARTS + 1];
    for (int k = 0; k <= parts; k++) first[k] = part_first(n, parts, k);
    for (int k = 0; k < parts && !rc; k++) {
      prc[k] = oneshot_enqueue(ctxs[k], c0->copy_stream, xy_host + first[k] * pb, scalars_host + first[k] * 32, first[k + 1] - first[k], &phe[k], &queued[k]);
      if (prc[k] && !queued[k]) rc = prc[k];  // nothing of this part is in flight: stop queueing, drain the earlier ones
    }
    for (int k = 0; k < parts; k++) {
      if (!queued[k]) continue;
      const int crc = oneshot_collect(ctxs[k], prc[k], phe[k], parts == 1 ? out_xyz : sums + (size_t)k * jb);
      if (!rc) rc = crc;
    }
    if (!rc && parts > 1 && !c0->ops->combine_windows(sums, parts, 0, out_xyz)) rc = MSM_HIP_ERR_NONCANONICAL;  // (window_bits = 0: the plain sum of the records)
  }
  if (!keep)
    for (msm_hip_ctx* c : ctxs)
      if (c) msm_hip_ctx_destroy(c);
  return rc;
}

int msm_hip_msm_bn254_g1(const uint8_t* xy_host, const uint8_t* scalars_host, size_t n, uint8_t out_xyz[96]) {
  return msm_hip_msm_curve(MSM_HIP_CURVE_BN254_G1, xy_host, scalars_host, n, out_xyz);
}

// test hook: the one-shot call's part policy (0, 0 restores the default: 2 parts from 2^19 points on) -- lets a test run several parts on small inputs
int msm_hip_test_oneshot_parts(int parts, size_t min_points) {
  if (parts < 0 || parts > ONESHOT_MAX_PARTS) return MSM_HIP_ERR_INVALID_ARG;
  g_oneshot_parts.store(parts);
  g_oneshot_parts_min_n.store(min_points);
  return MSM_HIP_OK;
}

void msm_hip_oneshot_release(void) {
  std::lock_guard<std::mutex> lock(g_oneshot_mutex);
  for (auto& per_curve : g_oneshot_ctx)
    for (auto& per_device : per_curve)
      for (msm_hip_ctx*& c : per_device) {
        if (c) msm_hip_ctx_destroy(c);
        c = nullptr;
      }
}

int msm_hip_sample_scalars_device(msm_hip_ctx* ctx, uint64_t seed, size_t n, void* scalars_dev) {
  if (!ctx || (!scalars_dev && n)) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  hipLaunchKernelGGL(ctx->ops->sample_scalars, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, seed, n, static_cast<uint32_t*>(scalars_dev));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_sample_points_device(msm_hip_ctx* ctx, uint64_t seed, size_t n, void* xy_dev) {
  if (!ctx || (!xy_dev && n)) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0) return MSM_HIP_OK;
  if (!ctx->ops->sample_points) return MSM_HIP_ERR_INVALID_ARG;  // (no device sampler for this curve: none at present)
  ON_DEVICE(ctx);
  hipLaunchKernelGGL(ctx->ops->sample_points, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, seed, n, static_cast<uint32_t*>(xy_dev));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_last_stage_ms(msm_hip_ctx* ctx, float* ms, int cap) {
  if (!ctx || !ms) return MSM_HIP_ERR_INVALID_ARG;
  int k = cap < 9 ? cap : 9;
  for (int i = 0; i < k; i++) ms[i] = ctx->stage_ms[i];
  return k;
}

// ---- stage read-back ------------------------------------------------------------------------------------------------
static int read_back(msm_hip_ctx* ctx, void* out, const void* src, size_t bytes, size_t cap_bytes) {
  if (!ctx || !out) return MSM_HIP_ERR_INVALID_ARG;
  if (bytes > cap_bytes) return MSM_HIP_ERR_INVALID_ARG;
  if (bytes == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  for (hipStream_t r : ctx->reduce_stream) HIP_TRY(ctx, hipStreamSynchronize(r));
  HIP_TRY(ctx, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_set_stage_timing(msm_hip_ctx* ctx, int level) {
  if (!ctx || level < 0 || level > 2) return MSM_HIP_ERR_INVALID_ARG;
  ctx->timing_level = level;
  return MSM_HIP_OK;
}

int msm_hip_set_scalar_format(msm_hip_ctx* ctx, uint32_t format) {
  if (!ctx || (format != MSM_HIP_SCALARS_CANONICAL && format != MSM_HIP_SCALARS_MONT256 && !narrow_bytes(format))) return MSM_HIP_ERR_INVALID_ARG;
  if (format == MSM_HIP_SCALARS_MONT256 && !ctx->ops->scalars_from_mont256) return MSM_HIP_ERR_INVALID_ARG;
  ctx->scalar_format = format;
  return MSM_HIP_OK;
}

int msm_hip_set_window_bits(msm_hip_ctx* ctx, int bits) {
  if (!ctx || (bits != 0 && bits != 12 && bits != 14 && bits != 16)) return MSM_HIP_ERR_INVALID_ARG;
  ctx->window_bits = bits;
  return MSM_HIP_OK;
}

int msm_hip_set_wide_bits(msm_hip_ctx* ctx, int bits) {
  if (!ctx || (bits != 0 && (bits < 16 || bits > 20))) return MSM_HIP_ERR_INVALID_ARG;
  ctx->wide_bits_choice = bits;
  return MSM_HIP_OK;
}

int msm_hip_wide_bits(const msm_hip_ctx* ctx) { return ctx ? ctx->wide_bits : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_wide_config(int curve, int bits, size_t n, int* digit_bits, int* tables, int* virtual_windows, int* top_shift) {
  if (curve < MSM_HIP_CURVE_BN254_G1 || curve > MSM_HIP_CURVE_BLS12_381_G2 || (bits != 0 && (bits < 16 || bits > 20))) return MSM_HIP_ERR_INVALID_ARG;
  msm_hip_ctx probe;  // (only the two fields the policy reads)
  probe.curve = curve;
  probe.wide_bits_choice = bits;
  const int wb = pick_wide_bits(&probe, n);
  if (wb < 0) return MSM_HIP_ERR_INVALID_ARG;
  if (digit_bits) *digit_bits = wb;
  if (tables) *tables = wide_tables_of(wb);
  if (virtual_windows) *virtual_windows = wide_vwin_of(wb);
  if (top_shift) *top_shift = wide_top_shift(curve, wb);
  return MSM_HIP_OK;
}

int msm_hip_window_config(int bits, int* num_windows, int* buckets_per_window) {
  if (bits != 12 && bits != 14 && bits != 16) return MSM_HIP_ERR_INVALID_ARG;
  if (num_windows) *num_windows = nwin_of(bits);
  if (buckets_per_window) *buckets_per_window = 1 << (bits - 1);
  return MSM_HIP_OK;
}

int msm_hip_last_window_bits(msm_hip_ctx* ctx) { return ctx ? ctx->last.wbits : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_endomorphism_window_count(int bits) {
  if (bits != 12 && bits != 14 && bits != 16) return MSM_HIP_ERR_INVALID_ARG;
  return nwin_of(bits, true);
}

int msm_hip_uses_endomorphism(const msm_hip_ctx* ctx) { return ctx ? (ctx->endo ? 1 : 0) : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_batch_group_size(msm_hip_ctx* ctx, size_t n) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  return (int)batch_group(ctx, n, (size_t)MAXLW);
}

int msm_hip_set_fine_hist_min_n(msm_hip_ctx* ctx, size_t n) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  ctx->fine_hist_min_n = n;
  return MSM_HIP_OK;
}

int msm_hip_test_skew_credit(const msm_hip_ctx* ctx) { return ctx ? ctx->skew_credit : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_test_env_report(const msm_hip_ctx* ctx, char* out, size_t cap) {
  if (!out || !cap) return MSM_HIP_ERR_INVALID_ARG;
  size_t len = 0;
  bool fits = true;
  auto put = [&](const char* key, long long v) {
    const int w = snprintf(out + len, cap - len, "%s=%lld\n", key, v);
    if (w < 0 || (size_t)w >= cap - len) fits = false;
    else len += (size_t)w;
  };
  // the settings as the library resolved them (read once per process)
  put("target_lanes", (long long)target_lanes());
  put("chunk_search", chunk_search());
  put("window_bits", env_window_bits());
  put("bpr_logr", bpr_force_logr());
  put("planes_max_w", planes_max_w());
  put("planes_whole", planes_whole());
  put("inline_reduce", inline_reduce_on());
  put("reduce_priority", reduce_priority_on());
  put("smvp_lds_pad", smvp_lds_pad());
  put("bases_auto", bases_auto());
  put("debug_sync", debug_sync());
  put("wide_bits", env_wide_bits());
  put("wide_top_shift", env_wide_top_shift());
  put("wide_slack_ppm", llround(wide_slack() * 1e6));
  put("wide_share_lists", wide_share_lists());
  put("oneshot_parts", env_oneshot_parts());
  put("oneshot_keep", oneshot_keep());
  put("oneshot_overlap", oneshot_overlap());
  put("oneshot_chunk", (long long)oneshot_chunk());
  put("combine_helpers", CombinePool::helpers_wanted());
  put("combine_started", combine_pool().helpers_started());
  // the last upload-bound call (msm_hip_msm_curve, msm_hip_run): its parts and the most upload chunks of one part
  put("upload_parts", g_probe_upload_parts.load());
  put("upload_chunks", g_probe_upload_chunks.load());
  if (ctx) {  // the context's last launch
    put("fine_hist_min_n", (long long)ctx->fine_hist_min_n);
    put("last_wbits", ctx->last.wbits);
    put("last_chunk_len", ctx->last.chunk_len);
    put("last_chunks", ctx->last.chunks);
    put("last_planes", ctx->last.planes);
    put("last_list_path", ctx->last.list_path);
    put("last_mode", ctx->last.mode);
    put("last_w_count", ctx->last.w_count);
    put("last_wide_top_shift", ctx->last.mode == MODE_WIDE ? wide_top_shift(ctx->curve, ctx->last.wide_bits) : 0);
    put("last_logr", ctx->last_logr);
    put("last_inline_reduce", ctx->last_inline_reduce);
    put("last_fine_hist", ctx->last.fine_hist);
    put("last_identity_mask", ctx->last.mask);
  }
  return fits ? (int)len : MSM_HIP_ERR_INVALID_ARG;
}

int msm_hip_set_debug(msm_hip_ctx* ctx, int keep_digit_planes) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  ctx->debug = keep_digit_planes != 0;
  return MSM_HIP_OK;
}

int msm_hip_read_digits(msm_hip_ctx* ctx, uint16_t* out, size_t cap_elems) {
  if (!ctx || !ctx->last.digits) return MSM_HIP_ERR_INVALID_ARG;
  return read_back(ctx, out, ctx->d_digits, ctx->last.n_sc * ctx->last.w_count * 2, cap_elems * 2);
}
int msm_hip_read_col_ptr(msm_hip_ctx* ctx, uint32_t* out, size_t cap_elems) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t half = (size_t)1 << (ctx->last.wbits - 1);  // [w][half + 1]
  return read_back(ctx, out, ctx->slot[ctx->last_slot].d_col_ptr, (size_t)ctx->last.w_count * (half + 1) * 4, cap_elems * 4);
}
int msm_hip_read_val_idxs(msm_hip_ctx* ctx, uint32_t* out, size_t cap_elems) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  // out[w][n]; only the first col_ptr[w][32768] entries of each window are meaningful
  const size_t n = ctx->last.n_sc;
  if (!out || n * ctx->last.w_count > cap_elems) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  HIP_TRY(ctx, hipMemcpy2DAsync(out, n * 4, ctx->d_val, ctx->last.stride * 4, n * 4, (size_t)ctx->last.w_count, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_read_buckets(msm_hip_ctx* ctx, uint8_t* out, size_t cap_bytes) {
  if (!ctx || !out) return MSM_HIP_ERR_INVALID_ARG;
  const size_t count = (size_t)ctx->last.w_count << (ctx->last.wbits - 1);  // [w][2^(bits-1)]
  if (count * ctx->jb > cap_bytes) return MSM_HIP_ERR_INVALID_ARG;
  if (count == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  for (hipStream_t r : ctx->reduce_stream) HIP_TRY(ctx, hipStreamSynchronize(r));
  int rc = ensure_stage(ctx, count * ctx->jb);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->export_buckets, dim3(blocks_for(count, 256)), dim3(256), 0, ctx->stream, ctx->slot[ctx->last_slot].d_buckets,
                     reinterpret_cast<uint32_t*>(ctx->d_stage), count);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, ctx->d_stage, count * ctx->jb, cap_bytes);
}

int msm_hip_read_window_sums(msm_hip_ctx* ctx, uint8_t* out, size_t cap_bytes) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const Slot& s = ctx->slot[ctx->last_slot];
  if (!s.parts) return read_back(ctx, out, s.d_wsums, (size_t)ctx->last.w_count * ctx->jb, cap_bytes);
  // the last launch handed its window sums to the host as bit-plane sums (k_bpr_planes): finish them here
  const size_t w = (size_t)ctx->last.w_count;
  if (!out || w * ctx->jb > cap_bytes || w > 24) return MSM_HIP_ERR_INVALID_ARG;
  const size_t plane_bytes = PLANES_PER_WINDOW * ctx->jb;
  {  // (the plane sums were written into the slot's pinned buffer by the launch's last kernel: complete once its reduce stream has drained)
    ON_DEVICE(ctx);
    for (hipStream_t r : ctx->reduce_stream) HIP_TRY(ctx, hipStreamSynchronize(r));
  }
  const uint8_t* planes = s.h_wsums;
  bool ok = true;
  for (size_t k = 0; k < w; k++) ok &= ctx->ops->window_from_planes(planes + k * plane_bytes, out + k * ctx->jb);
  return ok ? MSM_HIP_OK : MSM_HIP_ERR_NONCANONICAL;
}

// ---- op hooks -------------------------------------------------------------------------------------------------------
static int run_hook(msm_hip_ctx* ctx, const uint8_t* a, size_t a_bytes, const uint8_t* b, size_t b_bytes, uint8_t* out,
                    size_t out_bytes, uint8_t*& da, uint8_t*& db, uint8_t*& dout) {
  if (!ctx || !a || !out) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  int rc = ensure_stage(ctx, up16(a_bytes) + up16(b_bytes) + up16(out_bytes) + 16);
  if (rc) return rc;
  da = ctx->d_stage;
  db = da + up16(a_bytes);
  dout = db + up16(b_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(da, a, a_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (b && b_bytes) HIP_TRY(ctx, hipMemcpyAsync(db, b, b_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!b) db = nullptr;
  return MSM_HIP_OK;
}

int msm_hip_test_fq_op(msm_hip_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  if (n == 0) return MSM_HIP_OK;
  if (op < 0 || op > 9) return MSM_HIP_ERR_INVALID_ARG;
  uint8_t *da, *db, *dout;
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t cb = ctx->cb;
  int rc = run_hook(ctx, a, n * cb, b, b ? n * cb : 0, out, n * cb, da, db, dout);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->test_fq, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, op, (const uint32_t*)da, (const uint32_t*)db,
                     (uint32_t*)dout, n);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, dout, n * cb, n * cb);
}

int msm_hip_test_g1_op(msm_hip_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  if (n == 0) return MSM_HIP_OK;
  if (op < 0 || op > 4 || (op != 1 && !b)) return MSM_HIP_ERR_INVALID_ARG;
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t jb = ctx->jb;
  const size_t b_bytes = op == 0 ? n * jb : (op >= 2 ? n * ctx->pb : 0);
  uint8_t *da, *db, *dout;
  int rc = run_hook(ctx, a, n * jb, op == 1 ? nullptr : b, b_bytes, out, n * jb, da, db, dout);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->test_g1, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, op, (const uint32_t*)da, (const uint32_t*)db,
                     (uint32_t*)dout, n);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, dout, n * jb, n * jb);
}

int msm_hip_test_g1_mul_u32(msm_hip_ctx* ctx, const uint8_t* a, const uint32_t* k, uint8_t* out, size_t n) {
  if (n == 0) return MSM_HIP_OK;
  if (!k) return MSM_HIP_ERR_INVALID_ARG;
  uint8_t *da, *db, *dout;
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t jb = ctx->jb;
  int rc = run_hook(ctx, a, n * jb, reinterpret_cast<const uint8_t*>(k), n * 4, out, n * jb, da, db, dout);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->test_g1_mul_u32, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)da,
                     (const uint32_t*)db, (uint32_t*)dout, n);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, dout, n * jb, n * jb);
}

}  // extern "C"

// ---- batch scalar multiplication: out[i] = s_i * P_i (mul_each) and out[i] = s_i * P_base (mul_base) ------------------------------------------
namespace {
constexpr size_t MUL_TILE = (size_t)1 << 20;  // outputs per kernel pair: bounds the scratch (Z values + prefix products: 64 MiB on BN254 G1) whatever n is

inline bool prime_order_curve(int curve) {
  return curve == MSM_HIP_CURVE_BN254_G1 || curve == MSM_HIP_CURVE_GRUMPKIN || curve == MSM_HIP_CURVE_PALLAS || curve == MSM_HIP_CURVE_VESTA;
}
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// The fixed-base table of msm_hip_mul_base: which digit width C, if any, serves n outputs of base `base`.  Measured on BN254 G1 (profiles/mul_each.txt,
// tools/bench_mul.py --crossover: broadcast ladder against the table forced at C = 8 .. 16, n = 2^10 .. 2^20, the building call timed apart):
//   - a table the context already holds beats the ladder at every n (0.34 against 1.23 ms at 2^10, 1.2 - 2.2 against 14.4 ms at 2^20): it is reused;
//   - a call that has to build its table loses to the ladder up to 2^16 (1.64 against 1.39 ms) and wins from 2^18 (1.87 against 4.01 ms): the
//     threshold is 2^17;
//   - with the build in the call, C = 12 is the fastest width at 2^18 and 2^20 (2.87 ms; C = 10: 3.10, C = 14: 3.73, C = 16: 6.73).  A wider table
//     costs 1.0 ms (C = 14) and 4.2 ms (C = 16) more to build than C = 12 and saves 0.13 and 0.33 ns per output: C = 14 from 2^23, C = 16 from 2^24.
// C <= 16: at most W 2^15 records, 32 MiB on BN254 G1.  msm_hip_test_mul_policy replaces either decision.
constexpr int MUL_TABLE_MAX_BITS = 16;
constexpr size_t MUL_TABLE_MIN_N = (size_t)1 << 17;
inline int mul_table_windows(const msm_hip_ctx* ctx, int c) { return (ctx->ops->r_bits + 1 + c) / c; }
int pick_mul_table_bits(const msm_hip_ctx* ctx, size_t base, size_t n, bool endo) {
  const bool held = ctx->mul_table_bits != 0 && ctx->mul_table_base == base && ctx->mul_table_endo == endo;
  if (ctx->mul_policy_min_n) {  // the hook: the table exactly from this n on
    if (n < ctx->mul_policy_min_n) return 0;
  } else if (!held && n < MUL_TABLE_MIN_N) {
    return 0;
  }
  if (ctx->mul_policy_bits) return ctx->mul_policy_bits;
  if (held) return ctx->mul_table_bits;
  return n < ((size_t)1 << 23) ? 12 : n < ((size_t)1 << 24) ? 14 : 16;
}

// `host`: scalars and out are host memory (staged through d_mul tile by tile); else device memory, read and written in place.
// Everything is enqueued on the main stream; the call returns when the output is complete.
int mul_impl(msm_hip_ctx* ctx, bool broadcast, size_t base_index, const void* scalars, size_t n, void* out, uint32_t flags, bool host) {
  if (!ctx) return no_context_code();
  if (flags & ~MSM_HIP_MUL_BASES_ORDER_R) return MSM_HIP_ERR_INVALID_ARG;
  if (ctx->scalar_format != MSM_HIP_SCALARS_CANONICAL && ctx->scalar_format != MSM_HIP_SCALARS_MONT256) return MSM_HIP_ERR_INVALID_ARG;  // 32-byte formats only
  if (n == 0) return MSM_HIP_OK;
  if (!scalars || !out || n > MAX_POINTS) return MSM_HIP_ERR_INVALID_ARG;
  if (ctx->n_bases == 0) return MSM_HIP_ERR_NO_BASES;
  if (broadcast ? base_index >= ctx->n_bases : n > ctx->n_bases) return MSM_HIP_ERR_INVALID_ARG;
  if (ranges_overlap(scalars, n * 32, out, n * ctx->pb)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && ((reinterpret_cast<uintptr_t>(scalars) | reinterpret_cast<uintptr_t>(out)) & 15u)) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  ON_DEVICE(ctx);
  const CurveOps* ops = ctx->ops;
  const size_t cw = (size_t)ops->coord_words, ptw = 2 * cw;
  const bool mont = ctx->scalar_format == MSM_HIP_SCALARS_MONT256;
  const bool endo = ops->glv && (ctx->mul_force_ladder ? ctx->mul_force_ladder == 2 : prime_order_curve(ctx->curve) || (flags & MSM_HIP_MUL_BASES_ORDER_R));
  hipStream_t st = ctx->stream;
  const uint64_t* id_bits = ctx->n_identity ? ctx->d_id_bits : nullptr;
  if (broadcast && id_bits) {  // one base for every output: is it the identity?  Then every output is, whatever the scalars hold
    uint64_t word = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&word, id_bits + (base_index >> 6), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if ((word >> (base_index & 63u)) & 1u) {
      if (host) {
        memset(out, 0, n * ctx->pb);
      } else {
        HIP_TRY(ctx, hipMemsetAsync(out, 0, n * ctx->pb, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
      }
      ctx->mul_last_path = 0;
      ctx->mul_last_bits = 0;
      return MSM_HIP_OK;
    }
    id_bits = nullptr;
  }
  const size_t tile = n < MUL_TILE ? n : MUL_TILE;
  // mul_base: through the fixed-base table?  (decided before the scratch is sized: a table's build runs the ladder over its entries)
  const int tbits = broadcast ? pick_mul_table_bits(ctx, base_index, n, endo) : 0;
  const size_t n_tab = tbits ? (size_t)mul_table_windows(ctx, tbits) << (tbits - 1) : 0;
  const bool build_table = tbits && !(ctx->mul_table_bits == tbits && ctx->mul_table_base == base_index && ctx->mul_table_endo == endo);
  const size_t tab_tile = build_table ? (n_tab < MUL_TILE ? n_tab : MUL_TILE) : 0;
  const size_t stile = tile > tab_tile ? tile : tab_tile;
  const size_t tile4 = (stile + 3) & ~(size_t)3;  // (every part of the scratch stays 16-byte aligned)
  const size_t words = tile4 * (2 * cw + 16) + (host ? tile4 * (8 + ptw) : 0);
  int rc = grow(ctx, ctx->cap_mul, words, true, [&](size_t c) { return dev_alloc(ctx, ctx->d_mul, c); });
  if (rc) return rc;
  uint32_t* zbuf = ctx->d_mul;
  uint32_t* prefix = zbuf + tile4 * cw;
  uint32_t* conv = prefix + tile4 * cw;
  uint32_t* masked = conv + tile4 * 8;
  uint32_t* stage_sc = masked + tile4 * 8;
  uint32_t* stage_out = stage_sc + tile4 * 8;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, 4, st));
  if (build_table) {  // T_w[j] = j 2^(C w) P: the ladder over the entries' scalars (integers: not compared with r), normalised like any output, then to Montgomery records
    if ((rc = grow(ctx, ctx->cap_mul_table, n_tab * ptw, true, [&](size_t c) { return dev_alloc(ctx, ctx->d_mul_table, c); }))) return rc;
    ctx->mul_table_bits = 0;
    uint32_t* table = ctx->d_mul_table;
    for (size_t off = 0; off < n_tab; off += tab_tile) {
      const size_t t = n_tab - off < tab_tile ? n_tab - off : tab_tile;
      hipLaunchKernelGGL(ops->mul_table_scalars, dim3(blocks_for(t, 256)), dim3(256), 0, st, tbits, off, t, conv);  // (this tile's scalars: in the scratch)
      AFTER_KERNEL(ctx, "k_mul_table_scalars", st);
      hipLaunchKernelGGL(ops->mul_each[endo ? 1 : 0], dim3(blocks_for(t, 256)), dim3(256), 0, st, (const uint32_t*)ctx->d_bases, (const uint32_t*)conv, t, base_index, 1u,
                         (const uint64_t*)nullptr, table + off * ptw, zbuf, ctx->d_err, 0u);
      AFTER_KERNEL(ctx, "k_mul_each (table)", st);
      hipLaunchKernelGGL(ops->mul_normalize, dim3(blocks_for(t, 256 * (size_t)ops->mul_chunk)), dim3(256), 0, st, table + off * ptw, (const uint32_t*)zbuf, prefix, t);
      AFTER_KERNEL(ctx, "k_mul_normalize (table)", st);
    }
    hipLaunchKernelGGL(ops->convert_points, dim3(blocks_for(n_tab, 256)), dim3(256), 0, st, (const uint32_t*)table, table, n_tab, 0u, ctx->d_err);
    AFTER_KERNEL(ctx, "k_convert_points (table)", st);
    HIP_TRY(ctx, hipGetLastError());
    ctx->mul_table_bits = tbits;
    ctx->mul_table_base = base_index;
    ctx->mul_table_endo = endo;
  }
  for (size_t off = 0; off < n; off += tile) {
    const size_t t = n - off < tile ? n - off : tile;
    const uint32_t* d_sc;
    if (host) {
      HIP_TRY(ctx, hipMemcpyAsync(stage_sc, static_cast<const uint8_t*>(scalars) + off * 32, t * 32, hipMemcpyHostToDevice, st));
      d_sc = stage_sc;
    } else {
      d_sc = static_cast<const uint32_t*>(scalars) + off * 8;
    }
    if (mont) {  // canonical copies first; ahead of them, the scalars of identity bases zeroed: they are not validated either
      if (id_bits) {
        hipLaunchKernelGGL(k_mask_identity<32>, dim3(blocks_for(t, 256), 1), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(d_sc), reinterpret_cast<uint8_t*>(masked), t,
                           off, id_bits, (uint32_t)ctx->n_bases, (const uint32_t*)nullptr);
        AFTER_KERNEL(ctx, "k_mask_identity", st);
        d_sc = masked;
      }
      hipLaunchKernelGGL(ops->scalars_from_mont256, dim3(blocks_for(t, 256)), dim3(256), 0, st, d_sc, conv, t, ctx->d_err);
      AFTER_KERNEL(ctx, "k_scalars_from_mont256", st);
      d_sc = conv;
    }
    uint32_t* d_out = host ? stage_out : static_cast<uint32_t*>(out) + off * ptw;
    if (tbits) {
      hipLaunchKernelGGL(ops->mul_fixed, dim3(blocks_for(t, 256)), dim3(256), 0, st, (const uint32_t*)ctx->d_mul_table, tbits, d_sc, t, d_out, zbuf, ctx->d_err);
      AFTER_KERNEL(ctx, "k_mul_fixed", st);
    } else {
      hipLaunchKernelGGL(ops->mul_each[endo ? 1 : 0], dim3(blocks_for(t, 256)), dim3(256), 0, st, (const uint32_t*)ctx->d_bases, d_sc, t, broadcast ? base_index : off,
                         broadcast ? 1u : 0u, id_bits, d_out, zbuf, ctx->d_err, 1u);
      AFTER_KERNEL(ctx, "k_mul_each", st);
    }
    hipLaunchKernelGGL(ops->mul_normalize, dim3(blocks_for(t, 256 * (size_t)ops->mul_chunk)), dim3(256), 0, st, d_out, (const uint32_t*)zbuf, prefix, t);
    AFTER_KERNEL(ctx, "k_mul_normalize", st);
    HIP_TRY(ctx, hipGetLastError());
    if (host) {  // (the staging area is this tile's alone until its output has left)
      HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(out) + off * ctx->pb, stage_out, t * ctx->pb, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
    }
  }
  uint32_t bits = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&bits, ctx->d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->mul_last_path = tbits ? (build_table ? 4 : 3) : endo ? 2 : 1;
  ctx->mul_last_bits = tbits;
  return err_from_bits(bits);
}
}  // namespace

extern "C" {
int msm_hip_mul_each(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, uint8_t* out_xy_host, uint32_t flags) {
  return mul_impl(ctx, false, 0, scalars_host, n, out_xy_host, flags, true);
}
int msm_hip_mul_each_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, void* out_xy_dev, uint32_t flags) {
  return mul_impl(ctx, false, 0, scalars_dev, n, out_xy_dev, flags, false);
}
int msm_hip_mul_base(msm_hip_ctx* ctx, size_t base_index, const uint8_t* scalars_host, size_t n, uint8_t* out_xy_host, uint32_t flags) {
  return mul_impl(ctx, true, base_index, scalars_host, n, out_xy_host, flags, true);
}
int msm_hip_mul_base_device(msm_hip_ctx* ctx, size_t base_index, const void* scalars_dev, size_t n, void* out_xy_dev, uint32_t flags) {
  return mul_impl(ctx, true, base_index, scalars_dev, n, out_xy_dev, flags, false);
}
int msm_hip_test_mul_policy(msm_hip_ctx* ctx, size_t table_min_n, int table_bits) {
  if (!ctx || (table_bits && (table_bits < 4 || table_bits > MUL_TABLE_MAX_BITS))) return MSM_HIP_ERR_INVALID_ARG;
  ctx->mul_policy_min_n = table_min_n;
  ctx->mul_policy_bits = table_bits;
  return MSM_HIP_OK;
}
int msm_hip_test_mul_ladder(msm_hip_ctx* ctx, int ladder) {
  if (!ctx || ladder < 0 || ladder > 2) return MSM_HIP_ERR_INVALID_ARG;
  ctx->mul_force_ladder = ladder;
  return MSM_HIP_OK;
}
int msm_hip_test_mul_last(const msm_hip_ctx* ctx, int* path, int* table_bits, int* chunk) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  if (path) *path = ctx->mul_last_path;
  if (table_bits) *table_bits = ctx->mul_last_bits;
  if (chunk) *chunk = ctx->ops->mul_chunk;
  return MSM_HIP_OK;
}
}  // extern "C"

// ---- group FFT over the resident bases: out[i] = c * sum_j omega^(i j) P_j (include/msm_hip.h, msm_hip_bases_fft) -----------------------------------
namespace {
// `host`: out is host memory (the last pass writes into the scratch, copied out at the end); else device memory, written in place.
// Every argument is checked before anything is enqueued.  log_n stages on the main stream (msm_kernels.h, k_fft_stage): the first reads the resident
// bases through the bit-reversed index into the scratch, the others run in place there -- a butterfly touches its own two elements only -- and the
// last pass of the call (the last stage, or the scale pass behind it) writes the output records, which k_mul_normalize makes wire records.
int fft_impl(msm_hip_ctx* ctx, const uint8_t* omega, int log_n, void* out, uint32_t flags, bool host) {
  if (!ctx) return no_context_code();
  if (flags & ~(MSM_HIP_MUL_BASES_ORDER_R | MSM_HIP_FFT_SCALE_INV_N)) return MSM_HIP_ERR_INVALID_ARG;
  const CurveOps* ops = ctx->ops;
  if (!ops->fft_normalize) return MSM_HIP_ERR_INVALID_ARG;  // the G2 groups
  if (!omega || !out || log_n < 0 || log_n > 28) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (reinterpret_cast<uintptr_t>(out) & 15u)) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  if (ctx->n_bases == 0) return MSM_HIP_ERR_NO_BASES;
  const size_t n = (size_t)1 << log_n;
  if (n > ctx->n_bases) return MSM_HIP_ERR_INVALID_ARG;
  const host_fr::Field fr(ops->fr_r);
  if (!host_fr::is_primitive_root(fr, omega, log_n)) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  const size_t cw = (size_t)ops->coord_words, ptw = 2 * cw;
  const bool endo = ops->glv && (ctx->mul_force_ladder ? ctx->mul_force_ladder == 2 : prime_order_curve(ctx->curve) || (flags & MSM_HIP_MUL_BASES_ORDER_R));
  const bool scale = (flags & MSM_HIP_FFT_SCALE_INV_N) && log_n > 0;  // (1 / 1 = 1)
  hipStream_t st = ctx->stream;
  const uint64_t* id_bits = ctx->n_identity ? ctx->d_id_bits : nullptr;
  const size_t n4 = (n + 3) & ~(size_t)3;  // (every part of the scratch stays 16-byte aligned)
  int rc = grow(ctx, ctx->cap_fft, n4 * (ptw + 2 * cw) + 8 + (host ? n4 * ptw : 0), true, [&](size_t c) { return dev_alloc(ctx, ctx->d_fft, c); });
  if (rc) return rc;
  uint32_t* work = ctx->d_fft;
  uint32_t* zbuf = work + n4 * ptw;
  uint32_t* prefix = zbuf + n4 * cw;
  uint32_t* d_scalar = prefix + n4 * cw;
  uint32_t* d_out = host ? d_scalar + 8 : static_cast<uint32_t*>(out);
  if (log_n >= 2 && !(ctx->fft_tw_log_n == log_n && memcmp(ctx->fft_tw_omega, omega, 32) == 0)) {  // (stage 0's twiddles are all 1)
    std::vector<uint32_t> tw;
    host_fr::twiddle_table(fr, omega, log_n, tw);
    if ((rc = grow(ctx, ctx->cap_fft_tw, tw.size(), true, [&](size_t c) { return dev_alloc(ctx, ctx->d_fft_tw, c); }))) return rc;
    ctx->fft_tw_log_n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_fft_tw, tw.data(), tw.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (an earlier call's kernels no longer read the old table; `tw` may go)
    ctx->fft_tw_log_n = log_n;
    memcpy(ctx->fft_tw_omega, omega, 32);
  }
  uint32_t k[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (scale) host_fr::inverse_of_n(fr, log_n, k);
  if (scale || log_n == 0) {
    HIP_TRY(ctx, hipMemcpyAsync(d_scalar, k, 32, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  const int ladder = endo ? 2 : 1;
  const unsigned norm_blocks = blocks_for(n, 256 * (size_t)ops->mul_chunk);
  if (log_n == 0) {  // one element: the base itself, through the ladder's kernel with the scalar 1 (an identity base gives the all-zero record)
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, 4, st));
    hipLaunchKernelGGL(ops->mul_each[0], dim3(1), dim3(256), 0, st, (const uint32_t*)ctx->d_bases, (const uint32_t*)d_scalar, (size_t)1, (size_t)0, 1u, id_bits, d_out, zbuf,
                       ctx->d_err, 1u);
    AFTER_KERNEL(ctx, "k_mul_each (fft, n = 1)", st);
  }
  for (int s = 0; s < log_n; s++) {
    const bool last = s == log_n - 1 && !scale;
    hipLaunchKernelGGL(ops->fft_stage[s == 0 ? 0 : ladder], dim3(blocks_for(n / 2, 256)), dim3(256), 0, st, s == 0 ? (const uint32_t*)ctx->d_bases : (const uint32_t*)work,
                       last ? d_out : work, zbuf, (const uint32_t*)ctx->d_fft_tw, log_n, s, s == 0 ? 1u : 0u, id_bits);
    AFTER_KERNEL(ctx, "k_fft_stage", st);
    if (!last) {
      hipLaunchKernelGGL(ops->fft_normalize, dim3(norm_blocks), dim3(256), 0, st, work, (const uint32_t*)zbuf, prefix, n);
      AFTER_KERNEL(ctx, "k_fft_normalize", st);
    }
  }
  if (scale) {
    hipLaunchKernelGGL(ops->fft_scale[ladder - 1], dim3(blocks_for(n, 256)), dim3(256), 0, st, (const uint32_t*)work, d_out, zbuf, (const uint32_t*)d_scalar, n);
    AFTER_KERNEL(ctx, "k_fft_scale", st);
  }
  hipLaunchKernelGGL(ops->mul_normalize, dim3(norm_blocks), dim3(256), 0, st, d_out, (const uint32_t*)zbuf, prefix, n);
  AFTER_KERNEL(ctx, "k_mul_normalize (fft)", st);
  HIP_TRY(ctx, hipGetLastError());
  if (host) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, n * ctx->pb, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->fft_last_stages = log_n;
  ctx->fft_last_ladder = (log_n >= 2 || scale) ? ladder : 0;
  return MSM_HIP_OK;
}
}  // namespace

extern "C" {
int msm_hip_bases_fft(msm_hip_ctx* ctx, const uint8_t omega[32], int log_n, uint8_t* out_xy_host, uint32_t flags) {
  return fft_impl(ctx, omega, log_n, out_xy_host, flags, true);
}
int msm_hip_bases_fft_device(msm_hip_ctx* ctx, const uint8_t omega[32], int log_n, void* out_xy_dev, uint32_t flags) {
  return fft_impl(ctx, omega, log_n, out_xy_dev, flags, false);
}
int msm_hip_test_fft_last(const msm_hip_ctx* ctx, int* stages, int* ladder) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  if (stages) *stages = ctx->fft_last_stages;
  if (ladder) *ladder = ctx->fft_last_ladder;
  return MSM_HIP_OK;
}
}  // extern "C"

#include "msm_mgpu.h"

// ---- the `_bn254` names of rounds 1 - 4: aliases of the curve-neutral entry points (include/msm_hip.h, last block)
extern "C" {
int msm_hip_set_bases_bn254(msm_hip_ctx* ctx, const uint8_t* xy_host, size_t n, uint32_t flags) { return msm_hip_set_bases(ctx, xy_host, n, flags); }
int msm_hip_set_bases_device_bn254(msm_hip_ctx* ctx, const void* xy_dev, size_t n, uint32_t flags) { return msm_hip_set_bases_device(ctx, xy_dev, n, flags); }
int msm_hip_run_bn254(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, uint8_t out_xyz[96]) { return msm_hip_run(ctx, scalars_host, n, out_xyz); }
int msm_hip_run_device_bn254(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, uint8_t out_xyz[96]) { return msm_hip_run_device(ctx, scalars_dev, n, out_xyz); }
int msm_hip_launch_device_bn254(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int slot) { return msm_hip_launch_device(ctx, scalars_dev, n, slot); }
int msm_hip_finish_bn254(msm_hip_ctx* ctx, int slot, uint8_t out_xyz[96]) { return msm_hip_finish(ctx, slot, out_xyz); }
int msm_hip_launch_bn254(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, int slot) { return msm_hip_launch(ctx, scalars_host, n, slot); }
int msm_hip_run_batch_device_bn254(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, size_t batch, uint8_t* out_xyz) {
  return msm_hip_run_batch_device(ctx, scalars_dev, n, batch, out_xyz);
}
int msm_hip_run_batch_bn254(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, size_t batch, uint8_t* out_xyz) {
  return msm_hip_run_batch(ctx, scalars_host, n, batch, out_xyz);
}
int msm_hip_run_windows_device_bn254(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int w_begin, int w_end, void* window_sums_dev) {
  return msm_hip_run_windows_device(ctx, scalars_dev, n, w_begin, w_end, window_sums_dev);
}
int msm_hip_launch_windows_device_bn254(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int w_begin, int w_end, int slot, void* window_sums_dev) {
  return msm_hip_launch_windows_device(ctx, scalars_dev, n, w_begin, w_end, slot, window_sums_dev);
}
int msm_hip_launch_windows_batch_device_bn254(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int nvec, int w_begin, int w_end, int slot,
                                              void* window_sums_dev) {
  return msm_hip_launch_windows_batch_device(ctx, scalars_dev, n, nvec, w_begin, w_end, slot, window_sums_dev);
}
int msm_hip_finish_batch_bn254(msm_hip_ctx* ctx, int slot, uint8_t* out_xyz) { return msm_hip_finish_batch(ctx, slot, out_xyz); }
int msm_hip_launch_half_windows_batch_device_bn254(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, int nvec, int hw_begin, int hw_end, int slot,
                                                   void* window_sums_dev) {
  return msm_hip_launch_half_windows_batch_device(ctx, scalars_dev, n, nvec, hw_begin, hw_end, slot, window_sums_dev);
}
int msm_hip_mgpu_set_bases_bn254(msm_hip_mgpu* m, const uint8_t* xy_host, size_t n, uint32_t flags) { return msm_hip_mgpu_set_bases(m, xy_host, n, flags); }
int msm_hip_mgpu_run_bn254(msm_hip_mgpu* m, const uint8_t* scalars_host, size_t n, uint8_t out_xyz[96]) { return msm_hip_mgpu_run(m, scalars_host, n, out_xyz); }
int msm_hip_mgpu_launch_batch_bn254(msm_hip_mgpu* m, const uint8_t* scalars_host, size_t n, int nvec, int slot) {
  return msm_hip_mgpu_launch_batch(m, scalars_host, n, nvec, slot);
}
int msm_hip_mgpu_launch_batch_device_bn254(msm_hip_mgpu* m, const void* const* scalars_dev, size_t n, int nvec, int slot) {
  return msm_hip_mgpu_launch_batch_device(m, scalars_dev, n, nvec, slot);
}
int msm_hip_mgpu_finish_batch_bn254(msm_hip_mgpu* m, int slot, uint8_t* out_xyz) { return msm_hip_mgpu_finish_batch(m, slot, out_xyz); }
int msm_hip_mgpu_run_batch_bn254(msm_hip_mgpu* m, const uint8_t* scalars_host, size_t n, size_t batch, uint8_t* out_xyz) {
  return msm_hip_mgpu_run_batch(m, scalars_host, n, batch, out_xyz);
}
}  // extern "C"
