// The context of libmsm_hip.so and its buffer pools: the result slots (Slot), msm_hip_ctx with the state of the batch scalar multiplication
// (MulState) and of the group FFT (FftState), the error-returning wrappers around HIP calls (HIP_TRY, AFTER_KERNEL), pooled device buffers that
// grow (dev_alloc, grow, ensure_stage, setup_slot, ensure_work), the device guard, num_cus() and the wait for a slot (wait_slot, drain_slots).
// Assumes <hip/hip_runtime.h>, curve_ops.h (CurveOps) and msm_plan.h (PlanInputs, LaunchPlan, piece_records_for, NSLOT) before it.
#pragma once

namespace {
constexpr int N_MAIN_EVENTS = 7;  // boundaries of the 6 timed stages on the main stream
constexpr size_t MAX_JB = 288;  // the largest Jacobian record of any curve (BLS12-381 G2: 3 x 96 B; BN254 G2: 3 x 64 B; BLS12-381 G1: 3 x 48 B; the 254 / 255-bit G1 curves: 96 B)
constexpr size_t WSUM_BYTES = (size_t)24 * PLANES_PER_WINDOW * MAX_JB;  // MAXLW window sums or, for one host-combined MSM, the bit-plane sums (k_bpr_planes) of its <= 22 windows
static_assert(WSUM_BYTES >= (size_t)2 * MAXLW * MAX_JB, "window-sum buffer (pairs of records for shares of the wide tables' virtual windows)");
constexpr int NREDUCE = 2;  // reduce streams (slot k uses stream k % NREDUCE): two bucket reduces may be in flight when the
                            // main-stream work of one MSM is shorter than its bucket reduce (few windows per GPU).  The context
                            // then owns 3 streams; streams beyond the process's hardware queues (GPU_MAX_HW_QUEUES) share
                            // them: correct, with less overlap.

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

// msm_hip_mul_each / msm_hip_mul_base (msm_mul.h)
struct MulState {
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
};
// msm_hip_bases_fft (msm_fft.h)
struct FftState {
  uint32_t* d_fft = nullptr;   // group FFT over the resident bases (msm_hip_bases_fft): n Montgomery point records, their Z values and prefix products, the
  size_t cap_fft = 0;          // broadcast scalar and, for the host entry point, the staged output; in words
  uint32_t* d_fft_tw = nullptr;  // ... its twiddles omega^j, j < n / 2 (canonical, 8 words each), cached under the key (fft_tw_log_n, fft_tw_omega): they do
  size_t cap_fft_tw = 0;         // not depend on the bases.  In words
  int fft_tw_log_n = 0;          // (0: no table held)
  uint8_t fft_tw_omega[32] = {};
  int fft_last_stages = 0;     // the last such call (test hook msm_hip_test_fft_last): butterfly stages run, and the ladder of its twiddled stages and of the
  int fft_last_ladder = 0;     // scale pass: 0 none ran, 1 the plain ladder, 2 the endomorphism's
};
}  // namespace

struct msm_hip_ctx : PlanInputs {
  int device = 0;
  const CurveOps* ops = nullptr;
  size_t cb = 32, pb = 64, jb = 96;     // bytes of a coordinate, an affine point and a Jacobian record on this curve's wire (48 / 96 / 144: BLS12-381)
  hipStream_t stream = nullptr;         // main
  hipStream_t reduce_stream[NREDUCE] = {};  // bucket reduce + result copies
  int last_hip_error = 0;

  uint32_t* d_bases = nullptr;  // n_bases x 16 words
  size_t cap_bases = 0;         // capacity in point records (16 x n_bases with fixed-base tables)
  uint64_t* d_id_bits = nullptr;      // MSM_HIP_BASES_ZERO_IS_IDENTITY: bit i = base i is the identity (ceil(n / 64) words; k_convert_points_zero_id)
  size_t cap_id_bits = 0;             // in words
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
  uint32_t* d_part_hist = nullptr;  // [MAXLW][128][FINE_SPLIT][256] sub-range histograms of huge coarse bins (k_fine_hist), on first use
  size_t fine_hist_min_n = FINE_BIG + 1;  // any n that can produce a coarse bin beyond FINE_BIG: run k_fine_hist (3 us when none does)
  int skew_credit = 0;  // launches left for which k_fine_hist runs although uniform scalars could not fill a bin: set when a launch met a huge bin (wait_slot)
  uint32_t* d_err = nullptr;
  uint8_t* d_stage = nullptr;  // staging for host byte inputs of set_bases / test hooks
  size_t cap_stage = 0;
  MulState mul;
  FftState fft;

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

// compute units of the current device (the devices of a node are alike: asked once)
inline size_t num_cus() {
  static const size_t v = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) return (size_t)cus;
    return (size_t)256;
  }();
  return v;
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

}  // namespace
