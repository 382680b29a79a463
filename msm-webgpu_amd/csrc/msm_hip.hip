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
}  // namespace

// the host code, by concern, in dependency order (each file's head says what it holds and what it expects before it)
#include "msm_plan.h"
#include "msm_ctx.h"
#include "msm_enqueue.h"
#include "msm_bases.h"

namespace {
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
                  ctx->d_tmp_val, ctx->d_tmp_fine, ctx->d_val,    ctx->d_chunk_slot, ctx->d_err,       ctx->d_stage, ctx->d_id_bits, ctx->mul.d_mul, ctx->mul.d_mul_table, ctx->fft.d_fft, ctx->fft.d_fft_tw};
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

}  // extern "C"

#include "msm_oneshot.h"
#include "msm_hooks.h"
#include "msm_mul.h"
#include "msm_fft.h"
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
