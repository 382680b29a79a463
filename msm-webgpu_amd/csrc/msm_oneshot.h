// The one-shot call msm_hip_msm_curve (bases and scalars from the host, one result): the contexts it keeps per device, the overlapped upload in parts
// (oneshot_enqueue, oneshot_collect), msm_hip_test_oneshot_parts and msm_hip_oneshot_release.
// Assumes msm_plan.h (upload_parts and its probes), msm_ctx.h, msm_enqueue.h, msm_bases.h and, of msm_hip.hip, stage_host and part_first.
#pragma once


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

}  // extern "C"
