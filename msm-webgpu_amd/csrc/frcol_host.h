// Host side of libmsm_frcol.so (include/msm_frcol.h): argument checks, the plan (csrc/frcol_plan.h), staging, and the launches of
// csrc/frcol_kernels.h.  One translation unit (csrc/frcol.hip) for all curves.
//
// A call enqueues everything on one stream, the check of the total included -- the output kernels read the total the top level's scan left in
// the result words and write nothing where it is not n_out --, copies the result words into the device's pinned buffer in ONE copy and waits for
// the stream (DESIGN.md sections 4.19, 4.26).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>

#include "../../include/msm_frcol.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers and the state scheme every scalar-field library shares
#include "frcol_kernels.h"
#include "frcol_plan.h"

namespace frcol {

using fr_host::Buffer;
using fr_host::DeviceGuard;
using fr_host::grow;
using fr_host::hip_ok;

struct DeviceState {
  hipStream_t stream = nullptr;
  Buffer result;    // FRCOL_RESULT_WORDS words: the error word, the total, the entries in use
  Buffer h_result;  // pinned: what the one copy of a call fills
  Buffer scratch;   // the nodes of the scan's levels, rel, used, z (frcol::Layout)
  Buffer staging;   // the host forms' operands
};
struct Hooks {
  uint32_t tile = 0;  // 0: FRCOL_TILE
  int launches = 0, levels = 0;
};

inline std::mutex& lock() { return fr_host::lock_of<DeviceState>(); }
inline std::map<int, DeviceState>& states() { return fr_host::states_of<DeviceState>(); }
inline Hooks& hooks() {
  static Hooks h;
  return h;
}

// the device's state, its stream and the two result buffers (the caller holds the guard and the lock)
inline int device_state(int device, DeviceState** out) {
  DeviceState& ds = states()[device];
  if (!ds.stream && hipStreamCreateWithFlags(&ds.stream, hipStreamNonBlocking) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;
  int rc = grow(ds.result, FRCOL_RESULT_WORDS);
  if (!rc) rc = grow(ds.h_result, FRCOL_RESULT_WORDS, true);
  *out = &ds;
  return rc;
}

// the scan of (counts + bias, counts > 0) on `st`: afterwards the scratch buffer holds the tile bases, rel and -- pair -- used and z, and the result
// words the totals
inline int enqueue_scan(DeviceState& ds, hipStream_t st, const uint32_t* counts, const FrcolArgs& g, const Layout& y) {
  if (int rc = grow(ds.scratch, y.words)) return rc;
  FrcNode* const nodes = reinterpret_cast<FrcNode*>(ds.scratch.p);
  const size_t top = y.len.size() - 1;
  const dim3 threads(FRCOL_THREADS);
  for (size_t l = 0; l < top; l++) {  // the sums, upwards
    FrcNode* const above = nodes + y.node_at[l + 1];
    if (l == 0)
      hipLaunchKernelGGL(k_frcol_sums<true>, dim3((uint32_t)y.len[1]), threads, 0, st, counts, nullptr, above, (uint32_t)y.len[0], (uint32_t)y.len[1], g);
    else
      hipLaunchKernelGGL(k_frcol_sums<false>, dim3((uint32_t)y.len[l + 1]), threads, 0, st, nullptr, nodes + y.node_at[l], above, (uint32_t)y.len[l], (uint32_t)y.len[l + 1], g);
  }
  for (size_t l = top; l >= 1; l--) {  // the inner levels, downwards and in place
    const FrcNode* const above = l == top ? nullptr : nodes + y.node_at[l + 1];
    const uint32_t tiles = l == top ? 1u : (uint32_t)y.len[l + 1];
    hipLaunchKernelGGL(k_frcol_scan<false>, dim3(tiles), threads, 0, st, nullptr, nodes + y.node_at[l], above, (uint32_t)y.len[l], nullptr, nullptr, nullptr, ds.result.p, g);
  }
  hipLaunchKernelGGL(k_frcol_scan<true>, dim3((uint32_t)y.len[1]), threads, 0, st, counts, nullptr, nodes + y.node_at[1], (uint32_t)y.len[0], ds.scratch.p + y.rel_at,
                     ds.scratch.p + y.used_at, ds.scratch.p + y.z_at, ds.result.p, g);
  hooks().launches = (int)(2 * top + 2), hooks().levels = (int)y.len.size();  // (sums, inner scans, the leaf, and the caller's output kernel)
  return hip_ok(hipGetLastError()) ? MSM_HIP_OK : MSM_HIP_ERR_HIP;
}
// the result words back, the stream complete
inline int collect(DeviceState& ds, hipStream_t st) {
  if (!hip_ok(hipGetLastError()) || !hip_ok(hipMemcpyAsync(ds.h_result.p, ds.result.p, FRCOL_RESULT_WORDS * 4, hipMemcpyDeviceToHost, st)) || !hip_ok(hipStreamSynchronize(st)))
    return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}
inline uint64_t word64(const uint32_t* p) { return (uint64_t)p[0] | (uint64_t)p[1] << 32; }

// expand (s_out null) and pair (s_out set, n_out = n_t, bias 0)
inline int runs_impl(int device, void* stream, void* out, void* s_out, const void* t, const uint32_t* counts, size_t n_t, uint32_t bias, size_t n_out, uint64_t* total,
                     uint64_t* used, bool pair, bool host) {
  if (device < 0) return MSM_HIP_ERR_INVALID_ARG;
  if (pair ? !pair_args_ok(out, s_out, t, counts, n_t, host) : !expand_args_ok(out, t, counts, n_t, bias, n_out, host)) return MSM_HIP_ERR_INVALID_ARG;
  int rc = fr_host::have_device(device);
  if (rc) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  DeviceState* dsp = nullptr;
  if ((rc = device_state(device, &dsp))) return rc;
  DeviceState& ds = *dsp;
  const hipStream_t st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  const uint32_t tile = tile_of(hooks().tile);
  const FrcolArgs g = plan_args(n_t, tile, bias, n_out, pair);
  const Layout y = plan_layout(n_t, tile);
  const uint32_t* dt = static_cast<const uint32_t*>(t);
  const uint32_t* dcounts = counts;
  uint32_t* dout = static_cast<uint32_t*>(out);
  uint32_t* dsout = static_cast<uint32_t*>(s_out);
  if (host) {  // staging: t, out, s_out (scalars first: 16-byte aligned), then counts
    const size_t outs = pair ? 2 * n_out : n_out;
    if ((rc = grow(ds.staging, (n_t + outs) * 8 + n_t))) return rc;
    uint32_t* const s = ds.staging.p;
    if (!hip_ok(hipMemcpyAsync(s, t, n_t * 32, hipMemcpyHostToDevice, st)) || !hip_ok(hipMemcpyAsync(s + (n_t + outs) * 8, counts, n_t * 4, hipMemcpyHostToDevice, st)))
      return MSM_HIP_ERR_HIP;
    dt = s, dout = s + n_t * 8, dsout = pair ? s + (n_t + n_out) * 8 : nullptr, dcounts = s + (n_t + outs) * 8;
  }
  if (!hip_ok(hipMemsetAsync(ds.result.p, 0, FRCOL_RESULT_WORDS * 4, st))) return MSM_HIP_ERR_HIP;
  if ((rc = enqueue_scan(ds, st, dcounts, g, y))) return rc;
  const FrcNode* const bases = reinterpret_cast<const FrcNode*>(ds.scratch.p) + y.node_at[1];
  const dim3 grid((uint32_t)((n_out + FRCOL_THREADS - 1) / FRCOL_THREADS));
  if (pair)
    hipLaunchKernelGGL(k_frcol_pair, grid, dim3(FRCOL_THREADS), 0, st, ds.result.p, bases, ds.scratch.p + y.rel_at, ds.scratch.p + y.used_at, ds.scratch.p + y.z_at, dt, dout, dsout, g);
  else
    hipLaunchKernelGGL(k_frcol_expand, grid, dim3(FRCOL_THREADS), 0, st, ds.result.p, bases, ds.scratch.p + y.rel_at, dt, dout, g);
  if ((rc = collect(ds, st))) return rc;
  const uint64_t sum = word64(ds.h_result.p + FRCOL_RES_TOTAL);
  if (total) *total = sum;
  if (used) *used = word64(ds.h_result.p + FRCOL_RES_USED);
  if (sum != n_out) return MSM_HIP_ERR_INVALID_ARG;  // (nothing was written)
  if (host) {
    if (!hip_ok(hipMemcpy(out, dout, n_out * 32, hipMemcpyDeviceToHost)) || (pair && !hip_ok(hipMemcpy(s_out, dsout, n_out * 32, hipMemcpyDeviceToHost)))) return MSM_HIP_ERR_HIP;
  }
  return MSM_HIP_OK;
}

inline int gather_impl(int device, void* stream, void* out, const void* a, size_t n_a, const uint32_t* idx, size_t n, bool host) {
  if (device < 0 || !gather_args_ok(out, a, n_a, idx, n, host)) return MSM_HIP_ERR_INVALID_ARG;
  int rc = fr_host::have_device(device);
  if (rc) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  DeviceState* dsp = nullptr;
  if ((rc = device_state(device, &dsp))) return rc;
  DeviceState& ds = *dsp;
  const hipStream_t st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  const uint32_t* da = static_cast<const uint32_t*>(a);
  const uint32_t* didx = idx;
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = grow(ds.staging, (n_a + n) * 8 + n))) return rc;
    uint32_t* const s = ds.staging.p;
    if (!hip_ok(hipMemcpyAsync(s, a, n_a * 32, hipMemcpyHostToDevice, st)) || !hip_ok(hipMemcpyAsync(s + (n_a + n) * 8, idx, n * 4, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
    da = s, dout = s + n_a * 8, didx = s + (n_a + n) * 8;
  }
  if (!hip_ok(hipMemsetAsync(ds.result.p, 0, FRCOL_RESULT_WORDS * 4, st))) return MSM_HIP_ERR_HIP;
  hipLaunchKernelGGL(k_frcol_gather, dim3((uint32_t)((n + FRCOL_THREADS - 1) / FRCOL_THREADS)), dim3(FRCOL_THREADS), 0, st, da, (uint32_t)n_a, didx, (uint32_t)n, dout, ds.result.p);
  if (host && !hip_ok(hipMemcpyAsync(out, dout, n * 32, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if ((rc = collect(ds, st))) return rc;
  return ds.h_result.p[FRCOL_RES_ERR] ? MSM_HIP_ERR_INVALID_ARG : MSM_HIP_OK;
}

}  // namespace frcol

extern "C" {
int msm_frcol_abi_version(void) { return 1; }

int msm_frcol_expand_device(int device, void* stream, void* out, const void* t, const uint32_t* counts, size_t n_t, uint32_t bias, size_t n_out, uint64_t* total) {
  return frcol::runs_impl(device, stream, out, nullptr, t, counts, n_t, bias, n_out, total, nullptr, false, false);
}
int msm_frcol_expand(int device, uint8_t* out, const uint8_t* t, const uint32_t* counts, size_t n_t, uint32_t bias, size_t n_out, uint64_t* total) {
  return frcol::runs_impl(device, nullptr, out, nullptr, t, counts, n_t, bias, n_out, total, nullptr, false, true);
}
int msm_frcol_pair_device(int device, void* stream, void* a_out, void* s_out, const void* t, const uint32_t* counts, size_t n, uint64_t* total, uint64_t* used) {
  return frcol::runs_impl(device, stream, a_out, s_out, t, counts, n, 0, n, total, used, true, false);
}
int msm_frcol_pair(int device, uint8_t* a_out, uint8_t* s_out, const uint8_t* t, const uint32_t* counts, size_t n, uint64_t* total, uint64_t* used) {
  return frcol::runs_impl(device, nullptr, a_out, s_out, t, counts, n, 0, n, total, used, true, true);
}
int msm_frcol_gather_device(int device, void* stream, void* out, const void* a, size_t n_a, const uint32_t* idx, size_t n) {
  return frcol::gather_impl(device, stream, out, a, n_a, idx, n, false);
}
int msm_frcol_gather(int device, uint8_t* out, const uint8_t* a, size_t n_a, const uint32_t* idx, size_t n) {
  return frcol::gather_impl(device, nullptr, out, a, n_a, idx, n, true);
}

void msm_frcol_release(void) {
  std::lock_guard<std::mutex> hold(frcol::lock());
  for (auto& kv : frcol::states()) {
    frcol::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    frcol::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    fr_host::drop(ds.scratch);
    fr_host::drop(ds.staging);
  }
}

int msm_frcol_test_tile(int entries) {
  if (entries != 0 && (entries < 2 || entries > FRCOL_TILE)) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(frcol::lock());
  frcol::hooks().tile = (uint32_t)entries;
  return MSM_HIP_OK;
}
int msm_frcol_test_last(int* launches, int* levels) {
  std::lock_guard<std::mutex> hold(frcol::lock());
  if (launches) *launches = frcol::hooks().launches;
  if (levels) *levels = frcol::hooks().levels;
  return MSM_HIP_OK;
}
}  // extern "C"
