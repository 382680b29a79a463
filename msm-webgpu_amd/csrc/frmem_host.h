// Host side of libmsm_frmem.so (include/msm_frmem.h): argument checks, the plan (csrc/frmem_plan.h), staging, and the launches of
// csrc/frmem_kernels.h.  One translation unit (csrc/frmem.hip), no field.
//
// A call enqueues everything on one stream, the check of the keys included -- the first pass's k_frmem_hist sets the error word, and every launch
// that writes an output reads it and writes nothing where it is set --, copies the result words into the device's pinned buffer in ONE copy and
// waits for the stream (DESIGN.md sections 4.19, 4.27).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>

#include "../../include/msm_frmem.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers and the state scheme every scalar-field library shares
#include "frmem_kernels.h"
#include "frmem_plan.h"

namespace frmem {

using fr_host::Buffer;
using fr_host::DeviceGuard;
using fr_host::grow;
using fr_host::hip_ok;

struct DeviceState {
  hipStream_t stream = nullptr;
  Buffer result;    // FRMEM_RESULT_WORDS words: the error word, the total, the distinct keys
  Buffer h_result;  // pinned: what the one copy of a call fills
  Buffer scratch;   // the (key, index) buffers, the digit counts, start[], the nodes of the scans' levels (frmem::Plan)
  Buffer staging;   // the host forms' operands
};
struct Hooks {
  uint32_t tile = 0;  // 0: FRMEM_TILE
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
  int rc = grow(ds.result, FRMEM_RESULT_WORDS);
  if (!rc) rc = grow(ds.h_result, FRMEM_RESULT_WORDS, true);
  *out = &ds;
  return rc;
}

// one scan on `st`: the sums upwards, the scans from the top level down.  KIND: what level 0 is (FRMEM_WORDS: the digit counts, in place;
// FRMEM_HEADS: the sorted keys, into start); nodes: the levels above it; res_at: the result word that takes the total
template <int KIND, class KEY>
inline void enqueue_scan(hipStream_t st, void* leaf, FrmNode* nodes, const std::vector<size_t>& len, const std::vector<size_t>& node_at, uint32_t* start, uint32_t* res,
                         uint32_t res_at, uint32_t tile) {
  const size_t top = len.size() - 1;
  const dim3 threads(FRMEM_THREADS);
  for (size_t l = 0; l < top; l++) {
    FrmNode* const above = nodes + node_at[l + 1];
    if (l == 0)
      hipLaunchKernelGGL((k_frmem_sums<KIND, KEY>), dim3((uint32_t)len[1]), threads, 0, st, leaf, above, (uint32_t)len[0], (uint32_t)len[1], tile);
    else
      hipLaunchKernelGGL((k_frmem_sums<FRMEM_INNER, uint32_t>), dim3((uint32_t)len[l + 1]), threads, 0, st, nodes + node_at[l], above, (uint32_t)len[l], (uint32_t)len[l + 1], tile);
  }
  for (size_t l = top + 1; l-- > 0;) {
    const FrmNode* const above = l == top ? nullptr : nodes + node_at[l + 1];
    const dim3 grid(l == top ? 1u : (uint32_t)len[l + 1]);
    if (l == 0)
      hipLaunchKernelGGL((k_frmem_scan<KIND, KEY>), grid, threads, 0, st, leaf, above, (uint32_t)len[0], start, res, res_at, tile);
    else
      hipLaunchKernelGGL((k_frmem_scan<FRMEM_INNER, uint32_t>), grid, threads, 0, st, nodes + node_at[l], above, (uint32_t)len[l], nullptr, res, res_at, tile);
  }
}

// the passes of the sort on `st`.  The last pass writes (final_keys, final_idx) -- final_keys may be null: the keys are then not kept -- or, where
// final_idx is null, its buffer of the scratch like every other pass (access reads it there).
template <class KEY>
inline void enqueue_sort(DeviceState& ds, hipStream_t st, const Plan& y, const KEY* keys, uint64_t max_key, KEY* final_keys, uint32_t* final_idx) {
  uint32_t* const s = ds.scratch.p;
  uint32_t* const hist = s + y.hist_at;
  FrmNode* const nodes = reinterpret_cast<FrmNode*>(s + y.dnodes_at);
  const dim3 threads(FRMEM_THREADS), grid(y.tiles);
  for (uint32_t pass = 0; pass < y.passes; pass++) {
    const FrmemArgs g = plan_args(y, pass, max_key);
    const int from = src_buffer(pass), to = dst_buffer(pass);
    const KEY* const src_keys = from < 0 ? keys : reinterpret_cast<const KEY*>(s + y.keys_at[from]);
    const uint32_t* const src_idx = from < 0 ? nullptr : s + y.idx_at[from];
    const bool last = pass + 1 == y.passes && final_idx;
    KEY* const dst_keys = last ? final_keys : reinterpret_cast<KEY*>(s + y.keys_at[to]);
    uint32_t* const dst_idx = last ? final_idx : s + y.idx_at[to];
    hipLaunchKernelGGL(k_frmem_hist<KEY>, grid, threads, 0, st, src_keys, hist, ds.result.p, g);
    enqueue_scan<FRMEM_WORDS, uint32_t>(st, hist, nodes, y.dlen, y.dnode_at, nullptr, ds.result.p, FRMEM_RES_TOTAL, y.tile);
    hipLaunchKernelGGL(k_frmem_scatter<KEY>, grid, threads, 0, st, src_keys, src_idx, hist, dst_keys, dst_idx, ds.result.p, g);
  }
}

// the rest of access: counts and last filled, the heads' scan over the sorted keys, the writes
template <class KEY>
inline void enqueue_access(DeviceState& ds, hipStream_t st, const Plan& y, size_t n_t, uint32_t* rank, uint32_t* prev, uint32_t* counts, uint32_t* last) {
  uint32_t* const s = ds.scratch.p;
  const int in = dst_buffer(y.passes - 1);
  KEY* const keys = reinterpret_cast<KEY*>(s + y.keys_at[in]);
  const dim3 threads(FRMEM_THREADS);
  if (y.table) hipLaunchKernelGGL(k_frmem_fill, dim3((uint32_t)((n_t + FRMEM_THREADS - 1) / FRMEM_THREADS)), threads, 0, st, ds.result.p, counts, last, (uint32_t)n_t);
  enqueue_scan<FRMEM_HEADS, KEY>(st, keys, reinterpret_cast<FrmNode*>(s + y.hnodes_at), y.hlen, y.hnode_at, s + y.start_at, ds.result.p, FRMEM_RES_DISTINCT, y.tile);
  hipLaunchKernelGGL(k_frmem_access<KEY>, dim3((y.n + FRMEM_THREADS - 1) / FRMEM_THREADS), threads, 0, st, y.n, y.table ? (uint32_t)n_t : 0u, ds.result.p, keys, s + y.idx_at[in],
                     s + y.start_at, rank, prev, counts, last);
}

// the result words back, the stream complete
inline int collect(DeviceState& ds, hipStream_t st) {
  if (!hip_ok(hipGetLastError()) || !hip_ok(hipMemcpyAsync(ds.h_result.p, ds.result.p, FRMEM_RESULT_WORDS * 4, hipMemcpyDeviceToHost, st)) || !hip_ok(hipStreamSynchronize(st)))
    return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}

// sort (access false: out[0] = perm_out, out[1] = keys_out) and access (out = rank, prev, counts, last)
inline int call_impl(int device, void* stream, bool access, void* const out[4], size_t n_t, const void* keys, size_t key_bytes, uint32_t key_bits, size_t n, uint64_t* distinct,
                     bool host) {
  if (device < 0) return MSM_HIP_ERR_INVALID_ARG;
  if (access ? !access_args_ok(out[0], out[1], out[2], out[3], n_t, keys, key_bytes, key_bits, n) : !sort_args_ok(out[0], out[1], keys, key_bytes, key_bits, n))
    return MSM_HIP_ERR_INVALID_ARG;
  int rc = fr_host::have_device(device);
  if (rc) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  DeviceState* dsp = nullptr;
  if ((rc = device_state(device, &dsp))) return rc;
  DeviceState& ds = *dsp;
  const hipStream_t st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  const bool table = access && (out[2] || out[3]);
  if (!tile_ok(n, tile_of(hooks().tile))) return MSM_HIP_ERR_INVALID_ARG;  // (the test hook alone: csrc/frmem_plan.h)
  const Plan y = plan_call(n, key_bytes, key_bits, tile_of(hooks().tile), access, table);
  const uint64_t max_key = max_key_of(key_bits, table ? n_t : 0);
  if ((rc = grow(ds.scratch, y.words))) return rc;
  // what each output holds, in words (sort: perm, keys; access: rank, prev, counts, last)
  const size_t words[4] = {n, access ? n : n * y.kw, table ? n_t : 0, table ? n_t : 0};
  const void* dkeys = keys;
  void* dout[4] = {out[0], out[1], access ? out[2] : nullptr, access ? out[3] : nullptr};
  if (host) {  // staging: the keys, then sort's keys_out (words of 8 bytes first), then the outputs of 32-bit words
    size_t total = n * y.kw + (n * y.kw & 1);
    size_t at[4];
    const int order[4] = {access ? 0 : 1, access ? 1 : 0, 2, 3};
    for (int k : order) at[k] = total, total += dout[k] ? words[k] + (words[k] & 1) : 0;
    if ((rc = grow(ds.staging, total))) return rc;
    uint32_t* const s = ds.staging.p;
    if (!hip_ok(hipMemcpyAsync(s, keys, n * key_bytes, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
    dkeys = s;
    for (int k = 0; k < 4; k++)
      if (dout[k]) dout[k] = s + at[k];
  }
  if (!hip_ok(hipMemsetAsync(ds.result.p, 0, FRMEM_RESULT_WORDS * 4, st))) return MSM_HIP_ERR_HIP;
  uint32_t* w[4];
  for (int k = 0; k < 4; k++) w[k] = static_cast<uint32_t*>(dout[k]);
  if (key_bytes == 4) {
    enqueue_sort<uint32_t>(ds, st, y, static_cast<const uint32_t*>(dkeys), max_key, access ? nullptr : static_cast<uint32_t*>(dout[1]), access ? nullptr : w[0]);
    if (access) enqueue_access<uint32_t>(ds, st, y, n_t, w[0], w[1], w[2], w[3]);
  } else {
    enqueue_sort<uint64_t>(ds, st, y, static_cast<const uint64_t*>(dkeys), max_key, access ? nullptr : static_cast<uint64_t*>(dout[1]), access ? nullptr : w[0]);
    if (access) enqueue_access<uint64_t>(ds, st, y, n_t, w[0], w[1], w[2], w[3]);
  }
  hooks().launches = y.launches, hooks().levels = y.levels;
  if ((rc = collect(ds, st))) return rc;
  if (ds.h_result.p[FRMEM_RES_ERR]) return MSM_HIP_ERR_INVALID_ARG;  // (nothing was written)
  if (distinct) *distinct = ds.h_result.p[FRMEM_RES_DISTINCT];
  if (host)
    for (int k = 0; k < 4; k++)
      if (dout[k] && !hip_ok(hipMemcpy(out[k], dout[k], words[k] * 4, hipMemcpyDeviceToHost))) return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}

}  // namespace frmem

extern "C" {
int msm_frmem_abi_version(void) { return 1; }

int msm_frmem_sort_device(int device, void* stream, uint32_t* perm_out, void* keys_out, const void* keys, size_t key_bytes, uint32_t key_bits, size_t n) {
  void* const out[4] = {perm_out, keys_out, nullptr, nullptr};
  return frmem::call_impl(device, stream, false, out, 0, keys, key_bytes, key_bits, n, nullptr, false);
}
int msm_frmem_sort(int device, uint32_t* perm_out, void* keys_out, const void* keys, size_t key_bytes, uint32_t key_bits, size_t n) {
  void* const out[4] = {perm_out, keys_out, nullptr, nullptr};
  return frmem::call_impl(device, nullptr, false, out, 0, keys, key_bytes, key_bits, n, nullptr, true);
}
int msm_frmem_access_device(int device, void* stream, uint32_t* rank_out, uint32_t* prev_out, uint32_t* counts_out, uint32_t* last_out, size_t n_t, const void* keys,
                            size_t key_bytes, uint32_t key_bits, size_t n, uint64_t* distinct) {
  void* const out[4] = {rank_out, prev_out, counts_out, last_out};
  return frmem::call_impl(device, stream, true, out, n_t, keys, key_bytes, key_bits, n, distinct, false);
}
int msm_frmem_access(int device, uint32_t* rank_out, uint32_t* prev_out, uint32_t* counts_out, uint32_t* last_out, size_t n_t, const void* keys, size_t key_bytes,
                     uint32_t key_bits, size_t n, uint64_t* distinct) {
  void* const out[4] = {rank_out, prev_out, counts_out, last_out};
  return frmem::call_impl(device, nullptr, true, out, n_t, keys, key_bytes, key_bits, n, distinct, true);
}

void msm_frmem_release(void) {
  std::lock_guard<std::mutex> hold(frmem::lock());
  for (auto& kv : frmem::states()) {
    frmem::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    frmem::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    fr_host::drop(ds.scratch);
    fr_host::drop(ds.staging);
  }
}

int msm_frmem_test_tile(int entries) {
  if (entries != 0 && (entries < 2 || entries > FRMEM_TILE)) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(frmem::lock());
  frmem::hooks().tile = (uint32_t)entries;
  return MSM_HIP_OK;
}
int msm_frmem_test_last(int* launches, int* levels) {
  std::lock_guard<std::mutex> hold(frmem::lock());
  if (launches) *launches = frmem::hooks().launches;
  if (levels) *levels = frmem::hooks().levels;
  return MSM_HIP_OK;
}
}  // extern "C"
