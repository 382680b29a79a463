// Host side of libmsm_frhash.so (include/msm_frhash.h): the handle, argument checks, the table of a permutation and the levels of a tree
// (csrc/frhash_plan.h), their way to the device, staging, and the launches of csrc/frhash_kernels.h through each field's FrhashOps.  Compiled
// once, by the unit that defines MSM_FRHASH_HOST_UNIT (csrc/frhash_bn254.hip).
//
// A handle keeps its table in host memory until its first call.  The error word of a call comes back in one copy into one pinned buffer per
// device (DESIGN.md sections 4.19 - 4.24).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/msm_frhash.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "frhash_plan.h"
// (csrc/frhash_kernels.h -- FrhashArgs, FrhashOps -- is already in: csrc/frhash_unit.h includes this file behind the unit's kernels)

extern "C" const FrhashOps* msm_frhash_ops_bn254(void);
extern "C" const FrhashOps* msm_frhash_ops_grumpkin(void);
extern "C" const FrhashOps* msm_frhash_ops_pallas(void);
extern "C" const FrhashOps* msm_frhash_ops_vesta(void);
extern "C" const FrhashOps* msm_frhash_ops_bls12_381(void);

struct msm_frhash {
  uint32_t magic = 0;
  const FrhashOps* ops = nullptr;
  int device = 0;
  uint32_t t = 0, full_rounds = 0, partial_rounds = 0;
  uint32_t kind = 0;                    // FRHASH_KIND_*: Poseidon, or Poseidon2 (MSM_FRHASH_POSEIDON2)
  std::vector<uint32_t> h_table;        // what csrc/frhash_plan.h made of the constants
  mutable uint32_t* d_table = nullptr;  // the same on the device, from the first call on
};

namespace frhash {

using namespace fr_host;

using namespace msm_frhash_plan;

constexpr uint32_t MAGIC = 0x48534148u;

struct DeviceState {
  hipStream_t stream = nullptr;
  Buffer result;    // word 0: the error word
  Buffer h_result;  // pinned: what the one copy of a call fills
  Buffer staging;   // the host forms' vectors
};

inline std::mutex& lock() { return lock_of<DeviceState>(); }
inline std::map<int, DeviceState>& states() { return states_of<DeviceState>(); }
inline uint32_t& tile_hook() {
  static uint32_t lanes = 0;
  return lanes;
}

inline const FrhashOps* field_of(int curve) {
  return fr_host::field_of<FrhashOps>(curve, msm_frhash_ops_bn254, msm_frhash_ops_grumpkin, msm_frhash_ops_pallas, msm_frhash_ops_vesta, msm_frhash_ops_bls12_381);
}

inline bool is_handle(const msm_frhash* h) { return h && h->magic == MAGIC; }

// What every call does once its arguments have passed: the device, its state and stream, the handle's table on the device, a clear error
// word.  Holds the guard and the lock for as long as it lives.
struct Call {
  DeviceGuard guard;
  std::unique_lock<std::mutex> hold;
  DeviceState* ds = nullptr;
  hipStream_t st = nullptr;
  uint32_t tile = 0;
  int rc = MSM_HIP_OK;
  Call(const msm_frhash* h, void* stream, bool host) : guard(h->device), hold(lock(), std::defer_lock) {
    if (!guard.ok) {
      rc = MSM_HIP_ERR_NO_DEVICE;
      return;
    }
    hold.lock();
    ds = &states()[h->device];
    tile = tile_hook();
    if (!ds->stream && hipStreamCreateWithFlags(&ds->stream, hipStreamNonBlocking) != hipSuccess) {
      rc = MSM_HIP_ERR_NO_DEVICE;
      return;
    }
    if ((rc = grow(ds->result, FRHASH_RESULT_HEAD)) || (rc = grow(ds->h_result, FRHASH_RESULT_HEAD, true))) return;
    st = stream && !host ? static_cast<hipStream_t>(stream) : ds->stream;
    if (!h->d_table) {
      if (!hip_ok(hipMalloc(reinterpret_cast<void**>(&h->d_table), h->h_table.size() * 4))) {
        h->d_table = nullptr;
        rc = MSM_HIP_ERR_OUT_OF_MEMORY;
        return;
      }
      if (!hip_ok(hipMemcpyAsync(h->d_table, h->h_table.data(), h->h_table.size() * 4, hipMemcpyHostToDevice, st))) {  // (h_table lives as long as the handle)
        rc = MSM_HIP_ERR_HIP;
        return;
      }
    }
    if (!hip_ok(hipMemsetAsync(ds->result.p, 0, 4, st))) rc = MSM_HIP_ERR_HIP;
  }
  // the error word, behind everything the call enqueued
  int finish() {
    if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
    if (!hip_ok(hipMemcpyAsync(ds->h_result.p, ds->result.p, 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
    if (!hip_ok(hipStreamSynchronize(st))) return MSM_HIP_ERR_HIP;
    return ds->h_result.p[0] ? MSM_HIP_ERR_NONCANONICAL : MSM_HIP_OK;
  }
};

inline int create_impl(int curve, int device, uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, uint32_t alpha, const uint8_t* rc, const uint8_t* mds, uint32_t flags,
                       msm_frhash** out) {
  const FrhashOps* ops = field_of(curve);
  if (!out) return MSM_HIP_ERR_INVALID_ARG;
  *out = nullptr;
  if (!ops || device < 0 || !rc || !mds || !shape_ok(t, full_rounds, partial_rounds, alpha, flags)) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  const uint32_t kind = kind_of(flags);
  if (!all_below_r(f, rc, constants_of(kind, t, full_rounds, partial_rounds)) || !all_below_r(f, mds, matrix_of(kind, t))) return MSM_HIP_ERR_NONCANONICAL;
  msm_frhash* h = new msm_frhash();
  h->magic = MAGIC, h->ops = ops, h->device = device, h->t = t, h->full_rounds = full_rounds, h->partial_rounds = partial_rounds, h->kind = kind;
  plan_table(f, t, full_rounds, partial_rounds, rc, mds, h->h_table, kind);
  *out = h;
  return MSM_HIP_OK;
}

inline int permute_impl(const msm_frhash* h, void* stream, void* out, const void* state, size_t n, uint32_t flags, bool host) {
  if (!is_handle(h) || !out || !state || !permute_args_ok(h->t, n, flags)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(out) || misaligned(state))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  const size_t total = n * h->t;
  if (out != state && !apart(out, total * 32, state, total * 32)) return MSM_HIP_ERR_INVALID_ARG;  // in place, or apart
  int rc = have_device(h->device);
  if (rc) return rc;
  Call call(h, stream, host);
  if (call.rc) return call.rc;
  const hipStream_t st = call.st;
  const FrhashArgs g = plan_args(h->t, h->full_rounds, h->partial_rounds, n, flags, call.tile, h->kind);
  uint32_t* dout = static_cast<uint32_t*>(out);
  const uint32_t* din = static_cast<const uint32_t*>(state);
  if (host) {  // staging: the states, permuted in place
    if ((rc = grow(call.ds->staging, total * 8))) return rc;
    dout = call.ds->staging.p;
    din = dout;
    if (!hip_ok(hipMemcpyAsync(dout, state, total * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
  }
  h->ops->permute(blocks_of(g), st, dout, din, h->d_table, &g, call.ds->result.p);
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  if (host && !hip_ok(hipMemcpyAsync(out, dout, total * 32, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  return call.finish();
}

inline int hash_impl(const msm_frhash* h, void* stream, void* out, const void* a, size_t rows, size_t len, size_t stride, const uint8_t* capacity, uint32_t capacity_at,
                     uint32_t out_at, uint32_t flags, bool host) {
  if (!is_handle(h) || !out || !a || !hash_args_ok(h->t, rows, len, stride, capacity_at, out_at, flags)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(out) || misaligned(a))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  const size_t span = (rows - 1) * stride + len;
  if (!apart(out, rows * 32, a, span * 32)) return MSM_HIP_ERR_INVALID_ARG;
  FrhashArgs g = plan_args(h->t, h->full_rounds, h->partial_rounds, rows, flags, 0, h->kind);
  g.len = (uint32_t)len, g.stride = (uint32_t)stride, g.capacity_at = capacity_at, g.out_at = out_at;
  if (!plan_capacity(Field(h->ops->r32), capacity, g)) return MSM_HIP_ERR_NONCANONICAL;
  int rc = have_device(h->device);
  if (rc) return rc;
  Call call(h, stream, host);
  if (call.rc) return call.rc;
  const hipStream_t st = call.st;
  if (call.tile) g.tile = call.tile;
  uint32_t* dout = static_cast<uint32_t*>(out);
  const uint32_t* da = static_cast<const uint32_t*>(a);
  if (host) {  // staging: a, then out
    if ((rc = grow(call.ds->staging, (span + rows) * 8))) return rc;
    uint32_t* const sa = call.ds->staging.p;
    dout = sa + span * 8;
    da = sa;
    if (!hip_ok(hipMemcpyAsync(sa, a, span * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
  }
  h->ops->hash(blocks_of(g), st, dout, da, h->d_table, &g, call.ds->result.p);
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  if (host && !hip_ok(hipMemcpyAsync(out, dout, rows * 32, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  return call.finish();
}

inline int merkle_impl(const msm_frhash* h, void* stream, void* nodes, const void* leaves, size_t n_leaves, const uint8_t* capacity, uint32_t capacity_at, uint32_t out_at,
                       uint32_t flags, bool host) {
  if (!is_handle(h) || !nodes || !leaves || (flags & ~KNOWN_FLAGS) || capacity_at >= h->t || out_at >= h->t) return MSM_HIP_ERR_INVALID_ARG;
  std::vector<size_t> levels;
  if (!plan_levels(h->t, n_leaves, levels)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(nodes) || misaligned(leaves))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  const size_t below = leaf_count(h->t, n_leaves), above = node_count(levels), arity = h->t - 1;
  if (!apart(nodes, above * 32, leaves, below * 32)) return MSM_HIP_ERR_INVALID_ARG;
  FrhashArgs g = plan_args(h->t, h->full_rounds, h->partial_rounds, 1, flags, 0, h->kind);
  g.len = g.stride = (uint32_t)arity, g.capacity_at = capacity_at, g.out_at = out_at;
  if (!plan_capacity(Field(h->ops->r32), capacity, g)) return MSM_HIP_ERR_NONCANONICAL;
  int rc = have_device(h->device);
  if (rc) return rc;
  Call call(h, stream, host);
  if (call.rc) return call.rc;
  const hipStream_t st = call.st;
  if (call.tile) g.tile = call.tile;
  uint32_t* dnodes = static_cast<uint32_t*>(nodes);
  const uint32_t* dleaves = static_cast<const uint32_t*>(leaves);
  if (host) {  // staging: the leaves, then the nodes
    if ((rc = grow(call.ds->staging, (below + above) * 8))) return rc;
    uint32_t* const sl = call.ds->staging.p;
    dnodes = sl + below * 8;
    dleaves = sl;
    if (!hip_ok(hipMemcpyAsync(sl, leaves, below * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
  }
  const uint32_t* from = dleaves;  // one launch per level, each behind the one below it on the stream
  uint32_t* to = dnodes;
  for (size_t count : levels) {
    g.n = (uint32_t)count;
    h->ops->hash(blocks_of(g), st, to, from, h->d_table, &g, call.ds->result.p);
    if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
    from = to;
    to += count * 8;
  }
  if (host && !hip_ok(hipMemcpyAsync(nodes, dnodes, above * 32, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  return call.finish();
}

}  // namespace frhash

extern "C" {
int msm_frhash_abi_version(void) { return 1; }

int msm_frhash_create(int curve, int device, uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, uint32_t alpha, const uint8_t* round_constants, const uint8_t* mds,
                      uint32_t flags, msm_frhash** out) {
  return frhash::create_impl(curve, device, t, full_rounds, partial_rounds, alpha, round_constants, mds, flags, out);
}

int msm_frhash_info(const msm_frhash* h, uint32_t* t, uint32_t* full_rounds, uint32_t* partial_rounds) {
  if (!frhash::is_handle(h)) return MSM_HIP_ERR_INVALID_ARG;
  if (t) *t = h->t;
  if (full_rounds) *full_rounds = h->full_rounds;
  if (partial_rounds) *partial_rounds = h->partial_rounds;
  return MSM_HIP_OK;
}

void msm_frhash_destroy(msm_frhash* h) {
  if (!frhash::is_handle(h)) return;
  {
    std::lock_guard<std::mutex> hold(frhash::lock());
    if (h->d_table) {
      frhash::DeviceGuard guard(h->device);
      if (guard.ok) (void)hipFree(h->d_table);
      h->d_table = nullptr;
    }
  }
  h->magic = 0;
  delete h;
}

int msm_frhash_permute_device(const msm_frhash* h, void* stream, void* out, const void* state, size_t n, uint32_t flags) {
  return frhash::permute_impl(h, stream, out, state, n, flags, false);
}
int msm_frhash_permute(const msm_frhash* h, uint8_t* out, const uint8_t* state, size_t n, uint32_t flags) { return frhash::permute_impl(h, nullptr, out, state, n, flags, true); }

int msm_frhash_hash_device(const msm_frhash* h, void* stream, void* out, const void* a, size_t rows, size_t len, size_t stride, const uint8_t* capacity, uint32_t capacity_at,
                           uint32_t out_at, uint32_t flags) {
  return frhash::hash_impl(h, stream, out, a, rows, len, stride, capacity, capacity_at, out_at, flags, false);
}
int msm_frhash_hash(const msm_frhash* h, uint8_t* out, const uint8_t* a, size_t rows, size_t len, size_t stride, const uint8_t* capacity, uint32_t capacity_at, uint32_t out_at,
                    uint32_t flags) {
  return frhash::hash_impl(h, nullptr, out, a, rows, len, stride, capacity, capacity_at, out_at, flags, true);
}

int msm_frhash_merkle_device(const msm_frhash* h, void* stream, void* nodes, const void* leaves, size_t n_leaves, const uint8_t* capacity, uint32_t capacity_at,
                             uint32_t out_at, uint32_t flags) {
  return frhash::merkle_impl(h, stream, nodes, leaves, n_leaves, capacity, capacity_at, out_at, flags, false);
}
int msm_frhash_merkle(const msm_frhash* h, uint8_t* nodes, const uint8_t* leaves, size_t n_leaves, const uint8_t* capacity, uint32_t capacity_at, uint32_t out_at,
                      uint32_t flags) {
  return frhash::merkle_impl(h, nullptr, nodes, leaves, n_leaves, capacity, capacity_at, out_at, flags, true);
}

void msm_frhash_release(void) {
  std::lock_guard<std::mutex> hold(frhash::lock());
  for (auto& kv : frhash::states()) {
    frhash::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    frhash::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    fr_host::drop(ds.staging);
  }
}

int msm_frhash_test_tile(int lanes) {
  if (lanes < 0 || lanes > FRHASH_THREADS) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(frhash::lock());
  frhash::tile_hook() = (uint32_t)lanes;
  return MSM_HIP_OK;
}
}  // extern "C"
