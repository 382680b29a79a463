// Host side of libmsm_frlook.so (include/msm_frlook.h): the handle, argument checks, the plan of a table (csrc/frlook_plan.h), its way to the
// device, staging, and the launches of csrc/frlook_kernels.h through each field's FrlookOps.  Compiled once, by the unit that defines
// MSM_FRLOOK_HOST_UNIT (csrc/frlook_bn254.hip).
//
// A handle made from device memory is resident when create returns; one made from host memory keeps its keys in host memory until its first
// count.  The error word, `distinct`, `missing` and `first_missing` of a call come back in one copy into one pinned buffer per device
// (DESIGN.md sections 4.19 - 4.23).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/msm_frlook.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "frlook_plan.h"
// (csrc/frlook_kernels.h -- FrlookArgs, FrlookOps -- is already in: csrc/frlook_unit.h includes this file behind the unit's kernels)

extern "C" const FrlookOps* msm_frlook_ops_bn254(void);
extern "C" const FrlookOps* msm_frlook_ops_grumpkin(void);
extern "C" const FrlookOps* msm_frlook_ops_pallas(void);
extern "C" const FrlookOps* msm_frlook_ops_vesta(void);
extern "C" const FrlookOps* msm_frlook_ops_bls12_381(void);

struct msm_frlook {
  uint32_t magic = 0;
  const FrlookOps* ops = nullptr;
  int device = 0;
  size_t n_t = 0, distinct = 0;
  uint32_t flags = 0;
  FrlookArgs g = {};
  mutable std::vector<uint32_t> h_keys;  // the host form's keys, until they are resident
  mutable bool resident = false;
  mutable uint32_t* d_keys = nullptr;    // n_t x 8 words: the handle's own copy
  mutable uint32_t* d_slots = nullptr;   // slot_mask + 1 words
  mutable uint32_t* d_counts = nullptr;  // n_t words, cleared before every count
};

namespace frlook {

using namespace fr_host;

constexpr uint32_t MAGIC = 0x4b4f4f4cu;

struct DeviceState {
  hipStream_t stream = nullptr;
  Buffer result;    // FRLOOK_RESULT_WORDS words: the error word, distinct, missing, first_missing
  Buffer h_result;  // pinned: what the one copy of a call fills
  Buffer staging;   // the host form's f, m, counts and idx
};

inline std::mutex& lock() { return lock_of<DeviceState>(); }
inline std::map<int, DeviceState>& states() { return states_of<DeviceState>(); }
inline uint32_t& hash_bits_hook() {
  static uint32_t b = 0;
  return b;
}

inline const FrlookOps* field_of(int curve) {
  return fr_host::field_of<FrlookOps>(curve, msm_frlook_ops_bn254, msm_frlook_ops_grumpkin, msm_frlook_ops_pallas, msm_frlook_ops_vesta, msm_frlook_ops_bls12_381);
}

// the device's state, its stream and the two result buffers (the caller holds the guard and the lock)
inline int device_state(int device, DeviceState** out) {
  DeviceState& ds = states()[device];
  if (!ds.stream && hipStreamCreateWithFlags(&ds.stream, hipStreamNonBlocking) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;
  int rc = grow(ds.result, FRLOOK_RESULT_WORDS);
  if (!rc) rc = grow(ds.h_result, FRLOOK_RESULT_WORDS, true);
  *out = &ds;
  return rc;
}
// error word, distinct, missing: 0; first_missing: all ones
inline bool clear_result(DeviceState& ds, hipStream_t st) {
  return hip_ok(hipMemsetAsync(ds.result.p, 0, FRLOOK_RESULT_WORDS * 4, st)) && hip_ok(hipMemsetAsync(ds.result.p + FRLOOK_RES_FIRST, 0xff, 8, st));
}
inline void free_table(const msm_frlook* t) {
  if (t->d_keys) (void)hipFree(t->d_keys);
  if (t->d_slots) (void)hipFree(t->d_slots);
  if (t->d_counts) (void)hipFree(t->d_counts);
  t->d_keys = t->d_slots = t->d_counts = nullptr;
  t->resident = false;
}
// the keys to the handle's own device memory -- from `d_src` (device memory) or from the handle's host copy -- and the build; the caller holds
// the guard and the lock.  `distinct`: what the build claimed.
inline int make_resident(const msm_frlook* t, DeviceState& ds, hipStream_t st, const void* d_src, size_t* distinct) {
  const size_t slots = (size_t)t->g.slot_mask + 1;
  int rc = MSM_HIP_OK;
  if (!hip_ok(hipMalloc(reinterpret_cast<void**>(&t->d_keys), t->n_t * 32)) || !hip_ok(hipMalloc(reinterpret_cast<void**>(&t->d_slots), slots * 4)) ||
      !hip_ok(hipMalloc(reinterpret_cast<void**>(&t->d_counts), t->n_t * 4)))
    rc = MSM_HIP_ERR_OUT_OF_MEMORY;
  if (!rc) {
    const bool copied = d_src ? hip_ok(hipMemcpyAsync(t->d_keys, d_src, t->n_t * 32, hipMemcpyDeviceToDevice, st))
                              : hip_ok(hipMemcpyAsync(t->d_keys, t->h_keys.data(), t->n_t * 32, hipMemcpyHostToDevice, st));
    if (!copied || !hip_ok(hipMemsetAsync(t->d_slots, 0xff, slots * 4, st)) || !clear_result(ds, st)) rc = MSM_HIP_ERR_HIP;
  }
  if (!rc) {
    t->ops->build(st, t->d_keys, t->d_slots, &t->g, ds.result.p);
    if (!hip_ok(hipGetLastError()) || !hip_ok(hipMemcpyAsync(ds.h_result.p, ds.result.p, FRLOOK_RESULT_WORDS * 4, hipMemcpyDeviceToHost, st)) ||
        !hip_ok(hipStreamSynchronize(st)))
      rc = MSM_HIP_ERR_HIP;
  }
  if (!rc && ds.h_result.p[FRLOOK_RES_ERR]) rc = MSM_HIP_ERR_NONCANONICAL;
  if (rc) {
    free_table(t);
    return rc;
  }
  *distinct = ds.h_result.p[FRLOOK_RES_DISTINCT];
  t->resident = true;
  std::vector<uint32_t>().swap(t->h_keys);
  return MSM_HIP_OK;
}

inline int create_impl(int curve, int device, void* stream, const void* table, size_t n_t, uint32_t flags, msm_frlook** out, bool host) {
  const FrlookOps* ops = field_of(curve);
  if (!out) return MSM_HIP_ERR_INVALID_ARG;
  *out = nullptr;
  if (!ops || device < 0 || !table || !table_args_ok(n_t, flags)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && misaligned(table, 16)) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  const Field f(ops->r32);
  if (host && !all_below_r(f, static_cast<const uint8_t*>(table), n_t)) return MSM_HIP_ERR_NONCANONICAL;
  msm_frlook* t = new msm_frlook();
  t->magic = MAGIC, t->ops = ops, t->device = device, t->n_t = n_t, t->flags = flags;
  {
    std::lock_guard<std::mutex> hold(lock());
    t->g = plan_args(f, n_t, hash_bits_hook(), (flags & MSM_FRLOOK_MONT256) != 0);
  }
  if (host) {  // no device is touched: the build, serially, for `distinct`; the keys wait for the first count
    t->h_keys.resize(n_t * 8);
    memcpy(t->h_keys.data(), table, n_t * 32);
    std::vector<uint32_t> slots;
    t->distinct = build_serial(t->g, t->h_keys.data(), slots);
    *out = t;
    return MSM_HIP_OK;
  }
  int rc = have_device(device);
  if (!rc) {
    DeviceGuard guard(device);
    std::lock_guard<std::mutex> hold(lock());
    DeviceState* ds = nullptr;
    rc = guard.ok ? device_state(device, &ds) : MSM_HIP_ERR_NO_DEVICE;
    if (!rc) rc = make_resident(t, *ds, stream ? static_cast<hipStream_t>(stream) : ds->stream, table, &t->distinct);
  }
  if (rc) {
    delete t;
    return rc;
  }
  *out = t;
  return MSM_HIP_OK;
}

inline int count_impl(const msm_frlook* t, void* stream, void* m_out, uint32_t* counts_out, uint32_t* idx_out, const void* f, size_t n, size_t batch, size_t stride,
                      uint32_t flags, uint64_t* missing, uint64_t* first_missing, bool host) {
  if (!t || t->magic != MAGIC || !f) return MSM_HIP_ERR_INVALID_ARG;
  if ((flags & ~MSM_FRLOOK_MONT256) || flags != t->flags || !count_args_ok(n, batch, stride)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(f, 16) || misaligned(m_out, 16))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  if (misaligned(counts_out, 4) || misaligned(idx_out, 4)) return MSM_HIP_ERR_INVALID_ARG;
  const size_t total = batch * n, span = (batch - 1) * stride + n;  // the device form's rows are all of f[0 .. batch stride)
  const void* part[4] = {f, m_out, counts_out, idx_out};
  const size_t bytes[4] = {(host ? span : batch * stride) * 32, t->n_t * 32, t->n_t * 4, total * 4};
  for (int a = 1; a < 4; a++)
    for (int b = 0; b < a; b++)
      if (part[a] && part[b] && !apart(part[a], bytes[a], part[b], bytes[b])) return MSM_HIP_ERR_INVALID_ARG;
  if (host) {  // the comparison with r, before a device is asked for
    const Field fld(t->ops->r32);
    for (size_t row = 0; row < batch; row++)
      if (!all_below_r(fld, static_cast<const uint8_t*>(f) + row * stride * 32, n)) return MSM_HIP_ERR_NONCANONICAL;
  }
  int rc = have_device(t->device);
  if (rc) return rc;
  DeviceGuard guard(t->device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  DeviceState* dsp = nullptr;
  if ((rc = device_state(t->device, &dsp))) return rc;
  DeviceState& ds = *dsp;
  const hipStream_t st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  if (!t->resident) {
    size_t distinct = 0;
    if ((rc = make_resident(t, ds, st, nullptr, &distinct))) return rc;
    if (distinct != t->distinct) return MSM_HIP_ERR_HIP;  // (the host's serial build and the device's agree)
  }
  const uint32_t* df = static_cast<const uint32_t*>(f);
  uint32_t* dm = static_cast<uint32_t*>(m_out);
  uint32_t* dcounts = counts_out;
  uint32_t* didx = idx_out;
  if (host) {  // staging: f, then m, counts and idx as far as they are asked for
    if ((rc = grow(ds.staging, span * 8 + t->n_t * 9 + total))) return rc;
    uint32_t* const sf = ds.staging.p;
    if (!hip_ok(hipMemcpyAsync(sf, f, span * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
    df = sf;
    if (m_out) dm = sf + span * 8;
    if (counts_out) dcounts = sf + span * 8 + t->n_t * 8;
    if (idx_out) didx = sf + span * 8 + t->n_t * 9;
  }
  if (!hip_ok(hipMemsetAsync(t->d_counts, 0, t->n_t * 4, st)) || !clear_result(ds, st)) return MSM_HIP_ERR_HIP;
  t->ops->count(st, t->d_keys, t->d_slots, t->d_counts, didx, df, (uint32_t)n, (uint32_t)total, stride, &t->g, ds.result.p);
  if (dm || dcounts) t->ops->finish(st, t->d_counts, dm, dcounts, &t->g);
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  if (host) {
    if (m_out && !hip_ok(hipMemcpyAsync(m_out, dm, t->n_t * 32, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
    if (counts_out && !hip_ok(hipMemcpyAsync(counts_out, dcounts, t->n_t * 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
    if (idx_out && !hip_ok(hipMemcpyAsync(idx_out, didx, total * 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  }
  if (!hip_ok(hipMemcpyAsync(ds.h_result.p, ds.result.p, FRLOOK_RESULT_WORDS * 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipStreamSynchronize(st))) return MSM_HIP_ERR_HIP;
  if (ds.h_result.p[FRLOOK_RES_ERR]) return MSM_HIP_ERR_NONCANONICAL;
  if (missing) memcpy(missing, ds.h_result.p + FRLOOK_RES_MISSING, 8);
  if (first_missing) memcpy(first_missing, ds.h_result.p + FRLOOK_RES_FIRST, 8);
  return MSM_HIP_OK;
}

}  // namespace frlook

extern "C" {
int msm_frlook_abi_version(void) { return 1; }

int msm_frlook_create_device(int curve, int device, void* stream, const void* table, size_t n_t, uint32_t flags, msm_frlook** out) {
  return frlook::create_impl(curve, device, stream, table, n_t, flags, out, false);
}
int msm_frlook_create(int curve, int device, const uint8_t* table, size_t n_t, uint32_t flags, msm_frlook** out) {
  return frlook::create_impl(curve, device, nullptr, table, n_t, flags, out, true);
}

int msm_frlook_info(const msm_frlook* t, size_t* n_t, size_t* distinct, uint32_t* flags) {
  if (!t || t->magic != frlook::MAGIC) return MSM_HIP_ERR_INVALID_ARG;
  if (n_t) *n_t = t->n_t;
  if (distinct) *distinct = t->distinct;
  if (flags) *flags = t->flags;
  return MSM_HIP_OK;
}

void msm_frlook_destroy(msm_frlook* t) {
  if (!t || t->magic != frlook::MAGIC) return;
  {
    std::lock_guard<std::mutex> hold(frlook::lock());
    if (t->resident) {
      frlook::DeviceGuard guard(t->device);
      if (guard.ok) frlook::free_table(t);
    }
  }
  t->magic = 0;
  delete t;
}

int msm_frlook_count_device(const msm_frlook* t, void* stream, void* m_out, uint32_t* counts_out, uint32_t* idx_out, const void* f, size_t n, size_t batch, size_t stride,
                            uint32_t flags, uint64_t* missing, uint64_t* first_missing) {
  return frlook::count_impl(t, stream, m_out, counts_out, idx_out, f, n, batch, stride, flags, missing, first_missing, false);
}
int msm_frlook_count(const msm_frlook* t, uint8_t* m_out, uint32_t* counts_out, uint32_t* idx_out, const uint8_t* f, size_t n, size_t batch, size_t stride, uint32_t flags,
                     uint64_t* missing, uint64_t* first_missing) {
  return frlook::count_impl(t, nullptr, m_out, counts_out, idx_out, f, n, batch, stride, flags, missing, first_missing, true);
}

void msm_frlook_release(void) {
  std::lock_guard<std::mutex> hold(frlook::lock());
  for (auto& kv : frlook::states()) {
    frlook::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    frlook::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    fr_host::drop(ds.staging);
  }
}

int msm_frlook_test_hash_bits(int bits) {
  if (bits < 0 || bits > 32) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(frlook::lock());
  frlook::hash_bits_hook() = (uint32_t)bits;
  return MSM_HIP_OK;
}
}  // extern "C"
