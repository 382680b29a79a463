// Host side of libmsm_fr.so (include/msm_fr.h): argument checks, the plan of a transform's passes, the twiddle tables (built with host_fr.h,
// cached on the device per field, log_n and base), scratch, and the launches of csrc/ntt_kernels.h through each field's FrOps.  Compiled once, by
// the unit that defines MSM_FR_HOST_UNIT (csrc/fr_bn254.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/msm_fr.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "host_fr.h"
#include "ntt_plan.h"
// (csrc/ntt_kernels.h -- NttPass, NttTables, FrOps -- is already in: csrc/fr_unit.h includes this file behind the unit's kernels)

extern "C" const FrOps* msm_fr_ops_bn254(void);
extern "C" const FrOps* msm_fr_ops_pallas(void);
extern "C" const FrOps* msm_fr_ops_vesta(void);
extern "C" const FrOps* msm_fr_ops_bls12_381(void);

namespace msm_fr {

using namespace fr_host;

struct Table {  // a two-level power table on the device: lo[k] = g^k (k < 2^lo_bits), hi[k] = c g^(k 2^lo_bits), all times 2^261, canonical
  uint32_t *lo = nullptr, *hi = nullptr;
  uint32_t lo_bits = 0, mode = 0;
};
struct DeviceState {
  hipStream_t stream = nullptr;
  uint32_t* d_err = nullptr;
  uint32_t* h_err = nullptr;  // pinned: the error word comes back without a staging copy
  Buffer scratch, staging;
  std::map<std::string, Table> tables;
  std::map<std::string, uint32_t*> butterflies;
};

inline std::mutex& lock() { return lock_of<DeviceState>(); }
inline std::map<int, DeviceState>& states() { return states_of<DeviceState>(); }
inline int& pass_bits_cap() {
  static int b = 0;
  return b;
}
inline int (&last_shape())[2] {
  static int s[2] = {0, 0};
  return s;
}

inline const FrOps* field_of(int curve, int* field_id) {  // (Grumpkin: r - 1 = 2 * odd, so no unit)
  return fr_host::field_of<FrOps>(curve, msm_fr_ops_bn254, nullptr, msm_fr_ops_pallas, msm_fr_ops_vesta, msm_fr_ops_bls12_381, field_id);
}

inline std::string key_of(const char* kind, int field, int bits, const uint8_t* g, int extra) {
  std::string s(kind);
  s += (char)('0' + field);
  s += (char)bits;
  s += (char)extra;
  s.append(reinterpret_cast<const char*>(g), 32);
  return s;
}

inline int upload(uint32_t** dst, const std::vector<uint32_t>& src, hipStream_t st) {
  if (hipMalloc(reinterpret_cast<void**>(dst), src.size() * 4) != hipSuccess) return MSM_HIP_ERR_OUT_OF_MEMORY;
  if (hipMemcpyAsync(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}

// a two-level power table (csrc/ntt_plan.h: build_power_table) on the device, built at its first use
inline int power_table(DeviceState& ds, const host_fr::Field& f, int field, const uint8_t* g, int bits, int inv_log_n, hipStream_t st, Table* out) {
  static const uint8_t none[32] = {0};
  const std::string key = key_of(g ? "p" : "c", field, bits, g ? g : none, inv_log_n);
  auto it = ds.tables.find(key);
  if (it != ds.tables.end()) {
    *out = it->second;
    return MSM_HIP_OK;
  }
  const HostTable h = build_power_table(f, g, bits, inv_log_n);
  Table t;
  t.lo_bits = h.lo_bits, t.mode = h.mode;
  int rc;
  if (!h.lo.empty() && (rc = upload(&t.lo, h.lo, st))) return rc;
  if (!h.hi.empty() && (rc = upload(&t.hi, h.hi, st))) return rc;
  ds.tables[key] = t;
  *out = t;
  return MSM_HIP_OK;
}

// the butterflies' twiddles (csrc/ntt_plan.h: build_butterfly_table) on the device
inline int butterfly_table(DeviceState& ds, const host_fr::Field& f, int field, const uint8_t* omega, int log_n, int tw_log, hipStream_t st, uint32_t** out) {
  const std::string key = key_of("b", field, log_n, omega, tw_log);
  auto it = ds.butterflies.find(key);
  if (it != ds.butterflies.end()) {
    *out = it->second;
    return MSM_HIP_OK;
  }
  uint32_t* d = nullptr;
  const int rc = upload(&d, build_butterfly_table(f, omega, log_n, tw_log), st);
  if (rc) return rc;
  ds.butterflies[key] = d;
  *out = d;
  return MSM_HIP_OK;
}

// every argument is checked before anything is enqueued; `host`: data is host memory, staged through the device
inline int ntt_impl(int curve, int device, void* stream, void* data, int log_n, size_t batch, const uint8_t* omega, const uint8_t* pre, const uint8_t* post, uint32_t flags,
                    bool host) {
  int field = 0;
  const FrOps* ops = field_of(curve, &field);
  if (!ops) return MSM_HIP_ERR_INVALID_ARG;
  if (flags & ~(MSM_FR_SCALE_INV_N | MSM_FR_MONT256)) return MSM_HIP_ERR_INVALID_ARG;
  if (!data || !omega || batch == 0 || device < 0) return MSM_HIP_ERR_INVALID_ARG;
  if (log_n < 0 || log_n > 26 || log_n > ops->two_adicity) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (reinterpret_cast<uintptr_t>(data) & 15u)) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  const host_fr::Field f(ops->r32);
  if (!host_fr::is_primitive_root(f, omega, log_n)) return MSM_HIP_ERR_INVALID_ARG;
  if ((pre && !below_r(f, pre)) || (post && !below_r(f, post))) return MSM_HIP_ERR_INVALID_ARG;
  const int cap = pass_bits_cap() ? pass_bits_cap() : NTT_PASS_BITS;
  const std::vector<uint32_t> dig = plan_digits(log_n, cap);
  std::vector<NttPass> passes = plan_passes(log_n, dig);
  const size_t n = (size_t)1 << log_n;
  if (batch > ((size_t)1 << 40) / n) return MSM_HIP_ERR_INVALID_ARG;
  for (const NttPass& p : passes)
    if ((batch << (p.log_n - p.b - p.log_c)) >= ((size_t)1 << 31)) return MSM_HIP_ERR_INVALID_ARG;  // (workgroups of one launch)
  int rc = have_device(device);
  if (rc) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  DeviceState& ds = states()[device];
  if (!ds.stream && hipStreamCreateWithFlags(&ds.stream, hipStreamNonBlocking) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;
  if (!ds.d_err && hipMalloc(reinterpret_cast<void**>(&ds.d_err), 4) != hipSuccess) return MSM_HIP_ERR_OUT_OF_MEMORY;
  if (!ds.h_err && hipHostMalloc(reinterpret_cast<void**>(&ds.h_err), 4, hipHostMallocDefault) != hipSuccess) return MSM_HIP_ERR_OUT_OF_MEMORY;
  hipStream_t st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  const size_t words = batch * n * 8;
  if (host && (rc = grow(ds.staging, words))) return rc;
  if (passes.size() > 1 && (rc = grow(ds.scratch, words))) return rc;
  uint32_t* d_data = host ? ds.staging.p : static_cast<uint32_t*>(data);

  NttTables t;
  memset(&t, 0, sizeof t);
  uint32_t* bt = nullptr;
  if (log_n > 0 && (rc = butterfly_table(ds, f, field, omega, log_n, (int)passes[0].tw_log, st, &bt))) return rc;
  t.bt = bt;
  Table tw, tpre, tpost;
  if (passes.size() > 1) {
    if ((rc = power_table(ds, f, field, omega, log_n, 0, st, &tw))) return rc;
    t.tw_lo = tw.lo, t.tw_hi = tw.hi;
  }
  const int inv = (flags & MSM_FR_SCALE_INV_N) && log_n > 0 ? log_n : 0;  // (1 / 1 = 1)
  if (pre) {
    if ((rc = power_table(ds, f, field, pre, log_n, 0, st, &tpre))) return rc;
    t.pre_lo = tpre.lo, t.pre_hi = tpre.hi;
  }
  if (post || inv) {
    if ((rc = power_table(ds, f, field, post, log_n, inv, st, &tpost))) return rc;
    t.post_lo = tpost.lo, t.post_hi = tpost.hi;
  }
  for (NttPass& p : passes) {
    p.tw_mode = tw.mode, p.tw_lo_bits = tw.lo_bits;
    p.pre_mode = p.first ? tpre.mode : 0, p.pre_lo_bits = tpre.lo_bits;
    p.post_mode = p.last ? tpost.mode : 0, p.post_lo_bits = tpost.lo_bits;
  }

  if (host && !hip_ok(hipMemcpyAsync(d_data, data, words * 4, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipMemsetAsync(ds.d_err, 0, 4, st))) return MSM_HIP_ERR_HIP;
  // all but the last two passes run in place; the last but one writes the scratch (same addresses), the last reads it and writes the data
  const size_t k = passes.size();
  for (size_t q = 0; q < k; q++) {
    const NttPass& p = passes[q];
    const uint32_t* src = (k > 1 && q == k - 1) ? ds.scratch.p : d_data;
    uint32_t* dst = (k > 1 && q == k - 2) ? ds.scratch.p : d_data;
    const unsigned blocks = (unsigned)(batch << (p.log_n - p.b - p.log_c));
    ops->launch(blocks, st, src, dst, &p, &t, ds.d_err);
    if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  }
  if (!hip_ok(hipMemcpyAsync(ds.h_err, ds.d_err, 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if (host && !hip_ok(hipMemcpyAsync(data, d_data, words * 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipStreamSynchronize(st))) return MSM_HIP_ERR_HIP;
  if (*ds.h_err) return MSM_HIP_ERR_NONCANONICAL;
  last_shape()[0] = (int)k;
  last_shape()[1] = (int)dig[0];
  return MSM_HIP_OK;
}

}  // namespace msm_fr

extern "C" {
int msm_fr_abi_version(void) { return 1; }

int msm_fr_ntt_device(int curve, int device, void* stream, void* data_dev, int log_n, size_t batch, const uint8_t omega[32], const uint8_t* pre_shift,
                      const uint8_t* post_shift, uint32_t flags) {
  return msm_fr::ntt_impl(curve, device, stream, data_dev, log_n, batch, omega, pre_shift, post_shift, flags, false);
}

int msm_fr_ntt(int curve, int device, uint8_t* data_host, int log_n, size_t batch, const uint8_t omega[32], const uint8_t* pre_shift, const uint8_t* post_shift,
               uint32_t flags) {
  return msm_fr::ntt_impl(curve, device, nullptr, data_host, log_n, batch, omega, pre_shift, post_shift, flags, true);
}

void msm_fr_release(void) {
  std::lock_guard<std::mutex> hold(msm_fr::lock());
  for (auto& kv : msm_fr::states()) {
    msm_fr::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    msm_fr::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    for (auto& t : ds.tables) {
      if (t.second.lo) (void)hipFree(t.second.lo);
      if (t.second.hi) (void)hipFree(t.second.hi);
    }
    for (auto& b : ds.butterflies) (void)hipFree(b.second);
    ds.tables.clear();
    ds.butterflies.clear();
    fr_host::drop(ds.scratch);
    fr_host::drop(ds.staging);
  }
}

int msm_fr_test_pass_bits(int b) {
  if (b < 0 || b > NTT_PASS_BITS) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_fr::lock());
  msm_fr::pass_bits_cap() = b;
  return MSM_HIP_OK;
}

int msm_fr_test_last(int* passes, int* pass_bits) {
  if (!passes || !pass_bits) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_fr::lock());
  *passes = msm_fr::last_shape()[0];
  *pass_bits = msm_fr::last_shape()[1];
  return MSM_HIP_OK;
}
}  // extern "C"
