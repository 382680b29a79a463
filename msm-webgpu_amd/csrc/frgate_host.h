// Host side of libmsm_frgate.so (include/msm_frgate.h): argument checks and the term records of a call (csrc/frgate_plan.h), their way to the
// device, staging, and the one launch of csrc/frgate_kernels.h through each field's FrgateOps.  Compiled once, by the unit that defines
// MSM_FRGATE_HOST_UNIT (csrc/frgate_bn254.hip).
//
// The error word of a call comes back in one copy into one pinned buffer per device (DESIGN.md sections 4.19 - 4.22).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/msm_frgate.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "frgate_plan.h"
// (csrc/frgate_kernels.h -- FrgateArgs, FrgateOps -- is already in: csrc/frgate_unit.h includes this file behind the unit's kernels)

extern "C" const FrgateOps* msm_frgate_ops_bn254(void);
extern "C" const FrgateOps* msm_frgate_ops_grumpkin(void);
extern "C" const FrgateOps* msm_frgate_ops_pallas(void);
extern "C" const FrgateOps* msm_frgate_ops_vesta(void);
extern "C" const FrgateOps* msm_frgate_ops_bls12_381(void);

namespace msm_frgate {

using namespace fr_host;

struct DeviceState {
  hipStream_t stream = nullptr;
  Buffer result;    // word 0: the error word
  Buffer h_result;  // pinned: what the one copy of a call fills
  Buffer consts;    // the term records
  Buffer staging;   // the host form's a, scale and out
  std::vector<uint32_t> h_consts;  // what is on its way into consts (it outlives the call that uploads it)
};

inline std::mutex& lock() { return lock_of<DeviceState>(); }
inline std::map<int, DeviceState>& states() { return states_of<DeviceState>(); }

inline const FrgateOps* field_of(int curve) {
  return fr_host::field_of<FrgateOps>(curve, msm_frgate_ops_bn254, msm_frgate_ops_grumpkin, msm_frgate_ops_pallas, msm_frgate_ops_vesta, msm_frgate_ops_bls12_381);
}

inline int apply_impl(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, size_t stride, const msm_frgate_term* terms, size_t num_terms,
                      size_t step, const void* scale, size_t scale_len, uint32_t flags, bool host) {
  const FrgateOps* ops = field_of(curve);
  if (!ops || device < 0 || !out || !a) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if (!args_ok(f, n, batch, stride, terms, num_terms, step, scale != nullptr, scale_len, flags)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(out) || misaligned(a) || misaligned(scale))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  // a lane reads elements that other lanes write to: never in place.  The device form's rows are all of a[0 .. batch stride); the host form
  // reads (batch - 1) stride + n elements
  const size_t span = (batch - 1) * stride + n;
  if (!apart(out, n * 32, a, (host ? span : batch * stride) * 32)) return MSM_HIP_ERR_INVALID_ARG;
  if (scale && !apart(out, n * 32, scale, scale_len * 32)) return MSM_HIP_ERR_INVALID_ARG;
  int rc = have_device(device);
  if (rc) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  DeviceState& ds = states()[device];
  if (!ds.stream && hipStreamCreateWithFlags(&ds.stream, hipStreamNonBlocking) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;
  if ((rc = grow(ds.result, FRGATE_RESULT_HEAD))) return rc;
  if ((rc = grow(ds.h_result, FRGATE_RESULT_HEAD, true))) return rc;
  const hipStream_t st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  uint32_t* const err = ds.result.p;
  if (!hip_ok(hipMemsetAsync(err, 0, 4, st))) return MSM_HIP_ERR_HIP;
  const FrgateArgs g = plan_apply(f, n, stride, terms, num_terms, step, scale != nullptr, scale_len, flags, ds.h_consts);
  if ((rc = grow(ds.consts, ds.h_consts.size()))) return rc;
  if (!hip_ok(hipMemcpyAsync(ds.consts.p, ds.h_consts.data(), ds.h_consts.size() * 4, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
  const uint32_t* da = static_cast<const uint32_t*>(a);
  const uint32_t* dscale = static_cast<const uint32_t*>(scale);
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {  // staging: a, then scale, then out
    const size_t scale_words = scale ? scale_len * 8 : 0;
    if ((rc = grow(ds.staging, (span + n) * 8 + scale_words))) return rc;
    uint32_t* const sa = ds.staging.p;
    uint32_t* const ss = sa + span * 8;
    dout = ss + scale_words;
    if (!hip_ok(hipMemcpyAsync(sa, a, span * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
    if (scale && !hip_ok(hipMemcpyAsync(ss, scale, scale_len * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
    if (g.accumulate && !hip_ok(hipMemcpyAsync(dout, out, n * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
    da = sa;
    dscale = scale ? ss : nullptr;
  }
  ops->apply((unsigned)((n + FRGATE_THREADS - 1) / FRGATE_THREADS), st, dout, da, ds.consts.p, dscale, &g, err);
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  if (host && !hip_ok(hipMemcpyAsync(out, dout, n * 32, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipMemcpyAsync(ds.h_result.p, err, 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipStreamSynchronize(st))) return MSM_HIP_ERR_HIP;
  if (ds.h_result.p[0]) return MSM_HIP_ERR_NONCANONICAL;
  return MSM_HIP_OK;
}

}  // namespace msm_frgate

extern "C" {
int msm_frgate_abi_version(void) { return 1; }

int msm_frgate_apply_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, size_t stride, const msm_frgate_term* terms,
                            size_t num_terms, size_t step, const void* scale, size_t scale_len, uint32_t flags) {
  return msm_frgate::apply_impl(curve, device, stream, out, a, n, batch, stride, terms, num_terms, step, scale, scale_len, flags, false);
}
int msm_frgate_apply(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, size_t stride, const msm_frgate_term* terms, size_t num_terms,
                     size_t step, const uint8_t* scale, size_t scale_len, uint32_t flags) {
  return msm_frgate::apply_impl(curve, device, nullptr, out, a, n, batch, stride, terms, num_terms, step, scale, scale_len, flags, true);
}

void msm_frgate_release(void) {
  std::lock_guard<std::mutex> hold(msm_frgate::lock());
  for (auto& kv : msm_frgate::states()) {
    msm_frgate::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    msm_frgate::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    for (fr_host::Buffer* b : {&ds.consts, &ds.staging}) fr_host::drop(*b);
  }
}
}  // extern "C"
