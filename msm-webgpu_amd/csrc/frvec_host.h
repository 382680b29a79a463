// Host side of libmsm_frvec.so (include/msm_frvec.h): argument checks, the constants and levels of a call (csrc/frvec_plan.h), scratch and staging,
// and the launches of csrc/frvec_kernels.h through each field's FrvecOps.  Compiled once, by the unit that defines MSM_FRVEC_HOST_UNIT
// (csrc/frvec_bn254.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/msm_frvec.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "frvec_plan.h"
// (csrc/frvec_kernels.h -- the Frvec*Args, FrvecOps -- is already in: csrc/frvec_unit.h includes this file behind the unit's kernels)

extern "C" const FrvecOps* msm_frvec_ops_bn254(void);
extern "C" const FrvecOps* msm_frvec_ops_pallas(void);
extern "C" const FrvecOps* msm_frvec_ops_vesta(void);
extern "C" const FrvecOps* msm_frvec_ops_bls12_381(void);

// the kernels number the ops themselves (csrc/frvec_kernels.h does not read the public header: the host program of the tests includes it alone)
static_assert(FRVEC_ADD == MSM_FRVEC_ADD && FRVEC_SUB == MSM_FRVEC_SUB && FRVEC_MUL == MSM_FRVEC_MUL && FRVEC_MUL_ADD == MSM_FRVEC_MUL_ADD &&
                  FRVEC_MUL_SUB == MSM_FRVEC_MUL_SUB && FRVEC_SUM == MSM_FRVEC_SUM && FRVEC_PRODUCT == MSM_FRVEC_PRODUCT,
              "csrc/frvec_kernels.h and include/msm_frvec.h disagree on an op's number");

namespace msm_frvec {

using namespace fr_host;

constexpr size_t MAX_ELEMENTS = (size_t)1 << 26;

struct DeviceState {
  hipStream_t stream = nullptr;
  uint32_t* d_err = nullptr;
  uint32_t* h_err = nullptr;  // pinned: the error word comes back without a staging copy
  Buffer scratch;             // a scan's tile totals, level by level, and its row totals; an inverse's tile products
  Buffer staging[3];          // the host forms' a (and out), b, c
};

inline std::mutex& lock() { return lock_of<DeviceState>(); }
inline std::map<int, DeviceState>& states() { return states_of<DeviceState>(); }
inline uint32_t& tile_hook() {
  static uint32_t t = 0;
  return t;
}
inline int (&last_shape())[2] {
  static int s[2] = {0, 0};
  return s;
}

inline const FrvecOps* field_of(int curve) {  // (Grumpkin: no constants for its scalar field, so no unit)
  return fr_host::field_of<FrvecOps>(curve, msm_frvec_ops_bn254, nullptr, msm_frvec_ops_pallas, msm_frvec_ops_vesta, msm_frvec_ops_bls12_381);
}

// an output is one of its inputs exactly, or apart from it
inline bool overlap_ok(const void* out, const void* in, size_t bytes) {
  if (!in || in == out) return true;
  const uintptr_t o = reinterpret_cast<uintptr_t>(out), i = reinterpret_cast<uintptr_t>(in);
  return o + bytes <= i || i + bytes <= o;
}

// what every call shares once its own arguments are checked: the device, the state, the stream, the error word
struct Call {
  DeviceState* ds = nullptr;
  hipStream_t st = nullptr;
};
inline int enter(int device, void* stream, bool host, Call* c) {  // (the caller holds the guard and the lock)
  DeviceState& ds = states()[device];
  if (!ds.stream && hipStreamCreateWithFlags(&ds.stream, hipStreamNonBlocking) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;
  if (!ds.d_err && hipMalloc(reinterpret_cast<void**>(&ds.d_err), 4) != hipSuccess) return MSM_HIP_ERR_OUT_OF_MEMORY;
  if (!ds.h_err && hipHostMalloc(reinterpret_cast<void**>(&ds.h_err), 4, hipHostMallocDefault) != hipSuccess) return MSM_HIP_ERR_OUT_OF_MEMORY;
  c->ds = &ds;
  c->st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  return MSM_HIP_OK;
}
// host form: vector `src` of `words` words into staging buffer k
inline int stage_in(Call& c, int k, const void* src, size_t words, const uint32_t** dev) {
  int rc = grow(c.ds->staging[k], words);
  if (rc) return rc;
  if (!hip_ok(hipMemcpyAsync(c.ds->staging[k].p, src, words * 4, hipMemcpyHostToDevice, c.st))) return MSM_HIP_ERR_HIP;
  *dev = c.ds->staging[k].p;
  return MSM_HIP_OK;
}
// the end of every call: the error word, the host form's result, the wait
inline int leave(Call& c, void* out_host, const uint32_t* out_dev, size_t words, int launches, int levels) {
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipMemcpyAsync(c.ds->h_err, c.ds->d_err, 4, hipMemcpyDeviceToHost, c.st))) return MSM_HIP_ERR_HIP;
  if (out_host && !hip_ok(hipMemcpyAsync(out_host, out_dev, words * 4, hipMemcpyDeviceToHost, c.st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipStreamSynchronize(c.st))) return MSM_HIP_ERR_HIP;
  if (*c.ds->h_err) return MSM_HIP_ERR_NONCANONICAL;
  last_shape()[0] = launches, last_shape()[1] = levels;
  return MSM_HIP_OK;
}
inline uint32_t tile_in_use() { return tile_hook() ? tile_hook() : (uint32_t)FRVEC_TILE; }

inline int common_checks(const FrvecOps* ops, int device, const void* out, const void* a, size_t n, size_t batch, uint32_t flags, uint32_t known_flags, bool host) {
  if (!ops || device < 0 || !out || !a) return MSM_HIP_ERR_INVALID_ARG;
  if (flags & ~known_flags) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0 || batch == 0 || n > MAX_ELEMENTS || batch > MAX_ELEMENTS / n) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(out) || misaligned(a))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  if (!overlap_ok(out, a, batch * n * 32)) return MSM_HIP_ERR_INVALID_ARG;
  return MSM_HIP_OK;
}

inline int map_impl(int curve, int device, void* stream, void* out, const void* a, const void* b, const void* c, size_t n, int op, const uint8_t* b_const,
                    const uint8_t* c_const, uint32_t flags, bool host) {
  const FrvecOps* ops = field_of(curve);
  int rc = common_checks(ops, device, out, a, n, 1, flags, MSM_FRVEC_MONT256, host);
  if (rc) return rc;
  if (op < MSM_FRVEC_ADD || op > MSM_FRVEC_MUL_SUB) return MSM_HIP_ERR_INVALID_ARG;
  const bool three = op == MSM_FRVEC_MUL_ADD || op == MSM_FRVEC_MUL_SUB;
  if ((b != nullptr) == (b_const != nullptr)) return MSM_HIP_ERR_INVALID_ARG;  // an operand given twice, or missing
  if (three ? (c != nullptr) == (c_const != nullptr) : (c || c_const)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && ((b && misaligned(b)) || (c && misaligned(c)))) return MSM_HIP_ERR_INVALID_ARG;
  if (!overlap_ok(out, b, n * 32) || !overlap_ok(out, c, n * 32)) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if ((b_const && !below_r(f, b_const)) || (c_const && !below_r(f, c_const))) return MSM_HIP_ERR_INVALID_ARG;
  const FrvecMapArgs m = plan_map(f, op, b_const, c_const, (flags & MSM_FRVEC_MONT256) != 0);
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  Call call;
  if ((rc = enter(device, stream, host, &call))) return rc;
  const size_t words = n * 8;
  const uint32_t *da = static_cast<const uint32_t*>(a), *db = static_cast<const uint32_t*>(b), *dc = static_cast<const uint32_t*>(c);
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = stage_in(call, 0, a, words, &da))) return rc;
    if (b && (rc = stage_in(call, 1, b, words, &db))) return rc;
    if (c && (rc = stage_in(call, 2, c, words, &dc))) return rc;
    dout = call.ds->staging[0].p;  // in place on a
  }
  if (!hip_ok(hipMemsetAsync(call.ds->d_err, 0, 4, call.st))) return MSM_HIP_ERR_HIP;
  ops->map((unsigned)((n + FRVEC_THREADS - 1) / FRVEC_THREADS), call.st, da, db, dc, dout, n, &m, call.ds->d_err);
  return leave(call, host ? out : nullptr, dout, words, 1, 1);
}

inline int inverse_impl(int curve, int device, void* stream, void* out, const void* a, size_t n, uint32_t flags, bool host) {
  const FrvecOps* ops = field_of(curve);
  int rc = common_checks(ops, device, out, a, n, 1, flags, MSM_FRVEC_MONT256, host);
  if (rc) return rc;
  const Field f(ops->r32);
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  const FrvecInvArgs v = plan_inverse(f, tile_in_use(), (flags & MSM_FRVEC_MONT256) != 0);
  const std::vector<size_t> len = plan_levels(n, v.tile);  // len[l]: words at level l -- the data, then the tile products of the level below
  const size_t levels = len.size();
  Call call;
  if ((rc = enter(device, stream, host, &call))) return rc;
  std::vector<size_t> at(levels, 0);
  size_t scratch_words = 0;
  for (size_t l = 1; l < levels; l++) {
    at[l] = scratch_words;
    scratch_words += len[l] * 8;
  }
  if (scratch_words && (rc = grow(call.ds->scratch, scratch_words))) return rc;
  const size_t words = n * 8;
  const uint32_t* da = static_cast<const uint32_t*>(a);
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = stage_in(call, 0, a, words, &da))) return rc;
    dout = call.ds->staging[0].p;
  }
  auto level_in = [&](size_t l) { return l ? call.ds->scratch.p + at[l] : da; };
  auto level_out = [&](size_t l) { return l ? call.ds->scratch.p + at[l] : dout; };
  auto tiles_of = [&](size_t l) { return (unsigned)((len[l] + v.tile - 1) / v.tile); };
  if (!hip_ok(hipMemsetAsync(call.ds->d_err, 0, 4, call.st))) return MSM_HIP_ERR_HIP;
  int launches = 0;
  for (size_t l = 0; l + 1 < levels; l++, launches++)  // up: every tile's product
    ops->inverse(tiles_of(l), call.st, level_in(l), nullptr, len[l], &v, FRVEC_INV_TOTALS, call.ds->scratch.p + at[l + 1], call.ds->d_err);
  for (size_t l = levels; l-- > 0; launches++)  // the top level is one tile, inverted by Fermat; then down, every tile from its root
    ops->inverse(tiles_of(l), call.st, level_in(l), level_out(l), len[l], &v, l + 1 < levels ? FRVEC_INV_ROOTS : FRVEC_INV_WHOLE,
                 l + 1 < levels ? call.ds->scratch.p + at[l + 1] : nullptr, call.ds->d_err);
  return leave(call, host ? out : nullptr, dout, words, launches, (int)levels);
}

inline int scan_impl(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, int op, uint32_t flags, uint8_t* totals_host, bool host) {
  const FrvecOps* ops = field_of(curve);
  int rc = common_checks(ops, device, out, a, n, batch, flags, MSM_FRVEC_MONT256 | MSM_FRVEC_EXCLUSIVE, host);
  if (rc) return rc;
  if (op != MSM_FRVEC_SUM && op != MSM_FRVEC_PRODUCT) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  const FrvecScanArgs g = plan_scan(f, tile_in_use(), op, (flags & MSM_FRVEC_EXCLUSIVE) != 0, (flags & MSM_FRVEC_MONT256) != 0), gi = inner_level(g);
  const std::vector<size_t> len = plan_levels(n, g.tile);  // len[l]: values per row at level l
  const size_t levels = len.size();
  Call call;
  if ((rc = enter(device, stream, host, &call))) return rc;
  // the scratch: the row totals, then the totals of level 1, 2, ..
  std::vector<size_t> at(levels, 0);
  size_t scratch_words = batch * 8;
  for (size_t l = 1; l < levels; l++) {
    at[l] = scratch_words;
    scratch_words += batch * len[l] * 8;
  }
  if ((rc = grow(call.ds->scratch, scratch_words))) return rc;
  uint32_t* const row_totals = call.ds->scratch.p;
  const size_t words = batch * n * 8;
  const uint32_t* da = static_cast<const uint32_t*>(a);
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = stage_in(call, 0, a, words, &da))) return rc;
    dout = call.ds->staging[0].p;
  }
  auto level_in = [&](size_t l) { return l ? call.ds->scratch.p + at[l] : da; };
  auto level_out = [&](size_t l) { return l ? call.ds->scratch.p + at[l] : dout; };
  auto tiles_of = [&](size_t l) { return (uint32_t)((len[l] + g.tile - 1) / g.tile); };  // (= len[l + 1], or 1 at the top)
  if (!hip_ok(hipMemsetAsync(call.ds->d_err, 0, 4, call.st))) return MSM_HIP_ERR_HIP;
  int launches = 0;
  for (size_t l = 0; l + 1 < levels; l++, launches++)  // phase 1, level by level: every tile to one value
    ops->fold((unsigned)(batch * tiles_of(l)), call.st, level_in(l), call.ds->scratch.p + at[l + 1], len[l], tiles_of(l), l ? &gi : &g, call.ds->d_err);
  for (size_t l = levels; l-- > 0; launches++) {  // the top level has one tile per row and no carry-in; then down again, every tile from its carry-in
    const uint32_t* carry = l + 1 < levels ? call.ds->scratch.p + at[l + 1] : nullptr;
    ops->scan((unsigned)(batch * tiles_of(l)), call.st, level_in(l), level_out(l), carry, l ? nullptr : row_totals, len[l], tiles_of(l), l ? &gi : &g, call.ds->d_err);
  }
  if (totals_host && !hip_ok(hipMemcpyAsync(totals_host, row_totals, batch * 32, hipMemcpyDeviceToHost, call.st))) return MSM_HIP_ERR_HIP;
  return leave(call, host ? out : nullptr, dout, words, launches, (int)levels);
}

}  // namespace msm_frvec

extern "C" {
int msm_frvec_abi_version(void) { return 1; }

int msm_frvec_map_device(int curve, int device, void* stream, void* out, const void* a, const void* b, const void* c, size_t n, int op, const uint8_t* b_const,
                         const uint8_t* c_const, uint32_t flags) {
  return msm_frvec::map_impl(curve, device, stream, out, a, b, c, n, op, b_const, c_const, flags, false);
}
int msm_frvec_inverse_device(int curve, int device, void* stream, void* out, const void* a, size_t n, uint32_t flags) {
  return msm_frvec::inverse_impl(curve, device, stream, out, a, n, flags, false);
}
int msm_frvec_scan_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, int op, uint32_t flags, uint8_t* totals_host) {
  return msm_frvec::scan_impl(curve, device, stream, out, a, n, batch, op, flags, totals_host, false);
}
int msm_frvec_map(int curve, int device, uint8_t* out, const uint8_t* a, const uint8_t* b, const uint8_t* c, size_t n, int op, const uint8_t* b_const, const uint8_t* c_const,
                  uint32_t flags) {
  return msm_frvec::map_impl(curve, device, nullptr, out, a, b, c, n, op, b_const, c_const, flags, true);
}
int msm_frvec_inverse(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, uint32_t flags) {
  return msm_frvec::inverse_impl(curve, device, nullptr, out, a, n, flags, true);
}
int msm_frvec_scan(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, int op, uint32_t flags, uint8_t* totals_host) {
  return msm_frvec::scan_impl(curve, device, nullptr, out, a, n, batch, op, flags, totals_host, true);
}

void msm_frvec_release(void) {
  std::lock_guard<std::mutex> hold(msm_frvec::lock());
  for (auto& kv : msm_frvec::states()) {
    msm_frvec::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    msm_frvec::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    for (fr_host::Buffer* b : {&ds.scratch, &ds.staging[0], &ds.staging[1], &ds.staging[2]}) fr_host::drop(*b);
  }
}

int msm_frvec_test_tile(int elements) {
  if (elements != 0 && (elements < 2 || elements > FRVEC_TILE)) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_frvec::lock());
  msm_frvec::tile_hook() = (uint32_t)elements;
  return MSM_HIP_OK;
}

int msm_frvec_test_last(int* launches, int* levels) {
  if (!launches || !levels) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_frvec::lock());
  *launches = msm_frvec::last_shape()[0];
  *levels = msm_frvec::last_shape()[1];
  return MSM_HIP_OK;
}
}  // extern "C"
