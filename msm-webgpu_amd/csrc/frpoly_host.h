// Host side of libmsm_frpoly.so (include/msm_frpoly.h): argument checks, the constants and levels of a call (csrc/frpoly_plan.h), scratch and
// staging, and the launches of csrc/frpoly_kernels.h through each field's FrpolyOps.  Compiled once, by the unit that defines
// MSM_FRPOLY_HOST_UNIT (csrc/frpoly_bn254.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/msm_frpoly.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "frpoly_plan.h"
// (csrc/frpoly_kernels.h -- the Frpoly*Args, FrpolyOps -- is already in: csrc/frpoly_unit.h includes this file behind the unit's kernels)

extern "C" const FrpolyOps* msm_frpoly_ops_bn254(void);
extern "C" const FrpolyOps* msm_frpoly_ops_pallas(void);
extern "C" const FrpolyOps* msm_frpoly_ops_vesta(void);
extern "C" const FrpolyOps* msm_frpoly_ops_bls12_381(void);

static_assert(FRPOLY_MAX_ROWS == MSM_FRPOLY_MAX_ROWS, "csrc/frpoly_kernels.h and include/msm_frpoly.h disagree on the rows of a combination");

namespace msm_frpoly {

using namespace fr_host;

constexpr size_t MAX_ELEMENTS = (size_t)1 << 26;
constexpr uint32_t KNOWN_FLAGS = MSM_FRPOLY_MONT256;

struct DeviceState {
  hipStream_t stream = nullptr;
  uint32_t* d_err = nullptr;
  uint32_t* h_err = nullptr;  // pinned: the error word comes back without a staging copy
  Buffer scratch;             // the rows' values, then the tile totals, level by level
  Buffer consts;              // a combination's coefficients, the tables of the powers
  Buffer staging[2];          // the host forms' a (and out), b
  std::vector<uint32_t> h_consts;  // what is on its way into consts (it outlives the call that uploads it)
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

inline const FrpolyOps* field_of(int curve) {  // (Grumpkin: no constants for its scalar field, so no unit)
  return fr_host::field_of<FrpolyOps>(curve, msm_frpoly_ops_bn254, nullptr, msm_frpoly_ops_pallas, msm_frpoly_ops_vesta, msm_frpoly_ops_bls12_381);
}

// an output is its input exactly (the same first byte), or apart from it
inline bool overlap_ok(const void* out, size_t out_bytes, const void* in, size_t in_bytes) {
  if (!in || in == out) return true;
  const uintptr_t o = reinterpret_cast<uintptr_t>(out), i = reinterpret_cast<uintptr_t>(in);
  return o + out_bytes <= i || i + in_bytes <= o;
}

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
// ds.h_consts into the constants buffer, on the stream
inline int upload_consts(Call& c) {
  int rc = grow(c.ds->consts, c.ds->h_consts.size());
  if (rc) return rc;
  if (!hip_ok(hipMemcpyAsync(c.ds->consts.p, c.ds->h_consts.data(), c.ds->h_consts.size() * 4, hipMemcpyHostToDevice, c.st))) return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}
// the end of every call: the error word, the rows' values, the host form's result, the wait
inline int leave(Call& c, uint8_t* values_host, const uint32_t* values_dev, size_t rows, void* out_host, const uint32_t* out_dev, size_t words, int launches, int levels) {
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipMemcpyAsync(c.ds->h_err, c.ds->d_err, 4, hipMemcpyDeviceToHost, c.st))) return MSM_HIP_ERR_HIP;
  if (values_host && !hip_ok(hipMemcpyAsync(values_host, values_dev, rows * 32, hipMemcpyDeviceToHost, c.st))) return MSM_HIP_ERR_HIP;
  if (out_host && !hip_ok(hipMemcpyAsync(out_host, out_dev, words * 4, hipMemcpyDeviceToHost, c.st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipStreamSynchronize(c.st))) return MSM_HIP_ERR_HIP;
  if (*c.ds->h_err) return MSM_HIP_ERR_NONCANONICAL;
  last_shape()[0] = launches, last_shape()[1] = levels;
  return MSM_HIP_OK;
}
inline uint32_t tile_in_use() { return tile_hook() ? tile_hook() : (uint32_t)FRPOLY_TILE; }

inline int shape_checks(const FrpolyOps* ops, int device, size_t n, size_t batch, uint32_t flags, uint32_t known_flags) {
  if (!ops || device < 0) return MSM_HIP_ERR_INVALID_ARG;
  if (flags & ~known_flags) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0 || batch == 0 || n > MAX_ELEMENTS || batch > MAX_ELEMENTS / n) return MSM_HIP_ERR_INVALID_ARG;
  return MSM_HIP_OK;
}

// the levels of a call in the scratch buffer: the rows' values first, then level 1, 2, ..
struct Levels {
  std::vector<size_t> len, at;
  size_t words = 0;
  Levels(size_t n, size_t batch, uint32_t tile) : len(plan_levels(n, tile)), at(len.size(), 0) {
    words = batch * 8;
    for (size_t l = 1; l < len.size(); l++) {
      at[l] = words;
      words += batch * len[l] * 8;
    }
  }
  size_t count() const { return len.size(); }
};

// eval (out == NULL, divide == false), divide, and dot (b != NULL): `values` receives every row's value
inline int fold_impl(int curve, int device, void* stream, void* out, const void* a, const void* b, size_t n, size_t batch, const uint8_t* z, uint32_t flags,
                     uint8_t* values_host, bool divide, bool dot, bool host) {
  const FrpolyOps* ops = field_of(curve);
  int rc = shape_checks(ops, device, n, batch, flags, KNOWN_FLAGS | (dot ? MSM_FRPOLY_SHARED_B : 0u));
  if (rc) return rc;
  if (!a || (divide && !out) || (dot && !b) || (!dot && !z) || (!divide && !values_host)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(a) || (divide && misaligned(out)) || (dot && misaligned(b)))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  if (divide && !overlap_ok(out, batch * n * 32, a, batch * n * 32)) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if (!dot && !below_r(f, z)) return MSM_HIP_ERR_INVALID_ARG;
  const bool shared_b = (flags & MSM_FRPOLY_SHARED_B) != 0;
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  const uint32_t tile = tile_in_use();
  const Levels lv(n, batch, tile);
  const size_t levels = lv.count();
  const std::vector<FrpolyLevelArgs> g = dot ? plan_dot(f, tile, levels, shared_b, (flags & MSM_FRPOLY_MONT256) != 0) : plan_horner(f, tile, levels, z);
  Call call;
  if ((rc = enter(device, stream, host, &call))) return rc;
  if ((rc = grow(call.ds->scratch, lv.words))) return rc;
  uint32_t* const scratch = call.ds->scratch.p;
  const size_t words = batch * n * 8;
  const uint32_t *da = static_cast<const uint32_t*>(a), *db = static_cast<const uint32_t*>(b);
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = stage_in(call, 0, a, words, &da))) return rc;
    if (dot && (rc = stage_in(call, 1, b, (shared_b ? n : batch * n) * 8, &db))) return rc;
    if (divide) dout = call.ds->staging[0].p;  // in place on a
  }
  auto level_in = [&](size_t l) { return l ? scratch + lv.at[l] : da; };
  auto tiles_of = [&](size_t l) { return (uint32_t)((lv.len[l] + tile - 1) / tile); };  // (= len[l + 1], or 1 at the top)
  if (!hip_ok(hipMemsetAsync(call.ds->d_err, 0, 4, call.st))) return MSM_HIP_ERR_HIP;
  int launches = 0;
  // the way up: every tile to one word of the level above; eval and dot go all the way, and the top tile's word is the row's value
  for (size_t l = 0; l + (divide ? 1 : 0) < levels; l++, launches++)
    ops->fold((unsigned)(batch * tiles_of(l)), call.st, level_in(l), l ? nullptr : db, l + 1 < levels ? scratch + lv.at[l + 1] : scratch, lv.len[l], tiles_of(l), &g[l],
              call.ds->d_err);
  if (divide) {
    // the way down: the top level has one tile per row and no carry-in, and h[0] there is the row's value; below it every tile from its carry-in
    for (size_t l = levels; l-- > 0; launches++)
      ops->suffix((unsigned)(batch * tiles_of(l)), call.st, level_in(l), l ? scratch + lv.at[l] : dout, l + 1 < levels ? scratch + lv.at[l + 1] : nullptr,
                  l + 1 < levels ? nullptr : scratch, lv.len[l], tiles_of(l), &g[l], call.ds->d_err);
  }
  return leave(call, values_host, scratch, batch, host && divide ? out : nullptr, dout, words, launches, (int)levels);
}

inline int combine_impl(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, const uint8_t* coeffs, uint32_t flags, bool host) {
  const FrpolyOps* ops = field_of(curve);
  int rc = shape_checks(ops, device, n, batch, flags, KNOWN_FLAGS);
  if (rc) return rc;
  if (!out || !a || !coeffs || batch > MSM_FRPOLY_MAX_ROWS) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(out) || misaligned(a))) return MSM_HIP_ERR_INVALID_ARG;
  if (!overlap_ok(out, n * 32, a, batch * n * 32)) return MSM_HIP_ERR_INVALID_ARG;  // (row 0 exactly, or apart from every row)
  const Field f(ops->r32);
  for (size_t k = 0; k < batch; k++)
    if (!below_r(f, coeffs + 32 * k)) return MSM_HIP_ERR_INVALID_ARG;
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  Call call;
  if ((rc = enter(device, stream, host, &call))) return rc;
  plan_combine(f, coeffs, batch, call.ds->h_consts);
  if ((rc = upload_consts(call))) return rc;
  const uint32_t* da = static_cast<const uint32_t*>(a);
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = stage_in(call, 0, a, batch * n * 8, &da))) return rc;
    dout = call.ds->staging[0].p;  // in place on row 0
  }
  if (!hip_ok(hipMemsetAsync(call.ds->d_err, 0, 4, call.st))) return MSM_HIP_ERR_HIP;
  ops->combine((unsigned)((n + FRPOLY_THREADS - 1) / FRPOLY_THREADS), call.st, da, call.ds->consts.p, dout, n, (uint32_t)batch, call.ds->d_err);
  return leave(call, nullptr, nullptr, 0, host ? out : nullptr, dout, n * 8, 1, 1);
}

inline int powers_impl(int curve, int device, void* stream, void* out, size_t n, const uint8_t* g, const uint8_t* c, uint32_t flags, bool host) {
  const FrpolyOps* ops = field_of(curve);
  int rc = shape_checks(ops, device, n, 1, flags, KNOWN_FLAGS);
  if (rc) return rc;
  if (!out || !g || !c || (!host && misaligned(out))) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if (!below_r(f, g) || !below_r(f, c)) return MSM_HIP_ERR_INVALID_ARG;
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  Call call;
  if ((rc = enter(device, stream, host, &call))) return rc;
  const FrpolyPowersArgs p = plan_powers(f, n, g, c, (flags & MSM_FRPOLY_MONT256) != 0, call.ds->h_consts);
  if ((rc = upload_consts(call))) return rc;
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = grow(call.ds->staging[0], n * 8))) return rc;
    dout = call.ds->staging[0].p;
  }
  if (!hip_ok(hipMemsetAsync(call.ds->d_err, 0, 4, call.st))) return MSM_HIP_ERR_HIP;
  const size_t lanes = (n + FRPOLY_E - 1) / FRPOLY_E;
  ops->powers((unsigned)((lanes + FRPOLY_THREADS - 1) / FRPOLY_THREADS), call.st, dout, n, call.ds->consts.p, &p);
  return leave(call, nullptr, nullptr, 0, host ? out : nullptr, dout, n * 8, 1, 1);
}

}  // namespace msm_frpoly

extern "C" {
int msm_frpoly_abi_version(void) { return 1; }

int msm_frpoly_eval_device(int curve, int device, void* stream, const void* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags, uint8_t* values_host) {
  return msm_frpoly::fold_impl(curve, device, stream, nullptr, a, nullptr, n, batch, z, flags, values_host, false, false, false);
}
int msm_frpoly_divide_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags, uint8_t* values_host) {
  return msm_frpoly::fold_impl(curve, device, stream, out, a, nullptr, n, batch, z, flags, values_host, true, false, false);
}
int msm_frpoly_dot_device(int curve, int device, void* stream, const void* a, const void* b, size_t n, size_t batch, uint32_t flags, uint8_t* values_host) {
  return msm_frpoly::fold_impl(curve, device, stream, nullptr, a, b, n, batch, nullptr, flags, values_host, false, true, false);
}
int msm_frpoly_combine_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, const uint8_t* coeffs_host, uint32_t flags) {
  return msm_frpoly::combine_impl(curve, device, stream, out, a, n, batch, coeffs_host, flags, false);
}
int msm_frpoly_powers_device(int curve, int device, void* stream, void* out, size_t n, const uint8_t* g, const uint8_t* c, uint32_t flags) {
  return msm_frpoly::powers_impl(curve, device, stream, out, n, g, c, flags, false);
}
int msm_frpoly_eval(int curve, int device, const uint8_t* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags, uint8_t* values_host) {
  return msm_frpoly::fold_impl(curve, device, nullptr, nullptr, a, nullptr, n, batch, z, flags, values_host, false, false, true);
}
int msm_frpoly_divide(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags, uint8_t* values_host) {
  return msm_frpoly::fold_impl(curve, device, nullptr, out, a, nullptr, n, batch, z, flags, values_host, true, false, true);
}
int msm_frpoly_dot(int curve, int device, const uint8_t* a, const uint8_t* b, size_t n, size_t batch, uint32_t flags, uint8_t* values_host) {
  return msm_frpoly::fold_impl(curve, device, nullptr, nullptr, a, b, n, batch, nullptr, flags, values_host, false, true, true);
}
int msm_frpoly_combine(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, const uint8_t* coeffs_host, uint32_t flags) {
  return msm_frpoly::combine_impl(curve, device, nullptr, out, a, n, batch, coeffs_host, flags, true);
}
int msm_frpoly_powers(int curve, int device, uint8_t* out, size_t n, const uint8_t* g, const uint8_t* c, uint32_t flags) {
  return msm_frpoly::powers_impl(curve, device, nullptr, out, n, g, c, flags, true);
}

void msm_frpoly_release(void) {
  std::lock_guard<std::mutex> hold(msm_frpoly::lock());
  for (auto& kv : msm_frpoly::states()) {
    msm_frpoly::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    msm_frpoly::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    for (fr_host::Buffer* b : {&ds.scratch, &ds.consts, &ds.staging[0], &ds.staging[1]}) fr_host::drop(*b);
  }
}

int msm_frpoly_test_tile(int elements) {
  if (elements != 0 && (elements < 2 || elements > FRPOLY_TILE)) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_frpoly::lock());
  msm_frpoly::tile_hook() = (uint32_t)elements;
  return MSM_HIP_OK;
}

int msm_frpoly_test_last(int* launches, int* levels) {
  if (!launches || !levels) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_frpoly::lock());
  *launches = msm_frpoly::last_shape()[0];
  *levels = msm_frpoly::last_shape()[1];
  return MSM_HIP_OK;
}
}  // extern "C"
