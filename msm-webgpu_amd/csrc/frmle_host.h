// Host side of libmsm_frmle.so (include/msm_frmle.h): argument checks, the constants and levels of a call (csrc/frmle_plan.h), scratch and
// staging, and the launches of csrc/frmle_kernels.h through each field's FrmleOps.  Compiled once, by the unit that defines
// MSM_FRMLE_HOST_UNIT (csrc/frmle_bn254.hip).
//
// The result of a call -- the error word, then its values -- is one device buffer, copied once into one pinned buffer per device: a proof makes
// log2(n) dependent calls, so a second copy per call is a cost of every round (DESIGN.md sections 4.19, 4.20).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/msm_frmle.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "frmle_plan.h"
// (csrc/frmle_kernels.h -- the Frmle*Args, FrmleOps -- is already in: csrc/frmle_unit.h includes this file behind the unit's kernels)

extern "C" const FrmleOps* msm_frmle_ops_bn254(void);
extern "C" const FrmleOps* msm_frmle_ops_grumpkin(void);
extern "C" const FrmleOps* msm_frmle_ops_pallas(void);
extern "C" const FrmleOps* msm_frmle_ops_vesta(void);
extern "C" const FrmleOps* msm_frmle_ops_bls12_381(void);

static_assert(FRMLE_MAX_DEGREE == MSM_FRMLE_MAX_DEGREE && FRMLE_MAX_TERMS == MSM_FRMLE_MAX_TERMS && FRMLE_MAX_ROWS == MSM_FRMLE_MAX_ROWS,
              "csrc/frmle_kernels.h and include/msm_frmle.h disagree on the limits of a round");
static_assert(FRMLE_MAX_DEGREE == 4, "msm_frmle_term holds four rows");

namespace msm_frmle {

using namespace fr_host;

constexpr size_t MAX_ELEMENTS = (size_t)1 << 26;
constexpr uint32_t KNOWN_FLAGS = MSM_FRMLE_MONT256 | MSM_FRMLE_LOW_FIRST;

struct DeviceState {
  hipStream_t stream = nullptr;
  Buffer result;    // word 0: the error word; from word FRMLE_RESULT_HEAD: the values of the call
  Buffer h_result;  // pinned: what the one copy of a call fills
  Buffer scratch;   // the tile values, level by level; behind them the scratch rows of a low-first in-place bind
  Buffer consts;    // the tables of eq, the terms of a round
  Buffer staging;   // the host forms' table
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

inline const FrmleOps* field_of(int curve) {
  return fr_host::field_of<FrmleOps>(curve, msm_frmle_ops_bn254, msm_frmle_ops_grumpkin, msm_frmle_ops_pallas, msm_frmle_ops_vesta, msm_frmle_ops_bls12_381);
}

// an output is its input exactly (the same first byte), or apart from it
inline bool overlap_ok(const void* out, const void* in, size_t bytes) {
  if (in == out) return true;
  const uintptr_t o = reinterpret_cast<uintptr_t>(out), i = reinterpret_cast<uintptr_t>(in);
  return o + bytes <= i || i + bytes <= o;
}

struct Call {
  DeviceState* ds = nullptr;
  hipStream_t st = nullptr;
  uint32_t* err = nullptr;     // the error word on the device
  uint32_t* values = nullptr;  // where the last launch puts the values
};
// (the caller holds the guard and the lock)  `values`: how many the call reports
inline int enter(int device, void* stream, bool host, size_t values, Call* c) {
  DeviceState& ds = states()[device];
  if (!ds.stream && hipStreamCreateWithFlags(&ds.stream, hipStreamNonBlocking) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;
  const size_t words = FRMLE_RESULT_HEAD + 8 * (values < FRMLE_POINTS ? (size_t)FRMLE_POINTS : values);
  int rc = grow(ds.result, words);
  if (!rc) rc = grow(ds.h_result, words, true);
  if (rc) return rc;
  c->ds = &ds;
  c->st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  c->err = ds.result.p;
  c->values = ds.result.p + FRMLE_RESULT_HEAD;
  if (!hip_ok(hipMemsetAsync(c->err, 0, 4, c->st))) return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}
// ds.h_consts into the constants buffer, on the stream
inline int upload_consts(Call& c) {
  int rc = grow(c.ds->consts, c.ds->h_consts.size());
  if (rc) return rc;
  if (!hip_ok(hipMemcpyAsync(c.ds->consts.p, c.ds->h_consts.data(), c.ds->h_consts.size() * 4, hipMemcpyHostToDevice, c.st))) return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}
// host form: the rows of a -- (batch - 1) stride + n elements -- into the staging buffer
inline size_t span(size_t n, size_t batch, size_t stride) { return (batch - 1) * stride + n; }
inline int stage_in(Call& c, const void* src, size_t elements, uint32_t** dev) {
  int rc = grow(c.ds->staging, elements * 8);
  if (rc) return rc;
  if (src && !hip_ok(hipMemcpyAsync(c.ds->staging.p, src, elements * 32, hipMemcpyHostToDevice, c.st))) return MSM_HIP_ERR_HIP;
  *dev = c.ds->staging.p;
  return MSM_HIP_OK;
}
// host form: the first `width` elements of every row back
inline int stage_out(Call& c, void* dst, size_t width, size_t batch, size_t stride) {
  if (!hip_ok(hipMemcpy2DAsync(dst, stride * 32, c.ds->staging.p, stride * 32, width * 32, batch, hipMemcpyDeviceToHost, c.st))) return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}
// the end of every call: ONE copy of the error word and the values, the wait
inline int leave(Call& c, uint8_t* values_host, size_t values, int launches, int levels) {
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  const size_t words = values ? FRMLE_RESULT_HEAD + 8 * values : 1;
  if (!hip_ok(hipMemcpyAsync(c.ds->h_result.p, c.ds->result.p, words * 4, hipMemcpyDeviceToHost, c.st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipStreamSynchronize(c.st))) return MSM_HIP_ERR_HIP;
  if (c.ds->h_result.p[0]) return MSM_HIP_ERR_NONCANONICAL;
  if (values) memcpy(values_host, c.ds->h_result.p + FRMLE_RESULT_HEAD, values * 32);
  last_shape()[0] = launches, last_shape()[1] = levels;
  return MSM_HIP_OK;
}
inline uint32_t tile_in_use() { return tile_hook() ? tile_hook() : (uint32_t)FRMLE_TILE; }

// what every call with rows checks: the field, the device number, the flags, n = 2^k >= min_n, the rows within 2^26 elements
inline int shape_checks(const FrmleOps* ops, int device, size_t n, size_t min_n, size_t batch, size_t stride, uint32_t flags) {
  if (!ops || device < 0) return MSM_HIP_ERR_INVALID_ARG;
  if (flags & ~KNOWN_FLAGS) return MSM_HIP_ERR_INVALID_ARG;
  if (!power_of_two(n) || n < min_n || n > MAX_ELEMENTS) return MSM_HIP_ERR_INVALID_ARG;
  if (batch == 0 || stride < n || stride > MAX_ELEMENTS || batch > MAX_ELEMENTS / stride) return MSM_HIP_ERR_INVALID_ARG;
  return MSM_HIP_OK;
}

// the levels of a call in the scratch buffer: `rows` rows per level, level 1, 2, ..
struct Levels {
  std::vector<size_t> len, at;
  size_t words = 0;
  Levels(size_t n, size_t rows, uint32_t tile) : Levels(plan_levels(n, tile), rows) {}
  Levels(std::vector<size_t> lens, size_t rows) : len(std::move(lens)), at(len.size(), 0) {
    for (size_t l = 1; l < len.size(); l++) {
      at[l] = words;
      words += rows * len[l] * 8;
    }
  }
  size_t count() const { return len.size(); }
  uint32_t tiles(size_t l, uint32_t tile) const { return (uint32_t)((len[l] + tile - 1) / tile); }  // (= len[l + 1], or 1 at the top)
};

inline int fold_impl(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, size_t stride, const uint8_t* c, uint32_t flags, bool host) {
  const FrmleOps* ops = field_of(curve);
  int rc = shape_checks(ops, device, n, 2, batch, stride, flags);
  if (rc) return rc;
  if (!out || !a || !c) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(out) || misaligned(a))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  if (!host && !overlap_ok(out, a, span(n, batch, stride) * 32)) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if (!below_r(f, c)) return MSM_HIP_ERR_INVALID_ARG;
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  const FrmleFoldArgs g = plan_fold(f, c);
  Call call;
  if ((rc = enter(device, stream, host, 0, &call))) return rc;
  const uint32_t* da = static_cast<const uint32_t*>(a);
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host) {
    if ((rc = stage_in(call, a, span(n, batch, stride), &dout))) return rc;  // in place on the staged rows
    da = dout;
  }
  const size_t half = n / 2;
  int launches = 1;
  if (!(flags & MSM_FRMLE_LOW_FIRST)) {
    ops->fold((unsigned)((batch * half + FRMLE_THREADS - 1) / FRMLE_THREADS), call.st, dout, da, half, batch, stride, &g, call.err);
  } else if (dout != da) {  // apart: no slot is both read and written
    const FrmleFoldArgs low = plan_fold_low(f, c, LowLaunch{0, (uint32_t)half, false}, stride);
    ops->fold((unsigned)((batch * half + FRMLE_THREADS - 1) / FRMLE_THREADS), call.st, dout, da, half, batch, stride, &low, call.err);
  } else {
    const LowSchedule s = plan_low_in_place(n);
    if ((rc = grow(call.ds->scratch, batch * s.copy * 8))) return rc;
    launches = (int)s.launches.size();
    for (const LowLaunch& l : s.launches) {
      const FrmleFoldArgs low = plan_fold_low(f, c, l, l.to_scratch ? s.copy : stride);
      ops->fold((unsigned)((batch * l.count + FRMLE_THREADS - 1) / FRMLE_THREADS), call.st, l.to_scratch ? call.ds->scratch.p : dout, da, l.count, batch, stride, &low,
                call.err);
    }
    if (s.copy && !hip_ok(hipMemcpy2DAsync(dout, stride * 32, call.ds->scratch.p, s.copy * 32, s.copy * 32, batch, hipMemcpyDeviceToDevice, call.st))) return MSM_HIP_ERR_HIP;
  }
  if (host && (rc = stage_out(call, out, half, batch, stride))) return rc;
  return leave(call, nullptr, 0, launches, 1);
}

inline int eval_impl(int curve, int device, void* stream, const void* a, size_t n, size_t batch, size_t stride, const uint8_t* point, uint32_t flags, uint8_t* values_host,
                     bool host) {
  const FrmleOps* ops = field_of(curve);
  int rc = shape_checks(ops, device, n, 1, batch, stride, flags);
  if (rc) return rc;
  if (!a || !values_host || (n > 1 && !point) || (!host && misaligned(a))) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  const int k = log2_of(n);
  for (int j = 0; j < k; j++)
    if (!below_r(f, point + 32 * j)) return MSM_HIP_ERR_INVALID_ARG;
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  const uint32_t tile = tile_in_use();
  const Levels lv(n, batch, tile);
  const size_t levels = lv.count();
  const std::vector<uint8_t> reversed = flags & MSM_FRMLE_LOW_FIRST ? reversed_point(point, k) : std::vector<uint8_t>();
  if (flags & MSM_FRMLE_LOW_FIRST) point = reversed.data();                                       // (the kernel does not know the order)
  const std::vector<FrmleEvalArgs> g = plan_eval(f, tile, k, point);  // (as many levels: ceil(k / log2(tile)), 1 for k = 0)
  if (g.size() != levels) return MSM_HIP_ERR_INVALID_ARG;
  Call call;
  if ((rc = enter(device, stream, host, batch, &call))) return rc;
  if ((rc = grow(call.ds->scratch, lv.words))) return rc;
  uint32_t* const scratch = call.ds->scratch.p;
  const uint32_t* da = static_cast<const uint32_t*>(a);
  if (host) {
    uint32_t* staged = nullptr;
    if ((rc = stage_in(call, a, span(n, batch, stride), &staged))) return rc;
    da = staged;
  }
  for (size_t l = 0; l < levels; l++)
    ops->eval((unsigned)(batch * lv.tiles(l, tile)), call.st, l ? scratch + lv.at[l] : da, l + 1 < levels ? scratch + lv.at[l + 1] : call.values, l ? lv.len[l] : stride,
              lv.tiles(l, tile), &g[l], call.err);
  return leave(call, values_host, batch, (int)levels, (int)levels);
}

inline int eq_impl(int curve, int device, void* stream, void* out, size_t n, const uint8_t* point, const uint8_t* c, uint32_t flags, bool host) {
  const FrmleOps* ops = field_of(curve);
  int rc = shape_checks(ops, device, n, 1, 1, n, flags);
  if (rc) return rc;
  if (!out || !c || (n > 1 && !point) || (!host && misaligned(out))) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if (!below_r(f, c)) return MSM_HIP_ERR_INVALID_ARG;
  for (int j = 0; j < log2_of(n); j++)
    if (!below_r(f, point + 32 * j)) return MSM_HIP_ERR_INVALID_ARG;
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  Call call;
  if ((rc = enter(device, stream, host, 0, &call))) return rc;
  const std::vector<uint8_t> reversed = flags & MSM_FRMLE_LOW_FIRST ? reversed_point(point, log2_of(n)) : std::vector<uint8_t>();
  if (flags & MSM_FRMLE_LOW_FIRST) point = reversed.data();
  const FrmleEqArgs p = plan_eq(f, n, point, c, (flags & MSM_FRMLE_MONT256) != 0, call.ds->h_consts);
  if ((rc = upload_consts(call))) return rc;
  uint32_t* dout = static_cast<uint32_t*>(out);
  if (host && (rc = stage_in(call, nullptr, n, &dout))) return rc;
  const size_t lanes = (n + FRMLE_E - 1) / FRMLE_E;
  ops->eq((unsigned)((lanes + FRMLE_THREADS - 1) / FRMLE_THREADS), call.st, dout, n, call.ds->consts.p, &p);
  if (host && (rc = stage_out(call, out, n, 1, n))) return rc;
  return leave(call, nullptr, 0, 1, 1);
}

inline int round_impl(int curve, int device, void* stream, void* a, size_t n, size_t batch, size_t stride, const msm_frmle_term* terms, size_t num_terms,
                      const uint8_t* fold_by, uint32_t flags, uint8_t* values_host, bool host) {
  const FrmleOps* ops = field_of(curve);
  int rc = shape_checks(ops, device, n, fold_by ? 4 : 2, batch, stride, flags);
  if (rc) return rc;
  if (!a || !terms || !values_host || (!host && misaligned(a))) return MSM_HIP_ERR_INVALID_ARG;
  if (batch > MSM_FRMLE_MAX_ROWS || num_terms < 1 || num_terms > MSM_FRMLE_MAX_TERMS) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  if (fold_by && !below_r(f, fold_by)) return MSM_HIP_ERR_INVALID_ARG;
  Term plain[MSM_FRMLE_MAX_TERMS];
  for (size_t k = 0; k < num_terms; k++) {
    if (terms[k].degree < 1 || terms[k].degree > MSM_FRMLE_MAX_DEGREE || !below_r(f, terms[k].coeff)) return MSM_HIP_ERR_INVALID_ARG;
    for (uint32_t j = 0; j < terms[k].degree; j++)
      if (terms[k].rows[j] >= batch) return MSM_HIP_ERR_INVALID_ARG;
    plain[k] = Term{terms[k].coeff, terms[k].degree, terms[k].rows};
  }
  if ((rc = have_device(device))) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  const uint32_t tile = tile_in_use();
  const size_t half = fold_by ? n / 4 : n / 2;  // the pairs of the tables the round is of
  Call call;
  if ((rc = enter(device, stream, host, FRMLE_POINTS, &call))) return rc;
  FrmleRoundArgs g = plan_round(f, tile, plain, num_terms, batch, fold_by, (flags & MSM_FRMLE_MONT256) != 0, call.ds->h_consts);
  const bool low = (flags & MSM_FRMLE_LOW_FIRST) != 0;
  // low first with fold_by: the schedule of csrc/frmle_plan.h -- two launches over their own tiles and a copy; otherwise one launch over all pairs
  LowSchedule s;
  if (low && fold_by) s = plan_low_fused(n);
  else s.launches.push_back(LowLaunch{0, (uint32_t)half, false});
  const uint32_t launch_tile = low && fold_by ? low_fused_tile(tile) : tile;  // (the sums above always run over `tile`)
  const Levels lv = low && fold_by ? Levels(plan_levels_low_fused(s, half, launch_tile, tile), g.points) : Levels(half, g.points, tile);
  const size_t levels = lv.count();
  plan_round_launches(g, low, s, launch_tile, lv.words - (levels > 1 ? lv.at[1] : 0), call.ds->h_consts);  // (scratch rows: only where levels > 1)
  if ((rc = upload_consts(call))) return rc;
  if ((rc = grow(call.ds->scratch, lv.words + batch * s.copy * 8))) return rc;
  uint32_t* const scratch = call.ds->scratch.p;
  uint32_t* const rows = scratch + lv.words;  // the scratch rows of the schedule, s.copy elements apart
  uint32_t* da = static_cast<uint32_t*>(a);
  if (host && (rc = stage_in(call, a, span(n, batch, stride), &da))) return rc;
  uint32_t* const partial = levels > 1 ? scratch + lv.at[1] : call.values;
  uint32_t tile0 = 0;
  for (size_t k = 0; k < s.launches.size(); k++) {
    const uint32_t* const consts = call.ds->consts.p + low_block_words(num_terms) * k;
    ops->round(low_tiles(s.launches[k], launch_tile), call.st, da, (uint32_t)half, (uint32_t)stride, consts, partial + 8 * (size_t)tile0, &g, call.err);
    tile0 += low_tiles(s.launches[k], launch_tile);
  }
  if (s.copy && !hip_ok(hipMemcpy2DAsync(da, stride * 32, rows, s.copy * 32, s.copy * 32, batch, hipMemcpyDeviceToDevice, call.st))) return MSM_HIP_ERR_HIP;
  for (size_t l = 1; l < levels; l++)
    ops->sum((unsigned)(g.points * lv.tiles(l, tile)), call.st, scratch + lv.at[l], l + 1 < levels ? scratch + lv.at[l + 1] : call.values, lv.len[l], lv.tiles(l, tile), tile);
  if (host && fold_by && (rc = stage_out(call, a, n / 2, batch, stride))) return rc;
  return leave(call, values_host, g.points, (int)(levels - 1 + s.launches.size()), (int)levels);
}

}  // namespace msm_frmle

extern "C" {
int msm_frmle_abi_version(void) { return 1; }

int msm_frmle_fold_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, size_t stride, const uint8_t* c, uint32_t flags) {
  return msm_frmle::fold_impl(curve, device, stream, out, a, n, batch, stride, c, flags, false);
}
int msm_frmle_eval_device(int curve, int device, void* stream, const void* a, size_t n, size_t batch, size_t stride, const uint8_t* point, uint32_t flags,
                          uint8_t* values_host) {
  return msm_frmle::eval_impl(curve, device, stream, a, n, batch, stride, point, flags, values_host, false);
}
int msm_frmle_eq_device(int curve, int device, void* stream, void* out, size_t n, const uint8_t* point, const uint8_t* c, uint32_t flags) {
  return msm_frmle::eq_impl(curve, device, stream, out, n, point, c, flags, false);
}
int msm_frmle_round_device(int curve, int device, void* stream, void* a, size_t n, size_t batch, size_t stride, const msm_frmle_term* terms, size_t num_terms,
                           const uint8_t* fold_by, uint32_t flags, uint8_t* values_host) {
  return msm_frmle::round_impl(curve, device, stream, a, n, batch, stride, terms, num_terms, fold_by, flags, values_host, false);
}
int msm_frmle_fold(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, size_t stride, const uint8_t* c, uint32_t flags) {
  return msm_frmle::fold_impl(curve, device, nullptr, out, a, n, batch, stride, c, flags, true);
}
int msm_frmle_eval(int curve, int device, const uint8_t* a, size_t n, size_t batch, size_t stride, const uint8_t* point, uint32_t flags, uint8_t* values_host) {
  return msm_frmle::eval_impl(curve, device, nullptr, a, n, batch, stride, point, flags, values_host, true);
}
int msm_frmle_eq(int curve, int device, uint8_t* out, size_t n, const uint8_t* point, const uint8_t* c, uint32_t flags) {
  return msm_frmle::eq_impl(curve, device, nullptr, out, n, point, c, flags, true);
}
int msm_frmle_round(int curve, int device, uint8_t* a, size_t n, size_t batch, size_t stride, const msm_frmle_term* terms, size_t num_terms, const uint8_t* fold_by,
                    uint32_t flags, uint8_t* values_host) {
  return msm_frmle::round_impl(curve, device, nullptr, a, n, batch, stride, terms, num_terms, fold_by, flags, values_host, true);
}

void msm_frmle_release(void) {
  std::lock_guard<std::mutex> hold(msm_frmle::lock());
  for (auto& kv : msm_frmle::states()) {
    msm_frmle::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    msm_frmle::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    for (fr_host::Buffer* b : {&ds.scratch, &ds.consts, &ds.staging}) fr_host::drop(*b);
  }
}

int msm_frmle_test_tile(int elements) {
  if (elements != 0 && (elements < 2 || elements > FRMLE_TILE || (elements & (elements - 1)))) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_frmle::lock());
  msm_frmle::tile_hook() = (uint32_t)elements;
  return MSM_HIP_OK;
}

int msm_frmle_test_last(int* launches, int* levels) {
  if (!launches || !levels) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(msm_frmle::lock());
  *launches = msm_frmle::last_shape()[0];
  *levels = msm_frmle::last_shape()[1];
  return MSM_HIP_OK;
}
}  // extern "C"
