// Host side of libmsm_frmat.so (include/msm_frmat.h): the handle, argument checks, the plan of a matrix (csrc/frmat_plan.h), its way to the
// device, staging, and the launches of csrc/frmat_kernels.h through each field's FrmatOps.  Compiled once, by the unit that defines
// MSM_FRMAT_HOST_UNIT (csrc/frmat_bn254.hip).
//
// A handle keeps what create planned in host memory until its first product on a side (M or M^T): then the arrays go to the device, the values
// are lifted to v R there (k_frmat_lift), and the host copy is dropped.  The error word of a product comes back in one copy into one pinned
// buffer per device (DESIGN.md sections 4.19 - 4.21).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/msm_frmat.h"
#include "../../include/msm_hip.h"
#include "fr_host_common.h"  // the guard, buffers, pointer checks and the state scheme every scalar-field library shares
#include "frmat_plan.h"
// (csrc/frmat_kernels.h -- FrmatLevelArgs, FrmatOps -- is already in: csrc/frmat_unit.h includes this file behind the unit's kernels)

extern "C" const FrmatOps* msm_frmat_ops_bn254(void);
extern "C" const FrmatOps* msm_frmat_ops_grumpkin(void);
extern "C" const FrmatOps* msm_frmat_ops_pallas(void);
extern "C" const FrmatOps* msm_frmat_ops_vesta(void);
extern "C" const FrmatOps* msm_frmat_ops_bls12_381(void);

namespace frmat {

struct DevLevel {
  uint32_t* row_of = nullptr;
  uint32_t* slots = nullptr;
  uint32_t* part = nullptr;  // this level's partials: the entries of the next
  FrmatLevelArgs g = {0, 0, 0};
  uint32_t tiles = 0;
};
// M or M^T: what create planned (host), then what the products read (device)
struct Side {
  size_t out_len = 0, in_len = 0, nnz = 0;
  bool planned = false, resident = false;
  std::vector<uint32_t> col;
  std::vector<uint8_t> values;
  std::vector<Level> plan;
  uint32_t* d_values = nullptr;
  uint32_t* d_col = nullptr;
  std::vector<DevLevel> levels;
};

}  // namespace frmat

struct msm_frmat {
  const FrmatOps* ops = nullptr;
  int device = 0;
  size_t rows = 0, cols = 0, nnz = 0;
  uint32_t flags = 0, tile = 0;
  mutable frmat::Side side[2];  // M, M^T
};

namespace frmat {

using namespace fr_host;

constexpr uint32_t CREATE_FLAGS = MSM_FRMAT_WITH_TRANSPOSE;
constexpr uint32_t MUL_FLAGS = MSM_FRMAT_MONT256 | MSM_FRMAT_TRANSPOSE;

struct DeviceState {
  hipStream_t stream = nullptr;
  Buffer result;    // word 0: the error word
  Buffer h_result;  // pinned: what the one copy of a call fills
  Buffer staging;   // the host form's x and y
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

inline const FrmatOps* field_of(int curve) {
  return fr_host::field_of<FrmatOps>(curve, msm_frmat_ops_bn254, msm_frmat_ops_grumpkin, msm_frmat_ops_pallas, msm_frmat_ops_vesta, msm_frmat_ops_bls12_381);
}

inline size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }

// `words` words of device memory holding the `have` words at src, zero behind them
inline int to_device(uint32_t** dst, const void* src, size_t have, size_t words) {
  if (!hip_ok(hipMalloc(reinterpret_cast<void**>(dst), words * 4))) {
    *dst = nullptr;
    return MSM_HIP_ERR_OUT_OF_MEMORY;
  }
  if (have < words && !hip_ok(hipMemset(*dst + have, 0, (words - have) * 4))) return MSM_HIP_ERR_HIP;
  if (have && !hip_ok(hipMemcpy(*dst, src, have * 4, hipMemcpyHostToDevice))) return MSM_HIP_ERR_HIP;
  return MSM_HIP_OK;
}
inline void free_side(Side& s) {
  if (s.d_values) (void)hipFree(s.d_values);
  if (s.d_col) (void)hipFree(s.d_col);
  for (DevLevel& l : s.levels) {
    if (l.row_of) (void)hipFree(l.row_of);
    if (l.slots) (void)hipFree(l.slots);
    if (l.part) (void)hipFree(l.part);
  }
  s.d_values = s.d_col = nullptr;
  s.levels.clear();
  s.resident = false;
}
// the side's arrays to the device, the values to v R (the caller holds the guard and the lock)
inline int make_resident(const msm_frmat* m, Side& s, hipStream_t st) {
  if (s.resident) return MSM_HIP_OK;
  int rc = MSM_HIP_OK;
  if (s.nnz) {
    rc = to_device(&s.d_values, s.values.data(), s.nnz * 8, s.nnz * 8);
    if (!rc) rc = to_device(&s.d_col, s.col.data(), s.nnz, up4(s.nnz));
  }
  s.levels.assign(s.plan.size(), DevLevel());
  for (size_t l = 0; l < s.plan.size() && !rc; l++) {
    const Level& lv = s.plan[l];
    DevLevel& d = s.levels[l];
    d.g = level_args(lv, m->tile);
    d.tiles = lv.tiles;
    rc = to_device(&d.row_of, lv.row_of.data(), lv.row_of.size(), up4(lv.row_of.size()));
    if (!rc) rc = to_device(&d.slots, lv.slots.data(), lv.slots.size(), lv.slots.size());
    if (!rc && !lv.next.empty() && !hip_ok(hipMalloc(reinterpret_cast<void**>(&d.part), lv.next.size() * 32))) rc = MSM_HIP_ERR_OUT_OF_MEMORY;
  }
  if (!rc && s.nnz) {
    m->ops->lift((unsigned)((s.nnz + FRMAT_THREADS - 1) / FRMAT_THREADS), st, s.d_values, s.nnz);
    if (!hip_ok(hipGetLastError()) || !hip_ok(hipStreamSynchronize(st))) rc = MSM_HIP_ERR_HIP;
  }
  if (rc) {
    free_side(s);
    return rc;
  }
  s.resident = true;
  std::vector<uint32_t>().swap(s.col);
  std::vector<uint8_t>().swap(s.values);
  std::vector<Level>().swap(s.plan);
  return MSM_HIP_OK;
}

inline void plan_side(Side& s, size_t out_len, size_t in_len, const uint32_t* ptr, const uint32_t* idx, const uint8_t* values, const uint32_t* from, uint32_t tile) {
  s.out_len = out_len, s.in_len = in_len, s.nnz = ptr[out_len], s.planned = true;
  s.col.assign(idx, idx + s.nnz);
  s.values.resize(s.nnz * 32);
  for (size_t e = 0; e < s.nnz; e++) memcpy(s.values.data() + 32 * e, values + 32 * (from ? from[e] : e), 32);
  s.plan = plan_levels(expand_rows(out_len, ptr), tile);
}

inline int create_impl(int curve, int device, size_t rows, size_t cols, size_t nnz, const uint32_t* row_ptr, const uint32_t* col_idx, const uint8_t* values, uint32_t flags,
                       msm_frmat** out) {
  const FrmatOps* ops = field_of(curve);
  if (!out) return MSM_HIP_ERR_INVALID_ARG;
  *out = nullptr;
  if (!ops || device < 0 || (flags & ~CREATE_FLAGS)) return MSM_HIP_ERR_INVALID_ARG;
  const Field f(ops->r32);
  const Check c = check_matrix(f, rows, cols, nnz, row_ptr, col_idx, values);
  if (c != CHECK_OK) return c == CHECK_NONCANONICAL ? MSM_HIP_ERR_NONCANONICAL : MSM_HIP_ERR_INVALID_ARG;
  msm_frmat* m = new msm_frmat();
  m->ops = ops, m->device = device, m->rows = rows, m->cols = cols, m->nnz = nnz, m->flags = flags;
  {
    std::lock_guard<std::mutex> hold(lock());
    m->tile = tile_hook() ? tile_hook() : (uint32_t)FRMAT_TILE;
  }
  plan_side(m->side[0], rows, cols, row_ptr, col_idx, values, nullptr, m->tile);
  if (flags & MSM_FRMAT_WITH_TRANSPOSE) {
    std::vector<uint32_t> t_ptr, t_idx, from;
    transpose_csr(rows, cols, row_ptr, col_idx, t_ptr, t_idx, from);
    plan_side(m->side[1], cols, rows, t_ptr.data(), t_idx.data(), values, from.data(), m->tile);
  }
  *out = m;
  return MSM_HIP_OK;
}

inline int mul_impl(const msm_frmat* m, void* stream, void* y, size_t y_len, const void* x, size_t x_len, uint32_t flags, bool host) {
  if (!m || !y || !x || (flags & ~MUL_FLAGS)) return MSM_HIP_ERR_INVALID_ARG;
  Side& s = m->side[(flags & MSM_FRMAT_TRANSPOSE) ? 1 : 0];
  if (!s.planned) return MSM_HIP_ERR_INVALID_ARG;  // TRANSPOSE on a handle created without WITH_TRANSPOSE
  if (x_len != s.in_len || y_len < s.out_len || y_len > MAX_DIM) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (misaligned(y) || misaligned(x))) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  if (!apart(y, y_len * 32, x, x_len * 32)) return MSM_HIP_ERR_INVALID_ARG;
  int rc = have_device(m->device);
  if (rc) return rc;
  DeviceGuard guard(m->device);
  if (!guard.ok) return MSM_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> hold(lock());
  DeviceState& ds = states()[m->device];
  if (!ds.stream && hipStreamCreateWithFlags(&ds.stream, hipStreamNonBlocking) != hipSuccess) return MSM_HIP_ERR_NO_DEVICE;
  if ((rc = grow(ds.result, FRMAT_RESULT_HEAD))) return rc;
  if ((rc = grow(ds.h_result, FRMAT_RESULT_HEAD, true))) return rc;
  const hipStream_t st = stream && !host ? static_cast<hipStream_t>(stream) : ds.stream;
  if ((rc = make_resident(m, s, st))) return rc;
  uint32_t* const err = ds.result.p;
  if (!hip_ok(hipMemsetAsync(err, 0, 4, st))) return MSM_HIP_ERR_HIP;
  const uint32_t* dx = static_cast<const uint32_t*>(x);
  uint32_t* dy = static_cast<uint32_t*>(y);
  if (host) {
    if ((rc = grow(ds.staging, (x_len + y_len) * 8))) return rc;
    if (!hip_ok(hipMemcpyAsync(ds.staging.p, x, x_len * 32, hipMemcpyHostToDevice, st))) return MSM_HIP_ERR_HIP;
    dx = ds.staging.p;
    dy = ds.staging.p + x_len * 8;
  }
  // rows without entries and the tail: y is cleared first; every other word of it has exactly one writer among the launches behind
  if (!hip_ok(hipMemsetAsync(dy, 0, y_len * 32, st))) return MSM_HIP_ERR_HIP;
  for (size_t l = 0; l < s.levels.size(); l++) {
    const DevLevel& d = s.levels[l];
    if (l == 0) {
      m->ops->tile(d.tiles, st, s.d_values, s.d_col, d.row_of, d.slots, dx, dy, d.part, &d.g, err);
    } else {
      m->ops->stitch(d.tiles, st, s.levels[l - 1].part, d.row_of, d.slots, dy, d.part, &d.g);
    }
  }
  if (!hip_ok(hipGetLastError())) return MSM_HIP_ERR_HIP;
  if (host && !hip_ok(hipMemcpyAsync(y, dy, y_len * 32, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipMemcpyAsync(ds.h_result.p, err, 4, hipMemcpyDeviceToHost, st))) return MSM_HIP_ERR_HIP;
  if (!hip_ok(hipStreamSynchronize(st))) return MSM_HIP_ERR_HIP;
  if (ds.h_result.p[0]) return MSM_HIP_ERR_NONCANONICAL;
  last_shape()[0] = 1 + (int)s.levels.size(), last_shape()[1] = (int)s.levels.size();
  return MSM_HIP_OK;
}

}  // namespace frmat

extern "C" {
int msm_frmat_abi_version(void) { return 1; }

int msm_frmat_create(int curve, int device, size_t rows, size_t cols, size_t nnz, const uint32_t* row_ptr, const uint32_t* col_idx, const uint8_t* values, uint32_t flags,
                     msm_frmat** out) {
  return frmat::create_impl(curve, device, rows, cols, nnz, row_ptr, col_idx, values, flags, out);
}

int msm_frmat_info(const msm_frmat* m, size_t* rows, size_t* cols, size_t* nnz, uint32_t* flags) {
  if (!m) return MSM_HIP_ERR_INVALID_ARG;
  if (rows) *rows = m->rows;
  if (cols) *cols = m->cols;
  if (nnz) *nnz = m->nnz;
  if (flags) *flags = m->flags;
  return MSM_HIP_OK;
}

void msm_frmat_destroy(msm_frmat* m) {
  if (!m) return;
  {
    std::lock_guard<std::mutex> hold(frmat::lock());
    if (m->side[0].resident || m->side[1].resident) {
      frmat::DeviceGuard guard(m->device);
      if (guard.ok) {
        frmat::free_side(m->side[0]);
        frmat::free_side(m->side[1]);
      }
    }
  }
  delete m;
}

int msm_frmat_mul_device(const msm_frmat* m, void* stream, void* y, size_t y_len, const void* x, size_t x_len, uint32_t flags) {
  return frmat::mul_impl(m, stream, y, y_len, x, x_len, flags, false);
}
int msm_frmat_mul(const msm_frmat* m, uint8_t* y, size_t y_len, const uint8_t* x, size_t x_len, uint32_t flags) {
  return frmat::mul_impl(m, nullptr, y, y_len, x, x_len, flags, true);
}

void msm_frmat_release(void) {
  std::lock_guard<std::mutex> hold(frmat::lock());
  for (auto& kv : frmat::states()) {
    frmat::DeviceGuard guard(kv.first);
    if (!guard.ok) continue;
    frmat::DeviceState& ds = kv.second;
    if (ds.stream) (void)hipStreamSynchronize(ds.stream);
    fr_host::drop(ds.staging);
  }
}

int msm_frmat_test_tile(int entries) {
  if (entries != 0 && (entries < 2 || entries > FRMAT_TILE || (entries & (entries - 1)))) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(frmat::lock());
  frmat::tile_hook() = (uint32_t)entries;
  return MSM_HIP_OK;
}

int msm_frmat_test_last(int* launches, int* levels) {
  if (!launches || !levels) return MSM_HIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> hold(frmat::lock());
  *launches = frmat::last_shape()[0];
  *levels = frmat::last_shape()[1];
  return MSM_HIP_OK;
}
}  // extern "C"
