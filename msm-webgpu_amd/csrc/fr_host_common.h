// What the host side of every scalar-field library shares (csrc/ntt_host.h, csrc/frvec_host.h ... csrc/frhash_host.h include it; each is compiled
// once, by its library's bn254 unit): the device guard, buffers that grow, the pointer checks, the curve-to-field choice, and the scheme for
// the state a library keeps per device.  No entry point's flow is here: which HIP call a call makes, and in which order, is its library's own.
//
// The rule for state: nothing in this file holds any.  A static local of an inline function is a weak symbol that two
// libraries in one process may share, so the lock and the per-device map are templates over the library's OWN DeviceState -- one instance
// per library, named after its namespace -- and a library's test hooks stay inline functions of that namespace.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>

#include "../../include/msm_hip.h"

namespace fr_host {

struct DeviceGuard {  // every entry point runs on its device and leaves the caller's current device as it found it
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = prev == device || hipSetDevice(device) == hipSuccess;
    if (prev == device) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

struct Buffer {
  uint32_t* p = nullptr;
  size_t words = 0;
};

// at least want_words words, in device memory or (pinned) in page-locked host memory; what the buffer held is not kept
inline int grow(Buffer& b, size_t want_words, bool pinned = false) {
  if (b.words >= want_words) return MSM_HIP_OK;
  if (b.p) (void)(pinned ? hipHostFree(b.p) : hipFree(b.p));
  b.p = nullptr;
  b.words = 0;
  const hipError_t e = pinned ? hipHostMalloc(reinterpret_cast<void**>(&b.p), want_words * 4, hipHostMallocDefault) : hipMalloc(reinterpret_cast<void**>(&b.p), want_words * 4);
  if (e != hipSuccess) return MSM_HIP_ERR_OUT_OF_MEMORY;
  b.words = want_words;
  return MSM_HIP_OK;
}
// a device buffer given back (the release entry points)
inline void drop(Buffer& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.words = 0;
}

inline bool apart(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p + a_bytes <= q || q + b_bytes <= p;
}
inline bool misaligned(const void* p, uintptr_t to = 16) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }
inline bool hip_ok(hipError_t e) { return e == hipSuccess; }
inline int have_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device >= count) return MSM_HIP_ERR_NO_DEVICE;
  return MSM_HIP_OK;
}

// One lock and one map of per-device state for each State, that is for each library.
template <class State>
std::mutex& lock_of() {
  static std::mutex m;
  return m;
}
template <class State>
std::map<int, State>& states_of() {
  static std::map<int, State> s;
  return s;
}

// The scalar field of a curve, as the table of launchers its unit exports; only the chosen field's getter is called.  A null getter: the
// library has no unit for that field.  field_id: the field's number among the four with a transform (csrc/ntt_host.h keys its tables by it).
template <class Ops>
const Ops* field_of(int curve, const Ops* (*bn254)(), const Ops* (*grumpkin)(), const Ops* (*pallas)(), const Ops* (*vesta)(), const Ops* (*bls12_381)(), int* field_id = nullptr) {
  const Ops* (*get)() = nullptr;
  int id = 0;
  switch (curve) {
    case MSM_HIP_CURVE_BN254_G1:
    case MSM_HIP_CURVE_BN254_G2: get = bn254, id = 0; break;
    case MSM_HIP_CURVE_GRUMPKIN: get = grumpkin; break;
    case MSM_HIP_CURVE_PALLAS: get = pallas, id = 1; break;
    case MSM_HIP_CURVE_VESTA: get = vesta, id = 2; break;
    case MSM_HIP_CURVE_BLS12_381:
    case MSM_HIP_CURVE_BLS12_381_G2: get = bls12_381, id = 3; break;
    default: break;
  }
  if (!get) return nullptr;
  if (field_id) *field_id = id;
  return get();
}

}  // namespace fr_host
