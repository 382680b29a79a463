// The host side of libmsm_frcol.so that needs no HIP: the limits of include/msm_frcol.h, the argument checks, the levels of the scan and where each
// array lies in the scratch buffer (csrc/frcol_host.h launches what this plans; the host program of tests/test_frcol_host.py runs the same plan
// through the same per-lane code on the CPU).  Needs FrcolArgs and FrcNode of csrc/frcol_kernels.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace frcol {

constexpr size_t MAX_TABLE = (size_t)1 << 24;
constexpr size_t MAX_ELEMENTS = (size_t)1 << 26;

// (the two pointer checks of csrc/fr_host_common.h, which needs HIP: the host program runs the argument checks too)
inline bool apart(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p + a_bytes <= q || q + b_bytes <= p;
}
inline bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }
// every pointer there, aligned (scalars: `scalar_align` bytes -- 16 for device memory, 1 for host memory; words: 4) and every OUTPUT (the first
// `outputs` parts) apart from every other part
struct Part {
  const void* p;
  size_t bytes;
  bool scalars;
};
inline bool parts_ok(const Part* part, int parts, int outputs, uintptr_t scalar_align) {
  for (int a = 0; a < parts; a++)
    if (!part[a].p || misaligned(part[a].p, part[a].scalars ? scalar_align : 4)) return false;
  for (int a = 0; a < outputs; a++)
    for (int b = 0; b < parts; b++)
      if (a != b && !apart(part[a].p, part[a].bytes, part[b].p, part[b].bytes)) return false;
  return true;
}
inline bool expand_args_ok(const void* out, const void* t, const void* counts, size_t n_t, uint32_t bias, size_t n_out, bool host) {
  if (n_t < 1 || n_t > MAX_TABLE || n_out < 1 || n_out > MAX_ELEMENTS || bias > 1) return false;
  const Part part[3] = {{out, n_out * 32, true}, {t, n_t * 32, true}, {counts, n_t * 4, false}};
  return parts_ok(part, 3, 1, host ? 1 : 16);
}
inline bool pair_args_ok(const void* a_out, const void* s_out, const void* t, const void* counts, size_t n, bool host) {
  if (n < 1 || n > MAX_TABLE) return false;
  const Part part[4] = {{a_out, n * 32, true}, {s_out, n * 32, true}, {t, n * 32, true}, {counts, n * 4, false}};
  return parts_ok(part, 4, 2, host ? 1 : 16);
}
inline bool gather_args_ok(const void* out, const void* a, size_t n_a, const void* idx, size_t n, bool host) {
  if (n_a < 1 || n_a > MAX_ELEMENTS || n < 1 || n > MAX_ELEMENTS) return false;
  const Part part[3] = {{out, n * 32, true}, {a, n_a * 32, true}, {idx, n * 4, false}};
  return parts_ok(part, 3, 1, host ? 1 : 16);
}

// level 0 is the table; level l + 1 has one node per tile of level l; the last level fits one tile (there are always at least two levels, so
// that the tile bases an output searches exist for the smallest table too)
inline std::vector<size_t> plan_levels(size_t n_t, uint32_t tile) {
  std::vector<size_t> len(1, n_t);
  do len.push_back((len.back() + tile - 1) / tile);
  while (len.back() > tile);
  return len;
}
inline uint32_t tile_of(uint32_t hook) { return hook ? hook : FRCOL_TILE; }

// the scratch buffer, in 32-bit words: the nodes of levels 1 .. (four words each, the buffer is aligned for them), then rel, used and z
struct Layout {
  std::vector<size_t> len, node_at;  // node_at[l]: where level l's nodes begin, in nodes (node_at[0] unused)
  size_t rel_at, used_at, z_at, words;
};
inline Layout plan_layout(size_t n_t, uint32_t tile) {
  Layout y;
  y.len = plan_levels(n_t, tile);
  y.node_at.assign(y.len.size(), 0);
  size_t nodes = 0;
  for (size_t l = 1; l < y.len.size(); l++) y.node_at[l] = nodes, nodes += y.len[l];
  y.rel_at = nodes * 4, y.used_at = y.rel_at + n_t, y.z_at = y.used_at + n_t, y.words = y.z_at + n_t;
  return y;
}
inline FrcolArgs plan_args(size_t n_t, uint32_t tile, uint32_t bias, size_t n_out, bool pair) {
  FrcolArgs g;
  g.n_t = (uint32_t)n_t, g.tile = tile, g.bias = bias, g.n_out = (uint32_t)n_out;
  g.tiles = (uint32_t)((n_t + tile - 1) / tile), g.pair = pair ? 1u : 0u;
  return g;
}

}  // namespace frcol
