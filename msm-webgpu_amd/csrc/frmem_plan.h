// The host side of libmsm_frmem.so that needs no HIP: the limits of include/msm_frmem.h, the argument checks, the passes of the sort, the levels of
// its scans, the launches and where each array lies in the scratch buffer (csrc/frmem_host.h launches what this plans; the host program of
// tests/test_frmem_host.py runs the same plan through the same per-lane code on the CPU).  Needs FrmemArgs and FrmNode of csrc/frmem_kernels.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace frmem {

constexpr size_t MAX_ELEMENTS = (size_t)1 << 26;

// (the two pointer checks of csrc/fr_host_common.h, which needs HIP: the host program runs the argument checks too)
inline bool apart(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p + a_bytes <= q || q + b_bytes <= p;
}
inline bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }
// every part that is there aligned to its words, and every OUTPUT (the first `outputs` parts) apart from every other part; an output may be
// absent (null), the keys -- the last part -- may not
struct Part {
  const void* p;
  size_t bytes, align;
};
inline bool parts_ok(const Part* part, int parts, int outputs) {
  if (!part[parts - 1].p) return false;
  for (int a = 0; a < parts; a++)
    if (part[a].p && misaligned(part[a].p, part[a].align)) return false;
  for (int a = 0; a < outputs; a++)
    for (int b = 0; b < parts; b++)
      if (a != b && part[a].p && part[b].p && !apart(part[a].p, part[a].bytes, part[b].p, part[b].bytes)) return false;
  return true;
}
inline bool keys_ok(size_t key_bytes, uint32_t key_bits, size_t n) {
  return (key_bytes == 4 || key_bytes == 8) && key_bits >= 1 && key_bits <= 8 * key_bytes && n >= 1 && n <= MAX_ELEMENTS;
}
inline bool sort_args_ok(const void* perm_out, const void* keys_out, const void* keys, size_t key_bytes, uint32_t key_bits, size_t n) {
  if (!keys_ok(key_bytes, key_bits, n) || !perm_out) return false;
  const Part part[3] = {{perm_out, n * 4, 4}, {keys_out, n * key_bytes, key_bytes}, {keys, n * key_bytes, key_bytes}};
  return parts_ok(part, 3, 2);
}
inline bool access_args_ok(const void* rank_out, const void* prev_out, const void* counts_out, const void* last_out, size_t n_t, const void* keys, size_t key_bytes,
                           uint32_t key_bits, size_t n) {
  if (!keys_ok(key_bytes, key_bits, n) || (!rank_out && !prev_out && !counts_out && !last_out)) return false;
  const bool table = counts_out || last_out;
  if (table && (n_t < 1 || n_t > MAX_ELEMENTS)) return false;
  const size_t t = table ? n_t : 0;
  const Part part[5] = {{rank_out, n * 4, 4}, {prev_out, n * 4, 4}, {counts_out, t * 4, 4}, {last_out, t * 4, 4}, {keys, n * key_bytes, key_bytes}};
  return parts_ok(part, 5, 4);
}

inline uint32_t tile_of(uint32_t hook) { return hook ? hook : FRMEM_TILE; }
// the digit counts, 256 per tile of keys, are indexed in 32 bits: always so at the design's tile (2^24 words at most); a test tile of 4 keys or
// fewer with n near 2^26 is refused
inline bool tile_ok(size_t n, uint32_t tile) { return (uint64_t)FRMEM_DIGITS * ((n + tile - 1) / tile) <= 0xffffffffull; }
// the greatest key a call takes: 2^key_bits - 1, and n_t - 1 where counts or last are asked for (n_t = 0: they are not)
inline uint64_t max_key_of(uint32_t key_bits, size_t n_t) {
  const uint64_t m = key_bits >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << key_bits) - 1;
  return n_t && n_t - 1 < m ? n_t - 1 : m;
}
// a scan's levels: level 0 holds `len` entries, level l + 1 one node per tile of level l, until a level fits one tile
inline std::vector<size_t> plan_levels(size_t len, uint32_t tile) {
  std::vector<size_t> lv(1, len);
  while (lv.back() > tile) lv.push_back((lv.back() + tile - 1) / tile);
  return lv;
}

// One call.  The scratch buffer, in 32-bit words: the (key, index) buffers (keys first: 8-byte words stay aligned) -- two where the passes
// ping-pong, one for an access of one pass, none for a sort of one pass, which writes the caller's outputs --, the digit counts, start[], then the
// nodes (two words each) of the levels above the digit counts and above the sorted keys.
struct Plan {
  uint32_t n, tile, tiles, passes, kw, bufs;  // kw: words per key; bufs: (key, index) buffers in the scratch
  bool access, table;
  std::vector<size_t> dlen, dnode_at;  // the scan of the digit counts: dlen[0] = 256 * tiles; dnode_at[l]: where level l >= 1 begins, in nodes
  std::vector<size_t> hlen, hnode_at;  // access: the scan of the heads, hlen[0] = n
  size_t keys_at[2], idx_at[2], hist_at, start_at, dnodes_at, hnodes_at, words;
  int launches, levels;
};
inline Plan plan_call(size_t n, size_t key_bytes, uint32_t key_bits, uint32_t tile, bool access, bool table) {
  Plan y;
  y.n = (uint32_t)n, y.tile = tile, y.tiles = (uint32_t)((n + tile - 1) / tile), y.passes = (key_bits + FRMEM_DIGIT_BITS - 1) / FRMEM_DIGIT_BITS, y.kw = (uint32_t)(key_bytes / 4);
  y.access = access, y.table = access && table;
  y.dlen = plan_levels((size_t)FRMEM_DIGITS * y.tiles, tile);
  y.dnode_at.assign(y.dlen.size(), 0);
  size_t dnodes = 0, hnodes = 0;
  for (size_t l = 1; l < y.dlen.size(); l++) y.dnode_at[l] = dnodes, dnodes += y.dlen[l];
  if (access) {
    y.hlen = plan_levels(n, tile);
    y.hnode_at.assign(y.hlen.size(), 0);
    for (size_t l = 1; l < y.hlen.size(); l++) y.hnode_at[l] = hnodes, hnodes += y.hlen[l];
  }
  const size_t bufs = y.bufs = y.passes > 1 ? 2 : access ? 1 : 0;
  size_t at = 0;
  for (size_t b = 0; b < 2; b++) y.keys_at[b] = b < bufs ? at : 0, at += b < bufs ? n * y.kw : 0;
  for (size_t b = 0; b < 2; b++) y.idx_at[b] = b < bufs ? at : 0, at += b < bufs ? n : 0;
  y.hist_at = at, at += y.dlen[0];
  y.start_at = at, at += access ? n : 0;
  at += at & 1;
  y.dnodes_at = at, at += 2 * dnodes;
  y.hnodes_at = at, at += 2 * hnodes;
  y.words = at;
  // a pass: hist, the sums upwards, the scans downwards, scatter; access: fill (where there is a table), the heads' sums and scans, the writes
  y.launches = (int)(y.passes * (2 + 2 * (y.dlen.size() - 1) + 1));
  if (access) y.launches += (int)((y.table ? 1 : 0) + 2 * (y.hlen.size() - 1) + 1 + 1);
  y.levels = (int)(1 + y.dlen.size());  // the keys, their digit counts, the nodes above those
  return y;
}
inline FrmemArgs plan_args(const Plan& y, uint32_t pass, uint64_t max_key) {
  FrmemArgs g;
  g.n = y.n, g.tile = y.tile, g.tiles = y.tiles, g.shift = pass * FRMEM_DIGIT_BITS, g.first = pass == 0 ? 1u : 0u, g.pad = 0, g.max_key = max_key;
  return g;
}
// where pass `pass` reads and writes: the caller's keys first (-1), then the buffers in turn
inline int src_buffer(uint32_t pass) { return pass == 0 ? -1 : (int)((pass - 1) & 1); }
inline int dst_buffer(uint32_t pass) { return (int)(pass & 1); }

}  // namespace frmem
