// libmsm_frcol.so's kernels on the CPU (tests/test_frcol_host.py): the plan of csrc/frcol_plan.h and the per-lane functions of csrc/frcol_kernels.h,
// run workgroup by workgroup, lane by lane and phase by phase -- a barrier of the kernel is the end of a loop over the lanes here.  Every array
// is a heap allocation of exactly the size the library gives it, so that AddressSanitizer sees any access out of range.
//
//   frcol_harness run expand|pair n_t tile bias n_out in out      in: t (n_t x 32 bytes), counts (n_t words)
//   frcol_harness gather n_a n in out                              in: a (n_a x 32 bytes), idx (n words)
// out: eight words (error word, levels, total, used, launches, 0), then the outputs, which start as bytes 0xA5.  Exit status 0, or 2 where the library
// would return MSM_HIP_ERR_INVALID_ARG.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frcol_kernels.h"
#include "frcol_plan.h"

using namespace frcol;

static std::vector<uint8_t> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(10);
  std::vector<uint8_t> b;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
  fclose(f);
  return b;
}

// the inclusive scan of a workgroup's lane sums: k_frcol's block_scan, a loop over the lanes per phase
static void block_scan(FrcNode* lds, const std::vector<FrcLane>& s) {
  for (uint32_t lane = 0; lane < FRCOL_THREADS; lane++) frc_put(lds, lane, s[lane]);
  for (uint32_t step = 0; step < FRCOL_SCAN_STEPS; step++) {
    FrcNode v[FRCOL_THREADS];
    for (uint32_t lane = 0; lane < FRCOL_THREADS; lane++) v[lane] = frc_peek(lds, lane, step);
    for (uint32_t lane = 0; lane < FRCOL_THREADS; lane++) frc_add(lds, lane, v[lane]);
  }
}
template <bool LEAF>
static void load_tile(const FrcolArgs& g, const uint32_t* counts, const FrcNode* nodes, size_t len, size_t tile_at, std::vector<FrcLane>& s) {
  s.resize(FRCOL_THREADS);
  for (uint32_t lane = 0; lane < FRCOL_THREADS; lane++) frc_load<LEAF>(g, counts, nodes, len, tile_at, lane, s[lane]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 11;
  const std::string cmd = argv[1];
  if (cmd == "gather" && argc == 6) {
    const size_t n_a = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
    const std::vector<uint8_t> in = read_file(argv[4]);
    if (in.size() != n_a * 32 + n * 4) return 12;
    std::vector<uint32_t> a(n_a * 8), idx(n), out(n * 8), res(FRCOL_RESULT_WORDS, 0);
    memcpy(a.data(), in.data(), n_a * 32);
    memcpy(idx.data(), in.data() + n_a * 32, n * 4);
    memset(out.data(), 0xA5, n * 32);
    const uint32_t lanes = (uint32_t)((n + FRCOL_THREADS - 1) / FRCOL_THREADS) * FRCOL_THREADS;  // the whole grid, the lanes behind n included
    for (uint32_t i = 0; i < lanes; i++) frc_gather_lane(a.data(), (uint32_t)n_a, idx.data(), (uint32_t)n, out.data(), res.data(), i);
    FILE* f = fopen(argv[5], "wb");
    if (!f) return 13;
    fwrite(res.data(), 4, res.size(), f);
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return res[FRCOL_RES_ERR] ? 2 : 0;
  }
  if (cmd != "run" || argc != 9) return 11;
  const bool pair = std::string(argv[2]) == "pair";
  const size_t n_t = strtoull(argv[3], nullptr, 10), n_out = strtoull(argv[6], nullptr, 10);
  const uint32_t tile = tile_of((uint32_t)strtoul(argv[4], nullptr, 10)), bias = (uint32_t)strtoul(argv[5], nullptr, 10);
  const std::vector<uint8_t> in = read_file(argv[7]);
  if (in.size() != n_t * 36) return 12;
  std::vector<uint32_t> t(n_t * 8), counts(n_t), out(n_out * 8), s_out(pair ? n_out * 8 : 0), res(FRCOL_RESULT_WORDS, 0);
  memcpy(t.data(), in.data(), n_t * 32);
  memcpy(counts.data(), in.data() + n_t * 32, n_t * 4);
  memset(out.data(), 0xA5, out.size() * 4);
  if (pair) memset(s_out.data(), 0xA5, s_out.size() * 4);
  if (pair ? !pair_args_ok(out.data(), s_out.data(), t.data(), counts.data(), n_t, true) || n_out != n_t : !expand_args_ok(out.data(), t.data(), counts.data(), n_t, bias, n_out, true))
    return 14;

  const FrcolArgs g = plan_args(n_t, tile, bias, n_out, pair);
  const Layout y = plan_layout(n_t, tile);
  // the scratch buffer in its parts, each of its exact size
  std::vector<std::vector<FrcNode>> nodes(y.len.size());
  for (size_t l = 1; l < y.len.size(); l++) nodes[l].assign(y.len[l], FrcNode{0xdeadbeefdeadbeefull, 0xdeadbeefdeadbeefull});
  std::vector<uint32_t> rel(n_t, 0xdeadbeefu), used(n_t, 0xdeadbeefu), z(n_t, 0xdeadbeefu);
  const size_t top = y.len.size() - 1;
  FrcNode lds[FRCOL_THREADS];
  std::vector<FrcLane> s;
  int launches = 0;
  for (size_t l = 0; l < top; l++, launches++)  // k_frcol_sums
    for (size_t wg = 0; wg < y.len[l + 1]; wg++) {
      if (l == 0) load_tile<true>(g, counts.data(), nullptr, y.len[0], wg, s); else load_tile<false>(g, nullptr, nodes[l].data(), y.len[l], wg, s);
      block_scan(lds, s);
      frc_store_sum(lds, nodes[l + 1].data(), wg, y.len[l + 1]);
    }
  for (size_t l = top; l >= 1; l--, launches++) {  // k_frcol_scan<false>
    const FrcNode* above = l == top ? nullptr : nodes[l + 1].data();
    const size_t tiles = l == top ? 1 : y.len[l + 1];
    for (size_t wg = 0; wg < tiles; wg++) {
      load_tile<false>(g, nullptr, nodes[l].data(), y.len[l], wg, s);
      block_scan(lds, s);
      for (uint32_t lane = 0; lane < FRCOL_THREADS; lane++) frc_store_inner(g, lds, above, nodes[l].data(), y.len[l], wg, lane, s[lane]);
      if (!above) frc_store_totals(lds, res.data());
    }
  }
  for (size_t wg = 0; wg < y.len[1]; wg++) {  // k_frcol_scan<true>
    load_tile<true>(g, counts.data(), nullptr, y.len[0], wg, s);
    block_scan(lds, s);
    for (uint32_t lane = 0; lane < FRCOL_THREADS; lane++) frc_store_leaf(g, lds, nodes[1].data(), rel.data(), used.data(), z.data(), wg, lane, s[lane]);
  }
  launches += 2;
  const uint32_t lanes = (uint32_t)((n_out + FRCOL_THREADS - 1) / FRCOL_THREADS) * FRCOL_THREADS;
  for (uint32_t k = 0; k < lanes; k++) {
    if (pair)
      frc_pair_lane(g, res.data(), nodes[1].data(), rel.data(), used.data(), z.data(), t.data(), out.data(), s_out.data(), k);
    else
      frc_expand_lane(g, res.data(), nodes[1].data(), rel.data(), t.data(), out.data(), k);
  }
  res[1] = (uint32_t)y.len.size(), res[6] = (uint32_t)launches;
  FILE* f = fopen(argv[8], "wb");
  if (!f) return 13;
  fwrite(res.data(), 4, res.size(), f);
  fwrite(out.data(), 4, out.size(), f);
  if (pair) fwrite(s_out.data(), 4, s_out.size(), f);
  fclose(f);
  return frc_total(res.data()) == n_out ? 0 : 2;
}
