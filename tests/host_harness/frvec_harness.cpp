// Stand-alone host program for tests/test_frvec_host.py: libmsm_frvec.so's calls run on the CPU -- the constants and levels of csrc/frvec_plan.h,
// and per lane the very functions the kernels of csrc/frvec_kernels.h call, one "workgroup" after the other, with the kernels' own loops.  Built
// with g++ -DFQ_CHECK, so every limb and value bound of csrc/fq29.h is asserted along the way.
//   frvec_harness map     <n> <op> <b_const> <c_const> <mont> <in> <out>      in: b[32] c[32] a[n] b[n] c[n]      (a constant, or a vector, is read)
//   frvec_harness inverse <n> <tile> <mont> <in> <out>                        in: a[n]
//   frvec_harness scan    <n> <batch> <tile> <op> <exclusive> <mont> <in> <out>      in: a[batch n];   out: out[batch n] totals[batch]
//   exit status: 0 ok, 3 a value >= r among the inputs, 2 bad arguments
// Compile with -DMSM_FIELD_NS=frv_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frvec_kernels.h"
#include "frvec_plan.h"

using namespace MSM_FIELD_NS;

static bool read_file(const char* path, std::vector<uint8_t>& out, size_t want) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  out.resize(want);
  const bool ok = fread(out.data(), 1, want, f) == want;
  fclose(f);
  return ok;
}
static bool write_file(const char* path, const uint32_t* words, size_t count) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(words, 4, count, f) == count;
  fclose(f);
  return ok;
}
static std::vector<uint32_t> words_of(const uint8_t* bytes, size_t count) {
  std::vector<uint32_t> w(count * 8);
  if (count) memcpy(w.data(), bytes, count * 32);
  return w;
}

static int run_map(int argc, char** argv) {
  if (argc != 9) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  const int op = atoi(argv[3]), b_const = atoi(argv[4]), c_const = atoi(argv[5]), mont = atoi(argv[6]);
  std::vector<uint8_t> in;
  if (n < 1 || !read_file(argv[7], in, 64 + 3 * n * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  const FrvecMapArgs m = msm_frvec::plan_map(f, op, b_const ? in.data() : nullptr, c_const ? in.data() + 32 : nullptr, mont != 0);
  const std::vector<uint32_t> a = words_of(in.data() + 64, n), b = words_of(in.data() + 64 + n * 32, n), c = words_of(in.data() + 64 + 2 * n * 32, n);
  std::vector<uint32_t> out(n * 8);
  bool ok = true;
  for (size_t i = 0; i < n; i++) ok &= frv_map_element(m, i, a.data(), b.data(), c.data(), out.data());
  return write_file(argv[8], out.data(), out.size()) ? (ok ? 0 : 3) : 2;
}

static int run_inverse(int argc, char** argv) {
  if (argc != 7) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  const uint32_t tile = (uint32_t)atoi(argv[3]);
  std::vector<uint8_t> in;
  if (n < 1 || tile < 2 || tile > FRVEC_TILE || !read_file(argv[5], in, n * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  const FrvecInvArgs v = msm_frvec::plan_inverse(f, tile, atoi(argv[4]) != 0);
  const std::vector<size_t> len = msm_frvec::plan_levels(n, tile);
  const size_t levels = len.size();
  std::vector<std::vector<uint32_t>> level(levels);  // level[0]: the data, in place; above it the tile products
  level[0] = words_of(in.data(), n);
  for (size_t l = 1; l < levels; l++) level[l].resize(len[l] * 8);
  std::vector<fq> tree(2 * FRVEC_THREADS);
  std::vector<FrvInvLane> lanes(FRVEC_THREADS);
  bool ok = true;
  // one launch of k_frvec_inverse over level l
  auto launch = [&](size_t l, uint32_t mode) {
    uint32_t* data = level[l].data();
    for (size_t blk = 0; blk < (len[l] + tile - 1) / tile; blk++) {
      for (uint32_t lane = 0; lane < FRVEC_THREADS; lane++) ok &= frv_inv_forward(v, len[l], blk, lane, data, lanes[lane], tree.data());
      for (uint32_t w = FRVEC_THREADS / 2; w >= 1; w >>= 1)
        for (uint32_t lane = 0; lane < w; lane++) frv_inv_up(tree.data(), w, lane);
      if (mode == FRVEC_INV_TOTALS) {
        frv_inv_total_out(tree.data(), level[l + 1].data(), blk);
        continue;
      }
      if (mode == FRVEC_INV_ROOTS) frv_inv_root_in(tree.data(), level[l + 1].data(), blk);
      else frv_inv_root(v, tree.data());
      for (uint32_t w = 1; w < FRVEC_THREADS; w <<= 1)
        for (uint32_t lane = 0; lane < w; lane++) frv_inv_down(tree.data(), w, lane);
      for (uint32_t lane = 0; lane < FRVEC_THREADS; lane++) frv_inv_backward(v, blk, lane, lanes[lane], tree.data(), data);
    }
  };
  for (size_t l = 0; l + 1 < levels; l++) launch(l, FRVEC_INV_TOTALS);
  for (size_t l = levels; l-- > 0;) launch(l, l + 1 < levels ? FRVEC_INV_ROOTS : FRVEC_INV_WHOLE);
  return write_file(argv[6], level[0].data(), level[0].size()) ? (ok ? 0 : 3) : 2;
}

static bool fold_level(const FrvecScanArgs& g, size_t batch, size_t n, const uint32_t* in, uint32_t* totals) {
  const size_t tiles = (n + g.tile - 1) / g.tile;
  std::vector<fq> slot(FRVEC_THREADS);
  FrvScanLane s;
  bool ok = true;
  for (size_t blk = 0; blk < batch * tiles; blk++) {
    for (uint32_t lane = 0; lane < FRVEC_THREADS; lane++) ok &= frv_scan_load(g, n, blk / tiles, blk % tiles, lane, in, s, slot.data());
    for (uint32_t w = FRVEC_THREADS / 2; w >= 1; w >>= 1)
      for (uint32_t lane = 0; lane < w; lane++) frv_fold_step(g.op, slot.data(), w, lane);
    frv_fold_store(slot.data(), totals, blk);
  }
  return ok;
}
static bool scan_level(const FrvecScanArgs& g, size_t batch, size_t n, const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* row_total) {
  const size_t tiles = (n + g.tile - 1) / g.tile;
  std::vector<fq> buf(2 * FRVEC_THREADS);
  std::vector<FrvScanLane> lanes(FRVEC_THREADS);
  bool ok = true;
  for (size_t blk = 0; blk < batch * tiles; blk++) {
    for (uint32_t lane = 0; lane < FRVEC_THREADS; lane++) ok &= frv_scan_load(g, n, blk / tiles, blk % tiles, lane, in, lanes[lane], buf.data());
    uint32_t from = 0;
    for (uint32_t d = 1; d < FRVEC_THREADS; d <<= 1, from ^= 1u)
      for (uint32_t lane = 0; lane < FRVEC_THREADS; lane++) frv_scan_step(g.op, buf.data() + from * FRVEC_THREADS, buf.data() + (from ^ 1u) * FRVEC_THREADS, d, lane);
    for (uint32_t lane = 0; lane < FRVEC_THREADS; lane++)
      frv_scan_store(g, n, blk / tiles, blk % tiles, tiles, lane, lanes[lane], buf.data() + from * FRVEC_THREADS, carry, out, row_total);
  }
  return ok;
}

static int run_scan(int argc, char** argv) {
  if (argc != 10) return 2;
  const size_t n = (size_t)atoll(argv[2]), batch = (size_t)atoll(argv[3]);
  const uint32_t tile = (uint32_t)atoi(argv[4]);
  std::vector<uint8_t> in;
  if (n < 1 || batch < 1 || tile < 2 || tile > FRVEC_TILE || !read_file(argv[8], in, batch * n * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  const FrvecScanArgs g = msm_frvec::plan_scan(f, tile, atoi(argv[5]), atoi(argv[6]) != 0, atoi(argv[7]) != 0), gi = msm_frvec::inner_level(g);
  const std::vector<size_t> len = msm_frvec::plan_levels(n, tile);
  const size_t levels = len.size();
  std::vector<std::vector<uint32_t>> level(levels);  // level[0]: the data, in place; above it the tile totals
  level[0] = words_of(in.data(), batch * n);
  for (size_t l = 1; l < levels; l++) level[l].resize(batch * len[l] * 8);
  std::vector<uint32_t> totals(batch * 8);
  bool ok = true;
  for (size_t l = 0; l + 1 < levels; l++) ok &= fold_level(l ? gi : g, batch, len[l], level[l].data(), level[l + 1].data());
  for (size_t l = levels; l-- > 0;)
    ok &= scan_level(l ? gi : g, batch, len[l], level[l].data(), level[l].data(), l + 1 < levels ? level[l + 1].data() : nullptr, l ? nullptr : totals.data());
  level[0].insert(level[0].end(), totals.begin(), totals.end());
  return write_file(argv[9], level[0].data(), level[0].size()) ? (ok ? 0 : 3) : 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "map")) return run_map(argc, argv);
  if (!strcmp(argv[1], "inverse")) return run_inverse(argc, argv);
  if (!strcmp(argv[1], "scan")) return run_scan(argc, argv);
  return 2;
}
