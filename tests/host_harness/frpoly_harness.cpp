// Stand-alone host program for tests/test_frpoly_host.py: libmsm_frpoly.so's calls run on the CPU -- the constants and levels of
// csrc/frpoly_plan.h, and per lane the very functions the kernels of csrc/frpoly_kernels.h call, one "workgroup" after the other, with the kernels'
// own loops.  Built with g++ -DFQ_CHECK, so every limb and value bound of csrc/fq29.h is asserted along the way.
//   frpoly_harness eval    <n> <batch> <tile> <mont> <in> <out>      in: z[32] a[batch n];            out: values[batch]
//   frpoly_harness divide  <n> <batch> <tile> <mont> <in> <out>      in: z[32] a[batch n];            out: out[batch n] values[batch]
//   frpoly_harness dot     <n> <batch> <tile> <mont> <shared> <in> <out>     in: a[batch n] b[n or batch n];  out: values[batch]
//   frpoly_harness combine <n> <batch> <mont> <in> <out>             in: coeffs[batch] a[batch n];    out: out[n]  (computed in place on row 0)
//   frpoly_harness powers  <n> <mont> <in> <out>                     in: g[32] c[32];                 out: out[n]
//   exit status: 0 ok, 3 a value >= r among the inputs, 2 bad arguments
// Compile with -DMSM_FIELD_NS=frp_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frpoly_kernels.h"
#include "frpoly_plan.h"

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

// one launch of k_frpoly_fold
static bool fold_level(const FrpolyLevelArgs& g, size_t batch, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* totals) {
  const size_t tiles = (n + g.tile - 1) / g.tile;
  std::vector<fq> slot(FRPOLY_THREADS);
  bool ok = true;
  for (size_t blk = 0; blk < batch * tiles; blk++) {
    for (uint32_t lane = 0; lane < FRPOLY_THREADS; lane++) ok &= frp_fold_load(g, n, blk / tiles, blk % tiles, lane, a, b, slot.data());
    for (uint32_t step = FRPOLY_STEPS; step-- > 0;)
      for (uint32_t lane = 0; lane < (1u << step); lane++) frp_fold_step(g, slot.data(), step, lane);
    frp_fold_store(g, slot.data(), totals, blk);
  }
  return ok;
}
// one launch of k_frpoly_suffix (in place where in == out: every lane of a workgroup loads before the first one stores)
static bool suffix_level(const FrpolyLevelArgs& g, size_t batch, size_t n, const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* values) {
  const size_t tiles = (n + g.tile - 1) / g.tile;
  std::vector<fq> buf(2 * FRPOLY_THREADS);
  std::vector<FrpSuffixLane> lanes(FRPOLY_THREADS);
  bool ok = true;
  for (size_t blk = 0; blk < batch * tiles; blk++) {
    for (uint32_t lane = 0; lane < FRPOLY_THREADS; lane++) ok &= frp_suffix_load(g, n, blk / tiles, blk % tiles, tiles, lane, in, carry, lanes[lane], buf.data());
    uint32_t from = 0;
    for (uint32_t step = 0; step < FRPOLY_STEPS; step++, from ^= 1u)
      for (uint32_t lane = 0; lane < FRPOLY_THREADS; lane++) frp_suffix_step(g, buf.data() + from * FRPOLY_THREADS, buf.data() + (from ^ 1u) * FRPOLY_THREADS, step, lane);
    for (uint32_t lane = 0; lane < FRPOLY_THREADS; lane++) frp_suffix_store(g, n, blk / tiles, blk % tiles, lane, lanes[lane], buf.data() + from * FRPOLY_THREADS, out, values);
  }
  return ok;
}

// eval, divide (out the data in place) and dot, level by level as csrc/frpoly_host.h launches them
static int run_fold(int argc, char** argv, bool divide, bool dot) {
  if (argc != (dot ? 9 : 8)) return 2;
  const size_t n = (size_t)atoll(argv[2]), batch = (size_t)atoll(argv[3]);
  const uint32_t tile = (uint32_t)atoi(argv[4]);
  const bool mont = atoi(argv[5]) != 0, shared = dot && atoi(argv[6]) != 0;
  const char *in_path = argv[dot ? 7 : 6], *out_path = argv[dot ? 8 : 7];
  if (n < 1 || batch < 1 || tile < 2 || tile > FRPOLY_TILE) return 2;
  const size_t b_count = dot ? (shared ? n : batch * n) : 0, head = dot ? 0 : 32;
  std::vector<uint8_t> in;
  if (!read_file(in_path, in, head + (batch * n + b_count) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  const std::vector<size_t> len = msm_frpoly::plan_levels(n, tile);
  const size_t levels = len.size();
  const std::vector<FrpolyLevelArgs> g = dot ? msm_frpoly::plan_dot(f, tile, levels, shared, mont) : msm_frpoly::plan_horner(f, tile, levels, in.data());
  std::vector<std::vector<uint32_t>> level(levels);
  level[0] = words_of(in.data() + head, batch * n);
  const std::vector<uint32_t> b = words_of(in.data() + head + batch * n * 32, b_count);
  for (size_t l = 1; l < levels; l++) level[l].resize(batch * len[l] * 8);
  std::vector<uint32_t> values(batch * 8);
  bool ok = true;
  for (size_t l = 0; l + (divide ? 1 : 0) < levels; l++)
    ok &= fold_level(g[l], batch, len[l], level[l].data(), l ? nullptr : b.data(), l + 1 < levels ? level[l + 1].data() : values.data());
  if (divide) {
    for (size_t l = levels; l-- > 0;)
      ok &= suffix_level(g[l], batch, len[l], level[l].data(), level[l].data(), l + 1 < levels ? level[l + 1].data() : nullptr, l + 1 < levels ? nullptr : values.data());
  }
  std::vector<uint32_t> out;
  if (divide) out = level[0];
  out.insert(out.end(), values.begin(), values.end());
  return write_file(out_path, out.data(), out.size()) ? (ok ? 0 : 3) : 2;
}

static int run_combine(int argc, char** argv) {
  if (argc != 7) return 2;
  const size_t n = (size_t)atoll(argv[2]), batch = (size_t)atoll(argv[3]);
  std::vector<uint8_t> in;
  if (n < 1 || batch < 1 || batch > FRPOLY_MAX_ROWS || !read_file(argv[5], in, (batch + batch * n) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  std::vector<uint32_t> coeffs;
  msm_frpoly::plan_combine(f, in.data(), batch, coeffs);
  std::vector<uint32_t> a = words_of(in.data() + batch * 32, batch * n);
  bool ok = true;
  for (size_t i = 0; i < n; i++) ok &= frp_combine_element(i, n, (uint32_t)batch, a.data(), coeffs.data(), a.data());
  return write_file(argv[6], a.data(), n * 8) ? (ok ? 0 : 3) : 2;
}

static int run_powers(int argc, char** argv) {
  if (argc != 6) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  std::vector<uint8_t> in;
  if (n < 1 || !read_file(argv[4], in, 64)) return 2;
  const host_fr::Field f(FQ_P32);
  std::vector<uint32_t> tables;
  const FrpolyPowersArgs p = msm_frpoly::plan_powers(f, n, in.data(), in.data() + 32, atoi(argv[3]) != 0, tables);
  std::vector<uint32_t> out(n * 8);
  const size_t lanes = (n + FRPOLY_E - 1) / FRPOLY_E, blocks = (lanes + FRPOLY_THREADS - 1) / FRPOLY_THREADS;
  for (size_t lane = 0; lane < blocks * FRPOLY_THREADS; lane++) frp_powers_lane(p, lane, n, tables.data(), out.data());
  return write_file(argv[5], out.data(), out.size()) ? 0 : 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "eval")) return run_fold(argc, argv, false, false);
  if (!strcmp(argv[1], "divide")) return run_fold(argc, argv, true, false);
  if (!strcmp(argv[1], "dot")) return run_fold(argc, argv, false, true);
  if (!strcmp(argv[1], "combine")) return run_combine(argc, argv);
  if (!strcmp(argv[1], "powers")) return run_powers(argc, argv);
  return 2;
}
