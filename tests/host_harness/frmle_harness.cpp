// Stand-alone host program for tests/test_frmle_host.py: libmsm_frmle.so's calls run on the CPU -- the constants and levels of
// csrc/frmle_plan.h, and per lane the very functions the kernels of csrc/frmle_kernels.h call, one "workgroup" after the other, with the kernels'
// own loops.  Built with g++ -DFQ_CHECK, so every limb and value bound of csrc/fq29.h is asserted along the way.
//   frmle_harness fold  <n> <batch> <stride> <in> <out>                in: c[32] a[span];                        out: a[span], folded in place
//   frmle_harness eval  <n> <batch> <stride> <tile> <in> <out>         in: point[log2 n] a[span];                out: values[batch]
//   frmle_harness eq    <n> <mont> <in> <out>                          in: c[32] point[log2 n];                  out: out[n]
//   frmle_harness round <n> <batch> <stride> <tile> <mont> <fold> <terms> <in> <out>
//                                                                      in: [fold_by[32]] terms[terms x 52] a[span];  out: values[D + 1] a[span]
//   span = (batch - 1) stride + n; a term is coeff[32], degree, rows[4] (little-endian 32-bit words)
//   exit status: 0 ok, 3 a value >= r among the inputs, 2 bad arguments
// Compile with -DMSM_FIELD_NS=frm_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frmle_kernels.h"
#include "frmle_plan.h"

using namespace MSM_FIELD_NS;

static bool read_file(const char* path, std::vector<uint8_t>& out, size_t want) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  out.resize(want);
  const bool ok = want == 0 || fread(out.data(), 1, want, f) == want;
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
static bool shape_ok(size_t n, size_t batch, size_t stride) { return msm_frmle::power_of_two(n) && batch >= 1 && stride >= n; }
static size_t span(size_t n, size_t batch, size_t stride) { return (batch - 1) * stride + n; }

static int run_fold(int argc, char** argv) {
  if (argc != 7) return 2;
  const size_t n = (size_t)atoll(argv[2]), batch = (size_t)atoll(argv[3]), stride = (size_t)atoll(argv[4]);
  std::vector<uint8_t> in;
  if (!shape_ok(n, batch, stride) || n < 2 || !read_file(argv[5], in, 32 + span(n, batch, stride) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  const FrmleFoldArgs g = msm_frmle::plan_fold(f, in.data());
  std::vector<uint32_t> a = words_of(in.data() + 32, span(n, batch, stride));
  bool ok = true;
  const size_t half = n / 2;
  for (size_t idx = 0; idx < batch * half; idx++) ok &= frm_fold_pair(g, idx / half, idx % half, half, stride, a.data(), a.data());
  return write_file(argv[6], a.data(), a.size()) ? (ok ? 0 : 3) : 2;
}

// one launch of k_frmle_eval
static bool eval_level(const FrmleEvalArgs& g, size_t batch, size_t stride, size_t tiles, const uint32_t* a, uint32_t* totals) {
  std::vector<fq> slot(FRMLE_THREADS);
  bool ok = true;
  for (size_t blk = 0; blk < batch * tiles; blk++) {
    for (uint32_t lane = 0; lane < FRMLE_THREADS; lane++) ok &= frm_eval_load(g, stride, blk / tiles, blk % tiles, lane, a, slot.data());
    for (uint32_t step = FRMLE_STEPS; step-- > 0;)
      if (frm_eval_has_step(g, step))
        for (uint32_t lane = 0; lane < (1u << step); lane++) frm_eval_step(g, slot.data(), step, lane);
    frm_eval_store(slot.data(), totals, blk);
  }
  return ok;
}
static int run_eval(int argc, char** argv) {
  if (argc != 8) return 2;
  const size_t n = (size_t)atoll(argv[2]), batch = (size_t)atoll(argv[3]), stride = (size_t)atoll(argv[4]);
  const uint32_t tile = (uint32_t)atoi(argv[5]);
  if (!shape_ok(n, batch, stride) || tile < 2 || tile > FRMLE_TILE || !msm_frmle::power_of_two(tile)) return 2;
  const int k = msm_frmle::log2_of(n);
  std::vector<uint8_t> in;
  if (!read_file(argv[6], in, (size_t)k * 32 + span(n, batch, stride) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  const std::vector<size_t> len = msm_frmle::plan_levels(n, tile);
  const std::vector<FrmleEvalArgs> g = msm_frmle::plan_eval(f, tile, k, in.data());
  if (g.size() != len.size()) return 2;
  const size_t levels = len.size();
  std::vector<std::vector<uint32_t>> level(levels);
  level[0] = words_of(in.data() + (size_t)k * 32, span(n, batch, stride));
  for (size_t l = 1; l < levels; l++) level[l].resize(batch * len[l] * 8);
  std::vector<uint32_t> values(batch * 8);
  bool ok = true;
  for (size_t l = 0; l < levels; l++)
    ok &= eval_level(g[l], batch, l ? len[l] : stride, (len[l] + tile - 1) / tile, level[l].data(), l + 1 < levels ? level[l + 1].data() : values.data());
  return write_file(argv[7], values.data(), values.size()) ? (ok ? 0 : 3) : 2;
}

static int run_eq(int argc, char** argv) {
  if (argc != 6) return 2;
  const size_t n = (size_t)atoll(argv[2]);
  if (!msm_frmle::power_of_two(n)) return 2;
  std::vector<uint8_t> in;
  if (!read_file(argv[4], in, 32 + (size_t)msm_frmle::log2_of(n) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  std::vector<uint32_t> tables;
  const FrmleEqArgs p = msm_frmle::plan_eq(f, n, in.data() + 32, in.data(), atoi(argv[3]) != 0, tables);
  std::vector<uint32_t> out(n * 8);
  const size_t lanes = (n + FRMLE_E - 1) / FRMLE_E, blocks = (lanes + FRMLE_THREADS - 1) / FRMLE_THREADS;
  for (size_t lane = 0; lane < blocks * FRMLE_THREADS; lane++) frm_eq_lane(p, lane, n, tables.data(), out.data());
  return write_file(argv[5], out.data(), out.size()) ? 0 : 2;
}

// one launch of k_frmle_round<POINTS>
template <int POINTS>
static bool round_level(const FrmleRoundArgs& g, uint32_t* a, uint32_t half, uint32_t stride, uint32_t tiles, const uint32_t* terms, uint32_t* partial) {
  struct Acc {
    fq v[POINTS];
  };
  std::vector<Acc> acc(FRMLE_THREADS);
  std::vector<fq> slot(FRMLE_THREADS);
  bool ok = true;
  for (uint32_t k = 0; k < tiles; k++) {
    for (uint32_t lane = 0; lane < FRMLE_THREADS; lane++) ok &= frm_round_lane<POINTS>(g, a, half, stride, k, lane, terms, acc[lane].v);
    for (int t = 0; t < POINTS; t++) {
      for (uint32_t lane = 0; lane < FRMLE_THREADS; lane++) slot[lane] = frm_exact(acc[lane].v[t]);
      for (uint32_t step = FRMLE_STEPS; step-- > 0;)
        for (uint32_t lane = 0; lane < (1u << step); lane++) frm_sum_step(slot.data(), step, lane);
      frm_store(partial, (size_t)t * tiles + k, slot[0]);
    }
  }
  return ok;
}
// one launch of k_frmle_sum
static void sum_level(uint32_t tile, size_t rows, size_t len, const uint32_t* in, uint32_t* out) {
  const size_t tiles = (len + tile - 1) / tile;
  std::vector<fq> slot(FRMLE_THREADS);
  for (size_t blk = 0; blk < rows * tiles; blk++) {
    for (uint32_t lane = 0; lane < FRMLE_THREADS; lane++) frm_sum_load(tile, len, blk / tiles, blk % tiles, lane, in, slot.data());
    for (uint32_t step = FRMLE_STEPS; step-- > 0;)
      for (uint32_t lane = 0; lane < (1u << step); lane++) frm_sum_step(slot.data(), step, lane);
    frm_store(out, blk, slot[0]);
  }
}
static int run_round(int argc, char** argv) {
  if (argc != 11) return 2;
  const size_t n = (size_t)atoll(argv[2]), batch = (size_t)atoll(argv[3]), stride = (size_t)atoll(argv[4]);
  const uint32_t tile = (uint32_t)atoi(argv[5]);
  const bool mont = atoi(argv[6]) != 0, fold = atoi(argv[7]) != 0;
  const size_t num_terms = (size_t)atoll(argv[8]);
  const size_t term_bytes = 52;
  if (!shape_ok(n, batch, stride) || n < (fold ? 4u : 2u) || batch > FRMLE_MAX_ROWS || num_terms < 1 || num_terms > FRMLE_MAX_TERMS) return 2;
  if (tile < 2 || tile > FRMLE_TILE || !msm_frmle::power_of_two(tile)) return 2;
  std::vector<uint8_t> in;
  const size_t head = (fold ? 32 : 0) + num_terms * term_bytes;
  if (!read_file(argv[9], in, head + span(n, batch, stride) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  uint32_t rows[FRMLE_MAX_TERMS][4];
  msm_frmle::Term terms[FRMLE_MAX_TERMS];
  for (size_t k = 0; k < num_terms; k++) {
    const uint8_t* t = in.data() + (fold ? 32 : 0) + k * term_bytes;
    uint32_t degree;
    memcpy(&degree, t + 32, 4);
    memcpy(rows[k], t + 36, 16);
    if (degree < 1 || degree > FRMLE_MAX_DEGREE) return 2;
    terms[k] = msm_frmle::Term{t, degree, rows[k]};
  }
  std::vector<uint32_t> words;
  const FrmleRoundArgs g = msm_frmle::plan_round(f, tile, terms, num_terms, batch, fold ? in.data() : nullptr, mont, words);
  std::vector<uint32_t> a = words_of(in.data() + head, span(n, batch, stride));
  const size_t half = fold ? n / 4 : n / 2;
  const std::vector<size_t> len = msm_frmle::plan_levels(half, tile);
  const size_t levels = len.size();
  std::vector<std::vector<uint32_t>> level(levels);
  for (size_t l = 1; l < levels; l++) level[l].resize(g.points * len[l] * 8);
  std::vector<uint32_t> values(g.points * 8);
  uint32_t* first = levels > 1 ? level[1].data() : values.data();
  const uint32_t tiles = (uint32_t)((half + tile - 1) / tile);
  bool ok = true;
  switch (g.points) {
    case 2: ok = round_level<2>(g, a.data(), (uint32_t)half, (uint32_t)stride, tiles, words.data(), first); break;
    case 3: ok = round_level<3>(g, a.data(), (uint32_t)half, (uint32_t)stride, tiles, words.data(), first); break;
    case 4: ok = round_level<4>(g, a.data(), (uint32_t)half, (uint32_t)stride, tiles, words.data(), first); break;
    default: ok = round_level<5>(g, a.data(), (uint32_t)half, (uint32_t)stride, tiles, words.data(), first); break;
  }
  for (size_t l = 1; l < levels; l++) sum_level(tile, g.points, len[l], level[l].data(), l + 1 < levels ? level[l + 1].data() : values.data());
  values.insert(values.end(), a.begin(), a.end());
  return write_file(argv[10], values.data(), values.size()) ? (ok ? 0 : 3) : 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "fold")) return run_fold(argc, argv);
  if (!strcmp(argv[1], "eval")) return run_eval(argc, argv);
  if (!strcmp(argv[1], "eq")) return run_eq(argc, argv);
  if (!strcmp(argv[1], "round")) return run_round(argc, argv);
  return 2;
}
