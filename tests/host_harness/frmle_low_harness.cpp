// Stand-alone host program for tests/test_frmle_low_host.py: fold, round and the fused round of libmsm_frmle.so in BOTH variable orders, run on the
// CPU as csrc/frmle_host.h launches them -- the schedules of csrc/frmle_plan.h (for MSM_FRMLE_LOW_FIRST in place: the lower outputs into scratch
// rows, the upper ones in place, the copy home), launch after launch, and within a launch the lane functions of csrc/frmle_kernels.h in an order
// the caller picks:
//   order 0   workgroups and lanes ascending
//   order 1   workgroups and lanes descending
//   order 2   workgroups interleaved: lane 0 of every workgroup, then lane 1 of every workgroup, ..
// A schedule that lets one launch store where another of its lanes reads gives different bytes in one of them.  Built with g++ -DFQ_CHECK, so
// every limb and value bound of csrc/fq29.h is asserted along the way.
//   frmle_low_harness fold  <low> <order> <apart> <n> <batch> <stride> <in> <out>
//        in: c[32] a[span];   out: a[span] as the call leaves it, then (apart) out[span], which began as words of 0xEEEEEEEE
//   frmle_low_harness round <low> <order> <n> <batch> <stride> <tile> <mont> <fold> <terms> <in> <out>
//        in: [fold_by[32]] terms[terms x 52] a[span];   out: values[D + 1] a[span] launches[1 word, in a 32-byte slot] levels[likewise]
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
using msm_frmle::LowLaunch;
using msm_frmle::LowSchedule;

static bool read_file(const char* path, std::vector<uint8_t>& out, size_t want) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  out.resize(want);
  const bool ok = want == 0 || fread(out.data(), 1, want, f) == want;
  fclose(f);
  return ok;
}
static bool write_file(const char* path, const std::vector<uint32_t>& words) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(words.data(), 4, words.size(), f) == words.size();
  fclose(f);
  return ok;
}
static std::vector<uint32_t> words_of(const uint8_t* bytes, size_t count) {
  std::vector<uint32_t> w(count * 8);
  if (count) memcpy(w.data(), bytes, count * 32);
  return w;
}
static size_t span(size_t n, size_t batch, size_t stride) { return (batch - 1) * stride + n; }

// the (workgroup, lane) pairs of a launch of `blocks` workgroups in the order asked for
struct Slot {
  uint32_t block, lane;
};
static std::vector<Slot> lanes_in_order(size_t blocks, int order) {
  std::vector<Slot> out;
  out.reserve(blocks * FRMLE_THREADS);
  if (order == 2) {
    for (uint32_t lane = 0; lane < FRMLE_THREADS; lane++)
      for (size_t b = 0; b < blocks; b++) out.push_back(Slot{(uint32_t)b, lane});
  } else {
    for (size_t b = 0; b < blocks; b++)
      for (uint32_t lane = 0; lane < FRMLE_THREADS; lane++) out.push_back(Slot{(uint32_t)b, lane});
    if (order == 1) std::vector<Slot>(out.rbegin(), out.rend()).swap(out);
  }
  return out;
}
// hipMemcpy2DAsync, device to device: `width` elements of every row
static void copy_rows(uint32_t* dst, size_t dst_stride, const uint32_t* src, size_t src_stride, size_t width, size_t batch) {
  for (size_t row = 0; row < batch; row++) memcpy(dst + row * dst_stride * 8, src + row * src_stride * 8, width * 32);
}

// one launch of k_frmle_fold over `count` outputs per row
static bool fold_launch(const FrmleFoldArgs& g, int order, uint32_t* out, const uint32_t* a, size_t count, size_t batch, size_t stride) {
  bool ok = true;
  const size_t blocks = (batch * count + FRMLE_THREADS - 1) / FRMLE_THREADS;
  for (const Slot& s : lanes_in_order(blocks, order)) {
    const size_t idx = (size_t)s.block * FRMLE_THREADS + s.lane;
    if (idx >= batch * count) continue;
    ok &= frm_fold_pair(g, idx / count, idx % count, count, stride, a, out);
  }
  return ok;
}
static int run_fold(int argc, char** argv) {
  if (argc != 10) return 2;
  const bool low = atoi(argv[2]) != 0, apart = atoi(argv[4]) != 0;
  const int order = atoi(argv[3]);
  const size_t n = (size_t)atoll(argv[5]), batch = (size_t)atoll(argv[6]), stride = (size_t)atoll(argv[7]);
  std::vector<uint8_t> in;
  if (!msm_frmle::power_of_two(n) || n < 2 || batch < 1 || stride < n || order < 0 || order > 2) return 2;
  if (!read_file(argv[8], in, 32 + span(n, batch, stride) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  std::vector<uint32_t> a = words_of(in.data() + 32, span(n, batch, stride));
  std::vector<uint32_t> other(apart ? a.size() : 0, 0xEEEEEEEEu);
  uint32_t* const out = apart ? other.data() : a.data();
  const size_t half = n / 2;
  bool ok = true;
  if (!low) {  // (csrc/frmle_host.h: fold_impl, branch by branch)
    const FrmleFoldArgs g = msm_frmle::plan_fold(f, in.data());
    ok = fold_launch(g, order, out, a.data(), half, batch, stride);
  } else if (apart) {
    const FrmleFoldArgs g = msm_frmle::plan_fold_low(f, in.data(), LowLaunch{0, (uint32_t)half, false}, stride);
    ok = fold_launch(g, order, out, a.data(), half, batch, stride);
  } else {
    const LowSchedule s = msm_frmle::plan_low_in_place(n);
    std::vector<uint32_t> scratch(batch * s.copy * 8 + 8, 0xDDDDDDDDu);
    for (const LowLaunch& l : s.launches) {
      const FrmleFoldArgs g = msm_frmle::plan_fold_low(f, in.data(), l, l.to_scratch ? s.copy : stride);
      ok &= fold_launch(g, order, l.to_scratch ? scratch.data() : out, a.data(), l.count, batch, stride);
    }
    if (s.copy) copy_rows(out, stride, scratch.data(), s.copy, s.copy, batch);
  }
  a.insert(a.end(), other.begin(), other.end());
  return write_file(argv[9], a) ? (ok ? 0 : 3) : 2;
}

// one launch of k_frmle_round<POINTS>: `tiles` workgroups, whose tile sums go to partial[t * all_tiles + k]
template <int POINTS>
static bool round_launch(const FrmleRoundArgs& g, int order, uint32_t* a, uint32_t half, uint32_t stride, uint32_t tiles, const uint32_t* terms, uint32_t* partial) {
  struct Acc {
    fq v[POINTS];
  };
  std::vector<Acc> acc((size_t)tiles * FRMLE_THREADS);
  std::vector<fq> slot(FRMLE_THREADS);
  bool ok = true;
  for (const Slot& s : lanes_in_order(tiles, order)) ok &= frm_round_lane<POINTS>(g, a, half, stride, s.block, s.lane, terms, acc[(size_t)s.block * FRMLE_THREADS + s.lane].v, partial);
  const uint32_t all_tiles = terms[FRMLE_TERM_WORDS * g.num_terms + FRMLE_LOW_TILES];
  for (uint32_t k = 0; k < tiles; k++) {
    for (int t = 0; t < POINTS; t++) {
      for (uint32_t lane = 0; lane < FRMLE_THREADS; lane++) slot[lane] = frm_exact(acc[(size_t)k * FRMLE_THREADS + lane].v[t]);
      for (uint32_t step = FRMLE_STEPS; step-- > 0;)
        for (uint32_t lane = 0; lane < (1u << step); lane++) frm_sum_step(slot.data(), step, lane);
      frm_store(partial, (size_t)t * all_tiles + k, slot[0]);
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
  if (argc != 13) return 2;
  const bool low = atoi(argv[2]) != 0;
  const int order = atoi(argv[3]);
  const size_t n = (size_t)atoll(argv[4]), batch = (size_t)atoll(argv[5]), stride = (size_t)atoll(argv[6]);
  const uint32_t tile = (uint32_t)atoi(argv[7]);
  const bool mont = atoi(argv[8]) != 0, fold = atoi(argv[9]) != 0;
  const size_t num_terms = (size_t)atoll(argv[10]);
  const size_t term_bytes = 52;
  if (!msm_frmle::power_of_two(n) || batch < 1 || stride < n || n < (fold ? 4u : 2u) || batch > FRMLE_MAX_ROWS || num_terms < 1 || num_terms > FRMLE_MAX_TERMS) return 2;
  if (tile < 2 || tile > FRMLE_TILE || !msm_frmle::power_of_two(tile) || order < 0 || order > 2) return 2;
  std::vector<uint8_t> in;
  const size_t head = (fold ? 32 : 0) + num_terms * term_bytes;
  if (!read_file(argv[11], in, head + span(n, batch, stride) * 32)) return 2;
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
  // (csrc/frmle_host.h: round_impl, line by line)
  std::vector<uint32_t> words;
  FrmleRoundArgs g = msm_frmle::plan_round(f, tile, terms, num_terms, batch, fold ? in.data() : nullptr, mont, words);
  std::vector<uint32_t> a = words_of(in.data() + head, span(n, batch, stride));
  const size_t half = fold ? n / 4 : n / 2;
  LowSchedule s;
  if (low && fold) s = msm_frmle::plan_low_fused(n);
  else s.launches.push_back(LowLaunch{0, (uint32_t)half, false});
  const uint32_t launch_tile = low && fold ? msm_frmle::low_fused_tile(tile) : tile;
  const std::vector<size_t> len = low && fold ? msm_frmle::plan_levels_low_fused(s, half, launch_tile, tile) : msm_frmle::plan_levels(half, tile);
  const size_t levels = len.size();
  std::vector<size_t> at(levels, 0);
  size_t level_words = 0;
  for (size_t l = 1; l < levels; l++) {
    at[l] = level_words;
    level_words += g.points * len[l] * 8;
  }
  msm_frmle::plan_round_launches(g, low, s, launch_tile, level_words - (levels > 1 ? at[1] : 0), words);
  std::vector<uint32_t> scratch(level_words + batch * s.copy * 8 + 8, 0xDDDDDDDDu);
  std::vector<uint32_t> values(FRMLE_POINTS * 8);
  uint32_t* const partial = levels > 1 ? scratch.data() + at[1] : values.data();
  uint32_t tile0 = 0;
  bool ok = true;
  for (size_t k = 0; k < s.launches.size(); k++) {
    const uint32_t* consts = words.data() + msm_frmle::low_block_words(num_terms) * k;
    const uint32_t tiles = msm_frmle::low_tiles(s.launches[k], launch_tile);
    uint32_t* const p = partial + 8 * (size_t)tile0;
    switch (g.points) {
      case 2: ok &= round_launch<2>(g, order, a.data(), (uint32_t)half, (uint32_t)stride, tiles, consts, p); break;
      case 3: ok &= round_launch<3>(g, order, a.data(), (uint32_t)half, (uint32_t)stride, tiles, consts, p); break;
      case 4: ok &= round_launch<4>(g, order, a.data(), (uint32_t)half, (uint32_t)stride, tiles, consts, p); break;
      default: ok &= round_launch<5>(g, order, a.data(), (uint32_t)half, (uint32_t)stride, tiles, consts, p); break;
    }
    tile0 += tiles;
  }
  if (s.copy) copy_rows(a.data(), stride, scratch.data() + level_words, s.copy, s.copy, batch);
  for (size_t l = 1; l < levels; l++)
    sum_level(tile, g.points, len[l], scratch.data() + at[l], l + 1 < levels ? scratch.data() + at[l + 1] : values.data());
  values.resize(g.points * 8);
  values.insert(values.end(), a.begin(), a.end());
  for (uint32_t v : {(uint32_t)(levels - 1 + s.launches.size()), (uint32_t)levels}) {
    values.push_back(v);
    values.insert(values.end(), 7, 0u);
  }
  return write_file(argv[12], values) ? (ok ? 0 : 3) : 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "fold")) return run_fold(argc, argv);
  if (!strcmp(argv[1], "round")) return run_round(argc, argv);
  return 2;
}
