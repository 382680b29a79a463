// Stand-alone host program for tests/test_frmat_host.py: libmsm_frmat.so's product run on the CPU -- the checks, the transposed structure, the
// levels and the tiles' slots of csrc/frmat_plan.h, and per lane the very functions the kernels of csrc/frmat_kernels.h call, one "workgroup"
// after the other, with the kernels' own order of steps.  Built with g++ -DFQ_CHECK, so every limb and value bound of csrc/fq29.h is asserted
// along the way.
//   frmat_harness mul       <rows> <cols> <nnz> <tile> <transpose> <y_len> <in> <out>
//        in: row_ptr[rows + 1] col_idx[nnz] (32-bit words) values[nnz x 32] x[cols x 32, or rows x 32 with transpose]
//        out: eight words -- launches, levels, six of padding -- then y[y_len x 32]
//   frmat_harness transpose <rows> <cols> <nnz> <in> <out>
//        in: row_ptr[rows + 1] col_idx[nnz];  out: t_ptr[cols + 1] t_idx[nnz] from[nnz]
//   exit status: 0 ok, 3 a value or an element of x that is read >= r, 4 the matrix is rejected by the plan's checks, 2 bad arguments
// Compile with -DMSM_FIELD_NS=frt_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frmat_kernels.h"
#include "frmat_plan.h"

using namespace MSM_FIELD_NS;

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
  const bool ok = words.empty() || fwrite(words.data(), 4, words.size(), f) == words.size();
  fclose(f);
  return ok;
}
static std::vector<uint32_t> words_of(const uint8_t* bytes, size_t words) {
  std::vector<uint32_t> w(words);
  if (words) memcpy(w.data(), bytes, words * 4);
  return w;
}

// one launch of k_frmat_tile (MUL) or k_frmat_stitch
template <bool MUL>
static bool run_level(const frmat::Level& lv, uint32_t tile, const uint32_t* in, const uint32_t* col, const uint32_t* x, uint32_t* y, uint32_t* part) {
  const FrmatLevelArgs g = frmat::level_args(lv, tile);
  std::vector<FrtSeg> seg(FRMAT_THREADS);
  std::vector<fq> slot(FRMAT_THREADS);
  std::vector<uint32_t> flag(FRMAT_THREADS);
  bool ok = true;
  for (uint32_t k = 0; k < lv.tiles; k++) {
    for (uint32_t lane = 0; lane < FRMAT_THREADS; lane++) {
      ok &= frt_lane<MUL>(g, k, lane, in, col, lv.row_of.data(), x, y, seg[lane]);
      frt_publish(seg[lane], lane, slot.data(), flag.data());
    }
    for (uint32_t d = 1; d < FRMAT_THREADS; d <<= 1)
      for (uint32_t lane = FRMAT_THREADS; lane-- > d;) {  // (descending: lane - d still holds the step's input)
        fq v;
        uint32_t f;
        frt_scan_take(slot.data(), flag.data(), d, lane, v, f);
        frt_scan_put(slot.data(), flag.data(), lane, v, f);
      }
    for (uint32_t lane = 0; lane < FRMAT_THREADS; lane++) frt_finish(g, k, lane, seg[lane], slot.data(), lv.row_of.data(), lv.slots.data(), y, part);
  }
  return ok;
}

static int run_mul(int argc, char** argv) {
  if (argc != 10) return 2;
  const size_t rows = (size_t)atoll(argv[2]), cols = (size_t)atoll(argv[3]), nnz = (size_t)atoll(argv[4]);
  const uint32_t tile = (uint32_t)atoi(argv[5]);
  const bool transpose = atoi(argv[6]) != 0;
  const size_t y_len = (size_t)atoll(argv[7]);
  const size_t in_len = transpose ? rows : cols, out_len = transpose ? cols : rows;
  if (tile < 2 || tile > FRMAT_TILE || (tile & (tile - 1)) || rows < 1 || cols < 1 || y_len < out_len) return 2;
  std::vector<uint8_t> in;
  if (!read_file(argv[8], in, (rows + 1 + nnz) * 4 + (nnz + in_len) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  std::vector<uint32_t> ptr = words_of(in.data(), rows + 1), idx = words_of(in.data() + (rows + 1) * 4, nnz);
  const uint8_t* vbytes = in.data() + (rows + 1 + nnz) * 4;
  const frmat::Check c = frmat::check_matrix(f, rows, cols, nnz, ptr.data(), idx.data(), vbytes);
  if (c != frmat::CHECK_OK) return c == frmat::CHECK_NONCANONICAL ? 3 : 4;
  std::vector<uint32_t> values = words_of(vbytes, nnz * 8);
  const std::vector<uint32_t> x = words_of(vbytes + nnz * 32, in_len * 8);
  if (transpose) {
    std::vector<uint32_t> t_ptr, t_idx, from, moved(nnz * 8);
    frmat::transpose_csr(rows, cols, ptr.data(), idx.data(), t_ptr, t_idx, from);
    for (size_t e = 0; e < nnz; e++) memcpy(moved.data() + 8 * e, values.data() + 8 * from[e], 32);
    ptr.swap(t_ptr), idx.swap(t_idx), values.swap(moved);
  }
  for (size_t e = 0; e < nnz; e++) frt_lift_entry(values.data(), e);  // k_frmat_lift
  const std::vector<frmat::Level> levels = frmat::plan_levels(frmat::expand_rows(out_len, ptr.data()), tile);
  std::vector<uint32_t> out(8 + y_len * 8, 0xffffffffu);
  out[0] = (uint32_t)frmat::planned_launches(levels), out[1] = (uint32_t)levels.size();
  uint32_t* y = out.data() + 8;
  memset(y, 0, y_len * 32);  // the fill
  bool ok = true;
  std::vector<std::vector<uint32_t>> part(levels.size());
  for (size_t l = 0; l < levels.size(); l++) {
    part[l].assign(levels[l].next.size() * 8, 0xffffffffu);
    if (l == 0) {
      ok &= run_level<true>(levels[0], tile, values.data(), idx.data(), x.data(), y, part[0].data());
    } else {
      ok &= run_level<false>(levels[l], tile, part[l - 1].data(), nullptr, nullptr, y, part[l].data());
    }
  }
  return write_file(argv[9], out) ? (ok ? 0 : 3) : 2;
}

static int run_transpose(int argc, char** argv) {
  if (argc != 7) return 2;
  const size_t rows = (size_t)atoll(argv[2]), cols = (size_t)atoll(argv[3]), nnz = (size_t)atoll(argv[4]);
  std::vector<uint8_t> in;
  if (rows < 1 || cols < 1 || !read_file(argv[5], in, (rows + 1 + nnz) * 4)) return 2;
  const std::vector<uint32_t> ptr = words_of(in.data(), rows + 1), idx = words_of(in.data() + (rows + 1) * 4, nnz);
  const host_fr::Field f(FQ_P32);
  const std::vector<uint8_t> zeros(nnz * 32 + 1, 0);
  if (frmat::check_matrix(f, rows, cols, nnz, ptr.data(), idx.data(), zeros.data()) != frmat::CHECK_OK) return 4;
  std::vector<uint32_t> t_ptr, t_idx, from;
  frmat::transpose_csr(rows, cols, ptr.data(), idx.data(), t_ptr, t_idx, from);
  t_ptr.insert(t_ptr.end(), t_idx.begin(), t_idx.end());
  t_ptr.insert(t_ptr.end(), from.begin(), from.end());
  return write_file(argv[6], t_ptr) ? 0 : 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "mul")) return run_mul(argc, argv);
  if (!strcmp(argv[1], "transpose")) return run_transpose(argc, argv);
  return 2;
}
