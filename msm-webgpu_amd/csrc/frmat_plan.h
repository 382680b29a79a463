// The host side of libmsm_frmat.so that needs no HIP: the checks of a matrix, its transposed structure, the row of every entry, and per level the
// tiles' partial slots and the rows that cross tiles (csrc/frmat_host.h uploads and launches what this plans; the host program of
// tests/test_frmat_host.py runs the same plan through the same per-lane code on the CPU).  Needs FRMAT_NONE and FrmatLevelArgs of
// csrc/frmat_kernels.h.
#pragma once
#include <cstring>
#include <vector>

#include "host_fr.h"

namespace frmat {

using host_fr::Field;

constexpr size_t MAX_DIM = (size_t)1 << 26;
constexpr size_t MAX_NNZ = (size_t)1 << 28;
enum Check { CHECK_OK = 0, CHECK_INVALID = 1, CHECK_NONCANONICAL = 2 };

inline bool below_r(const Field& f, const uint8_t c[32]) { return !Field::geq(host_fr::load32(c), f.modulus()); }

// everything include/msm_frmat.h promises of a matrix: the limits, row_ptr from 0 to nnz without a step down, the columns below cols, the values
// below r (the structure first: a matrix with both faults is INVALID)
inline Check check_matrix(const Field& f, size_t rows, size_t cols, size_t nnz, const uint32_t* row_ptr, const uint32_t* col_idx, const uint8_t* values) {
  if (rows < 1 || rows > MAX_DIM || cols < 1 || cols > MAX_DIM || nnz > MAX_NNZ || !row_ptr) return CHECK_INVALID;
  if (nnz && (!col_idx || !values)) return CHECK_INVALID;
  if (row_ptr[0] != 0 || row_ptr[rows] != nnz) return CHECK_INVALID;
  for (size_t i = 0; i < rows; i++)
    if (row_ptr[i] > row_ptr[i + 1]) return CHECK_INVALID;
  for (size_t e = 0; e < nnz; e++)
    if (col_idx[e] >= cols) return CHECK_INVALID;
  for (size_t e = 0; e < nnz; e++)
    if (!below_r(f, values + 32 * e)) return CHECK_NONCANONICAL;
  return CHECK_OK;
}

// the row of every entry (4 bytes per entry on the device, read beside the column: a lane learns its rows without a search)
inline std::vector<uint32_t> expand_rows(size_t rows, const uint32_t* row_ptr) {
  std::vector<uint32_t> row_of(row_ptr[rows]);
  for (size_t i = 0; i < rows; i++)
    for (uint32_t e = row_ptr[i]; e < row_ptr[i + 1]; e++) row_of[e] = (uint32_t)i;
  return row_of;
}

// The CSR arrays of the transposed matrix by a counting sort over the columns: t_ptr[cols + 1], t_idx[nnz] (the rows, ascending within a
// column) and from[nnz], the entry of the matrix that entry e of the transposed one is.  Stable, so the order -- and with it every sum -- is fixed.
inline void transpose_csr(size_t rows, size_t cols, const uint32_t* row_ptr, const uint32_t* col_idx, std::vector<uint32_t>& t_ptr, std::vector<uint32_t>& t_idx,
                          std::vector<uint32_t>& from) {
  const size_t nnz = row_ptr[rows];
  t_ptr.assign(cols + 1, 0);
  for (size_t e = 0; e < nnz; e++) t_ptr[col_idx[e] + 1]++;
  for (size_t c = 0; c < cols; c++) t_ptr[c + 1] += t_ptr[c];
  std::vector<uint32_t> at(t_ptr.begin(), t_ptr.end() - 1);
  t_idx.resize(nnz);
  from.resize(nnz);
  for (size_t i = 0; i < rows; i++)
    for (uint32_t e = row_ptr[i]; e < row_ptr[i + 1]; e++) {
      const uint32_t to = at[col_idx[e]]++;
      t_idx[to] = (uint32_t)i;
      from[to] = e;
    }
}

// One level: n entries whose rows are row_of (non-decreasing), in ceil(n / tile) tiles.  slots[2 k] / slots[2 k + 1]: where tile k's first /
// last run goes among the level's partials -- FRMAT_NONE: to y.  The first run is a partial where its row has entries before the tile, the last
// where its row has entries behind it (one run that is both gets the first word only).  next: the rows of the partials, in slot order -- the
// partials of one row are consecutive --: the level above.  Empty: this level finishes every row.
struct Level {
  std::vector<uint32_t> row_of, slots, next;
  uint32_t tiles = 0;
};
inline Level plan_level(std::vector<uint32_t> row_of, uint32_t tile) {
  Level lv;
  const size_t n = row_of.size();
  lv.tiles = (uint32_t)((n + tile - 1) / tile);
  lv.slots.assign(2 * (size_t)lv.tiles, FRMAT_NONE);
  for (size_t k = 0; k < lv.tiles; k++) {
    const size_t s = k * tile, e = s + tile < n ? s + tile : n;
    const bool head = s > 0 && row_of[s - 1] == row_of[s], tail = e < n && row_of[e] == row_of[e - 1];
    if (head) {
      lv.slots[2 * k] = (uint32_t)lv.next.size();
      lv.next.push_back(row_of[s]);
    }
    if (tail && !(head && row_of[s] == row_of[e - 1])) {
      lv.slots[2 * k + 1] = (uint32_t)lv.next.size();
      lv.next.push_back(row_of[e - 1]);
    }
  }
  lv.row_of = std::move(row_of);
  return lv;
}
// every level of a structure: level 0 the entries, then the partials of the level below while there are any.  A level has at most
// 2 (tiles - 1) partials, fewer than its entries, so this ends: at the design's tile a level is 512 times shorter than the one below.
// No entries: no level.
inline std::vector<Level> plan_levels(std::vector<uint32_t> row_of, uint32_t tile) {
  std::vector<Level> levels;
  while (!row_of.empty()) {
    levels.push_back(plan_level(std::move(row_of), tile));
    row_of = levels.back().next;
  }
  return levels;
}
inline FrmatLevelArgs level_args(const Level& lv, uint32_t tile) { return FrmatLevelArgs{tile, (uint32_t)lv.row_of.size(), (uint32_t)(tile % 4 == 0)}; }
// a product is the fill of y and one launch per level
inline int planned_launches(const std::vector<Level>& levels) { return 1 + (int)levels.size(); }

}  // namespace frmat
