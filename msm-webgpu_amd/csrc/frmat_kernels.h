// Sparse matrix-vector products over the scalar field (libmsm_frmat.so, include/msm_frmat.h), written once and instantiated per field: a unit
// (csrc/frmat_<name>.hip) includes csrc/fq29.h over the field's constants (fr_<name>_constants.h) and then this file, inside its own MSM_FIELD_NS.
// Everything a lane does is an FQ_HD function, which the kernels at the bottom call and which the host program of tests/test_frmat_host.py runs
// serially on the CPU with every bound of csrc/fq29.h asserted.
//
// Representation.  x and y are a F: F = 1 (canonical) or F = 2^256 (MSM_FRMAT_MONT256).  The matrix values are stored as v R, R = 2^261 the
// device's Montgomery radix, so fq_mul(v R, x F) = v x F: the product is in the form of x whichever that is, and no kernel knows the form.
//
// A LEVEL is a list of n entries in row order with the row of every entry beside it (row_of[n], non-decreasing): level 0 is the matrix -- entry
// e is values[e] x[col[e]] --, level l + 1 the partial sums that level l could not finish (below).  A workgroup of 256 lanes owns a TILE of 1024
// consecutive entries, 4 consecutive ones to a lane, whatever rows they belong to: 1024 rows of one entry or a slice of one row are the same work.
//   the lane   loads its four columns and rows with one 16-byte load each, its four values with two each, gathers x[col] (32 bytes, compared
//              with r by this lane), multiplies, and adds lazily while the row does not change.  The entries of a lane form RUNS of equal row:
//              the first (head) may continue a run of the lanes before, the last (tail) may go on in the lanes behind, the ones in between lie
//              wholly inside the lane and are stored to y at once.  A lane with one run has head == tail.
//   the scan   slot[lane] = the lane's last run, flag[lane] = "that run starts in this lane"; an inclusive segmented scan over the 256 slots
//              (Hillis-Steele, 8 steps, canonical sums) leaves in slot[lane] the sum of the run that ends lane `lane`, from its start or the
//              tile's.  A run is stored by the lane in which it ends (the next entry has another row, or the tile ends): the last run's total is
//              slot[lane], the head's -- where another run follows it in the lane -- slot[lane - 1] + head.
//   the store  a run of a row that lies wholly inside the tile goes to y[row].  The tile's first run, where its row began before the tile, and
//              its last, where the row goes on behind it, go to the level's partials instead, at the slots the plan (csrc/frmat_plan.h) wrote
//              into the tile's two words of `slots`: the partials of one row are consecutive, in tile order, and with their rows they are the
//              next level.  A level without such rows is the last.  Nothing is added into memory: every word of y and of the partials has one
//              writer, and every sum has one fixed order.
// Rows without entries and y[rows .. y_len) are zero because the host clears y on the stream first.
//
// The bounds, for the tightest field (BLS12-381: FQ_HEADROOM = 70): a product of a stored value (canonical, < r) and an element of x (checked,
// < r) is r^2 <= 70 r^2, exact, < 2r.  A run inside a lane adds at most FRMAT_E such products lazily, with fq_norm after every addition (limbs
// < 2^29 + 8): < 2 FRMAT_E r = 8r <= 70r, which fq_tidy takes.  Everything that reaches LDS, the partials or y is canonical, and sums of canonical
// values are taken with one carry chain and one conditional subtraction (frt_add).  The static_assert below holds the lane's bound; the host
// program runs the pattern that reaches it (all values and all of x r - 1, one row over a full tile) under FQ_CHECK.
//
// frm_load / frm_store / frm_add of csrc/frmle_kernels.h are restated here (frt_load ..): including that file would instantiate libmsm_frmle.so's
// kernels in every unit of this library.
//
// LDS: k_frmat_tile and k_frmat_stitch 10240 bytes each (256 slots of nine limbs, 256 flags); k_frmat_lift none.  No kernel waits for another
// workgroup: the levels are launches of their own (csrc/frmat_host.h).
#pragma once
#include <cstddef>
#include <cstdint>

#define FRMAT_THREADS 256
#define FRMAT_E 4
#define FRMAT_TILE (FRMAT_THREADS * FRMAT_E)
#define FRMAT_NONE 0xffffffffu  // slots: the run goes to y
#define FRMAT_RESULT_HEAD 8     // the result buffer: the error word and seven words of padding

// what the host plans (csrc/frmat_plan.h) -- plain data, the same for every field's unit
struct FrmatLevelArgs {
  uint32_t tile;     // entries per tile in use (the test hook shrinks it), a power of two <= FRMAT_TILE
  uint32_t n;        // entries of this level, >= 1
  uint32_t aligned;  // tile % 4 == 0: a lane's four columns and rows are one 16-byte word (the arrays are padded to a multiple of four)
};

#if defined(__HIPCC__)
// what the host code (csrc/frmat_host.h) knows of a field's unit
struct FrmatOps {
  const uint32_t* r32;
  void (*lift)(unsigned blocks, hipStream_t st, uint32_t* values, size_t n);
  void (*tile)(unsigned blocks, hipStream_t st, const uint32_t* values, const uint32_t* col, const uint32_t* row_of, const uint32_t* slots, const uint32_t* x, uint32_t* y,
               uint32_t* part, const FrmatLevelArgs* g, uint32_t* err);
  void (*stitch)(unsigned blocks, hipStream_t st, const uint32_t* in, const uint32_t* row_of, const uint32_t* slots, uint32_t* y, uint32_t* part, const FrmatLevelArgs* g);
};
#endif

namespace MSM_FIELD_NS {

static_assert(2 * FRMAT_E <= FQ_HEADROOM, "a lane's lazy sum (FRMAT_E products of < 2r each) does not fit fq_tidy");

FQ_HD bool frt_words_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}
FQ_HD void frt_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FQ_HD void frt_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
// element `at` of a vector, exact and below r; false (and zero) where the stored value is not below r
FQ_HD bool frt_load(fq& x, const uint32_t* src, size_t at) {
  uint32_t w[8];
  frt_load_words(w, src, at);
  const bool ok = frt_words_below_r(w);
  x = ok ? fq_unpack(w) : fq_zero();
  return ok;
}
FQ_HD fq frt_trusted(const uint32_t* src, size_t at) {  // a word this library or its host code wrote: below r
  uint32_t w[8];
  frt_load_words(w, src, at);
  return fq_unpack(w);
}
FQ_HD void frt_store(uint32_t* dst, size_t at, const fq& x) {  // x canonical
  uint32_t w[8];
  fq_pack(w, x);
  frt_store_words(dst, at, w);
}
// a + b mod r for canonical a, b: one carry chain, one conditional subtraction.  Out: canonical.
FQ_HD fq frt_add(const fq& a, const fq& b) {
  fq t;
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < FQ_L; i++) {
    const uint32_t s = a.v[i] + b.v[i] + carry;
    t.v[i] = i < FQ_L - 1 ? (s & FQ_MASK) : s;
    carry = s >> FQ_W;
  }
  return fq_canonical(t);
}
// a lazy sum: a normal (limbs < 2^29 + 8), b exact or normal; out normal.  The value is the caller's to bound.
FQ_HD fq frt_acc(const fq& a, const fq& b) { return fq_norm(fq_add(a, b)); }
FQ_HD fq frt_exact(const fq& x) { return fq_canonical(fq_tidy(x)); }  // normal, <= FQ_HEADROOM r  ->  canonical

// ---- 0. lift: the values of the matrix, v -> v R, once, in place -----------------------------------------------------------------------------------
FQ_HD void frt_lift_entry(uint32_t* values, size_t e) { frt_store(values, e, fq_to_mont(frt_trusted(values, e))); }  // (the host checked v < r)

// ---- 1. the lane --------------------------------------------------------------------------------------------------------------------------------------
// four consecutive words of an index array from `first` on: one 16-byte load where the tile allows it, else word by word (never past `last`)
FQ_HD void frt_load4(uint32_t out[FRMAT_E], const uint32_t* src, uint32_t first, uint32_t last, bool aligned) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (aligned) {
    const uint4 q = reinterpret_cast<const uint4*>(src)[first / FRMAT_E];
    out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
    return;
  }
#else
  (void)aligned;
#endif
#pragma unroll
  for (uint32_t j = 0; j < FRMAT_E; j++) out[j] = src[first + j < last ? first + j : last];
}

// what a lane keeps between its entries and the end of the scan
struct FrtSeg {
  fq head, tail;       // canonical: the first run; the last run (the same run, and the same value, where the lane has one)
  uint32_t head_row, tail_row;
  uint32_t runs;       // 0: the lane has no entry; 1; 2: two or more
  uint32_t carry;      // the head continues the run that ends the lane before
  uint32_t next_row;   // the row of the entry behind the lane's last, FRMAT_NONE where the tile or the level ends there
};

// The lane's entries of tile k: in-tile offsets FRMAT_E lane .. + 3, as far as the tile and the level go.  MUL: level 0 (in = the values, col and
// x in use), else a level of partials (in = the partials; canonical words this library wrote).  Stores the runs that lie inside the lane to y.
template <bool MUL>
FQ_HD bool frt_lane(const FrmatLevelArgs& g, uint32_t k, uint32_t lane, const uint32_t* in, const uint32_t* col, const uint32_t* row_of, const uint32_t* x, uint32_t* y,
                    FrtSeg& seg) {
  const uint32_t off = lane * FRMAT_E, start = k * g.tile, first = start + off;
  seg.runs = 0, seg.carry = 0, seg.next_row = FRMAT_NONE, seg.head_row = seg.tail_row = FRMAT_NONE;
  seg.head = seg.tail = fq_zero();
  if (off >= g.tile || first >= g.n) return true;
  const uint32_t end = start + g.tile < g.n ? start + g.tile : g.n;  // the tile's entries are [start, end)
  const uint32_t cnt = end - first < FRMAT_E ? end - first : FRMAT_E;
  uint32_t rw[FRMAT_E], cl[FRMAT_E];
  frt_load4(rw, row_of, first, g.n - 1, g.aligned != 0);
  if (MUL) frt_load4(cl, col, first, g.n - 1, g.aligned != 0);
  if (off && row_of[first - 1] == rw[0]) seg.carry = 1;
  if (first + cnt < end) seg.next_row = row_of[first + cnt];
  bool ok = true;
  fq term[FRMAT_E];
#pragma unroll
  for (uint32_t j = 0; j < FRMAT_E; j++) {  // (an entry the lane does not have repeats its first: the loads are unconditional, nothing new is read)
    const uint32_t e = j < cnt ? first + j : first;
    if (MUL) {
      fq xv;
      ok &= frt_load(xv, x, j < cnt ? cl[j] : cl[0]);
      term[j] = fq_mul(frt_trusted(in, e), xv);
    } else {
      term[j] = frt_trusted(in, e);
    }
  }
  fq acc = term[0];
  uint32_t cur = rw[0];
#pragma unroll
  for (uint32_t j = 1; j < FRMAT_E; j++) {
    if (j >= cnt) break;
    if (rw[j] == cur) {
      acc = frt_acc(acc, term[j]);
      continue;
    }
    const fq done = frt_exact(acc);
    if (seg.runs == 0) {
      seg.head = done, seg.head_row = cur;
    } else {
      frt_store(y, cur, done);  // between the lane's first and last rows: wholly inside the lane
    }
    seg.runs = 2, acc = term[j], cur = rw[j];
  }
  if (seg.runs == 0) {
    seg.runs = 1, seg.head = seg.tail = frt_exact(acc), seg.head_row = seg.tail_row = cur;
  } else {
    seg.tail = frt_exact(acc), seg.tail_row = cur;
  }
  return ok;
}

// ---- 2. the scan --------------------------------------------------------------------------------------------------------------------------------------
FQ_HD void frt_publish(const FrtSeg& seg, uint32_t lane, fq* slot, uint32_t* flag) {
  slot[lane] = seg.tail;  // (no entry: zero)
  flag[lane] = seg.runs != 1 || !seg.carry;
}
// step d = 1, 2, .. 128, for the lanes >= d: take (all lanes), then put (all lanes).  Run serially, lanes in DESCENDING order may take and put in one go.
FQ_HD void frt_scan_take(const fq* slot, const uint32_t* flag, uint32_t d, uint32_t lane, fq& v, uint32_t& f) { v = slot[lane - d], f = flag[lane - d]; }
FQ_HD void frt_scan_put(fq* slot, uint32_t* flag, uint32_t lane, const fq& v, uint32_t f) {
  if (flag[lane]) return;
  slot[lane] = frt_add(slot[lane], v);
  flag[lane] = f;
}

// ---- 3. the store -------------------------------------------------------------------------------------------------------------------------------------
// a finished run of the tile: to the partials where its row goes on outside the tile, else to y
FQ_HD void frt_emit(uint32_t row, const fq& v, uint32_t first_row, uint32_t last_row, uint32_t head_slot, uint32_t tail_slot, uint32_t* y, uint32_t* part) {
  if (head_slot != FRMAT_NONE && row == first_row) {
    frt_store(part, head_slot, v);
  } else if (tail_slot != FRMAT_NONE && row == last_row) {
    frt_store(part, tail_slot, v);
  } else {
    frt_store(y, row, v);
  }
}
// after the scan: the lane stores the runs that end in it
FQ_HD void frt_finish(const FrmatLevelArgs& g, uint32_t k, uint32_t lane, const FrtSeg& seg, const fq* slot, const uint32_t* row_of, const uint32_t* slots, uint32_t* y,
                      uint32_t* part) {
  if (seg.runs == 0) return;
  const uint32_t start = k * g.tile, end = start + g.tile < g.n ? start + g.tile : g.n;
  const uint32_t first_row = row_of[start], last_row = row_of[end - 1], head_slot = slots[2 * k], tail_slot = slots[2 * k + 1];
  if (seg.runs == 2) {
    fq head = seg.head;
    if (seg.carry) head = frt_add(slot[lane - 1], head);
    frt_emit(seg.head_row, head, first_row, last_row, head_slot, tail_slot, y, part);
    if (seg.next_row != seg.tail_row) frt_emit(seg.tail_row, slot[lane], first_row, last_row, head_slot, tail_slot, y, part);
  } else if (seg.next_row != seg.head_row) {
    frt_emit(seg.head_row, slot[lane], first_row, last_row, head_slot, tail_slot, y, part);
  }
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(FRMAT_THREADS) k_frmat_lift(uint32_t* values, size_t n) {
  const size_t e = (size_t)blockIdx.x * FRMAT_THREADS + threadIdx.x;
  if (e < n) frt_lift_entry(values, e);
}

// the part of a tile behind the lane's entries: the scan and the stores (all 256 lanes come here)
__device__ __forceinline__ void frt_tile_tail(const FrmatLevelArgs& g, const FrtSeg& seg, fq* slot, uint32_t* flag, const uint32_t* row_of, const uint32_t* slots, uint32_t* y,
                                              uint32_t* part) {
  const uint32_t lane = threadIdx.x;
  frt_publish(seg, lane, slot, flag);
#pragma unroll 1
  for (uint32_t d = 1; d < FRMAT_THREADS; d <<= 1) {
    fq v = fq_zero();
    uint32_t f = 0;
    __syncthreads();
    if (lane >= d) frt_scan_take(slot, flag, d, lane, v, f);
    __syncthreads();
    if (lane >= d) frt_scan_put(slot, flag, lane, v, f);
  }
  __syncthreads();
  frt_finish(g, blockIdx.x, lane, seg, slot, row_of, slots, y, part);
}

// block = tile k of level 0
__global__ void __launch_bounds__(FRMAT_THREADS) k_frmat_tile(const uint32_t* values, const uint32_t* col, const uint32_t* row_of, const uint32_t* slots, const uint32_t* x,
                                                              uint32_t* y, uint32_t* part, const FrmatLevelArgs g, uint32_t* err) {
  __shared__ uint32_t lds[FQ_LIMBS * FRMAT_THREADS];
  __shared__ uint32_t flag[FRMAT_THREADS];
  FrtSeg seg;
  if (!frt_lane<true>(g, blockIdx.x, threadIdx.x, values, col, row_of, x, y, seg)) atomicOr(err, 1u);
  frt_tile_tail(g, seg, reinterpret_cast<fq*>(lds), flag, row_of, slots, y, part);
}

// block = tile k of a level of partials
__global__ void __launch_bounds__(FRMAT_THREADS) k_frmat_stitch(const uint32_t* in, const uint32_t* row_of, const uint32_t* slots, uint32_t* y, uint32_t* part,
                                                                const FrmatLevelArgs g) {
  __shared__ uint32_t lds[FQ_LIMBS * FRMAT_THREADS];
  __shared__ uint32_t flag[FRMAT_THREADS];
  FrtSeg seg;
  (void)frt_lane<false>(g, blockIdx.x, threadIdx.x, in, nullptr, row_of, nullptr, y, seg);
  frt_tile_tail(g, seg, reinterpret_cast<fq*>(lds), flag, row_of, slots, y, part);
}

inline void frmat_launch_lift(unsigned blocks, hipStream_t st, uint32_t* values, size_t n) { hipLaunchKernelGGL(k_frmat_lift, dim3(blocks), dim3(FRMAT_THREADS), 0, st, values, n); }
inline void frmat_launch_tile(unsigned blocks, hipStream_t st, const uint32_t* values, const uint32_t* col, const uint32_t* row_of, const uint32_t* slots, const uint32_t* x,
                              uint32_t* y, uint32_t* part, const FrmatLevelArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frmat_tile, dim3(blocks), dim3(FRMAT_THREADS), 0, st, values, col, row_of, slots, x, y, part, *g, err);
}
inline void frmat_launch_stitch(unsigned blocks, hipStream_t st, const uint32_t* in, const uint32_t* row_of, const uint32_t* slots, uint32_t* y, uint32_t* part,
                                const FrmatLevelArgs* g) {
  hipLaunchKernelGGL(k_frmat_stitch, dim3(blocks), dim3(FRMAT_THREADS), 0, st, in, row_of, slots, y, part, *g);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS
