// Polynomial opening over the scalar field (libmsm_frpoly.so, include/msm_frpoly.h), written once and instantiated per field: a unit
// (csrc/frpoly_<name>.hip) includes csrc/fq29.h over the field's constants (fr_<name>_constants.h) and then this file, inside its own MSM_FIELD_NS.
// Everything a lane does is an FQ_HD function, which the kernels at the bottom call and which the host program of tests/test_frpoly_host.py runs
// serially on the CPU with every bound of csrc/fq29.h asserted.
//
// Representation.  The data are x F: F = 1 (canonical) or F = 2^256 (MSM_FRPOLY_MONT256).  fq_mul(a, b) = a b / R, R = 2^261, so a point z that
// arrives as z R multiplies a stored value into a stored value: fq_mul(h F, z R) = h z F.  Horner's rule, the synthetic division and the linear
// combination are linear in the data, so nothing is converted; the host (csrc/frpoly_plan.h) hands every kernel its constants in that shape.
//   fold     a tile of level l to one word of level l + 1: sum_off x[off] z_l^off.  A lane runs Horner over its E = 4 elements (three products),
//            the 256 lane values are folded by a tree in LDS with the weights z_l^(4 width), width = 128 .. 1 -- eight constants w[k] =
//            z_l^(4 2^k) R in the kernel arguments.  Between two products a value is a lazy sum (csrc/fq29.h) that fq_norm keeps in limbs
//            below 2^29 + 8 and below 21 r in value; a tile's total is tidied (one product by 1) and stored canonical.
//   suffix   h[i] = x[i] + z h[i + 1] over a tile, out[i] = h[i + 1]: the lane values are scanned from the right by doubling between two LDS
//            buffers with the same eight weights, a lane takes h at its right-hand neighbour's first element from there and runs Horner once
//            more, storing as it goes.  The tile's carry-in -- h at the first element of the next tile, which is what the level above stored
//            for this tile -- enters as one more element at the in-tile offset `tile`.
//   dot      the fold with a second operand: sum_off a[off] b[off], raw products fq_mul(a, b) = a b F^2 / R summed canonically, and ONE product
//            by R^2 / F per tile that puts the total into the data's form; the levels above it are plain sums.
//   combine  out[i] = sum_k c[k] a[k][i], one lane per element, the c[k] R read from a small device buffer.
//   powers   out[i] = c g^i, one lane per four elements: the lane's first power from tables of 16 entries per 4 bits of the lane's number
//            (built by the host), the other three by products with g R.
//
// frv_load / frv_store / frv_add of csrc/frvec_kernels.h are restated here (frp_load ..): including that file would instantiate libmsm_frvec.so's
// four kernels in every unit of this library.
//
// A tile is FRPOLY_TILE = 1024 elements: 256 lanes of FRPOLY_E = 4 consecutive elements.  No kernel waits for another workgroup: the levels are
// launches of their own (csrc/frpoly_host.h).
#pragma once
#include <cstddef>
#include <cstdint>

#define FRPOLY_THREADS 256
#define FRPOLY_E 4
#define FRPOLY_TILE (FRPOLY_THREADS * FRPOLY_E)
#define FRPOLY_STEPS 8  // log2(FRPOLY_THREADS): the steps of the tree and of the doubling scan

#define FRPOLY_HORNER 0  // fold: sum x[off] z^off
#define FRPOLY_DOT 1     // fold: sum x[off] (y[off])

#define FRPOLY_MAX_ROWS 256     // combine: rows, and words / 8 of the constants buffer
#define FRPOLY_WINDOW_BITS 4    // powers: a table per 4 bits of the lane's number ...
#define FRPOLY_WINDOW_SIZE 16   // ... of 16 entries
#define FRPOLY_MAX_WINDOWS 6    // 2^26 elements are 2^24 lanes

// what the host plans (csrc/frpoly_plan.h) -- plain data, the same for every field's unit; every constant is 8 words, canonical
struct FrpolyLevelArgs {
  uint32_t tile;      // elements per tile in use (the test hook shrinks it), <= FRPOLY_TILE
  uint32_t mode;      // FRPOLY_HORNER, FRPOLY_DOT
  uint32_t second;    // dot, level 0: every element is multiplied by its element of b ...
  uint32_t shared_b;  // ... which is one row for every row of a
  uint32_t restore;   // dot, level 0: the tile's total times fix
  uint32_t z[8];      // z_l R
  uint32_t w[FRPOLY_STEPS][8];  // z_l^(4 2^k) R
  uint32_t fix[8];    // R^2 / F
};
struct FrpolyPowersArgs {
  uint32_t windows;  // tables in use: the lane numbers have 4 windows bits
  uint32_t g[8];     // g R
};

#if defined(__HIPCC__)
// what the host code (csrc/frpoly_host.h) knows of a field's unit
struct FrpolyOps {
  const uint32_t* r32;
  void (*fold)(unsigned blocks, hipStream_t st, const uint32_t* a, const uint32_t* b, uint32_t* totals, size_t n, uint32_t tiles, const FrpolyLevelArgs* g, uint32_t* err);
  void (*suffix)(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* values, size_t n, uint32_t tiles,
                 const FrpolyLevelArgs* g, uint32_t* err);
  void (*combine)(unsigned blocks, hipStream_t st, const uint32_t* a, const uint32_t* coeffs, uint32_t* out, size_t n, uint32_t batch, uint32_t* err);
  void (*powers)(unsigned blocks, hipStream_t st, uint32_t* out, size_t n, const uint32_t* tables, const FrpolyPowersArgs* p);
};
#endif

namespace MSM_FIELD_NS {

FQ_HD bool frp_words_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}
FQ_HD void frp_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FQ_HD void frp_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
// element `at` of a vector, exact and below r; false (and zero) where the stored value is not below r
FQ_HD bool frp_load(fq& x, const uint32_t* src, size_t at) {
  uint32_t w[8];
  frp_load_words(w, src, at);
  const bool ok = frp_words_below_r(w);
  x = ok ? fq_unpack(w) : fq_zero();
  return ok;
}
FQ_HD fq frp_trusted(const uint32_t* src, size_t at) {  // a word this library or its host code wrote: below r
  uint32_t w[8];
  frp_load_words(w, src, at);
  return fq_unpack(w);
}
FQ_HD void frp_store(uint32_t* dst, size_t at, const fq& x) {  // x exact, < 2r
  uint32_t w[8];
  fq_pack(w, fq_canonical(x));
  frp_store_words(dst, at, w);
}
FQ_HD fq frp_const(const uint32_t w[8]) { return fq_unpack(w); }

// a + b mod r for canonical a, b: one carry chain, one conditional subtraction.  Out: canonical.
FQ_HD fq frp_add(const fq& a, const fq& b) {
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
// a + b over the integers: a normal (limbs < 2^29 + 8) or lazy, b exact; out normal.  The value is the caller's to bound (< 21 r here).
FQ_HD fq frp_acc(const fq& a, const fq& b) { return fq_norm(fq_add(a, b)); }
FQ_HD fq frp_exact(const fq& x) { return fq_canonical(fq_tidy(x)); }  // normal, <= 84 r  ->  canonical

FQ_HD uint32_t frp_offset(uint32_t lane, int j) { return lane * FRPOLY_E + (uint32_t)j; }

// x[0] + z x[1] + z^2 x[2] + z^3 x[3]: canonical in, lazy out (limbs < 2^30, value < 3r)
FQ_HD fq frp_horner(const fq x[FRPOLY_E], const fq& z) {
  fq h = x[FRPOLY_E - 1];
#pragma unroll
  for (int j = FRPOLY_E - 2; j >= 0; j--) h = fq_add(x[j], fq_mul(h, z));
  return h;
}

// ---- 1. fold: eval, the way up of divide, dot ---------------------------------------------------------------------------------------------------
// Rows of n elements, tiled row by row: workgroup (row, k) owns the elements [k tile, (k + 1) tile) of its row.  Holes -- an in-tile offset >=
// tile under the hook, an index >= n -- count as 0.  The lane's value goes to slot[lane]: normal and < 3r (Horner), canonical (dot).
FQ_HD bool frp_fold_load(const FrpolyLevelArgs& g, size_t n, size_t row, size_t k, uint32_t lane, const uint32_t* a, const uint32_t* b, fq* slot) {
  bool ok = true;
  fq x[FRPOLY_E];
#pragma unroll
  for (int j = 0; j < FRPOLY_E; j++) {
    const size_t at = k * g.tile + frp_offset(lane, j);
    x[j] = fq_zero();
    if (frp_offset(lane, j) < g.tile && at < n) {
      ok &= frp_load(x[j], a, row * n + at);
      if (g.second) {
        fq y;
        ok &= frp_load(y, b, (g.shared_b ? 0 : row * n) + at);
        x[j] = fq_canonical(fq_mul(x[j], y));
      }
    }
  }
  if (g.mode == FRPOLY_DOT) slot[lane] = frp_add(frp_add(x[0], x[1]), frp_add(x[2], x[3]));
  else slot[lane] = fq_norm(frp_horner(x, frp_const(g.z)));
  return ok;
}
// slot[x] += z^(4 width) slot[x + width], x < width, width = 2^step = 128 .. 1; then slot[0] is the tile's total (Horner: normal, < 19r)
FQ_HD void frp_fold_step(const FrpolyLevelArgs& g, fq* slot, uint32_t step, uint32_t x) {
  const uint32_t width = 1u << step;
  if (g.mode == FRPOLY_DOT) slot[x] = frp_add(slot[x], slot[x + width]);
  else slot[x] = frp_acc(slot[x], fq_mul(slot[x + width], frp_const(g.w[step])));
}
FQ_HD void frp_fold_store(const FrpolyLevelArgs& g, const fq* slot, uint32_t* totals, size_t at) {
  if (g.mode == FRPOLY_DOT) frp_store(totals, at, g.restore ? fq_mul(slot[0], frp_const(g.fix)) : slot[0]);
  else frp_store(totals, at, fq_tidy(slot[0]));
}

// ---- 2. suffix scan: the way down of divide -----------------------------------------------------------------------------------------------------
struct FrpSuffixLane {
  fq x[FRPOLY_E];  // the lane's elements; a hole is 0, the slot at the in-tile offset `tile` holds the carry-in
  fq seed;         // the carry-in where that offset is past the last lane (tile = FRPOLY_TILE): h at the end of the last lane
  uint32_t live;   // bit j: element j is stored;  bit 8: the seed is set
};
// carry: the level above's output for this row (NULL at the top level: 0).  The lane's value, normal and < 5r, goes to buf[lane].
FQ_HD bool frp_suffix_load(const FrpolyLevelArgs& g, size_t n, size_t row, size_t k, size_t tiles, uint32_t lane, const uint32_t* in, const uint32_t* carry,
                           FrpSuffixLane& s, fq* buf) {
  bool ok = true;
  s.live = 0;
#pragma unroll
  for (int j = 0; j < FRPOLY_E; j++) {
    const uint32_t off = frp_offset(lane, j);
    const size_t at = k * g.tile + off;
    s.x[j] = fq_zero();
    if (off < g.tile && at < n) {
      ok &= frp_load(s.x[j], in, row * n + at);
      s.live |= 1u << j;
    } else if (off == g.tile && carry) {
      s.x[j] = frp_trusted(carry, row * tiles + k);
    }
  }
  fq h = frp_horner(s.x, frp_const(g.z));
  s.seed = fq_zero();
  if (carry && g.tile == FRPOLY_TILE && lane == FRPOLY_THREADS - 1) {
    s.seed = frp_trusted(carry, row * tiles + k);
    s.live |= 0x100u;
    h = fq_add(h, fq_mul(s.seed, frp_const(g.w[0])));  // (limbs < 2^30 + 2^29: fq_norm takes them)
  }
  buf[lane] = fq_norm(h);
  return ok;
}
// a suffix scan of the lane values, doubling the distance d = 2^step from one buffer into the other (src and dst differ): normal, < 21r
FQ_HD void frp_suffix_step(const FrpolyLevelArgs& g, const fq* src, fq* dst, uint32_t step, uint32_t lane) {
  const uint32_t d = 1u << step;
  dst[lane] = lane + d < FRPOLY_THREADS ? frp_acc(src[lane], fq_mul(src[lane + d], frp_const(g.w[step]))) : src[lane];
}
// scan[lane]: h at the lane's first element.  values (NULL below the top level): receives h[0] of the row, the polynomial's value.
FQ_HD void frp_suffix_store(const FrpolyLevelArgs& g, size_t n, size_t row, size_t k, uint32_t lane, const FrpSuffixLane& s, const fq* scan, uint32_t* out,
                            uint32_t* values) {
  if (values && k == 0 && lane == 0) frp_store(values, row, fq_tidy(scan[0]));
  if (!(s.live & 0xffu)) return;
  fq h = fq_zero();  // h behind the lane's last element
  if (lane + 1 < FRPOLY_THREADS) h = frp_exact(scan[lane + 1]);
  if (s.live & 0x100u) h = s.seed;
  const fq z = frp_const(g.z);
#pragma unroll
  for (int j = FRPOLY_E - 1; j >= 0; j--) {
    if ((s.live >> j) & 1u) frp_store(out, row * n + k * g.tile + frp_offset(lane, j), h);
    if (j) h = frp_add(s.x[j], fq_canonical(fq_mul(h, z)));
  }
}

// ---- 3. combine ---------------------------------------------------------------------------------------------------------------------------------
// element i: out[i] = sum_k c[k] a[k][i]; coeffs holds the c[k] R.  The sum is lazy (normal limbs), tidied every eight terms: < 18r.
FQ_HD bool frp_combine_element(size_t i, size_t n, uint32_t batch, const uint32_t* a, const uint32_t* coeffs, uint32_t* out) {
  bool ok = true;
  fq acc = fq_zero();
  for (uint32_t k = 0; k < batch; k++) {
    fq x;
    ok &= frp_load(x, a, (size_t)k * n + i);
    const fq t = fq_mul(x, frp_trusted(coeffs, k));
    acc = k ? frp_acc(acc, t) : t;
    if (k && ((k & 7u) == 7u || k == batch - 1)) acc = fq_tidy(acc);
  }
  frp_store(out, i, acc);
  return ok;
}

// ---- 4. powers ----------------------------------------------------------------------------------------------------------------------------------
// lane: out[4 lane + j] = c g^(4 lane + j).  tables[16 w + d]: c g^(4 d) F for w = 0, g^(4 16^w d) R above.
FQ_HD void frp_powers_lane(const FrpolyPowersArgs& p, size_t lane, size_t n, const uint32_t* tables, uint32_t* out) {
  const size_t first = lane * FRPOLY_E;
  if (first >= n) return;
  fq acc = frp_trusted(tables, lane & (FRPOLY_WINDOW_SIZE - 1));
  for (uint32_t w = 1; w < p.windows; w++) {
    const uint32_t d = (uint32_t)(lane >> (FRPOLY_WINDOW_BITS * w)) & (FRPOLY_WINDOW_SIZE - 1);
    if (d) acc = fq_mul(acc, frp_trusted(tables, FRPOLY_WINDOW_SIZE * w + d));
  }
  const fq g = frp_const(p.g);
#pragma unroll
  for (int j = 0; j < FRPOLY_E; j++) {
    if (first + j < n) frp_store(out, first + j, acc);
    if (j < FRPOLY_E - 1) acc = fq_mul(acc, g);
  }
}

#if defined(__HIPCC__)
// block = row * tiles + k
__global__ void __launch_bounds__(FRPOLY_THREADS) k_frpoly_fold(const uint32_t* a, const uint32_t* b, uint32_t* totals, size_t n, uint32_t tiles, const FrpolyLevelArgs g,
                                                                uint32_t* err) {
  __shared__ uint32_t lds[FQ_LIMBS * FRPOLY_THREADS];
  fq* slot = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  const size_t row = blockIdx.x / tiles, k = blockIdx.x % tiles;
  if (!frp_fold_load(g, n, row, k, lane, a, b, slot)) atomicOr(err, 1u);
  for (uint32_t step = FRPOLY_STEPS; step-- > 0;) {
    __syncthreads();
    if (lane < (1u << step)) frp_fold_step(g, slot, step, lane);
  }
  __syncthreads();
  if (lane == 0) frp_fold_store(g, slot, totals, blockIdx.x);
}

// every input of the workgroup is read before its first store: in == out is safe
__global__ void __launch_bounds__(FRPOLY_THREADS) k_frpoly_suffix(const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* values, size_t n, uint32_t tiles,
                                                                  const FrpolyLevelArgs g, uint32_t* err) {
  __shared__ uint32_t lds[2 * FQ_LIMBS * FRPOLY_THREADS];
  fq* buf = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  const size_t row = blockIdx.x / tiles, k = blockIdx.x % tiles;
  FrpSuffixLane s;
  if (!frp_suffix_load(g, n, row, k, tiles, lane, in, carry, s, buf)) atomicOr(err, 1u);
  uint32_t from = 0;
  for (uint32_t step = 0; step < FRPOLY_STEPS; step++) {  // (8 steps: the result is back in the first buffer)
    __syncthreads();
    frp_suffix_step(g, buf + from * FRPOLY_THREADS, buf + (from ^ 1u) * FRPOLY_THREADS, step, lane);
    from ^= 1u;
  }
  __syncthreads();
  frp_suffix_store(g, n, row, k, lane, s, buf + from * FRPOLY_THREADS, out, values);
}

__global__ void __launch_bounds__(FRPOLY_THREADS) k_frpoly_combine(const uint32_t* a, const uint32_t* coeffs, uint32_t* out, size_t n, uint32_t batch, uint32_t* err) {
  const size_t i = (size_t)blockIdx.x * FRPOLY_THREADS + threadIdx.x;
  if (i >= n) return;
  if (!frp_combine_element(i, n, batch, a, coeffs, out)) atomicOr(err, 1u);
}

__global__ void __launch_bounds__(FRPOLY_THREADS) k_frpoly_powers(uint32_t* out, size_t n, const uint32_t* tables, const FrpolyPowersArgs p) {
  frp_powers_lane(p, (size_t)blockIdx.x * FRPOLY_THREADS + threadIdx.x, n, tables, out);
}

inline void frpoly_launch_fold(unsigned blocks, hipStream_t st, const uint32_t* a, const uint32_t* b, uint32_t* totals, size_t n, uint32_t tiles, const FrpolyLevelArgs* g,
                               uint32_t* err) {
  hipLaunchKernelGGL(k_frpoly_fold, dim3(blocks), dim3(FRPOLY_THREADS), 0, st, a, b, totals, n, tiles, *g, err);
}
inline void frpoly_launch_suffix(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* values, size_t n, uint32_t tiles,
                                 const FrpolyLevelArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frpoly_suffix, dim3(blocks), dim3(FRPOLY_THREADS), 0, st, in, out, carry, values, n, tiles, *g, err);
}
inline void frpoly_launch_combine(unsigned blocks, hipStream_t st, const uint32_t* a, const uint32_t* coeffs, uint32_t* out, size_t n, uint32_t batch, uint32_t* err) {
  hipLaunchKernelGGL(k_frpoly_combine, dim3(blocks), dim3(FRPOLY_THREADS), 0, st, a, coeffs, out, n, batch, err);
}
inline void frpoly_launch_powers(unsigned blocks, hipStream_t st, uint32_t* out, size_t n, const uint32_t* tables, const FrpolyPowersArgs* p) {
  hipLaunchKernelGGL(k_frpoly_powers, dim3(blocks), dim3(FRPOLY_THREADS), 0, st, out, n, tables, *p);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS
