// Vector arithmetic over the scalar field (libmsm_frvec.so, include/msm_frvec.h), written once and instantiated per field: a unit
// (csrc/frvec_<name>.hip) includes csrc/fq29.h over the field's constants (fr_<name>_constants.h) and then this file, inside its own MSM_FIELD_NS.
// Everything a lane does is an FQ_HD function, which the kernels at the bottom call and which the host program of tests/test_frvec_host.py runs
// serially on the CPU with every bound of csrc/fq29.h asserted.
//
// Representation.  The data are x F: F = 1 (canonical) or F = 2^256 (MSM_FRVEC_MONT256).  fq_mul(a, b) = a b / R, R = 2^261, so a product of two
// stored values is not a stored value; the host (csrc/frvec_plan.h) hands every kernel the constants that put it right:
//   map      a vector times a vector: one more product by R^2 / F;  times a broadcast constant: the constant arrives as b R, nothing more.
//            Sums and differences are linear: a constant arrives as c F.
//   inverse  a stored value x F is read as the Montgomery form of u = x F / R, and Montgomery's trick runs on the u: it ends with u^-1 R =
//            x^-1 R^2 / F per element, which is x^-1 F times R^2 / F^2 -- a factor that the ONE inverse of a tile carries (every output is
//            linear in it), so that the elements cost three products each and no conversion.  With the factor S = F^2 / R the kernel maps a
//            stored word w to S R / w whatever w stands for; the tile products of a level are such words, and the inverse the level below
//            needs of them is S R / w again -- so the levels above the data run the same kernel with the same constants.
//   scan     the number of factors differs from element to element, so the values do go into Montgomery form (one product by R^2 / F on the
//            way in); the way out (times F / R) is folded into the tile's carry-in.  Sums stay in the data's form.
//
// A tile is FRVEC_TILE = 1024 elements: 256 lanes of FRVEC_E = 4 consecutive elements (a lane reads and writes 128 contiguous bytes with 16-byte
// accesses).  No kernel waits for another workgroup: the phases of a scan are launches of their own (csrc/frvec_host.h).
#pragma once
#include <cstddef>
#include <cstdint>

#define FRVEC_THREADS 256
#define FRVEC_E 4
#define FRVEC_TILE (FRVEC_THREADS * FRVEC_E)

// the ops, as include/msm_frvec.h numbers them
#define FRVEC_ADD 0
#define FRVEC_SUB 1
#define FRVEC_MUL 2
#define FRVEC_MUL_ADD 3
#define FRVEC_MUL_SUB 4
#define FRVEC_SUM 0
#define FRVEC_PRODUCT 1
// what a launch of the inverse kernel does with its tile's product (csrc/frvec_host.h: one level is one tile per workgroup)
#define FRVEC_INV_WHOLE 0   // inverts it by Fermat's theorem: the top level
#define FRVEC_INV_TOTALS 1  // stores it and stops: the way up
#define FRVEC_INV_ROOTS 2   // reads its inverse, which the level above computed: the way down

// what the host plans (csrc/frvec_plan.h) -- plain data, the same for every field's unit; every constant is 8 words, canonical
struct FrvecMapArgs {
  uint32_t op;
  uint32_t b_const, c_const;  // 1: the operand is the broadcast constant below, and its pointer is not read
  uint32_t b[8], c[8];        // b F (ADD, SUB) or b R (the products); c F
  uint32_t fix[8];            // R^2 / F: restores a product of two vectors
};
struct FrvecInvArgs {
  uint32_t tile;      // elements per tile in use (the test hook shrinks it), <= FRVEC_TILE
  uint32_t pm2[8];    // r - 2
  uint32_t scale[8];  // F^2 / R
};
struct FrvecScanArgs {
  uint32_t tile, op, exclusive;
  uint32_t conv_in, conv_out;  // products at level 0: into Montgomery form on the way in, back into the data's form with the carry-in
  uint32_t k_in[8], f_out[8];  // R^2 / F;  F
};

#if defined(__HIPCC__)
// what the host code (csrc/frvec_host.h) knows of a field's unit
struct FrvecOps {
  const uint32_t* r32;
  void (*map)(unsigned blocks, hipStream_t st, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n, const FrvecMapArgs* m, uint32_t* err);
  void (*inverse)(unsigned blocks, hipStream_t st, const uint32_t* a, uint32_t* out, size_t n, const FrvecInvArgs* v, uint32_t mode, uint32_t* aux, uint32_t* err);
  void (*fold)(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* totals, size_t n, uint32_t tiles, const FrvecScanArgs* g, uint32_t* err);
  void (*scan)(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* row_total, size_t n, uint32_t tiles,
               const FrvecScanArgs* g, uint32_t* err);
};
#endif

namespace MSM_FIELD_NS {

FQ_HD bool frv_words_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}
FQ_HD void frv_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FQ_HD void frv_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
// element `at` of a vector, exact and below r; false (and zero) where the stored value is not below r
FQ_HD bool frv_load(fq& x, const uint32_t* src, size_t at) {
  uint32_t w[8];
  frv_load_words(w, src, at);
  const bool ok = frv_words_below_r(w);
  x = ok ? fq_unpack(w) : fq_zero();
  return ok;
}
FQ_HD void frv_store(uint32_t* dst, size_t at, const fq& x) {  // x exact, < 2r
  uint32_t w[8];
  fq_pack(w, fq_canonical(x));
  frv_store_words(dst, at, w);
}
FQ_HD fq frv_const(const uint32_t w[8]) { return fq_unpack(w); }

// a + b mod r for canonical a, b: one carry chain, one conditional subtraction.  Out: canonical.
FQ_HD fq frv_add(const fq& a, const fq& b) {
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
FQ_HD fq frv_sub(const fq& a, const fq& b) { return frv_add(a, fq_neg_canonical(b)); }

// ---- 1. map ------------------------------------------------------------------------------------------------------------------------------------
// element i: out[i] = a[i] (+ - *) b[i] (+ - c[i]).  False: an operand not below r.
FQ_HD bool frv_map_element(const FrvecMapArgs& m, size_t i, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
  fq x, y, z = fq_zero();
  bool ok = frv_load(x, a, i);
  if (m.b_const) y = frv_const(m.b);
  else ok &= frv_load(y, b, i);
  const bool three = m.op == FRVEC_MUL_ADD || m.op == FRVEC_MUL_SUB;
  if (three) {
    if (m.c_const) z = frv_const(m.c);
    else ok &= frv_load(z, c, i);
  }
  fq res;
  if (m.op == FRVEC_ADD) res = frv_add(x, y);
  else if (m.op == FRVEC_SUB) res = frv_sub(x, y);
  else {
    fq t = fq_mul(x, y);  // (exact, < 2r)
    if (!m.b_const) t = fq_mul(t, frv_const(m.fix));
    t = fq_canonical(t);
    res = m.op == FRVEC_MUL ? t : m.op == FRVEC_MUL_ADD ? frv_add(t, z) : frv_sub(t, z);
  }
  frv_store(out, i, res);
  return ok;
}

// ---- 2. batch inverse --------------------------------------------------------------------------------------------------------------------------
// Montgomery's trick on a tile: every lane multiplies its E elements up (zeros and rejected values enter as 1), a product tree over the 256 lane
// totals is built in LDS (heap order: node k has the children 2k and 2k + 1, the leaves are 256 + lane), the root is inverted by Fermat's theorem
// and scaled, the tree is walked down again -- a node's inverse times its sibling's product is the child's inverse --, and every lane sweeps
// backwards through its elements from the inverse of its own total.  Three products per element, 2 x 255 in the tree, one chain of ~380.
// One chain per tile is 380 products by one wave against the 70 of the rest of the tile, so only a vector of ONE tile runs that way
// (FRVEC_INV_WHOLE).  A longer one goes up first: every tile stores its product (FRVEC_INV_TOTALS), the products are inverted -- the same call one
// level up, until one tile is left --, and on the way down every tile takes its root from there (FRVEC_INV_ROOTS): four products per element
// and one chain per call, whatever n is.
struct FrvInvLane {
  fq u[FRVEC_E];  // the elements (1 for a zero, a hole or a rejected value)
  fq p[FRVEC_E];  // p[j] = u[0] .. u[j]
  uint32_t live;  // bit j: element j is stored;  bit 8 + j: ... and is zero
};
FQ_HD size_t frv_element(uint32_t tile, size_t tile_no, uint32_t lane, int j) { return tile_no * tile + (size_t)lane * FRVEC_E + j; }
FQ_HD bool frv_in_tile(uint32_t tile, uint32_t lane, int j) { return lane * FRVEC_E + (uint32_t)j < tile; }

FQ_HD bool frv_inv_forward(const FrvecInvArgs& v, size_t n, size_t tile_no, uint32_t lane, const uint32_t* a, FrvInvLane& s, fq* tree) {
  bool ok = true;
  s.live = 0;
#pragma unroll
  for (int j = 0; j < FRVEC_E; j++) {
    const size_t at = frv_element(v.tile, tile_no, lane, j);
    fq x = fq_one();
    if (frv_in_tile(v.tile, lane, j) && at < n) {
      const bool good = frv_load(x, a, at);
      ok &= good;
      s.live |= 1u << j;
      if (!good || fq_is_zero_exact(x)) {
        s.live |= 0x100u << j;
        x = fq_one();
      }
    }
    s.u[j] = x;
    s.p[j] = j ? fq_mul(s.p[j - 1], x) : x;
  }
  tree[FRVEC_THREADS + lane] = s.p[FRVEC_E - 1];
  return ok;
}
FQ_HD void frv_inv_up(fq* tree, uint32_t width, uint32_t x) {  // level of `width` nodes, x < width
  const uint32_t k = width + x;
  tree[k] = fq_mul(tree[2 * k], tree[2 * k + 1]);
}
FQ_HD fq frv_pow(const fq& a, const uint32_t e[8]) {  // a exact and nonzero; out exact, < 2r
  fq acc = fq_one();
  for (int bit = 255; bit >= 0; bit--) {
    acc = fq_sqr(acc);
    if ((e[bit >> 5] >> (bit & 31)) & 1u) acc = fq_mul(acc, a);
  }
  return acc;
}
FQ_HD void frv_inv_root(const FrvecInvArgs& v, fq* tree) { tree[1] = fq_mul(frv_pow(tree[1], v.pm2), frv_const(v.scale)); }
// the two halves of a level that is not the top one: the tile's product out (canonical), and its inverse -- the level above's output -- in
FQ_HD void frv_inv_total_out(const fq* tree, uint32_t* totals, size_t tile_no) { frv_store(totals, tile_no, tree[1]); }
FQ_HD void frv_inv_root_in(fq* tree, const uint32_t* roots, size_t tile_no) { (void)frv_load(tree[1], roots, tile_no); }  // (written by this library: below r)
FQ_HD void frv_inv_down(fq* tree, uint32_t width, uint32_t x) {  // the children of the level of `width` nodes; one lane writes both
  const uint32_t k = width + x;
  const fq inv = tree[k], left = tree[2 * k], right = tree[2 * k + 1];
  tree[2 * k] = fq_mul(inv, right);
  tree[2 * k + 1] = fq_mul(inv, left);
}
FQ_HD void frv_inv_backward(const FrvecInvArgs& v, size_t tile_no, uint32_t lane, const FrvInvLane& s, const fq* tree, uint32_t* out) {
  fq inv = tree[FRVEC_THREADS + lane];
#pragma unroll
  for (int j = FRVEC_E - 1; j >= 0; j--) {
    if ((s.live >> j) & 1u) frv_store(out, frv_element(v.tile, tile_no, lane, j), (s.live >> (8 + j)) & 1u ? fq_zero() : j ? fq_mul(inv, s.p[j - 1]) : inv);
    if (j) inv = fq_mul(inv, s.u[j]);
  }
}

// ---- 3. scan -----------------------------------------------------------------------------------------------------------------------------------
// Rows of n elements, tiled row by row: workgroup (row, k) owns the elements [k tile, (k + 1) tile) of its row.  Phase 1 (frv_fold_*) folds every
// tile to one value; the host scans those values -- exclusively, row by row, with these same kernels one level up -- and phase 3 (frv_scan_*)
// scans every tile from its carry-in.  Values between the levels are canonical words: Montgomery form for products, the data's form for sums.
FQ_HD fq frv_identity(uint32_t op) { return op == FRVEC_PRODUCT ? fq_one() : fq_zero(); }
FQ_HD fq frv_fold2(uint32_t op, const fq& a, const fq& b) { return op == FRVEC_PRODUCT ? fq_mul(a, b) : frv_add(a, b); }  // sums: a, b canonical

struct FrvScanLane {
  fq q[FRVEC_E];  // q[j] = w[0] o .. o w[j] over the lane's own elements
  uint32_t live;
};
// the lane's elements folded; the lane's total goes to slot[lane]
FQ_HD bool frv_scan_load(const FrvecScanArgs& g, size_t n, size_t row, size_t k, uint32_t lane, const uint32_t* in, FrvScanLane& s, fq* slot) {
  bool ok = true;
  s.live = 0;
#pragma unroll
  for (int j = 0; j < FRVEC_E; j++) {
    const size_t at = frv_element(g.tile, k, lane, j);
    fq x = frv_identity(g.op);
    if (frv_in_tile(g.tile, lane, j) && at < n) {
      fq w;
      const bool good = frv_load(w, in, row * n + at);
      ok &= good;
      s.live |= 1u << j;
      if (good) x = g.conv_in ? fq_mul(w, frv_const(g.k_in)) : w;
    }
    s.q[j] = j ? frv_fold2(g.op, s.q[j - 1], x) : x;  // (sums: x is below r, and frv_add keeps it so)
  }
  slot[lane] = s.q[FRVEC_E - 1];
  return ok;
}
// phase 1: slot[x] = slot[x] o slot[x + width], x < width, width = 128 .. 1; then slot[0] is the tile's total
FQ_HD void frv_fold_step(uint32_t op, fq* slot, uint32_t width, uint32_t x) { slot[x] = frv_fold2(op, slot[x], slot[x + width]); }
FQ_HD void frv_fold_store(const fq* slot, uint32_t* totals, size_t at) { frv_store(totals, at, slot[0]); }
// phase 3: an inclusive scan of the lane totals, doubling the distance from one buffer into the other (src and dst differ)
FQ_HD void frv_scan_step(uint32_t op, const fq* src, fq* dst, uint32_t d, uint32_t lane) { dst[lane] = lane >= d ? frv_fold2(op, src[lane - d], src[lane]) : src[lane]; }
// slot: the inclusive scan of the lane totals.  carry: the tile's carry-in (NULL: the identity).  row_total (NULL at the inner levels): receives
// the row's total from the lane that holds the row's last element.
FQ_HD void frv_scan_store(const FrvecScanArgs& g, size_t n, size_t row, size_t k, size_t tiles, uint32_t lane, const FrvScanLane& s, const fq* slot, const uint32_t* carry,
                          uint32_t* out, uint32_t* row_total) {
  fq base = frv_identity(g.op);
  if (carry) (void)frv_load(base, carry, row * tiles + k);  // (written by this library: below r)
  if (g.conv_out) base = fq_mul(base, frv_const(g.f_out));  // C R -> C F: what follows is in the data's form
  if (g.op == FRVEC_PRODUCT) base = fq_mul(base, lane ? slot[lane - 1] : fq_one());
  else base = lane ? frv_add(base, slot[lane - 1]) : base;
  fq prev = base;  // the fold of everything before element j
#pragma unroll
  for (int j = 0; j < FRVEC_E; j++) {
    if (!((s.live >> j) & 1u)) break;
    const fq incl = g.op == FRVEC_PRODUCT ? fq_mul(base, s.q[j]) : frv_add(base, s.q[j]);
    const size_t at = frv_element(g.tile, k, lane, j);
    frv_store(out, row * n + at, g.exclusive ? prev : incl);
    if (row_total && at == n - 1) frv_store(row_total, row, incl);
    prev = incl;
  }
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(FRVEC_THREADS) k_frvec_map(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n, const FrvecMapArgs m, uint32_t* err) {
  const size_t i = (size_t)blockIdx.x * FRVEC_THREADS + threadIdx.x;
  if (i >= n) return;
  if (!frv_map_element(m, i, a, b, c, out)) atomicOr(err, 1u);
}

// aux: the level above -- written under FRVEC_INV_TOTALS, read under FRVEC_INV_ROOTS, not used under FRVEC_INV_WHOLE
__global__ void __launch_bounds__(FRVEC_THREADS) k_frvec_inverse(const uint32_t* a, uint32_t* out, size_t n, const FrvecInvArgs v, uint32_t mode, uint32_t* aux, uint32_t* err) {
  __shared__ uint32_t lds[FQ_LIMBS * 2 * FRVEC_THREADS];
  fq* tree = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  FrvInvLane s;
  if (!frv_inv_forward(v, n, blockIdx.x, lane, a, s, tree)) atomicOr(err, 1u);
  for (uint32_t w = FRVEC_THREADS / 2; w >= 1; w >>= 1) {
    __syncthreads();
    if (lane < w) frv_inv_up(tree, w, lane);
  }
  __syncthreads();
  if (mode == FRVEC_INV_TOTALS) {  // (the same for every lane)
    if (lane == 0) frv_inv_total_out(tree, aux, blockIdx.x);
    return;
  }
  if (lane == 0) {
    if (mode == FRVEC_INV_ROOTS) frv_inv_root_in(tree, aux, blockIdx.x);
    else frv_inv_root(v, tree);
  }
  for (uint32_t w = 1; w < FRVEC_THREADS; w <<= 1) {
    __syncthreads();
    if (lane < w) frv_inv_down(tree, w, lane);
  }
  __syncthreads();
  frv_inv_backward(v, blockIdx.x, lane, s, tree, out);
}

// block = row * tiles + k
__global__ void __launch_bounds__(FRVEC_THREADS) k_frvec_fold(const uint32_t* in, uint32_t* totals, size_t n, uint32_t tiles, const FrvecScanArgs g, uint32_t* err) {
  __shared__ uint32_t lds[FQ_LIMBS * FRVEC_THREADS];
  fq* slot = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  const size_t row = blockIdx.x / tiles, k = blockIdx.x % tiles;
  FrvScanLane s;
  if (!frv_scan_load(g, n, row, k, lane, in, s, slot)) atomicOr(err, 1u);
  for (uint32_t w = FRVEC_THREADS / 2; w >= 1; w >>= 1) {
    __syncthreads();
    if (lane < w) frv_fold_step(g.op, slot, w, lane);
  }
  __syncthreads();
  if (lane == 0) frv_fold_store(slot, totals, blockIdx.x);
}

__global__ void __launch_bounds__(FRVEC_THREADS) k_frvec_scan(const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* row_total, size_t n, uint32_t tiles,
                                                              const FrvecScanArgs g, uint32_t* err) {
  __shared__ uint32_t lds[2 * FQ_LIMBS * FRVEC_THREADS];
  fq* buf = reinterpret_cast<fq*>(lds);
  const uint32_t lane = threadIdx.x;
  const size_t row = blockIdx.x / tiles, k = blockIdx.x % tiles;
  FrvScanLane s;
  if (!frv_scan_load(g, n, row, k, lane, in, s, buf)) atomicOr(err, 1u);
  uint32_t from = 0;
  for (uint32_t d = 1; d < FRVEC_THREADS; d <<= 1) {  // (8 steps: the result is back in the first buffer)
    __syncthreads();
    frv_scan_step(g.op, buf + from * FRVEC_THREADS, buf + (from ^ 1u) * FRVEC_THREADS, d, lane);
    from ^= 1u;
  }
  __syncthreads();
  frv_scan_store(g, n, row, k, tiles, lane, s, buf + from * FRVEC_THREADS, carry, out, row_total);
}

inline void frvec_launch_map(unsigned blocks, hipStream_t st, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n, const FrvecMapArgs* m, uint32_t* err) {
  hipLaunchKernelGGL(k_frvec_map, dim3(blocks), dim3(FRVEC_THREADS), 0, st, a, b, c, out, n, *m, err);
}
inline void frvec_launch_inverse(unsigned blocks, hipStream_t st, const uint32_t* a, uint32_t* out, size_t n, const FrvecInvArgs* v, uint32_t mode, uint32_t* aux,
                                 uint32_t* err) {
  hipLaunchKernelGGL(k_frvec_inverse, dim3(blocks), dim3(FRVEC_THREADS), 0, st, a, out, n, *v, mode, aux, err);
}
inline void frvec_launch_fold(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* totals, size_t n, uint32_t tiles, const FrvecScanArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frvec_fold, dim3(blocks), dim3(FRVEC_THREADS), 0, st, in, totals, n, tiles, *g, err);
}
inline void frvec_launch_scan(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, const uint32_t* carry, uint32_t* row_total, size_t n, uint32_t tiles,
                              const FrvecScanArgs* g, uint32_t* err) {
  hipLaunchKernelGGL(k_frvec_scan, dim3(blocks), dim3(FRVEC_THREADS), 0, st, in, out, carry, row_total, n, tiles, *g, err);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS
