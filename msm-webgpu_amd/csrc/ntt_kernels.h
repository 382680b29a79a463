// The scalar-field NTT of libmsm_fr.so (include/msm_fr.h), written once and instantiated per field: a unit (csrc/fr_<name>.hip) includes
// csrc/fq29.h over the field's constants (tools/gen_constants.py fr <name>) and then this file, inside its own MSM_FIELD_NS.
//
//     out[i] = c * t^i * sum_j s^j * omega^(i j) * a[j],      i, j < n = 2^log_n
//
// Shape.  log_n is cut into k = ceil(log_n / NTT_PASS_BITS) digits of (almost) equal width, the first digit on top of the index.  Pass p runs,
// for every value of the other index bits, a 2^b_p-point transform over digit p on a tile staged in LDS, then multiplies element (i_p, j') --
// j' the index bits below the digit -- by omega_p^(i_p j'), omega_p = omega^(2^(b_1 + .. + b_(p-1))): decimation in frequency, digit by digit.
// Passes 1 .. k - 1 leave every element where it was (a workgroup reads and writes the same addresses: they may run in place), the last pass
// writes element (i_1, .., i_k) to index i_1 + 2^b_1 i_2 + ..: natural order out of natural order in.  Inside a tile the transform is
// decimation in TIME on the bit-reversed digit (an element enters LDS at the bit-reversed slot): b_p radix-2 levels, a barrier between two.
//
// A workgroup takes 2^NTT_COL_BITS tiles at once so that every global access is a run of 2^NTT_COL_BITS * 32 bytes: in a pass over a strided digit the
// columns are the lowest index bits (runs on both sides); in the last pass (the contiguous digit: whole tiles are runs on the way in) they are
// the lowest bits of the FIRST digit, which become the lowest bits of the output index.
//
// Representation.  The data stay in the form they arrive in -- canonical a, or a 2^256 mod r (MSM_FR_MONT256): every factor (butterfly twiddle,
// the twiddles between passes, the shifts, 1 / n) is stored as w 2^261 mod r, canonical, so that fq_mul(data, factor) = data w in the data's own
// form; sums and differences are linear.  Only the last store reduces to [0, r).
//
// Lazy bounds (csrc/fq29.h; asserted by g++ -DFQ_CHECK in tests/test_ntt_host.py).  A tile is entered exact and below 2r (a validated input is
// below r; a stored intermediate is a Montgomery product).  One level:  t = b w  (exact, < 2r; operand product value(b) r),  b' = a - t + 3r
// (fq_sub<3>: normal),  a' = norm(a + t)  (normal): a value gains at most 3r per level, so after ten levels it is below 32r, and the largest
// multiplier operand product is 32 r * r -- the tightest field, BLS12-381's (2^261 / r = 70), allows 70 r^2 (the generator asserts 2 + 3 * 10 <=
// headroom).  Limbs 0..7 stay normal (< 2^29 + 8), the top limb below 2^28.
#pragma once
#include <cstddef>
#include <cstdint>

#define NTT_PASS_BITS 10  // B: radix-2 levels per pass, i.e. 2^10 elements per tile
#define NTT_COL_BITS 1    // 2 tiles per workgroup: 64-byte runs; 2 * 1024 elements of 9 limbs = 72 KiB of LDS, two workgroups per CU
#define NTT_THREADS 256
#define NTT_MAX_DIGITS 26  // (a test hook may cap a pass at one level)
#define NTT_TABLE_LO_BITS 13  // two-level power tables: g^e = lo[e mod 2^13] * hi[e >> 13]

// one pass, as the host plans it (csrc/ntt_host.h) -- plain data, shared by every field's unit
struct NttPass {
  uint32_t log_n;
  uint32_t lo, b, shift;      // the digit: index bits [lo, lo + b); shift = b_1 + .. + b_(p-1)
  uint32_t log_c, col_at;     // 2^log_c columns: index bits [col_at, col_at + log_c)
  uint32_t ins_at[2], ins_w[2];  // the two fields a workgroup's number is spread around (ascending positions)
  uint32_t first, last;
  uint32_t tw_log;            // the butterfly table holds the powers of the primitive 2^tw_log-th root
  uint32_t pre_mode, post_mode;  // factor tables in use: bit 0 the low level, bit 1 the high level (0: no factor)
  uint32_t pre_lo_bits, post_lo_bits, tw_lo_bits, tw_mode;
  uint32_t ndig;
  uint8_t dig_w[NTT_MAX_DIGITS + 2];
};
struct NttTables {
  const uint32_t* bt;                 // butterfly twiddles: 2^(tw_log - 1) entries of 8 words
  const uint32_t *tw_lo, *tw_hi;      // omega^e, e < n: the twiddles between passes
  const uint32_t *pre_lo, *pre_hi;    // s^j
  const uint32_t *post_lo, *post_hi;  // c t^i  (c folded into the high level)
};

#if defined(__HIPCC__)
// what the host code (csrc/ntt_host.h) knows of a field's unit
struct FrOps {
  const uint32_t* r32;  // the modulus, 8 words
  int two_adicity;
  void (*launch)(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, const NttPass* p, const NttTables* t, uint32_t* err);
};
#endif

namespace MSM_FIELD_NS {

FQ_HD uint32_t ntt_insert_zeros(uint32_t x, uint32_t at, uint32_t w) { return ((x >> at) << (at + w)) | (x & ((1u << at) - 1u)); }
FQ_HD uint32_t ntt_bitrev(uint32_t x, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return bits ? __brev(x) >> (32u - bits) : 0u;
#else
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
#endif
}
// index (i_1 .. i_k, first digit on top)  ->  i_1 + 2^b_1 i_2 + ..
FQ_HD uint32_t ntt_digit_reverse(uint32_t pos, const NttPass& p) {
  uint32_t at = p.log_n, sh = 0, out = 0;
  for (uint32_t q = 0; q < p.ndig; q++) {
    const uint32_t w = p.dig_w[q];
    at -= w;
    out |= ((pos >> at) & ((1u << w) - 1u)) << sh;
    sh += w;
  }
  return out;
}

FQ_HD fq ntt_load_entry(const uint32_t* table, uint32_t k) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = table[8 * (size_t)k + i];
  return fq_unpack(w);
}
// x g^e for a two-level table of g's powers (entries g^k 2^261 mod r, canonical): one product per level in use, so x stays in its own form.
// x normal, value(x) r <= headroom r^2.  Out: exact, < 2r.
FQ_HD fq ntt_times_factor(const fq& x, const uint32_t* lo, const uint32_t* hi, uint32_t mode, uint32_t lo_bits, uint32_t e) {
  fq y = x;
  if (mode & 1u) y = fq_mul(y, ntt_load_entry(lo, e & ((1u << lo_bits) - 1u)));
  if (mode & 2u) y = fq_mul(y, ntt_load_entry(hi, e >> lo_bits));
  return y;
}

// a, b  ->  a + b w, a - b w.   a normal, value(a) < V;  b normal, value(b) r <= headroom r^2;  w < r.   Out: normal, values < V + 3r.
FQ_HD void ntt_butterfly(fq& a, fq& b, const fq& w, bool w_is_one) {
  const fq t = w_is_one ? b : fq_mul(b, w);  // (level 0: b is the tile's input, exact and below 2r as it stands)
  b = fq_sub<3>(a, t);
  a = fq_norm(fq_add(a, t));
}

// butterfly x (x < 2^(b - 1)) of level s of one tile: elements k, k + 2^s with the twiddle omega_(2^(s+1))^(k mod 2^s)
FQ_HD void ntt_level_butterfly(fq* tile, const uint32_t* bt, uint32_t tw_log, uint32_t s, uint32_t x) {
  const uint32_t half = 1u << s, j = x & (half - 1u);
  const uint32_t k = ((x >> s) << (s + 1)) | j;
  fq a = tile[k], b = tile[k + half];
  ntt_butterfly(a, b, s == 0 ? a : ntt_load_entry(bt, j << (tw_log - 1u - s)), s == 0);
  tile[k] = a;
  tile[k + half] = b;
}

FQ_HD bool ntt_words_below_r(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i] != FQ_P32[i]) return w[i] < FQ_P32[i];
  return false;
}


// ---- one pass, element by element: what a lane of k_ntt_pass does, and what the host program of tests/test_ntt_host.py runs serially ----------
struct NttBlock {
  uint32_t base;  // the index bits this workgroup fixes
  size_t vec;     // first element of its vector of the batch
};
FQ_HD NttBlock ntt_block(const NttPass& p, uint32_t block) {
  const uint32_t rest_bits = p.log_n - p.b - p.log_c;
  NttBlock k;
  k.base = ntt_insert_zeros(ntt_insert_zeros(block & ((1u << rest_bits) - 1u), p.ins_at[0], p.ins_w[0]), p.ins_at[1], p.ins_w[1]);
  k.vec = ((size_t)(block >> rest_bits)) << p.log_n;
  return k;
}
FQ_HD void ntt_load_words(uint32_t w[8], const uint32_t* src, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  const uint4 q0 = s4[2 * at], q1 = s4[2 * at + 1];
  w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w, w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
#else
  for (int i = 0; i < 8; i++) w[i] = src[8 * at + i];
#endif
}
FQ_HD void ntt_store_words(uint32_t* dst, size_t at, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[2 * at] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[2 * at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; i++) dst[8 * at + i] = w[i];
#endif
}
// element e (< 2^(b + log_c)) of the workgroup's tiles: global -> LDS slot (the digit bit-reversed).  False: a first-pass input >= r.
FQ_HD bool ntt_pass_load(const NttPass& p, const NttTables& t, const NttBlock& k, uint32_t e, const uint32_t* in, fq* tile) {
  // a run of consecutive lanes reads consecutive addresses: the columns in a strided pass, the digit itself in the last one
  const uint32_t cmask = (1u << p.log_c) - 1u, dmask = (1u << p.b) - 1u;
  const uint32_t c = p.last ? e >> p.b : e & cmask, d = p.last ? e & dmask : e >> p.log_c;
  const uint32_t pos = k.base | (d << p.lo) | (c << p.col_at);
  uint32_t w[8];
  ntt_load_words(w, in, k.vec + pos);
  const bool ok = !p.first || ntt_words_below_r(w);
  fq x = ok ? fq_unpack(w) : fq_zero();  // (a rejected value must not carry the lazy sums past their bounds: the call fails, the data are unspecified)
  if (p.pre_mode) x = ntt_times_factor(x, t.pre_lo, t.pre_hi, p.pre_mode, p.pre_lo_bits, pos);
  tile[(c << p.b) | ntt_bitrev(d, p.b)] = x;
  return ok;
}
// butterfly x (< 2^(b + log_c - 1)) of level s over the workgroup's tiles
FQ_HD void ntt_pass_level(const NttPass& p, const NttTables& t, uint32_t s, uint32_t x, fq* tile) {
  ntt_level_butterfly(tile + ((x >> (p.b - 1u)) << p.b), t.bt, p.tw_log, s, x & ((1u << (p.b - 1u)) - 1u));
}
// element e: LDS -> global, times the twiddle between passes, or -- last pass -- times c t^i, reduced, at its natural index
FQ_HD void ntt_pass_store(const NttPass& p, const NttTables& t, const NttBlock& k, uint32_t e, const fq* tile, uint32_t* out) {
  const uint32_t c = e & ((1u << p.log_c) - 1u), i = e >> p.log_c;
  const uint32_t pos = k.base | (i << p.lo) | (c << p.col_at);
  const fq x = tile[(c << p.b) | i];
  uint32_t w[8];
  if (p.last) {
    const uint32_t at = ntt_digit_reverse(pos, p);
    // (without a factor: times 1 = R mod r, which takes any tile value -- normal, < 32r -- below 2r)
    fq_pack(w, fq_canonical(p.post_mode ? ntt_times_factor(x, t.post_lo, t.post_hi, p.post_mode, p.post_lo_bits, at) : fq_mul(x, fq_one())));
    ntt_store_words(out, k.vec + at, w);
  } else {
    const uint32_t expo = ((pos & ((1u << p.lo) - 1u)) * i) << p.shift;
    fq_pack(w, ntt_times_factor(x, t.tw_lo, t.tw_hi, p.tw_mode, p.tw_lo_bits, expo));  // exact, < 2r < 2^256
    ntt_store_words(out, k.vec + pos, w);
  }
}

#if defined(__HIPCC__)
// `in` and `out` may be the same buffer in every pass but the last (which moves elements)
__global__ void __launch_bounds__(NTT_THREADS) k_ntt_pass(const uint32_t* in, uint32_t* out, const NttPass p, const NttTables t, uint32_t* err) {
  __shared__ uint32_t lds[(FQ_LIMBS << (NTT_PASS_BITS + NTT_COL_BITS))];
  fq* tile = reinterpret_cast<fq*>(lds);
  const uint32_t tid = threadIdx.x, elems = 1u << (p.b + p.log_c);
  const NttBlock k = ntt_block(p, blockIdx.x);
  bool ok = true;
  for (uint32_t e = tid; e < elems; e += NTT_THREADS) ok &= ntt_pass_load(p, t, k, e, in, tile);
  if (!ok) atomicOr(err, 1u);
  for (uint32_t s = 0; s < p.b; s++) {
    __syncthreads();
    for (uint32_t x = tid; x < (elems >> 1); x += NTT_THREADS) ntt_pass_level(p, t, s, x, tile);
  }
  __syncthreads();
  for (uint32_t e = tid; e < elems; e += NTT_THREADS) ntt_pass_store(p, t, k, e, tile, out);
}

inline void ntt_launch_pass(unsigned blocks, hipStream_t st, const uint32_t* in, uint32_t* out, const NttPass* p, const NttTables* t, uint32_t* err) {
  hipLaunchKernelGGL(k_ntt_pass, dim3(blocks), dim3(NTT_THREADS), 0, st, in, out, *p, *t, err);
}
#endif  // __HIPCC__

}  // namespace MSM_FIELD_NS
