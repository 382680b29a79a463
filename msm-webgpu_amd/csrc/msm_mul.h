// Batch scalar multiplication, host side (the kernels: scalar_mul.h, in every curve unit).  Its state is the context's MulState (msm_ctx.h).
// Assumes msm_plan.h (MAX_POINTS), msm_ctx.h and, of msm_hip.hip, no_context_code.
#pragma once


// ---- batch scalar multiplication: out[i] = s_i * P_i (mul_each) and out[i] = s_i * P_base (mul_base) ------------------------------------------
namespace {
constexpr size_t MUL_TILE = (size_t)1 << 20;  // outputs per kernel pair: bounds the scratch (Z values + prefix products: 64 MiB on BN254 G1) whatever n is

inline bool prime_order_curve(int curve) {
  return curve == MSM_HIP_CURVE_BN254_G1 || curve == MSM_HIP_CURVE_GRUMPKIN || curve == MSM_HIP_CURVE_PALLAS || curve == MSM_HIP_CURVE_VESTA;
}
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// The fixed-base table of msm_hip_mul_base: which digit width C, if any, serves n outputs of base `base`.  Measured on BN254 G1 (profiles/mul_each.txt,
// tools/bench_mul.py --crossover: broadcast ladder against the table forced at C = 8 .. 16, n = 2^10 .. 2^20, the building call timed apart):
//   - a table the context already holds beats the ladder at every n (0.34 against 1.23 ms at 2^10, 1.2 - 2.2 against 14.4 ms at 2^20): it is reused;
//   - a call that has to build its table loses to the ladder up to 2^16 (1.64 against 1.39 ms) and wins from 2^18 (1.87 against 4.01 ms): the
//     threshold is 2^17;
//   - with the build in the call, C = 12 is the fastest width at 2^18 and 2^20 (2.87 ms; C = 10: 3.10, C = 14: 3.73, C = 16: 6.73).  A wider table
//     costs 1.0 ms (C = 14) and 4.2 ms (C = 16) more to build than C = 12 and saves 0.13 and 0.33 ns per output: C = 14 from 2^23, C = 16 from 2^24.
// C <= 16: at most W 2^15 records, 32 MiB on BN254 G1.  msm_hip_test_mul_policy replaces either decision.
constexpr int MUL_TABLE_MAX_BITS = 16;
constexpr size_t MUL_TABLE_MIN_N = (size_t)1 << 17;
inline int mul_table_windows(const msm_hip_ctx* ctx, int c) { return (ctx->ops->r_bits + 1 + c) / c; }
int pick_mul_table_bits(const msm_hip_ctx* ctx, size_t base, size_t n, bool endo) {
  const bool held = ctx->mul.mul_table_bits != 0 && ctx->mul.mul_table_base == base && ctx->mul.mul_table_endo == endo;
  if (ctx->mul.mul_policy_min_n) {  // the hook: the table exactly from this n on
    if (n < ctx->mul.mul_policy_min_n) return 0;
  } else if (!held && n < MUL_TABLE_MIN_N) {
    return 0;
  }
  if (ctx->mul.mul_policy_bits) return ctx->mul.mul_policy_bits;
  if (held) return ctx->mul.mul_table_bits;
  return n < ((size_t)1 << 23) ? 12 : n < ((size_t)1 << 24) ? 14 : 16;
}

// `host`: scalars and out are host memory (staged through d_mul tile by tile); else device memory, read and written in place.
// Everything is enqueued on the main stream; the call returns when the output is complete.
int mul_impl(msm_hip_ctx* ctx, bool broadcast, size_t base_index, const void* scalars, size_t n, void* out, uint32_t flags, bool host) {
  if (!ctx) return no_context_code();
  if (flags & ~MSM_HIP_MUL_BASES_ORDER_R) return MSM_HIP_ERR_INVALID_ARG;
  if (ctx->scalar_format != MSM_HIP_SCALARS_CANONICAL && ctx->scalar_format != MSM_HIP_SCALARS_MONT256) return MSM_HIP_ERR_INVALID_ARG;  // 32-byte formats only
  if (n == 0) return MSM_HIP_OK;
  if (!scalars || !out || n > MAX_POINTS) return MSM_HIP_ERR_INVALID_ARG;
  if (ctx->n_bases == 0) return MSM_HIP_ERR_NO_BASES;
  if (broadcast ? base_index >= ctx->n_bases : n > ctx->n_bases) return MSM_HIP_ERR_INVALID_ARG;
  if (ranges_overlap(scalars, n * 32, out, n * ctx->pb)) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && ((reinterpret_cast<uintptr_t>(scalars) | reinterpret_cast<uintptr_t>(out)) & 15u)) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  ON_DEVICE(ctx);
  const CurveOps* ops = ctx->ops;
  const size_t cw = (size_t)ops->coord_words, ptw = 2 * cw;
  const bool mont = ctx->scalar_format == MSM_HIP_SCALARS_MONT256;
  const bool endo = ops->glv && (ctx->mul.mul_force_ladder ? ctx->mul.mul_force_ladder == 2 : prime_order_curve(ctx->curve) || (flags & MSM_HIP_MUL_BASES_ORDER_R));
  hipStream_t st = ctx->stream;
  const uint64_t* id_bits = ctx->n_identity ? ctx->d_id_bits : nullptr;
  if (broadcast && id_bits) {  // one base for every output: is it the identity?  Then every output is, whatever the scalars hold
    uint64_t word = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&word, id_bits + (base_index >> 6), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if ((word >> (base_index & 63u)) & 1u) {
      if (host) {
        memset(out, 0, n * ctx->pb);
      } else {
        HIP_TRY(ctx, hipMemsetAsync(out, 0, n * ctx->pb, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
      }
      ctx->mul.mul_last_path = 0;
      ctx->mul.mul_last_bits = 0;
      return MSM_HIP_OK;
    }
    id_bits = nullptr;
  }
  const size_t tile = n < MUL_TILE ? n : MUL_TILE;
  // mul_base: through the fixed-base table?  (decided before the scratch is sized: a table's build runs the ladder over its entries)
  const int tbits = broadcast ? pick_mul_table_bits(ctx, base_index, n, endo) : 0;
  const size_t n_tab = tbits ? (size_t)mul_table_windows(ctx, tbits) << (tbits - 1) : 0;
  const bool build_table = tbits && !(ctx->mul.mul_table_bits == tbits && ctx->mul.mul_table_base == base_index && ctx->mul.mul_table_endo == endo);
  const size_t tab_tile = build_table ? (n_tab < MUL_TILE ? n_tab : MUL_TILE) : 0;
  const size_t stile = tile > tab_tile ? tile : tab_tile;
  const size_t tile4 = (stile + 3) & ~(size_t)3;  // (every part of the scratch stays 16-byte aligned)
  const size_t words = tile4 * (2 * cw + 16) + (host ? tile4 * (8 + ptw) : 0);
  int rc = grow(ctx, ctx->mul.cap_mul, words, true, [&](size_t c) { return dev_alloc(ctx, ctx->mul.d_mul, c); });
  if (rc) return rc;
  uint32_t* zbuf = ctx->mul.d_mul;
  uint32_t* prefix = zbuf + tile4 * cw;
  uint32_t* conv = prefix + tile4 * cw;
  uint32_t* masked = conv + tile4 * 8;
  uint32_t* stage_sc = masked + tile4 * 8;
  uint32_t* stage_out = stage_sc + tile4 * 8;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, 4, st));
  if (build_table) {  // T_w[j] = j 2^(C w) P: the ladder over the entries' scalars (integers: not compared with r), normalised like any output, then to Montgomery records
    if ((rc = grow(ctx, ctx->mul.cap_mul_table, n_tab * ptw, true, [&](size_t c) { return dev_alloc(ctx, ctx->mul.d_mul_table, c); }))) return rc;
    ctx->mul.mul_table_bits = 0;
    uint32_t* table = ctx->mul.d_mul_table;
    for (size_t off = 0; off < n_tab; off += tab_tile) {
      const size_t t = n_tab - off < tab_tile ? n_tab - off : tab_tile;
      hipLaunchKernelGGL(ops->mul_table_scalars, dim3(blocks_for(t, 256)), dim3(256), 0, st, tbits, off, t, conv);  // (this tile's scalars: in the scratch)
      AFTER_KERNEL(ctx, "k_mul_table_scalars", st);
      hipLaunchKernelGGL(ops->mul_each[endo ? 1 : 0], dim3(blocks_for(t, 256)), dim3(256), 0, st, (const uint32_t*)ctx->d_bases, (const uint32_t*)conv, t, base_index, 1u,
                         (const uint64_t*)nullptr, table + off * ptw, zbuf, ctx->d_err, 0u);
      AFTER_KERNEL(ctx, "k_mul_each (table)", st);
      hipLaunchKernelGGL(ops->mul_normalize, dim3(blocks_for(t, 256 * (size_t)ops->mul_chunk)), dim3(256), 0, st, table + off * ptw, (const uint32_t*)zbuf, prefix, t);
      AFTER_KERNEL(ctx, "k_mul_normalize (table)", st);
    }
    hipLaunchKernelGGL(ops->convert_points, dim3(blocks_for(n_tab, 256)), dim3(256), 0, st, (const uint32_t*)table, table, n_tab, 0u, ctx->d_err);
    AFTER_KERNEL(ctx, "k_convert_points (table)", st);
    HIP_TRY(ctx, hipGetLastError());
    ctx->mul.mul_table_bits = tbits;
    ctx->mul.mul_table_base = base_index;
    ctx->mul.mul_table_endo = endo;
  }
  for (size_t off = 0; off < n; off += tile) {
    const size_t t = n - off < tile ? n - off : tile;
    const uint32_t* d_sc;
    if (host) {
      HIP_TRY(ctx, hipMemcpyAsync(stage_sc, static_cast<const uint8_t*>(scalars) + off * 32, t * 32, hipMemcpyHostToDevice, st));
      d_sc = stage_sc;
    } else {
      d_sc = static_cast<const uint32_t*>(scalars) + off * 8;
    }
    if (mont) {  // canonical copies first; ahead of them, the scalars of identity bases zeroed: they are not validated either
      if (id_bits) {
        hipLaunchKernelGGL(k_mask_identity<32>, dim3(blocks_for(t, 256), 1), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(d_sc), reinterpret_cast<uint8_t*>(masked), t,
                           off, id_bits, (uint32_t)ctx->n_bases, (const uint32_t*)nullptr);
        AFTER_KERNEL(ctx, "k_mask_identity", st);
        d_sc = masked;
      }
      hipLaunchKernelGGL(ops->scalars_from_mont256, dim3(blocks_for(t, 256)), dim3(256), 0, st, d_sc, conv, t, ctx->d_err);
      AFTER_KERNEL(ctx, "k_scalars_from_mont256", st);
      d_sc = conv;
    }
    uint32_t* d_out = host ? stage_out : static_cast<uint32_t*>(out) + off * ptw;
    if (tbits) {
      hipLaunchKernelGGL(ops->mul_fixed, dim3(blocks_for(t, 256)), dim3(256), 0, st, (const uint32_t*)ctx->mul.d_mul_table, tbits, d_sc, t, d_out, zbuf, ctx->d_err);
      AFTER_KERNEL(ctx, "k_mul_fixed", st);
    } else {
      hipLaunchKernelGGL(ops->mul_each[endo ? 1 : 0], dim3(blocks_for(t, 256)), dim3(256), 0, st, (const uint32_t*)ctx->d_bases, d_sc, t, broadcast ? base_index : off,
                         broadcast ? 1u : 0u, id_bits, d_out, zbuf, ctx->d_err, 1u);
      AFTER_KERNEL(ctx, "k_mul_each", st);
    }
    hipLaunchKernelGGL(ops->mul_normalize, dim3(blocks_for(t, 256 * (size_t)ops->mul_chunk)), dim3(256), 0, st, d_out, (const uint32_t*)zbuf, prefix, t);
    AFTER_KERNEL(ctx, "k_mul_normalize", st);
    HIP_TRY(ctx, hipGetLastError());
    if (host) {  // (the staging area is this tile's alone until its output has left)
      HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(out) + off * ctx->pb, stage_out, t * ctx->pb, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
    }
  }
  uint32_t bits = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&bits, ctx->d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->mul.mul_last_path = tbits ? (build_table ? 4 : 3) : endo ? 2 : 1;
  ctx->mul.mul_last_bits = tbits;
  return err_from_bits(bits);
}
}  // namespace

extern "C" {
int msm_hip_mul_each(msm_hip_ctx* ctx, const uint8_t* scalars_host, size_t n, uint8_t* out_xy_host, uint32_t flags) {
  return mul_impl(ctx, false, 0, scalars_host, n, out_xy_host, flags, true);
}
int msm_hip_mul_each_device(msm_hip_ctx* ctx, const void* scalars_dev, size_t n, void* out_xy_dev, uint32_t flags) {
  return mul_impl(ctx, false, 0, scalars_dev, n, out_xy_dev, flags, false);
}
int msm_hip_mul_base(msm_hip_ctx* ctx, size_t base_index, const uint8_t* scalars_host, size_t n, uint8_t* out_xy_host, uint32_t flags) {
  return mul_impl(ctx, true, base_index, scalars_host, n, out_xy_host, flags, true);
}
int msm_hip_mul_base_device(msm_hip_ctx* ctx, size_t base_index, const void* scalars_dev, size_t n, void* out_xy_dev, uint32_t flags) {
  return mul_impl(ctx, true, base_index, scalars_dev, n, out_xy_dev, flags, false);
}
int msm_hip_test_mul_policy(msm_hip_ctx* ctx, size_t table_min_n, int table_bits) {
  if (!ctx || (table_bits && (table_bits < 4 || table_bits > MUL_TABLE_MAX_BITS))) return MSM_HIP_ERR_INVALID_ARG;
  ctx->mul.mul_policy_min_n = table_min_n;
  ctx->mul.mul_policy_bits = table_bits;
  return MSM_HIP_OK;
}
int msm_hip_test_mul_ladder(msm_hip_ctx* ctx, int ladder) {
  if (!ctx || ladder < 0 || ladder > 2) return MSM_HIP_ERR_INVALID_ARG;
  ctx->mul.mul_force_ladder = ladder;
  return MSM_HIP_OK;
}
int msm_hip_test_mul_last(const msm_hip_ctx* ctx, int* path, int* table_bits, int* chunk) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  if (path) *path = ctx->mul.mul_last_path;
  if (table_bits) *table_bits = ctx->mul.mul_last_bits;
  if (chunk) *chunk = ctx->ops->mul_chunk;
  return MSM_HIP_OK;
}
}  // extern "C"
