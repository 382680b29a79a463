// The resident base set: which mode a set is held in (resolve_base_flags), room for it (reserve_bases), wire bytes to device records with their
// tables or endomorphism images (set_bases_from_device), and the msm_hip_set_bases* entry points.
// Assumes msm_plan.h (pick_wide_bits, wide_top_shift, MAX_POINTS) and msm_ctx.h (the context, grow, HIP_TRY, blocks_for, err_from_bits).
#pragma once

namespace {
// room for n bases; no run may still be reading the old ones (the SMVP on the main stream)
constexpr size_t MAX_PRECOMPUTE_POINTS = (size_t)1 << 24;  // 16 tables: 16 GiB, and table indices stay below 2^28

// The mode a base set is held in.  Asked for explicitly (tables, endomorphism images, or MSM_HIP_BASES_PLAIN: the reference's 16 windows
// over n points), or -- none of the three -- the fastest the curve has: the drop-in call shape (flags = 0; msm_hip_msm_bn254_g1 ≙ compute_msm,
// src/cuzk/msm.rs:75-94) runs the mode the headline figure is measured in (656 vs 701 - 714 MSM/s at 2^20 in round 3, when it did not).
constexpr uint32_t BASE_FLAGS_ALL = MSM_HIP_CHECK_ON_CURVE | MSM_HIP_BASES_MONT256 | MSM_HIP_BASES_PRECOMPUTE | MSM_HIP_BASES_ENDOMORPHISM | MSM_HIP_BASES_PLAIN |
                                    MSM_HIP_BASES_PRECOMPUTE_WIDE | MSM_HIP_BASES_ZERO_IS_IDENTITY;
constexpr size_t MAX_WIDE_POINTS = (size_t)1 << 24;  // 13 tables of 20-bit digits: 13 GiB; sort arrays of 16 x 13 n entries: 31 GiB
inline bool reduce_priority_on() {  // MSM_HIP_REDUCE_PRIORITY=0: plain reduce streams (msm_hip_ctx_create_curve)
  static const bool v = [] { const char* e = getenv("MSM_HIP_REDUCE_PRIORITY"); return !e || atoi(e) != 0; }();
  return v;
}
inline bool bases_auto() {  // MSM_HIP_BASES_AUTO=0: flags = 0 means plain (rounds 1 - 3)
  static const bool v = [] { const char* e = getenv("MSM_HIP_BASES_AUTO"); return !e || atoi(e) != 0; }();
  return v;
}
inline uint32_t resolve_base_flags(const msm_hip_ctx* ctx, size_t n, uint32_t flags) {
  const bool auto_endo = bases_auto();
  if (flags & (MSM_HIP_BASES_PRECOMPUTE | MSM_HIP_BASES_PRECOMPUTE_WIDE | MSM_HIP_BASES_ENDOMORPHISM | MSM_HIP_BASES_PLAIN)) return flags;
  // ... on the curves of prime order only: phi(P) = lambda P holds on the subgroup of order r, and a base set of a curve with a cofactor
  // (BLS12-381, the G2 twists) may hold points outside it, for which the plain MSM is still defined -- there the mode stays an opt-in
  const bool prime_order = ctx->curve == MSM_HIP_CURVE_BN254_G1 || ctx->curve == MSM_HIP_CURVE_GRUMPKIN || ctx->curve == MSM_HIP_CURVE_PALLAS ||
                           ctx->curve == MSM_HIP_CURVE_VESTA;
  if (auto_endo && prime_order && ctx->ops->glv && n <= MAX_POINTS / 2) return flags | MSM_HIP_BASES_ENDOMORPHISM;
  return flags;
}

int reserve_bases(msm_hip_ctx* ctx, size_t n, uint32_t flags) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const bool wide = (flags & MSM_HIP_BASES_PRECOMPUTE_WIDE) != 0;
  const bool tables = (flags & MSM_HIP_BASES_PRECOMPUTE) != 0 || wide, endo = (flags & MSM_HIP_BASES_ENDOMORPHISM) != 0;
  if (n > MAX_POINTS || (tables && n > MAX_PRECOMPUTE_POINTS) || (wide && n > MAX_WIDE_POINTS) || (endo && n > MAX_POINTS / 2) || (tables && endo))
    return MSM_HIP_ERR_INVALID_ARG;
  if ((flags & ~BASE_FLAGS_ALL) || ((flags & MSM_HIP_BASES_PLAIN) && (tables || endo)) || (wide && (flags & MSM_HIP_BASES_PRECOMPUTE)))
    return MSM_HIP_ERR_INVALID_ARG;
  if ((endo && !ctx->ops->glv) || (tables && !ctx->ops->precompute_tables)) return MSM_HIP_ERR_INVALID_ARG;
  if (wide && pick_wide_bits(ctx, n) < 0) return MSM_HIP_ERR_INVALID_ARG;  // (msm_hip_set_wide_bits asked for a width that cannot hold this curve's scalars)
  ctx->n_bases = 0;
  ctx->precomputed = false;
  ctx->wide_bits = 0;
  ctx->endo = false;
  ctx->n_identity = 0;
  ctx->mul.mul_table_bits = 0;  // (msm_hip_mul_base's table belongs to the old set)
  const size_t records = wide ? n * (size_t)wide_tables_of(pick_wide_bits(ctx, n)) : tables ? n * NWIN : endo ? 2 * n : n;
  return grow(ctx, ctx->cap_bases, records, false, [&](size_t c) { return dev_alloc(ctx, ctx->d_bases, c * 2 * (size_t)ctx->ops->coord_words); });
}

// wire bytes at d_xy (may be ctx->d_bases itself: the conversion is element-wise) -> resident Montgomery bases
// (MSM_HIP_BASES_ZERO_IS_IDENTITY: all-zero records are the identity -- marked in d_id_bits, counted in the error word's neighbour d_err[1])
int set_bases_from_device(msm_hip_ctx* ctx, const uint32_t* d_xy, size_t n, uint32_t flags) {
  if (n == 0) return MSM_HIP_OK;
  const bool zero_id = (flags & MSM_HIP_BASES_ZERO_IS_IDENTITY) != 0;
  int rc;
  if (zero_id && (rc = grow(ctx, ctx->cap_id_bits, (n + 63) / 64, false, [&](size_t c) { return dev_alloc(ctx, ctx->d_id_bits, c); }))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, zero_id ? 8 : 4, ctx->stream));
  if (zero_id)
    hipLaunchKernelGGL(ctx->ops->convert_points_zero_id, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, d_xy, ctx->d_bases, n, flags, ctx->d_err,
                       ctx->d_id_bits, ctx->d_err + 1);
  else
    hipLaunchKernelGGL(ctx->ops->convert_points, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, d_xy, ctx->d_bases, n, flags, ctx->d_err);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t bits[2] = {0u, 0u};
  HIP_TRY(ctx, hipMemcpyAsync(bits, ctx->d_err, zero_id ? 8 : 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = err_from_bits(bits[0]))) return rc;
  if (flags & (MSM_HIP_BASES_PRECOMPUTE | MSM_HIP_BASES_PRECOMPUTE_WIDE)) {  // tables 1 .. 15 behind the plain set: T_w[i] = 2^(16 w) P_i (wide: 1 .. 13, 2^(19 w) P_i, the last one top_shift doublings short)
    const bool wide = (flags & MSM_HIP_BASES_PRECOMPUTE_WIDE) != 0;
    const int wb = wide ? pick_wide_bits(ctx, n) : 0;
    hipLaunchKernelGGL(ctx->ops->precompute_tables, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_bases, n, n, wide ? wide_tables_of(wb) : (int)NWIN,
                       wide ? wb : (int)WBITS, wide ? wb - wide_top_shift(ctx->curve, wb) : (int)WBITS);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->precomputed = !wide;
    ctx->wide_bits = wb;
  }
  if (flags & MSM_HIP_BASES_ENDOMORPHISM) {  // phi(P_i) = (beta x_i, y_i) behind the plain set
    hipLaunchKernelGGL(ctx->ops->endo_points, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_bases, n, (size_t)0, n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->endo = true;
  }
  ctx->n_identity = bits[1];
  ctx->n_bases = n;
  return MSM_HIP_OK;
}

}  // namespace

extern "C" {

int msm_hip_set_bases_device(msm_hip_ctx* ctx, const void* xy_dev, size_t n, uint32_t flags) {
  if (!ctx || (!xy_dev && n)) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  flags = resolve_base_flags(ctx, n, flags);
  int rc = reserve_bases(ctx, n, flags);
  if (rc) return rc;
  return set_bases_from_device(ctx, static_cast<const uint32_t*>(xy_dev), n, flags);
}

int msm_hip_set_bases(msm_hip_ctx* ctx, const uint8_t* xy_host, size_t n, uint32_t flags) {
  if (!ctx || (!xy_host && n)) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  flags = resolve_base_flags(ctx, n, flags);
  int rc = reserve_bases(ctx, n, flags);
  if (rc) return rc;
  // the wire bytes land in the bases array itself and are converted in place (same 64 B per point): no staging buffer
  if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bases, xy_host, n * ctx->pb, hipMemcpyHostToDevice, ctx->stream));
  return set_bases_from_device(ctx, ctx->d_bases, n, flags);
}

}  // extern "C"
