// Group FFT over the resident bases, host side (the kernels: msm_kernels.h, k_fft_stage ...).  Its state is the context's FftState (msm_ctx.h); the
// ladder choice is the batch scalar multiplication's (MulState::mul_force_ladder).
// Assumes host_fr.h, msm_ctx.h, msm_mul.h (prime_order_curve) and, of msm_hip.hip, no_context_code.
#pragma once


// ---- group FFT over the resident bases: out[i] = c * sum_j omega^(i j) P_j (include/msm_hip.h, msm_hip_bases_fft) -----------------------------------
namespace {
// `host`: out is host memory (the last pass writes into the scratch, copied out at the end); else device memory, written in place.
// Every argument is checked before anything is enqueued.  log_n stages on the main stream (msm_kernels.h, k_fft_stage): the first reads the resident
// bases through the bit-reversed index into the scratch, the others run in place there -- a butterfly touches its own two elements only -- and the
// last pass of the call (the last stage, or the scale pass behind it) writes the output records, which k_mul_normalize makes wire records.
int fft_impl(msm_hip_ctx* ctx, const uint8_t* omega, int log_n, void* out, uint32_t flags, bool host) {
  if (!ctx) return no_context_code();
  if (flags & ~(MSM_HIP_MUL_BASES_ORDER_R | MSM_HIP_FFT_SCALE_INV_N)) return MSM_HIP_ERR_INVALID_ARG;
  const CurveOps* ops = ctx->ops;
  if (!ops->fft_normalize) return MSM_HIP_ERR_INVALID_ARG;  // the G2 groups
  if (!omega || !out || log_n < 0 || log_n > 28) return MSM_HIP_ERR_INVALID_ARG;
  if (!host && (reinterpret_cast<uintptr_t>(out) & 15u)) return MSM_HIP_ERR_INVALID_ARG;  // (16-byte vector accesses)
  if (ctx->n_bases == 0) return MSM_HIP_ERR_NO_BASES;
  const size_t n = (size_t)1 << log_n;
  if (n > ctx->n_bases) return MSM_HIP_ERR_INVALID_ARG;
  const host_fr::Field fr(ops->fr_r);
  if (!host_fr::is_primitive_root(fr, omega, log_n)) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  const size_t cw = (size_t)ops->coord_words, ptw = 2 * cw;
  const bool endo = ops->glv && (ctx->mul.mul_force_ladder ? ctx->mul.mul_force_ladder == 2 : prime_order_curve(ctx->curve) || (flags & MSM_HIP_MUL_BASES_ORDER_R));
  const bool scale = (flags & MSM_HIP_FFT_SCALE_INV_N) && log_n > 0;  // (1 / 1 = 1)
  hipStream_t st = ctx->stream;
  const uint64_t* id_bits = ctx->n_identity ? ctx->d_id_bits : nullptr;
  const size_t n4 = (n + 3) & ~(size_t)3;  // (every part of the scratch stays 16-byte aligned)
  int rc = grow(ctx, ctx->fft.cap_fft, n4 * (ptw + 2 * cw) + 8 + (host ? n4 * ptw : 0), true, [&](size_t c) { return dev_alloc(ctx, ctx->fft.d_fft, c); });
  if (rc) return rc;
  uint32_t* work = ctx->fft.d_fft;
  uint32_t* zbuf = work + n4 * ptw;
  uint32_t* prefix = zbuf + n4 * cw;
  uint32_t* d_scalar = prefix + n4 * cw;
  uint32_t* d_out = host ? d_scalar + 8 : static_cast<uint32_t*>(out);
  if (log_n >= 2 && !(ctx->fft.fft_tw_log_n == log_n && memcmp(ctx->fft.fft_tw_omega, omega, 32) == 0)) {  // (stage 0's twiddles are all 1)
    std::vector<uint32_t> tw;
    host_fr::twiddle_table(fr, omega, log_n, tw);
    if ((rc = grow(ctx, ctx->fft.cap_fft_tw, tw.size(), true, [&](size_t c) { return dev_alloc(ctx, ctx->fft.d_fft_tw, c); }))) return rc;
    ctx->fft.fft_tw_log_n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->fft.d_fft_tw, tw.data(), tw.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (an earlier call's kernels no longer read the old table; `tw` may go)
    ctx->fft.fft_tw_log_n = log_n;
    memcpy(ctx->fft.fft_tw_omega, omega, 32);
  }
  uint32_t k[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (scale) host_fr::inverse_of_n(fr, log_n, k);
  if (scale || log_n == 0) {
    HIP_TRY(ctx, hipMemcpyAsync(d_scalar, k, 32, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  const int ladder = endo ? 2 : 1;
  const unsigned norm_blocks = blocks_for(n, 256 * (size_t)ops->mul_chunk);
  if (log_n == 0) {  // one element: the base itself, through the ladder's kernel with the scalar 1 (an identity base gives the all-zero record)
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, 4, st));
    hipLaunchKernelGGL(ops->mul_each[0], dim3(1), dim3(256), 0, st, (const uint32_t*)ctx->d_bases, (const uint32_t*)d_scalar, (size_t)1, (size_t)0, 1u, id_bits, d_out, zbuf,
                       ctx->d_err, 1u);
    AFTER_KERNEL(ctx, "k_mul_each (fft, n = 1)", st);
  }
  for (int s = 0; s < log_n; s++) {
    const bool last = s == log_n - 1 && !scale;
    hipLaunchKernelGGL(ops->fft_stage[s == 0 ? 0 : ladder], dim3(blocks_for(n / 2, 256)), dim3(256), 0, st, s == 0 ? (const uint32_t*)ctx->d_bases : (const uint32_t*)work,
                       last ? d_out : work, zbuf, (const uint32_t*)ctx->fft.d_fft_tw, log_n, s, s == 0 ? 1u : 0u, id_bits);
    AFTER_KERNEL(ctx, "k_fft_stage", st);
    if (!last) {
      hipLaunchKernelGGL(ops->fft_normalize, dim3(norm_blocks), dim3(256), 0, st, work, (const uint32_t*)zbuf, prefix, n);
      AFTER_KERNEL(ctx, "k_fft_normalize", st);
    }
  }
  if (scale) {
    hipLaunchKernelGGL(ops->fft_scale[ladder - 1], dim3(blocks_for(n, 256)), dim3(256), 0, st, (const uint32_t*)work, d_out, zbuf, (const uint32_t*)d_scalar, n);
    AFTER_KERNEL(ctx, "k_fft_scale", st);
  }
  hipLaunchKernelGGL(ops->mul_normalize, dim3(norm_blocks), dim3(256), 0, st, d_out, (const uint32_t*)zbuf, prefix, n);
  AFTER_KERNEL(ctx, "k_mul_normalize (fft)", st);
  HIP_TRY(ctx, hipGetLastError());
  if (host) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, n * ctx->pb, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->fft.fft_last_stages = log_n;
  ctx->fft.fft_last_ladder = (log_n >= 2 || scale) ? ladder : 0;
  return MSM_HIP_OK;
}
}  // namespace

extern "C" {
int msm_hip_bases_fft(msm_hip_ctx* ctx, const uint8_t omega[32], int log_n, uint8_t* out_xy_host, uint32_t flags) {
  return fft_impl(ctx, omega, log_n, out_xy_host, flags, true);
}
int msm_hip_bases_fft_device(msm_hip_ctx* ctx, const uint8_t omega[32], int log_n, void* out_xy_dev, uint32_t flags) {
  return fft_impl(ctx, omega, log_n, out_xy_dev, flags, false);
}
int msm_hip_test_fft_last(const msm_hip_ctx* ctx, int* stages, int* ladder) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  if (stages) *stages = ctx->fft.fft_last_stages;
  if (ladder) *ladder = ctx->fft.fft_last_ladder;
  return MSM_HIP_OK;
}
}  // extern "C"
