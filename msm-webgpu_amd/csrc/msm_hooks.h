// Samplers, the settings' setters and getters, msm_hip_test_env_report, the stage read-back of the last launch and the fq / g1 op hooks.
// Assumes everything of the launch path before it: msm_plan.h, msm_ctx.h, msm_enqueue.h, msm_bases.h and msm_oneshot.h (their environment readers
// are what the report prints), host_pool.h.
#pragma once

extern "C" {

int msm_hip_sample_scalars_device(msm_hip_ctx* ctx, uint64_t seed, size_t n, void* scalars_dev) {
  if (!ctx || (!scalars_dev && n)) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  hipLaunchKernelGGL(ctx->ops->sample_scalars, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, seed, n, static_cast<uint32_t*>(scalars_dev));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_sample_points_device(msm_hip_ctx* ctx, uint64_t seed, size_t n, void* xy_dev) {
  if (!ctx || (!xy_dev && n)) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0) return MSM_HIP_OK;
  if (!ctx->ops->sample_points) return MSM_HIP_ERR_INVALID_ARG;  // (no device sampler for this curve: none at present)
  ON_DEVICE(ctx);
  hipLaunchKernelGGL(ctx->ops->sample_points, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, seed, n, static_cast<uint32_t*>(xy_dev));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_last_stage_ms(msm_hip_ctx* ctx, float* ms, int cap) {
  if (!ctx || !ms) return MSM_HIP_ERR_INVALID_ARG;
  int k = cap < 9 ? cap : 9;
  for (int i = 0; i < k; i++) ms[i] = ctx->stage_ms[i];
  return k;
}

// ---- stage read-back ------------------------------------------------------------------------------------------------
static int read_back(msm_hip_ctx* ctx, void* out, const void* src, size_t bytes, size_t cap_bytes) {
  if (!ctx || !out) return MSM_HIP_ERR_INVALID_ARG;
  if (bytes > cap_bytes) return MSM_HIP_ERR_INVALID_ARG;
  if (bytes == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  for (hipStream_t r : ctx->reduce_stream) HIP_TRY(ctx, hipStreamSynchronize(r));
  HIP_TRY(ctx, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_set_stage_timing(msm_hip_ctx* ctx, int level) {
  if (!ctx || level < 0 || level > 2) return MSM_HIP_ERR_INVALID_ARG;
  ctx->timing_level = level;
  return MSM_HIP_OK;
}

int msm_hip_set_scalar_format(msm_hip_ctx* ctx, uint32_t format) {
  if (!ctx || (format != MSM_HIP_SCALARS_CANONICAL && format != MSM_HIP_SCALARS_MONT256 && !narrow_bytes(format))) return MSM_HIP_ERR_INVALID_ARG;
  if (format == MSM_HIP_SCALARS_MONT256 && !ctx->ops->scalars_from_mont256) return MSM_HIP_ERR_INVALID_ARG;
  ctx->scalar_format = format;
  return MSM_HIP_OK;
}

int msm_hip_set_window_bits(msm_hip_ctx* ctx, int bits) {
  if (!ctx || (bits != 0 && bits != 12 && bits != 14 && bits != 16)) return MSM_HIP_ERR_INVALID_ARG;
  ctx->window_bits = bits;
  return MSM_HIP_OK;
}

int msm_hip_set_wide_bits(msm_hip_ctx* ctx, int bits) {
  if (!ctx || (bits != 0 && (bits < 16 || bits > 20))) return MSM_HIP_ERR_INVALID_ARG;
  ctx->wide_bits_choice = bits;
  return MSM_HIP_OK;
}

int msm_hip_wide_bits(const msm_hip_ctx* ctx) { return ctx ? ctx->wide_bits : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_wide_config(int curve, int bits, size_t n, int* digit_bits, int* tables, int* virtual_windows, int* top_shift) {
  if (curve < MSM_HIP_CURVE_BN254_G1 || curve > MSM_HIP_CURVE_BLS12_381_G2 || (bits != 0 && (bits < 16 || bits > 20))) return MSM_HIP_ERR_INVALID_ARG;
  msm_hip_ctx probe;  // (only the two fields the policy reads)
  probe.curve = curve;
  probe.wide_bits_choice = bits;
  const int wb = pick_wide_bits(&probe, n);
  if (wb < 0) return MSM_HIP_ERR_INVALID_ARG;
  if (digit_bits) *digit_bits = wb;
  if (tables) *tables = wide_tables_of(wb);
  if (virtual_windows) *virtual_windows = wide_vwin_of(wb);
  if (top_shift) *top_shift = wide_top_shift(curve, wb);
  return MSM_HIP_OK;
}

int msm_hip_window_config(int bits, int* num_windows, int* buckets_per_window) {
  if (bits != 12 && bits != 14 && bits != 16) return MSM_HIP_ERR_INVALID_ARG;
  if (num_windows) *num_windows = nwin_of(bits);
  if (buckets_per_window) *buckets_per_window = 1 << (bits - 1);
  return MSM_HIP_OK;
}

int msm_hip_last_window_bits(msm_hip_ctx* ctx) { return ctx ? ctx->last.wbits : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_endomorphism_window_count(int bits) {
  if (bits != 12 && bits != 14 && bits != 16) return MSM_HIP_ERR_INVALID_ARG;
  return nwin_of(bits, true);
}

int msm_hip_uses_endomorphism(const msm_hip_ctx* ctx) { return ctx ? (ctx->endo ? 1 : 0) : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_batch_group_size(msm_hip_ctx* ctx, size_t n) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  return (int)batch_group(ctx, n, (size_t)MAXLW);
}

int msm_hip_set_fine_hist_min_n(msm_hip_ctx* ctx, size_t n) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  ctx->fine_hist_min_n = n;
  return MSM_HIP_OK;
}

int msm_hip_test_skew_credit(const msm_hip_ctx* ctx) { return ctx ? ctx->skew_credit : MSM_HIP_ERR_INVALID_ARG; }

int msm_hip_test_env_report(const msm_hip_ctx* ctx, char* out, size_t cap) {
  if (!out || !cap) return MSM_HIP_ERR_INVALID_ARG;
  size_t len = 0;
  bool fits = true;
  auto put = [&](const char* key, long long v) {
    const int w = snprintf(out + len, cap - len, "%s=%lld\n", key, v);
    if (w < 0 || (size_t)w >= cap - len) fits = false;
    else len += (size_t)w;
  };
  // the settings as the library resolved them (read once per process)
  put("target_lanes", (long long)target_lanes());
  put("chunk_search", chunk_search());
  put("window_bits", env_window_bits());
  put("bpr_logr", bpr_force_logr());
  put("planes_max_w", planes_max_w());
  put("planes_whole", planes_whole());
  put("inline_reduce", inline_reduce_on());
  put("reduce_priority", reduce_priority_on());
  put("smvp_lds_pad", smvp_lds_pad());
  put("bases_auto", bases_auto());
  put("debug_sync", debug_sync());
  put("wide_bits", env_wide_bits());
  put("wide_top_shift", env_wide_top_shift());
  put("wide_slack_ppm", llround(wide_slack() * 1e6));
  put("wide_share_lists", wide_share_lists());
  put("oneshot_parts", env_oneshot_parts());
  put("oneshot_keep", oneshot_keep());
  put("oneshot_overlap", oneshot_overlap());
  put("oneshot_chunk", (long long)oneshot_chunk());
  put("combine_helpers", CombinePool::helpers_wanted());
  put("combine_started", combine_pool().helpers_started());
  // the last upload-bound call (msm_hip_msm_curve, msm_hip_run): its parts and the most upload chunks of one part
  put("upload_parts", g_probe_upload_parts.load());
  put("upload_chunks", g_probe_upload_chunks.load());
  if (ctx) {  // the context's last launch
    put("fine_hist_min_n", (long long)ctx->fine_hist_min_n);
    put("last_wbits", ctx->last.wbits);
    put("last_chunk_len", ctx->last.chunk_len);
    put("last_chunks", ctx->last.chunks);
    put("last_planes", ctx->last.planes);
    put("last_list_path", ctx->last.list_path);
    put("last_mode", ctx->last.mode);
    put("last_w_count", ctx->last.w_count);
    put("last_wide_top_shift", ctx->last.mode == MODE_WIDE ? wide_top_shift(ctx->curve, ctx->last.wide_bits) : 0);
    put("last_logr", ctx->last_logr);
    put("last_inline_reduce", ctx->last_inline_reduce);
    put("last_fine_hist", ctx->last.fine_hist);
    put("last_identity_mask", ctx->last.mask);
  }
  return fits ? (int)len : MSM_HIP_ERR_INVALID_ARG;
}

int msm_hip_set_debug(msm_hip_ctx* ctx, int keep_digit_planes) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  ctx->debug = keep_digit_planes != 0;
  return MSM_HIP_OK;
}

int msm_hip_read_digits(msm_hip_ctx* ctx, uint16_t* out, size_t cap_elems) {
  if (!ctx || !ctx->last.digits) return MSM_HIP_ERR_INVALID_ARG;
  return read_back(ctx, out, ctx->d_digits, ctx->last.n_sc * ctx->last.w_count * 2, cap_elems * 2);
}
int msm_hip_read_col_ptr(msm_hip_ctx* ctx, uint32_t* out, size_t cap_elems) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t half = (size_t)1 << (ctx->last.wbits - 1);  // [w][half + 1]
  return read_back(ctx, out, ctx->slot[ctx->last_slot].d_col_ptr, (size_t)ctx->last.w_count * (half + 1) * 4, cap_elems * 4);
}
int msm_hip_read_val_idxs(msm_hip_ctx* ctx, uint32_t* out, size_t cap_elems) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  // out[w][n]; only the first col_ptr[w][32768] entries of each window are meaningful
  const size_t n = ctx->last.n_sc;
  if (!out || n * ctx->last.w_count > cap_elems) return MSM_HIP_ERR_INVALID_ARG;
  if (n == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  HIP_TRY(ctx, hipMemcpy2DAsync(out, n * 4, ctx->d_val, ctx->last.stride * 4, n * 4, (size_t)ctx->last.w_count, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM_HIP_OK;
}

int msm_hip_read_buckets(msm_hip_ctx* ctx, uint8_t* out, size_t cap_bytes) {
  if (!ctx || !out) return MSM_HIP_ERR_INVALID_ARG;
  const size_t count = (size_t)ctx->last.w_count << (ctx->last.wbits - 1);  // [w][2^(bits-1)]
  if (count * ctx->jb > cap_bytes) return MSM_HIP_ERR_INVALID_ARG;
  if (count == 0) return MSM_HIP_OK;
  ON_DEVICE(ctx);
  for (hipStream_t r : ctx->reduce_stream) HIP_TRY(ctx, hipStreamSynchronize(r));
  int rc = ensure_stage(ctx, count * ctx->jb);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->export_buckets, dim3(blocks_for(count, 256)), dim3(256), 0, ctx->stream, ctx->slot[ctx->last_slot].d_buckets,
                     reinterpret_cast<uint32_t*>(ctx->d_stage), count);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, ctx->d_stage, count * ctx->jb, cap_bytes);
}

int msm_hip_read_window_sums(msm_hip_ctx* ctx, uint8_t* out, size_t cap_bytes) {
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const Slot& s = ctx->slot[ctx->last_slot];
  if (!s.parts) return read_back(ctx, out, s.d_wsums, (size_t)ctx->last.w_count * ctx->jb, cap_bytes);
  // the last launch handed its window sums to the host as bit-plane sums (k_bpr_planes): finish them here
  const size_t w = (size_t)ctx->last.w_count;
  if (!out || w * ctx->jb > cap_bytes || w > 24) return MSM_HIP_ERR_INVALID_ARG;
  const size_t plane_bytes = PLANES_PER_WINDOW * ctx->jb;
  {  // (the plane sums were written into the slot's pinned buffer by the launch's last kernel: complete once its reduce stream has drained)
    ON_DEVICE(ctx);
    for (hipStream_t r : ctx->reduce_stream) HIP_TRY(ctx, hipStreamSynchronize(r));
  }
  const uint8_t* planes = s.h_wsums;
  bool ok = true;
  for (size_t k = 0; k < w; k++) ok &= ctx->ops->window_from_planes(planes + k * plane_bytes, out + k * ctx->jb);
  return ok ? MSM_HIP_OK : MSM_HIP_ERR_NONCANONICAL;
}

// ---- op hooks -------------------------------------------------------------------------------------------------------
static int run_hook(msm_hip_ctx* ctx, const uint8_t* a, size_t a_bytes, const uint8_t* b, size_t b_bytes, uint8_t* out,
                    size_t out_bytes, uint8_t*& da, uint8_t*& db, uint8_t*& dout) {
  if (!ctx || !a || !out) return MSM_HIP_ERR_INVALID_ARG;
  ON_DEVICE(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  int rc = ensure_stage(ctx, up16(a_bytes) + up16(b_bytes) + up16(out_bytes) + 16);
  if (rc) return rc;
  da = ctx->d_stage;
  db = da + up16(a_bytes);
  dout = db + up16(b_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(da, a, a_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (b && b_bytes) HIP_TRY(ctx, hipMemcpyAsync(db, b, b_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!b) db = nullptr;
  return MSM_HIP_OK;
}

int msm_hip_test_fq_op(msm_hip_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  if (n == 0) return MSM_HIP_OK;
  if (op < 0 || op > 9) return MSM_HIP_ERR_INVALID_ARG;
  uint8_t *da, *db, *dout;
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t cb = ctx->cb;
  int rc = run_hook(ctx, a, n * cb, b, b ? n * cb : 0, out, n * cb, da, db, dout);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->test_fq, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, op, (const uint32_t*)da, (const uint32_t*)db,
                     (uint32_t*)dout, n);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, dout, n * cb, n * cb);
}

int msm_hip_test_g1_op(msm_hip_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  if (n == 0) return MSM_HIP_OK;
  if (op < 0 || op > 4 || (op != 1 && !b)) return MSM_HIP_ERR_INVALID_ARG;
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t jb = ctx->jb;
  const size_t b_bytes = op == 0 ? n * jb : (op >= 2 ? n * ctx->pb : 0);
  uint8_t *da, *db, *dout;
  int rc = run_hook(ctx, a, n * jb, op == 1 ? nullptr : b, b_bytes, out, n * jb, da, db, dout);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->test_g1, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, op, (const uint32_t*)da, (const uint32_t*)db,
                     (uint32_t*)dout, n);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, dout, n * jb, n * jb);
}

int msm_hip_test_g1_mul_u32(msm_hip_ctx* ctx, const uint8_t* a, const uint32_t* k, uint8_t* out, size_t n) {
  if (n == 0) return MSM_HIP_OK;
  if (!k) return MSM_HIP_ERR_INVALID_ARG;
  uint8_t *da, *db, *dout;
  if (!ctx) return MSM_HIP_ERR_INVALID_ARG;
  const size_t jb = ctx->jb;
  int rc = run_hook(ctx, a, n * jb, reinterpret_cast<const uint8_t*>(k), n * 4, out, n * jb, da, db, dout);
  if (rc) return rc;
  hipLaunchKernelGGL(ctx->ops->test_g1_mul_u32, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)da,
                     (const uint32_t*)db, (uint32_t*)dout, n);
  HIP_TRY(ctx, hipGetLastError());
  return read_back(ctx, out, dout, n * jb, n * jb);
}

}  // extern "C"
