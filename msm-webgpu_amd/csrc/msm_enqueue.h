// The two stages of a launch's enqueue: enqueue_sort (main stream: mask, recode, the sort passes) and enqueue_reduce (SMVP on the main stream, stitch
// and bucket reduce on the slot's reduce stream), with what only they use -- dispatch (a runtime value to a kernel template's parameter), the row /
// column variant of the bucket reduce (pick_rowcol) and two tuning aids.  Nothing else lives here.
// Assumes sort_kernels.h (the curve-neutral kernels), curve_ops.h, msm_plan.h (LaunchPlan) and msm_ctx.h (the context, Slot, HIP_TRY, AFTER_KERNEL).
#pragma once

namespace {
// f(std::integral_constant<decltype(V), V>{}) for the V among V0, Vs... that equals the runtime value `v` -- the last one for any other value:
// a kernel template is instantiated for exactly the values listed
template <auto V0, auto... Vs, typename F>
void dispatch(decltype(V0) v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<decltype(V0), V0>{});
  else if (v == V0) f(std::integral_constant<decltype(V0), V0>{});
  else dispatch<Vs...>(v, f);
}

// The launch's first stage, on the main stream: everything that needs the scalars alone -- recode, the two sort passes and the fine sort (+ the
// debug read-back's ordering).  The slot's previous occupant (bucket reduce + copies on the reduce stream) must have drained; its error word was
// re-zeroed at the end of that chain.  Stage events cost a few microseconds of queue time each, so only the ones the current timing level asks
// for are recorded.
int enqueue_sort(msm_hip_ctx* ctx, LaunchPlan& p, Slot& s, const uint32_t* d_scalars) {
  const bool merge = p.mode == MODE_TABLES, halves = p.mode == MODE_HALVES, wide = p.mode == MODE_WIDE;
  const bool bytes = byte_windows(p.nb);  // U8 / U16, I8 / I16: byte windows with their own one-level sort (sort_kernels.h: k_byte_count ...)
  const size_t merge_nb = merge || wide ? ctx->n_bases : 0;
  hipStream_t st = ctx->stream;
  const dim3 grid(p.tiles, p.nvec), block(256);
  uint32_t* d_err = reinterpret_cast<uint32_t*>(s.d_wsums + WSUM_BYTES);
  // the SMVP chunk length the device settles on for this launch (k_scatter_coarse -> fine sort, SMVP, stitch): a word of the slot
  uint32_t* d_chunk_len = s.d_big_queue + BIGQ_CHUNK_LEN;
  const int tl = ctx->timing_level;
  auto mark = [&](int i) { return tl >= 2 ? hipEventRecord(s.ev[i], st) : hipSuccess; };
  HIP_TRY(ctx, hipStreamWaitEvent(st, s.done, 0));
  HIP_TRY(ctx, mark(0));
  const bool mont = ctx->scalar_format == MSM_HIP_SCALARS_MONT256 && !p.nb;
  if (p.mask) {  // identity records among the bases: a copy of the scalars with theirs zeroed, before anything validates or converts them (stage 0)
    uint8_t* masked = reinterpret_cast<uint8_t*>(ctx->d_scalar_conv) + (mont ? (size_t)p.nvec * p.n * 32 : 0);  // (behind the canonical copies)
    dispatch<32, 16, 8, 4, 2, 1>(p.nb ? p.nb : 32, [&](auto w) {  // (by width: zeroing does not ask about the sign)
      hipLaunchKernelGGL(k_mask_identity<decltype(w)::value>, dim3(blocks_for(p.n, 256), p.nvec), dim3(256), 0, st, (const uint8_t*)d_scalars, masked, p.n,
                         p.base_off, (const uint64_t*)ctx->d_id_bits, (uint32_t)ctx->n_bases, p.sparse ? p.indices : (const uint32_t*)nullptr);
    });
    AFTER_KERNEL(ctx, "k_mask_identity", st);
    d_scalars = reinterpret_cast<const uint32_t*>(masked);
  }
  if (mont) {  // Montgomery-form scalars: canonical copies first (part of stage 0)
    const size_t count = (size_t)p.nvec * p.n;
    hipLaunchKernelGGL(ctx->ops->scalars_from_mont256, dim3(blocks_for(count, 256)), dim3(256), 0, st, d_scalars, ctx->d_scalar_conv, count, d_err);
    AFTER_KERNEL(ctx, "k_scalars_from_mont256", st);
    d_scalars = ctx->d_scalar_conv;
  }
  const unsigned gpos_bytes = (unsigned)(merge ? p.nvec : p.nvec * p.w_count_vec) * NCOARSE * 4;  // k_scatter_coarse's run cursors (dynamic LDS)
  const int top_shift = wide ? wide_top_shift(ctx->curve, p.wide_bits) : 0;
  // inputs of the two-level sort: 32-byte scalars (8 words) or the endomorphism's halves (4), or narrow scalars of 4 / 8 / 16 bytes (1 / 2 / 4
  // words), unsigned or signed.  f(C, SW, NB) for the kernel parameters of this launch.
  const int sw = halves ? 4 : 8;
  auto sort_input = [&](auto f) {
    dispatch<16, 14, 12>(p.wbits, [&](auto c) {
      dispatch<4, 8, 16, -4, -8, -16, 0>(p.nb_kernel(), [&](auto b) {
        constexpr int NB = decltype(b)::value;
        if constexpr (NB != 0) f(c, std::integral_constant<int, (narrow_width(NB) + 3) / 4>{}, b);
        else dispatch<8, 4>(sw, [&](auto w) { f(c, w, b); });
      });
    });
  };
  // first pass: recode + coarse histogram (+ digit planes: 1 = debug read-back, 2 = the second pass reads them).  Endomorphism launches:
  // the same kernel splits every scalar k = k1 + k2 lambda itself and leaves the halves (interleaved: input 2 j = k1 of scalar j, 2 j + 1 =
  // k2; a vector's 2n halves take the room of its n scalars, vector stride n * 8 words either way) for a scalar-reading second pass.
  uint16_t* digits = p.digits ? ctx->d_digits : nullptr;
  uint16_t* plane_out = p.planes ? ctx->d_digits : digits;
  const int plane_mode = p.planes ? 2 : (digits ? 1 : 0);
  // sparse launches: the same passes instantiated with one more argument (msm_layout.h: SparseIdx) -- the count passes guard the indices, the
  // scatter passes write them in place of the positions
  const SparseIdx sp{p.indices, (uint32_t)ctx->n_bases, d_err};
  // k_count leaves the prefix over tiles and the bin totals itself (bin_fill); the other first passes are followed by a scan kernel
  const bool fused_scan = !wide && !bytes;
  const uint32_t* bin_total = fused_scan ? ctx->d_bin_fill : ctx->d_bin_total;
  if (fused_scan) {
    if (ctx->bin_fill_dirty) HIP_TRY(ctx, hipMemsetAsync(ctx->d_bin_fill, 0, (size_t)MAXLW * NCOARSE * 4, st));
    ctx->bin_fill_dirty = true;  // (until this launch's k_sort_fine is in the stream)
  }
  if (wide) {
    dispatch<16, 17, 18, 19, 20>(p.wide_bits, [&](auto c) {
      constexpr int C = decltype(c)::value;
      if (p.list_path)
        hipLaunchKernelGGL(k_count_wide_list<C>, grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.nvec, p.n * 8, ctx->d_counts, d_err, top_shift,
                           p.v_begin, p.v_count, ctx->d_val, ctx->d_list_len, p.stride, p.subtiles);
      else
        hipLaunchKernelGGL(k_count_wide<C>, grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.nvec, p.n * 8, ctx->d_counts, d_err, top_shift,
                           p.v_begin, p.v_count);
    });
  } else if (bytes) {
    dispatch<1, 2, -1, -2>(p.nb_kernel(), [&](auto b) {
      if (p.sparse)
        hipLaunchKernelGGL((k_byte_count<decltype(b)::value, SparseIdx>), grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.tile_len, p.tiles, ctx->d_counts, sp);
      else
        hipLaunchKernelGGL(k_byte_count<decltype(b)::value>, grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.tile_len, p.tiles, ctx->d_counts);
    });
  } else if (halves) {
    const int k = p.wbits == 16 ? 2 : p.wbits == 14 ? 1 : 0;
    if (p.sparse)
      hipLaunchKernelGGL(ctx->ops->count_split_sparse[k], grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin, p.w_count_vec, p.nvec, p.n * 8,
                         ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, (uint64_t*)nullptr, ctx->d_halves, d_err, merge_nb, sp);
    else
      hipLaunchKernelGGL(ctx->ops->count_split[k], grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin,
                         p.w_count_vec, p.nvec, p.n * 8, ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, p.planes ? ctx->d_negbits : nullptr,
                         p.planes ? nullptr : ctx->d_halves, d_err, merge_nb);
    d_scalars = ctx->d_halves;
  } else {
    sort_input([&](auto c, auto w, auto b) {
      constexpr int C = decltype(c)::value, SW = decltype(w)::value, NB = decltype(b)::value;
      if constexpr (NB != 0 || SW == 8) {  // (the halves were counted above, by the pass that splits them)
        const size_t vec_stride = p.n * (NB ? narrow_width(NB) : 8);
        if (p.sparse)
          hipLaunchKernelGGL((k_count<C, SW, void, NB, SparseIdx>), grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin, p.w_count_vec,
                             p.nvec, vec_stride, ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, (uint64_t*)nullptr, (uint32_t*)nullptr, d_err, merge_nb, sp);
        else
          hipLaunchKernelGGL((k_count<C, SW, void, NB>), grid, block, 0, st, d_scalars, p.n_sc, p.tile_len, p.tiles, p.w_begin, p.w_count_vec, p.nvec,
                             vec_stride, ctx->d_counts, ctx->d_bin_fill, plane_out, plane_mode, (uint64_t*)nullptr, (uint32_t*)nullptr, d_err, merge_nb);
      }
    });
  }
  AFTER_KERNEL(ctx, "k_count", st);
  HIP_TRY(ctx, mark(1));
  if (bytes) hipLaunchKernelGGL(k_byte_scan, dim3(BYTE_BINS / 4, p.w_count), dim3(256), 0, st, ctx->d_counts, p.tiles, ctx->d_bin_total);
  else if (!fused_scan) hipLaunchKernelGGL(k_scan_tiles, dim3(NCOARSE / 4, p.w_count), dim3(256), 0, st, ctx->d_counts, p.tiles, ctx->d_bin_total);  // all 128 bins: the scatter scans them
  if (!fused_scan) AFTER_KERNEL(ctx, "k_scan_tiles", st);
  HIP_TRY(ctx, mark(2));
  if (p.list_path) {  // shares of at most WIDE_SHARE_VWIN_MAX virtual windows: from the first pass's lists
    hipLaunchKernelGGL(k_scatter_list, dim3(p.tiles, p.w_count), dim3(256), 0, st, (const uint32_t*)ctx->d_val, (const uint32_t*)ctx->d_list_len, p.stride,
                       (uint32_t)(LIST_SUB * wide_tables_of(p.wide_bits)), p.subtiles, p.n_sc, p.tile_len, p.tiles, p.w_count, ctx->d_counts, ctx->d_bin_total,
                       ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine, merge_nb, p.chunks, p.chunk_len, d_chunk_len);
  } else if (wide) {  // (... or, MSM_HIP_WIDE_SHARE_LISTS=0, the small shape of the two-pass kernel: four workgroups per CU instead of one)
    dispatch<16, 17, 18, 19, 20>(p.wide_bits, [&](auto c) {
      dispatch<true, false>(p.share_shape, [&](auto share) {
        constexpr int C = decltype(c)::value;
        constexpr bool SHARE = decltype(share)::value;
        hipLaunchKernelGGL((k_scatter_wide<C, SHARE>), grid, dim3(WideScatterShape<C, SHARE>::THREADS), 0, st, d_scalars, p.n_sc, p.stride, p.tile_len, p.tiles,
                           p.nvec, p.n * 8, ctx->d_counts, ctx->d_bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine, merge_nb, p.chunks, p.chunk_len,
                           d_chunk_len, top_shift, p.v_begin, p.v_count);
      });
    });
  } else if (p.planes) {
    hipLaunchKernelGGL(k_scatter_planes, dim3(p.tiles), dim3(256), 0, st, ctx->d_digits, halves ? ctx->d_negbits : (const uint64_t*)nullptr, p.n_sc, p.stride,
                       p.tile_len, p.tiles, p.w_count, p.w_count_vec, ctx->d_counts, bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine,
                       (uint32_t)ctx->n_bases, p.chunks, p.chunk_len, d_chunk_len);
  } else if (bytes) {
    dispatch<1, 2, -1, -2>(p.nb_kernel(), [&](auto b) {
      if (p.sparse)
        hipLaunchKernelGGL((k_byte_scatter<decltype(b)::value, SparseIdx>), grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.stride, p.tile_len, p.tiles,
                           p.w_count, ctx->d_counts, ctx->d_bin_total, s.d_col_ptr, p.half, ctx->d_val, p.chunks, p.chunk_len, d_chunk_len, sp);
      else
        hipLaunchKernelGGL(k_byte_scatter<decltype(b)::value>, grid, block, 0, st, (const uint8_t*)d_scalars, p.n, p.stride, p.tile_len, p.tiles, p.w_count,
                           ctx->d_counts, ctx->d_bin_total, s.d_col_ptr, p.half, ctx->d_val, p.chunks, p.chunk_len, d_chunk_len);
    });
  } else {
    sort_input([&](auto c, auto w, auto b) {
      constexpr int C = decltype(c)::value, SW = decltype(w)::value, NB = decltype(b)::value;
      const size_t vec_stride = p.n * (NB ? narrow_width(NB) : 8);
      if (p.sparse)
        hipLaunchKernelGGL((k_scatter_coarse<C, SW, NB, SparseIdx>), grid, block, gpos_bytes, st, d_scalars, p.n_sc, p.stride, p.tile_len, p.tiles, p.w_begin,
                           p.w_count_vec, p.nvec, vec_stride, ctx->d_counts, bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine,
                           merge_nb, (uint32_t)p.n, halves ? (uint32_t)ctx->n_bases : 0u, p.chunks, p.chunk_len, d_chunk_len, sp);
      else
        hipLaunchKernelGGL((k_scatter_coarse<C, SW, NB>), grid, block, gpos_bytes, st, d_scalars, p.n_sc, p.stride, p.tile_len, p.tiles, p.w_begin,
                           p.w_count_vec, p.nvec, vec_stride, ctx->d_counts, bin_total, ctx->d_coarse_ptr, ctx->d_tmp_val, ctx->d_tmp_fine,
                           merge_nb, (uint32_t)p.n, halves ? (uint32_t)ctx->n_bases : 0u, p.chunks, p.chunk_len, d_chunk_len);
    });
  }
  AFTER_KERNEL(ctx, "k_scatter_coarse", st);
  HIP_TRY(ctx, mark(3));
  // large n: the sub-range histograms of huge coarse bins are made once, not by every sharer.  (round 5) Not launched at all while uniform scalars
  // cannot fill a coarse bin to three quarters of FINE_BIG -- 2^20 points and below: its 8192 workgroups found nothing to do and took 19 us of every
  // launch's main stream; skewed scalars that make such a bin after all take the sharers' own histograms (k_sort_fine's fallback path)
  // ... ADAPTIVELY (later in round 5): few distinct / small / equal scalars (witness vectors) fill huge bins at any size, and the fallback costs their
  // fine sort 2 - 2.5 x (profiles/r05_skew_hist.txt): k_sort_fine reports a huge bin in the slot's status word, and the 64 launches after such a
  // report run k_fine_hist (a prover's MSMs come in series of like inputs; the first of a series pays the fallback once).  The report means SKEW:
  // a bin of more than HUGE_BIN_MEANS mean bins -- the top window of endomorphism halves reaches two means, which at 2^20 is FINE_BIG, and used to
  // keep the kernel in every launch of uniform scalars; such bins are shared without histograms at no measurable cost (sort_kernels.h: k_sort_fine)
  // Narrow scalars always run it and leave the credit alone: their top window holds only the recode's carry (U8: all entries) -- one huge bin by
  // construction, which says nothing about the context's later 32-byte launches
  if (bytes) {  // byte windows: the scatter has grouped the entries by slot already; only the SMVP's chunk table is left
    hipLaunchKernelGGL(k_byte_chunks, dim3(blocks_for(p.chunks, 256), p.w_count), dim3(256), 0, st, (const uint32_t*)s.d_col_ptr, p.half, p.chunks,
                       (const uint32_t*)d_chunk_len, ctx->d_chunk_slot);
    AFTER_KERNEL(ctx, "k_byte_chunks", st);
  } else {
    const uint32_t* part_hist = nullptr;
    const bool hist_useful = p.nb || ctx->fine_hist_min_n != FINE_BIG + 1 || p.n_entries / p.ncoarse * 4 > (size_t)FINE_BIG * 3 || ctx->skew_credit > 0;
    if (ctx->skew_credit > 0 && !p.nb) ctx->skew_credit--;
    p.fine_hist = p.n_entries >= ctx->fine_hist_min_n && hist_useful;
    if (p.fine_hist) {
      hipLaunchKernelGGL(k_fine_hist, dim3(p.ncoarse, p.w_count, FINE_SPLIT), dim3(256), 0, st, ctx->d_tmp_fine, p.stride, ctx->d_coarse_ptr,
                         ctx->d_part_hist);
      AFTER_KERNEL(ctx, "k_fine_hist", st);
      part_hist = ctx->d_part_hist;
    }
    hipLaunchKernelGGL(k_sort_fine, dim3(p.ncoarse, p.w_count, FINE_SPLIT), dim3(256), 0, st, ctx->d_tmp_val, ctx->d_tmp_fine, p.stride, ctx->d_coarse_ptr,
                       s.d_col_ptr, ctx->d_val, p.chunks, d_chunk_len, ctx->d_chunk_slot, part_hist, d_err, fused_scan ? ctx->d_bin_fill : (uint32_t*)nullptr);
    AFTER_KERNEL(ctx, "k_sort_fine", st);
    if (fused_scan) ctx->bin_fill_dirty = false;
  }
  if (ctx->debug) {  // deterministic transpose for the stage read-back: every slot's run in ascending order
    hipLaunchKernelGGL(k_order_runs, dim3(blocks_for(p.n_entries, 256), p.w_count), dim3(256), 0, st, s.d_col_ptr, ctx->d_val, ctx->d_tmp_val, p.stride, p.half);
    hipLaunchKernelGGL(k_copy_runs, dim3(blocks_for(p.n_entries, 256), p.w_count), dim3(256), 0, st, s.d_col_ptr, ctx->d_tmp_val, ctx->d_val, p.stride, p.half);
    AFTER_KERNEL(ctx, "k_order_runs", st);
  }
  return MSM_HIP_OK;
}

// The bucket reduce's row / column pass: the curve's k_bpr_rowcol<LOG_R, LOG_ROWS> and its workgroups per window.  Serial run per thread before
// the LDS tree: 16 buckets when many windows are reduced at once (fewest wave-additions), 4 for a few windows (shallowest); measured optimum for 16
// and for 2 windows respectively
struct RowCol {
  void (*kernel)(const uint32_t*, uint32_t*, uint32_t*);
  int blocks;
  int logr;  // LOG_R of the variant (test hook msm_hip_test_env_report)
};
inline int bpr_force_logr() {  // tuning aid
  static const int v = [] { const char* e = getenv("MSM_HIP_BPR_LOGR"); return e ? atoi(e) : 0; }();
  return v;
}
RowCol pick_rowcol(const msm_hip_ctx* ctx, const LaunchPlan& p, const Slot& s) {
  const int force_logr = bpr_force_logr();
  const CurveOps* o = ctx->ops;
  if (p.wbits == 16) {
    // one small MSM alone in its launch (8 half-length windows, up to 2^18 points): 8 buckets per thread -- its latency is what counts
    // (-4 % at 2^16, -2.6 % at 2^18; the same setting costs grouped launches 3 - 16 % and a pipelined 2^20 MSM 0.5 %)
    // ... and so is a larger one that has the GPU to itself: no other result slot of the context is in flight when it is launched
    // (latency 1.81 -> 1.77 ms at 2^20; in a pipeline only the very first launch is alone: throughput unchanged)
    bool alone = p.nvec == 1 && p.w_count == 8;
    for (const Slot& q : ctx->slot) alone = alone && (&q == &s || !q.pending);
    const bool small_single = p.nvec == 1 && p.w_count == 8 && (p.n_entries <= ((size_t)1 << 19) || alone);
    if (force_logr == 4 || (force_logr == 0 && p.w_count >= 8 && !small_single)) return {o->rowcol_4_8, bpr_rowcol_blocks<4, 8>(), 4};
    if (force_logr == 3 || (force_logr == 0 && small_single)) return {o->rowcol_3_8, bpr_rowcol_blocks<3, 8>(), 3};
    return {o->rowcol_2_8, bpr_rowcol_blocks<2, 8>(), 2};
  }
  if (p.wbits == 14) {  // 64 rows x 128 columns
    if (force_logr == 4 || (force_logr == 0 && p.w_count > 2 * nwin_of(14))) return {o->rowcol_4_6, bpr_rowcol_blocks<4, 6>(), 4};
    return {o->rowcol_2_6, bpr_rowcol_blocks<2, 6>(), 2};
  }
  return {o->rowcol_2_4, bpr_rowcol_blocks<2, 4>(), 2};  // 16 rows x 128 columns
}

// The launch's second stage: the SMVP (it reads the bases) on the main stream, then stitch + bucket reduce on the slot's reduce stream, few waves
// of long dependent chains; the error word and, for the host, the window sums go to the slot's pinned buffer.  Returns without waiting.
inline bool inline_reduce_on() {  // MSM_HIP_INLINE_REDUCE=0: the stitch and the bucket reduce always on the reduce stream
  static const bool v = [] { const char* e = getenv("MSM_HIP_INLINE_REDUCE"); return !e || atoi(e) != 0; }();
  return v;
}
inline unsigned smvp_lds_pad() {  // A/B aid: dynamic LDS added to the SMVP's workgroups
  static const unsigned v = [] { const char* e = getenv("MSM_HIP_SMVP_LDS_PAD"); const long v = e ? atol(e) : 0; return v > 0 && v <= 65536 ? (unsigned)v : 0u; }();
  return v;
}
int enqueue_reduce(msm_hip_ctx* ctx, const LaunchPlan& p, Slot& s) {
  hipStream_t st = ctx->stream, rs = ctx->reduce_stream[(&s - ctx->slot) % NREDUCE];
  // a synchronous call with nothing else in flight (msm_hip_run_*: the caller waits for this launch before it issues another): the stitch and
  // the bucket reduce follow the SMVP on the MAIN stream -- no cross-stream hand-off (an event wait costs ~10 us more than an in-stream kernel
  // boundary), and no next launch exists whose sort the separate stream would let overlap.  MSM_HIP_INLINE_REDUCE=0: always the reduce stream.
  if (inline_reduce_on() && p.sync) {
    bool others = false;
    for (const Slot& o : ctx->slot) others = others || (&o != &s && o.pending);
    if (!others) rs = st;
  }
  const bool to_host = !p.sums_dev;
  uint32_t* wsums_out = static_cast<uint32_t*>(to_host ? s.d_wsums : p.sums_dev);
  uint32_t* d_err = reinterpret_cast<uint32_t*>(s.d_wsums + WSUM_BYTES);
  uint32_t* d_chunk_len = s.d_big_queue + BIGQ_CHUNK_LEN;
  const int tl = ctx->timing_level;
  // the SMVP's own begin / end timestamps: attached to its dispatch (hipExtLaunchKernelGGL) instead of two event packets around it -- a
  // packet between two kernels costs a few microseconds of queue time, and these two sat between every launch's sort and its SMVP and
  // between the SMVP and the next launch (bench.py times every launch's SMVP for the roofline figure).  Level 2 keeps the packets: its
  // stage boundaries are read as differences of consecutive events.
  HIP_TRY(ctx, tl >= 2 ? hipEventRecord(s.ev[4], st) : hipSuccess);
  hipExtLaunchKernelGGL(ctx->ops->smvp_chunks, dim3((p.chunks + 255) / 256, p.w_count), dim3(256), smvp_lds_pad(), st, tl == 1 ? s.ev[4] : nullptr,
                        tl == 1 ? s.ev[5] : nullptr, 0, (const uint32_t*)(ctx->d_bases + p.base_off * 2 * (size_t)ctx->ops->coord_words), (const uint32_t*)s.d_col_ptr,
                        (const uint32_t*)ctx->d_val, p.stride, p.chunks, (const uint32_t*)d_chunk_len, (const uint32_t*)ctx->d_chunk_slot, s.d_buckets, s.d_heads,
                        s.d_tails, p.half);
  AFTER_KERNEL(ctx, "k_smvp_chunks", st);
  HIP_TRY(ctx, tl >= 2 ? hipEventRecord(s.ev[5], st) : hipSuccess);
  if (rs != st) HIP_TRY(ctx, hipEventRecord(s.smvp_done, st));

  if (rs != st) HIP_TRY(ctx, hipStreamWaitEvent(rs, s.smvp_done, 0));
  hipLaunchKernelGGL(ctx->ops->smvp_stitch, dim3(p.half / 256, p.w_count), dim3(256), 0, rs, s.d_col_ptr, p.chunks, d_chunk_len, s.d_heads, s.d_tails,
                     s.d_buckets, s.d_big_queue);
  AFTER_KERNEL(ctx, "k_smvp_stitch", rs);
  hipLaunchKernelGGL(ctx->ops->smvp_stitch_big, dim3(STITCH_BLOCKS), dim3(256), 0, rs, s.d_col_ptr, p.chunks, s.d_heads, s.d_tails, s.d_buckets,
                     s.d_big_queue, p.half);
  AFTER_KERNEL(ctx, "k_smvp_stitch_big", rs);
  if (tl >= 2) {
    HIP_TRY(ctx, hipEventRecord(s.ev[6], rs));
    HIP_TRY(ctx, hipEventRecord(s.red0, rs));
  }
  uint32_t* d_rows = s.d_partials;
  uint32_t* d_cols = d_rows + (size_t)MAXLW * 256 * ctx->ops->xyzz_words;
  uint32_t* d_parts = d_cols + (size_t)MAXLW * 256 * ctx->ops->xyzz_words;
  const RowCol rowcol = pick_rowcol(ctx, p, s);
  hipLaunchKernelGGL(rowcol.kernel, dim3(rowcol.blocks, p.w_count), dim3(256), 0, rs, s.d_buckets, d_rows, d_cols);
  AFTER_KERNEL(ctx, "k_bpr_rowcol", rs);
  // A launch that carries ONE MSM whose sums the host combines anyway (finish): the narrow end of the reduction -- ~25 dependent group
  // operations at ~7 us each in k_bpr_w256 / k_bpr_final -- is replaced by 16 independent masked tree sums per window (k_bpr_planes, 8 deep)
  // and 29 operations per window on the host (0.3 us each).  Sums that stay on the device (window shards for the gather), grouped launches
  // (their host thread is on the critical path: several MSMs' worth of host work per launch) and debug read-backs get finished sums.
  // (a wide fixed-base launch always leaves the plane sums -- its finish needs every virtual window's plain total, which is one of them --: plan_launch
  //  admits it only as whole MSMs whose sums go to the host, at most 24 virtual windows together)
  const bool wide = p.mode == MODE_WIDE;
  const bool parts_mode = to_host && !p.pairs && (p.nvec == 1 || wide) && (!ctx->debug || wide) && p.w_count <= 24;
  // the kernel that ends the chain writes the launch's error word into the slot's pinned buffer itself and clears it (no copy, no fill); a
  // single MSM's bit-plane sums go to the pinned buffer directly as well (12 KB of stores over the host link instead of a copy behind the kernel)
  uint32_t* h_err = reinterpret_cast<uint32_t*>(s.h_wsums + WSUM_BYTES);
  const int bpr_cols = (int)(p.half / BPR_COLS);
  if (parts_mode) {
    hipLaunchKernelGGL(ctx->ops->bpr_planes, dim3(PLANES_PER_WINDOW, p.w_count), dim3(256), 0, rs, d_rows, d_cols, reinterpret_cast<uint32_t*>(s.h_wsums),
                       bpr_cols, s.d_big_queue, d_err, h_err);
    AFTER_KERNEL(ctx, "k_bpr_planes", rs);
  } else if (ctx->ops->use_w256) {
    hipLaunchKernelGGL(ctx->ops->bpr_w256, dim3(2, p.w_count), dim3(256), 0, rs, d_rows, d_cols, d_parts, bpr_cols);
    AFTER_KERNEL(ctx, "k_bpr_w256", rs);
    hipLaunchKernelGGL(ctx->ops->bpr_final, dim3(1), dim3(64), 0, rs, d_parts, p.w_count, wsums_out, s.d_big_queue, d_err, h_err, p.pairs ? 1 : 0);
    AFTER_KERNEL(ctx, "k_bpr_final", rs);
  } else {  // a field too wide for k_bpr_w256's LDS footprint (BLS12-381): the same bit-plane sums, finished on the device
    hipLaunchKernelGGL(ctx->ops->bpr_planes_xyzz, dim3(PLANES_PER_WINDOW, p.w_count), dim3(256), 0, rs, d_rows, d_cols, d_parts, bpr_cols, s.d_big_queue,
                       d_err, h_err);
    AFTER_KERNEL(ctx, "k_bpr_planes<xyzz>", rs);
    hipLaunchKernelGGL(ctx->ops->bpr_final_planes, dim3(1), dim3(64), 0, rs, d_parts, p.w_count, wsums_out, s.d_big_queue, d_err, h_err, p.pairs ? 1 : 0);
    AFTER_KERNEL(ctx, "k_bpr_final_planes", rs);
  }
  if (tl >= 2) HIP_TRY(ctx, hipEventRecord(s.red1, rs));
  if (to_host && !parts_mode) HIP_TRY(ctx, hipMemcpyAsync(s.h_wsums, wsums_out, (size_t)p.w_count * (p.pairs ? 2 : 1) * ctx->jb, hipMemcpyDeviceToHost, rs));
  HIP_TRY(ctx, hipEventRecord(s.done, rs));
  HIP_TRY(ctx, hipGetLastError());

  s.plan = p;
  s.parts = parts_mode;
  s.timed = tl >= 1;
  s.timing_level = tl;
  s.pending = true;
  s.to_host = to_host;
  ctx->last = p;
  ctx->last_slot = (int)(&s - ctx->slot);
  ctx->last_logr = rowcol.logr;
  ctx->last_inline_reduce = rs == st;
  return MSM_HIP_OK;
}

}  // namespace
