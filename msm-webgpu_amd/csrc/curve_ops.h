// The table through which the host code (msm_hip.hip) reaches one curve's kernels and host arithmetic.  Every curve is compiled as its
// own translation unit (curve_<name>.hip: csrc/curve_unit.h instantiated with that curve's constants) so that the units build in parallel;
// a unit fills its table by name (msm_kernels.h: curve_ops_table) and hands it over through one accessor.  The recode and the sort are not
// in it: no field enters them, and msm_hip.hip compiles and launches them itself (sort_kernels.h).
#pragma once
#include <cstddef>
#include <cstdint>

#include "msm_layout.h"  // SparseIdx

// What differs between the curves: the kernels that do field arithmetic, and the host's window combine.  A context holds one.
struct CurveOps {
  void (*convert_points)(const uint32_t*, uint32_t*, size_t, uint32_t, uint32_t*);
  // ... for MSM_HIP_BASES_ZERO_IS_IDENTITY: all-zero records are the identity (bitmap + count; k_convert_points_zero_id)
  void (*convert_points_zero_id)(const uint32_t*, uint32_t*, size_t, uint32_t, uint32_t*, uint64_t*, uint32_t*);
  void (*precompute_tables)(uint32_t*, size_t, size_t, int, int, int);
  void (*endo_points)(uint32_t*, size_t, size_t, size_t);
  // batch scalar multiplication (msm_hip_mul_each / msm_hip_mul_base): k_mul_each<false> (plain ladder), k_mul_each<true> (endomorphism), k_mul_normalize
  void (*mul_each[2])(const uint32_t*, const uint32_t*, size_t, size_t, uint32_t, const uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t);
  void (*mul_normalize)(uint32_t*, const uint32_t*, uint32_t*, size_t);
  int mul_chunk;    // results that share one inversion in k_mul_normalize
  // ... the fixed-base table of msm_hip_mul_base: k_mul_table_scalars, k_mul_fixed; bit length of r (the table has (r_bits + 1 + C) / C windows)
  void (*mul_table_scalars)(int, size_t, size_t, uint32_t*);
  void (*mul_fixed)(const uint32_t*, int, const uint32_t*, size_t, uint32_t*, uint32_t*, uint32_t*);
  int r_bits;
  // k_count<C, 4, glv_split_fn> (recode.h over the unit's split functor) for C = 12 / 14 / 16: the first sort pass of endomorphism launches, which splits the scalars itself (csrc/glv.h)
  void (*count_split[3])(const uint32_t*, size_t, uint32_t, uint32_t, int, int, int, size_t, uint32_t*, uint32_t*, uint16_t*, int, uint64_t*, uint32_t*, uint32_t*, size_t);
  // ... and of sparse endomorphism launches (k_count<C, 4, glv_split_fn, 0, SparseIdx>: the split of scalar j, whose base is idx[j])
  void (*count_split_sparse[3])(const uint32_t*, size_t, uint32_t, uint32_t, int, int, int, size_t, uint32_t*, uint32_t*, uint16_t*, int, uint64_t*, uint32_t*, uint32_t*, size_t,
                                SparseIdx);
  void (*scalars_from_mont256)(const uint32_t*, uint32_t*, size_t, uint32_t*);
  void (*smvp_chunks)(const uint32_t*, const uint32_t*, const uint32_t*, size_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*,
                      uint32_t*, uint32_t);
  void (*smvp_stitch)(const uint32_t*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*);
  void (*smvp_stitch_big)(const uint32_t*, uint32_t, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t);
  void (*rowcol_4_8)(const uint32_t*, uint32_t*, uint32_t*);
  void (*rowcol_2_8)(const uint32_t*, uint32_t*, uint32_t*);
  void (*rowcol_3_8)(const uint32_t*, uint32_t*, uint32_t*);
  void (*rowcol_4_6)(const uint32_t*, uint32_t*, uint32_t*);
  void (*rowcol_2_6)(const uint32_t*, uint32_t*, uint32_t*);
  void (*rowcol_2_4)(const uint32_t*, uint32_t*, uint32_t*);
  void (*bpr_w256)(const uint32_t*, const uint32_t*, uint32_t*, int);
  void (*bpr_final)(const uint32_t*, int, uint32_t*, uint32_t*, uint32_t*, uint32_t*, int);
  void (*bpr_planes)(const uint32_t*, const uint32_t*, uint32_t*, int, uint32_t*, uint32_t*, uint32_t*);
  void (*bpr_planes_xyzz)(const uint32_t*, const uint32_t*, uint32_t*, int, uint32_t*, uint32_t*, uint32_t*);
  void (*bpr_final_planes)(const uint32_t*, int, uint32_t*, uint32_t*, uint32_t*, uint32_t*, int);
  bool use_w256;    // the narrow reduce tail fits a workgroup's LDS (k_bpr_w256); else k_bpr_planes<true> + k_bpr_final_planes
  int coord_words;  // 32-bit words per coordinate on the wire: 8 (254 / 255-bit fields) or 12 (BLS12-381); point = 2, Jacobian record = 3 of them
  int rec_words, xyzz_words;  // device bucket record / scratch record sizes (words)
  bool glv;         // MSM_HIP_BASES_ENDOMORPHISM available
  void (*sample_scalars)(uint64_t, size_t, uint32_t*);
  void (*sample_points)(uint64_t, size_t, uint32_t*);
  void (*export_buckets)(const uint32_t*, uint32_t*, size_t);
  void (*test_fq)(int, const uint32_t*, const uint32_t*, uint32_t*, size_t);
  void (*test_g1)(int, const uint32_t*, const uint32_t*, uint32_t*, size_t);
  void (*test_g1_mul_u32)(const uint32_t*, const uint32_t*, uint32_t*, size_t);
  bool (*combine_windows)(const uint8_t*, int, int, uint8_t*);
  bool (*window_from_planes)(const uint8_t*, uint8_t*);
  bool (*combine_wide)(const uint8_t*, const uint8_t*, int, uint8_t*);
  bool (*combine_wide_pairs)(const uint8_t*, int, uint8_t*);
  int (*to_affine64)(const uint8_t*, uint8_t*);
  // group FFT over the resident bases (msm_hip_bases_fft): k_fft_stage<0 / 1 / 2> (additions only, plain ladder, endomorphism), k_fft_normalize,
  // k_fft_scale<1 / 2>; null in the G2 units, where the transform is not offered.  fr_r: the group order r, 8 words (the host's twiddle arithmetic)
  void (*fft_stage[3])(const uint32_t*, uint32_t*, uint32_t*, const uint32_t*, int, int, uint32_t, const uint64_t*);
  void (*fft_normalize)(uint32_t*, const uint32_t*, uint32_t*, size_t);
  void (*fft_scale[2])(const uint32_t*, uint32_t*, uint32_t*, const uint32_t*, size_t);
  const uint32_t* fr_r;
};
// accessors of the separately compiled units (hidden: not part of the C ABI)
extern "C" {
__attribute__((visibility("hidden"))) const CurveOps* msm_hip_curve_ops_bn254(void);
__attribute__((visibility("hidden"))) const CurveOps* msm_hip_curve_ops_grumpkin(void);
__attribute__((visibility("hidden"))) const CurveOps* msm_hip_curve_ops_pallas(void);
__attribute__((visibility("hidden"))) const CurveOps* msm_hip_curve_ops_vesta(void);
__attribute__((visibility("hidden"))) const CurveOps* msm_hip_curve_ops_bls12_381(void);
__attribute__((visibility("hidden"))) const CurveOps* msm_hip_curve_ops_bn254_g2(void);
__attribute__((visibility("hidden"))) const CurveOps* msm_hip_curve_ops_bls12_381_g2(void);
}
