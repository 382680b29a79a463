/* libmsm_frgate.so -- constraint evaluation on the device (gfx950): element-wise sums of products of rows of SCALAR-field elements, every factor
 * read at a rotation of its own, optionally scaled by a periodic vector and added onto the output -- the numerator of a PLONK / halo2-style
 * quotient polynomial over the extended coset domain, divided by Z_H in the same pass.
 *
 * The seventh library of the engine, beside libmsm_hip.so (include/msm_hip.h: commitments), libmsm_fr.so (include/msm_fr.h: transforms),
 * libmsm_frvec.so (include/msm_frvec.h: vector arithmetic), libmsm_frpoly.so (include/msm_frpoly.h: univariate openings), libmsm_frmle.so
 * (include/msm_frmle.h: sumcheck) and libmsm_frmat.so (include/msm_frmat.h: sparse products).  msm_frmle_round reduces sums of products of rows
 * to D + 1 values; this one writes the table.  It shares no kernel, no constant and no host state with the other six.  Error codes are those
 * of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * Data.  A scalar is 32 little-endian bytes: a canonical integer below r, or -- MSM_FRGATE_MONT256 -- a * 2^256 mod r; results are in the form
 * of the input and canonical (below r).  Every element a lane reads is compared with r by that lane -- the elements of `a` that a term names,
 * of `scale`, and of `out` under MSM_FRGATE_ACCUMULATE --: a value >= r makes the call return MSM_HIP_ERR_NONCANONICAL (the output is then
 * unspecified; the next call is unaffected).  A row that no term names is not read, nor are the elements between n and stride of any row, nor
 * is `out` without MSM_FRGATE_ACCUMULATE.  The coefficients of the terms are canonical integers below r in BOTH forms.
 *
 * Rows.  `batch` rows of n = 2^k elements, 0 <= k <= 26, start `stride` elements apart: stride >= n, batch * stride <= 2^26,
 * batch <= MSM_FRGATE_MAX_ROWS.
 *
 * Rotations.  Factor f of a term reads its row at (i + rots[f] * step) mod n: `step` (1 <= step <= n) is what one rotation is worth in
 * elements -- 1 on the domain H itself, 2^log_ext on a domain extended by that factor, where the next row of H is 2^log_ext elements on.
 * rots[f] * step is reduced mod n by the host in 64-bit signed arithmetic: a rotation of any sign and size wraps round the domain as often as
 * it takes.
 *
 * Scale.  scale == NULL, or a DEVICE vector (host memory for the host form) of scale_len elements in the data's form, scale_len a power of two
 * with 1 <= scale_len <= n: element i is multiplied by scale[i mod scale_len].  1 / Z_H on a coset extended by 2^log_ext has period 2^log_ext.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5), Grumpkin (1), Pallas (2), Vesta (3),
 * BLS12-381 (4 and 6).  No root of unity is needed, so Grumpkin's scalar field is offered, as by the sumcheck and the sparse products.
 *
 * What the host checks before a device is asked for (MSM_HIP_ERR_INVALID_ARG): n, batch, stride, step and scale_len within the ranges above; the
 * flags; 1 .. MSM_FRGATE_MAX_TERMS terms, each of degree 1 .. MSM_FRGATE_MAX_DEGREE, its rows below batch, its coefficient below r; device
 * pointers 16-byte aligned; `out` (n elements) apart from a[0 .. batch * stride) and from scale -- a lane reads what its neighbours write to,
 * so the call is never in place.
 *
 * Ordering: msm_frgate_apply_device enqueues on `stream` (a hipStream_t; NULL: a stream of the library's own) and returns after that stream
 * has completed, so that the error word can be reported -- it comes back in one device-to-host copy through one pinned buffer per device.  The
 * call runs on `device` and leaves the caller's current device as it found it.  Calls are serialised by the library.  The host form stages its
 * vectors through device memory.  The library reads no environment setting.
 *
 * How it runs (csrc/frgate_kernels.h): one launch, one lane per element, the terms one after the other from a table
 * that every lane reads at the same address.  No kernel waits for another workgroup.
 */
#ifndef MSM_FRGATE_H
#define MSM_FRGATE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRGATE_MONT256 2u    /* the data are a * 2^256 mod r; checked against r like canonical data, not otherwise */
#define MSM_FRGATE_ACCUMULATE 4u /* add onto what out holds (read and checked against r) instead of overwriting it */
#define MSM_FRGATE_MAX_DEGREE 8  /* the most factors of a term */
#define MSM_FRGATE_MAX_TERMS 64  /* the most terms */
#define MSM_FRGATE_MAX_ROWS 32   /* the most rows */

/* a term: coeff * prod_{f < degree} a[rows[f]][(i + rots[f] * step) mod n]; a row may repeat, with the same or another rotation */
typedef struct msm_frgate_term {
  uint8_t coeff[32]; /* canonical, below r, in both data forms */
  uint32_t degree;   /* 1 .. MSM_FRGATE_MAX_DEGREE */
  uint32_t rows[8];  /* the first `degree` are read: each < batch */
  int32_t rots[8];   /* the rotation of each factor, in units of `step`; any sign, any size */
} msm_frgate_term;   /* 100 bytes */

int msm_frgate_abi_version(void); /* 1 */

/* out[i] = (ACCUMULATE ? out[i] : 0) + scale[i mod scale_len] * sum_t coeff_t prod_f a[rows[f]][(i + rots[f] * step) mod n],  i < n
 * (without scale: the sum itself; scale_len is then ignored).  flags: MSM_FRGATE_MONT256, MSM_FRGATE_ACCUMULATE. */
int msm_frgate_apply_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, size_t stride, const msm_frgate_term* terms,
                            size_t num_terms, size_t step, const void* scale, size_t scale_len, uint32_t flags);

/* the host form: out, a and scale are host memory, staged through device memory; a holds (batch - 1) * stride + n elements */
int msm_frgate_apply(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, size_t stride, const msm_frgate_term* terms, size_t num_terms,
                     size_t step, const uint8_t* scale, size_t scale_len, uint32_t flags);

/* frees the constants and the staging buffers of every device (they come back with the next call) */
void msm_frgate_release(void);

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRGATE_H */
