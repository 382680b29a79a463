/* libmsm_fr.so -- number-theoretic transforms over the SCALAR field of the engine's curves, on the device (gfx950).
 *
 * The companion of libmsm_hip.so (include/msm_hip.h): that library commits to a vector of scalars, this one turns a polynomial's coefficients
 * into the evaluations that are committed (and back) without leaving the device.  It is a library of its own: it shares no kernel, no constant
 * and no host state with the curve units.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 *     out[i] = c * t^i * sum_j s^j * omega^(i j) * a[j],        i, j < n = 2^log_n
 *
 *   in place, natural order in and out, `batch` vectors of n scalars lying one after the other.  c = 1, or 1 / n under MSM_FR_SCALE_INV_N;
 *   s (pre_shift) and t (post_shift) are optional (NULL: 1).  An evaluation over the coset g H is s = g; its inverse is omega^-1,
 *   MSM_FR_SCALE_INV_N, t = g^-1.
 *
 * Scalars are 32 little-endian bytes: canonical integers below r, or -- MSM_FR_MONT256 -- a * 2^256 mod r, the engine's other scalar format
 * (msm_hip_set_scalar_format); the result is in the form of the input.  Either way every word must be below r: a value >= r makes the call
 * return MSM_HIP_ERR_NONCANONICAL (the data are then unspecified; the next call is unaffected).  omega, pre_shift and post_shift are canonical.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5; 2-adicity 28), Pallas (2; 32), Vesta
 * (3; 32), BLS12-381 (4 and 6; 32).  Grumpkin (1) is not offered: its r - 1 is divisible by 2 only once (MSM_HIP_ERR_INVALID_ARG).
 * log_n runs from 0 to min(2-adicity, 26).  omega is validated on the host before anything is enqueued: omega^(n / 2) = r - 1, and
 * omega = 1 at n = 1 (MSM_HIP_ERR_INVALID_ARG otherwise).
 *
 * How it runs (csrc/ntt_kernels.h): ceil(log_n / 10) passes of up to 10 radix-2 levels each on 2 x 1024-element
 * tiles staged in LDS (72 KiB per workgroup); up to 2^10 elements are one launch.  With two or more passes the call uses a scratch of the
 * size of the data.  Twiddles live on the device as two-level power tables (2 x 2^13 entries of 32 bytes at most, plus 2^9 butterfly
 * twiddles: 528 KiB at 2^26), cached per (field, log_n, omega); the shift tables are cached the same way.
 *
 * Ordering: msm_fr_ntt_device enqueues on `stream` (a hipStream_t; NULL: a stream of the library's own) and returns after that stream has
 * completed, so that the error word can be reported.  data_dev must be 16-byte aligned.  Every call runs on `device` and leaves the
 * caller's current device as it found it.  Calls are serialised by the library.
 */
#ifndef MSM_FR_H
#define MSM_FR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FR_SCALE_INV_N 1u /* c = 1 / n */
#define MSM_FR_MONT256 2u     /* the data are a * 2^256 mod r; checked against r like canonical data, not otherwise */

int msm_fr_abi_version(void); /* 1 */

int msm_fr_ntt_device(int curve, int device, void* stream, void* data_dev, int log_n, size_t batch, const uint8_t omega[32], const uint8_t* pre_shift,
                      const uint8_t* post_shift, uint32_t flags);

/* the host form: batch * n * 32 bytes staged through device memory, transformed in place */
int msm_fr_ntt(int curve, int device, uint8_t* data_host, int log_n, size_t batch, const uint8_t omega[32], const uint8_t* pre_shift, const uint8_t* post_shift,
               uint32_t flags);

/* frees the cached twiddles, the scratch and the staging buffer of every device (they come back with the next call) */
void msm_fr_release(void);

#define MSM_FR_TEST_HOOKS 1
#ifdef MSM_FR_TEST_HOOKS
/* caps the radix-2 levels of a pass at b (1 .. 10); 0 restores the design's 10 */
int msm_fr_test_pass_bits(int b);
/* shape of the last successful call: number of passes, and the widest pass's levels */
int msm_fr_test_last(int* passes, int* pass_bits);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FR_H */
