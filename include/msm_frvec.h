/* libmsm_frvec.so -- element-wise arithmetic, batch inversion and running sums / products over vectors of SCALAR-field elements, on the device
 * (gfx950).
 *
 * The third library of the engine: libmsm_fr.so (include/msm_fr.h) turns coefficients into evaluations, libmsm_hip.so (include/msm_hip.h) commits
 * to a vector; this one computes the vectors that are committed from the evaluations -- a quotient (a b - c) / Z on a coset, a permutation product
 * z[i + 1] = z[i] num[i] / den[i], a sum of 1 / (x + t[i]) -- without leaving the device.  It shares no kernel, no constant and no host state
 * with the other two.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * Data.  A vector is n scalars of 32 little-endian bytes, one after the other: canonical integers below r, or -- MSM_FRVEC_MONT256 -- a * 2^256
 * mod r, the engine's other scalar format (msm_hip_set_scalar_format); the result is in the form of the input and canonical (below r).  Either way
 * every input word must be below r: a value >= r makes the call return MSM_HIP_ERR_NONCANONICAL (the outputs are then unspecified; the next call
 * is unaffected).  The constants handed over from the host (b_const, c_const) are canonical integers below r in BOTH forms
 * (MSM_HIP_ERR_INVALID_ARG otherwise); totals_host receives values in the data's form.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5), Pallas (2), Vesta (3), BLS12-381 (4 and
 * 6).  Grumpkin (1) is not offered, as in msm_fr.h: the engine has no constants for its scalar field (MSM_HIP_ERR_INVALID_ARG).
 *
 * Lengths: n >= 1, any value -- not only a power of two --, with batch * n <= 2^26 (batch = 1 where a call has none).
 *
 * Aliasing: an output may be exactly one of the inputs (the same pointer: the call works in place) or lie apart from it; an output that overlaps
 * an input in part is MSM_HIP_ERR_INVALID_ARG, checked on the host.  Inputs may overlap one another freely.
 *
 * Ordering: the *_device calls enqueue on `stream` (a hipStream_t; NULL: a stream of the library's own) and return after that stream has
 * completed, so that the error word can be reported.  Device pointers must be 16-byte aligned.  Every call runs on `device` and leaves the
 * caller's current device as it found it.  Calls are serialised by the library.  The host forms stage their vectors through device memory.
 *
 * How it runs (csrc/frvec_kernels.h).  Inverse and scan work on tiles of 1024 elements, level by level: level 0 is the
 * data, level l + 1 holds one value per tile of level l, and the top level is a single tile (per row).  A vector of n elements has 1 level up to
 * 1024 elements, 2 up to 2^20, 3 beyond; a call of L levels is 2 L - 1 kernel launches, none of which waits for another workgroup.
 *   map      one kernel, one lane per element.
 *   inverse  Montgomery's trick: every tile's product on the way up, ONE Fermat inversion x^(r - 2) at the top, and on the way down every tile
 *            inverts its elements from the inverse of its product -- three products per element in a vector of one tile, four in a longer
 *            one.  A zero gives a zero and does not disturb its neighbours (it enters the products as 1).
 *   scan     rows are tiled one by one; a fold of every tile on the way up, an exclusive scan of the top level, and on the way down a scan of
 *            every tile from its carry-in.  The arithmetic is exact, so the result does not depend on the order of association.
 */
#ifndef MSM_FRVEC_H
#define MSM_FRVEC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRVEC_EXCLUSIVE 1u /* scan: out[i] folds the elements BEFORE i; out[0] is the identity (0 or 1, in the data's form) */
#define MSM_FRVEC_MONT256 2u   /* the data are a * 2^256 mod r; checked against r like canonical data, not otherwise */

/* map ops */
#define MSM_FRVEC_ADD 0     /* a + b */
#define MSM_FRVEC_SUB 1     /* a - b */
#define MSM_FRVEC_MUL 2     /* a * b */
#define MSM_FRVEC_MUL_ADD 3 /* a * b + c */
#define MSM_FRVEC_MUL_SUB 4 /* a * b - c */
/* scan ops */
#define MSM_FRVEC_SUM 0
#define MSM_FRVEC_PRODUCT 1

int msm_frvec_abi_version(void); /* 1 */

/* out[i] = a[i] op b[i] (op c[i]).  b and c are each EITHER a device vector of n scalars OR NULL with a 32-byte constant (b_const / c_const) that is
 * broadcast to every element; both given, or neither where the op reads the operand, is MSM_HIP_ERR_INVALID_ARG, and so is a c or c_const handed
 * to an op that does not read it.  flags: MSM_FRVEC_MONT256. */
int msm_frvec_map_device(int curve, int device, void* stream, void* out, const void* a, const void* b, const void* c, size_t n, int op, const uint8_t* b_const,
                         const uint8_t* c_const, uint32_t flags);

/* out[i] = 1 / a[i];  1 / 0 = 0.  flags: MSM_FRVEC_MONT256. */
int msm_frvec_inverse_device(int curve, int device, void* stream, void* out, const void* a, size_t n, uint32_t flags);

/* `batch` rows of n scalars, one after the other: out[i] = a[0] o .. o a[i] within each row (MSM_FRVEC_EXCLUSIVE: a[0] o .. o a[i - 1]).
 * totals_host: NULL, or batch * 32 bytes of HOST memory that receive every row's total a[0] o .. o a[n - 1].  flags: MSM_FRVEC_EXCLUSIVE,
 * MSM_FRVEC_MONT256. */
int msm_frvec_scan_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, int op, uint32_t flags, uint8_t* totals_host);

/* the host forms: every vector is host memory, staged through device memory */
int msm_frvec_map(int curve, int device, uint8_t* out, const uint8_t* a, const uint8_t* b, const uint8_t* c, size_t n, int op, const uint8_t* b_const,
                  const uint8_t* c_const, uint32_t flags);
int msm_frvec_inverse(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, uint32_t flags);
int msm_frvec_scan(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, int op, uint32_t flags, uint8_t* totals_host);

/* frees the scratch and the staging buffers of every device (they come back with the next call) */
void msm_frvec_release(void);

#define MSM_FRVEC_TEST_HOOKS 1
#ifdef MSM_FRVEC_TEST_HOOKS
/* shrinks the tile of the inverse and of the scan to `elements` (2 .. 1024); 0 restores the design's 1024 */
int msm_frvec_test_tile(int elements);
/* shape of the last successful call: kernel launches, and levels of the hierarchy (1 for a map) */
int msm_frvec_test_last(int* launches, int* levels);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRVEC_H */
