/* libmsm_frpoly.so -- opening a polynomial commitment on the device (gfx950): evaluation at a point, division by X - z, dot products, linear
 * combinations of rows and vectors of powers, over vectors of SCALAR-field elements.
 *
 * The fourth library of the engine: libmsm_fr.so (include/msm_fr.h) moves between coefficients and evaluations, libmsm_frvec.so
 * (include/msm_frvec.h) computes the vectors that are committed, libmsm_hip.so (include/msm_hip.h) commits; this one does what a KZG / PLONK /
 * EIP-4844 prover does after its last commitment -- fold the polynomials with powers of a challenge (combine), evaluate the fold at z (eval),
 * form the witness (f - f(z)) / (X - z) (divide), which msm_hip then commits -- without leaving the device.  It shares no kernel, no constant
 * and no host state with the other three.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * Data.  A vector is n scalars of 32 little-endian bytes, one after the other: canonical integers below r, or -- MSM_FRPOLY_MONT256 -- a * 2^256
 * mod r, the engine's other scalar format; results are in the form of the input and canonical (below r).  Either way every input word must be
 * below r: a value >= r makes the call return MSM_HIP_ERR_NONCANONICAL (the outputs are then unspecified; the next call is unaffected).  The
 * constants handed over from the host (z, g, c, the coefficients of a combination) are canonical integers below r in BOTH forms
 * (MSM_HIP_ERR_INVALID_ARG otherwise, before any device is touched); values_host receives values in the data's form.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5), Pallas (2), Vesta (3), BLS12-381 (4 and
 * 6).  Grumpkin (1) is not offered, as in msm_fr.h: the engine has no constants for its scalar field (MSM_HIP_ERR_INVALID_ARG).
 *
 * Lengths: n >= 1, any value -- not only a power of two --, with batch * n <= 2^26 (batch = 1 where a call has none).  `batch` rows of n
 * scalars lie one after the other.
 *
 * Aliasing: an output may be exactly its input (the same pointer: the call works in place; for a combination, row 0 of the input) or lie apart
 * from all of it; an output that overlaps the input in part is MSM_HIP_ERR_INVALID_ARG, checked on the host.
 *
 * Ordering: the *_device calls enqueue on `stream` (a hipStream_t; NULL: a stream of the library's own) and return after that stream has
 * completed, so that the values and the error word can be reported.  Device pointers must be 16-byte aligned.  Every call runs on `device` and
 * leaves the caller's current device as it found it.  Calls are serialised by the library.  The host forms stage their vectors through device
 * memory.
 *
 * How it runs (csrc/frpoly_kernels.h).  Eval, divide and dot work on tiles of 1024 elements, level by level: level 0 is
 * the data, level l + 1 holds one value per tile of level l, and the top level is a single tile per row: 1 level up to 1024 elements, 2 up to
 * 2^20, 3 beyond.  No kernel waits for another workgroup.
 *   eval     Horner's rule as a weighted reduction: a tile of level l folds to sum x[off] z_l^off with z_l = z^(1024^l); L launches.
 *   divide   the same folds on the way up, then a weighted suffix scan of every tile on the way down, from the carry-in that the level above
 *            stored for it; 2 L - 1 launches.  Every workgroup reads all it needs before its first store: in place is safe.
 *   dot      the fold with a second operand at level 0 and plain sums above it; L launches.
 *   combine  one launch, one lane per element.
 *   powers   one launch, one lane per four elements, from small tables of powers that the host builds.
 */
#ifndef MSM_FRPOLY_H
#define MSM_FRPOLY_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRPOLY_SHARED_B 1u /* dot: b is ONE row of n scalars, used for every row of a */
#define MSM_FRPOLY_MONT256 2u  /* the data are a * 2^256 mod r; checked against r like canonical data, not otherwise */
#define MSM_FRPOLY_MAX_ROWS 256 /* combine: the most rows */

int msm_frpoly_abi_version(void); /* 1 */

/* values_host[row] = sum_j a[row][j] z^j: batch * 32 bytes of HOST memory.  Reads a once and writes no vector.  flags: MSM_FRPOLY_MONT256. */
int msm_frpoly_eval_device(int curve, int device, void* stream, const void* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags, uint8_t* values_host);

/* per row, out[i] = sum_{j > i} a[j] z^(j - i - 1) for i <= n - 2 and out[n - 1] = 0: the coefficients of (a(X) - a(z)) / (X - z), kept at length
 * n so that the MSM over the same bases commits them.  values_host: NULL, or batch * 32 bytes of HOST memory that receive every a(z).  z = 0 is a
 * shift; n = 1 gives [0] and a[0].  flags: MSM_FRPOLY_MONT256. */
int msm_frpoly_divide_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags,
                             uint8_t* values_host);

/* values_host[row] = sum_j a[row][j] b[row][j].  flags: MSM_FRPOLY_SHARED_B (b is one row of n), MSM_FRPOLY_MONT256. */
int msm_frpoly_dot_device(int curve, int device, void* stream, const void* a, const void* b, size_t n, size_t batch, uint32_t flags, uint8_t* values_host);

/* out[i] = sum_k coeffs[k] a[k][i] over the `batch` rows of a, 1 <= batch <= MSM_FRPOLY_MAX_ROWS; coeffs_host: batch * 32 bytes of HOST memory.
 * out is n scalars and may be exactly row 0 of a.  flags: MSM_FRPOLY_MONT256. */
int msm_frpoly_combine_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, const uint8_t* coeffs_host, uint32_t flags);

/* out[i] = c g^i, i < n.  No vector input; g = 0 gives (c, 0, 0, ..).  flags: MSM_FRPOLY_MONT256 (the form of out). */
int msm_frpoly_powers_device(int curve, int device, void* stream, void* out, size_t n, const uint8_t* g, const uint8_t* c, uint32_t flags);

/* the host forms: every vector is host memory, staged through device memory */
int msm_frpoly_eval(int curve, int device, const uint8_t* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags, uint8_t* values_host);
int msm_frpoly_divide(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, const uint8_t* z, uint32_t flags, uint8_t* values_host);
int msm_frpoly_dot(int curve, int device, const uint8_t* a, const uint8_t* b, size_t n, size_t batch, uint32_t flags, uint8_t* values_host);
int msm_frpoly_combine(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, const uint8_t* coeffs_host, uint32_t flags);
int msm_frpoly_powers(int curve, int device, uint8_t* out, size_t n, const uint8_t* g, const uint8_t* c, uint32_t flags);

/* frees the scratch, the constants and the staging buffers of every device (they come back with the next call) */
void msm_frpoly_release(void);

#define MSM_FRPOLY_TEST_HOOKS 1
#ifdef MSM_FRPOLY_TEST_HOOKS
/* shrinks the tile of eval, divide and dot to `elements` (2 .. 1024); 0 restores the design's 1024 */
int msm_frpoly_test_tile(int elements);
/* shape of the last successful call: kernel launches, and levels of the hierarchy (1 for combine and powers) */
int msm_frpoly_test_last(int* launches, int* levels);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRPOLY_H */
