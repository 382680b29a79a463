/* libmsm_frmat.so -- sparse matrix-vector products over the SCALAR field on the device (gfx950): y = M x and y = M^T x for a matrix that is
 * handed over once and stays resident.  The rows Az, Bz, Cz of an R1CS -- the tables a Spartan / Nova-style sumcheck runs over, and the first
 * step of a Groth16 prover -- are three such products over the witness vector.
 *
 * The sixth library of the engine, beside libmsm_hip.so (include/msm_hip.h: commitments), libmsm_fr.so (include/msm_fr.h: transforms),
 * libmsm_frvec.so (include/msm_frvec.h: vector arithmetic), libmsm_frpoly.so (include/msm_frpoly.h: univariate openings) and libmsm_frmle.so
 * (include/msm_frmle.h: the sumcheck): this one fills the place between "commit to the witness" and "run the sumcheck".  It shares no kernel, no
 * constant and no host state with the other five.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * Data.  The matrix comes from HOST memory in CSR form: row_ptr (rows + 1 words, row_ptr[0] = 0, never decreasing, row_ptr[rows] = nnz),
 * col_idx (nnz words, each below cols) and values (nnz x 32 little-endian bytes).  The values are canonical integers below r and ALWAYS plain
 * integers, whatever form the vectors have (as the constants of msm_frmle.h).  Within a row the columns may come in any order and may repeat:
 * repeated entries add.  Values of 0 are allowed.  1 <= rows, cols <= 2^26; 0 <= nnz <= 2^28.  The vectors x and y are scalars of 32
 * little-endian bytes, one after the other: canonical integers below r, or -- MSM_FRMAT_MONT256 -- a * 2^256 mod r; y is in the form of x and
 * canonical.
 *
 * Checks.  msm_frmat_create checks all of the above on the host and touches no device: MSM_HIP_ERR_INVALID_ARG for a bad structure,
 * MSM_HIP_ERR_NONCANONICAL for a value >= r.  It also plans the products (and, with MSM_FRMAT_WITH_TRANSPOSE, builds the transposed structure
 * with a counting sort).  The arrays go to `device` -- and the values are converted to the device's own form, once -- when the handle is first
 * used; from then on the matrix is resident until msm_frmat_destroy.  msm_frmat_mul* checks, before any device is touched
 * (MSM_HIP_ERR_INVALID_ARG): the handle, the flags, MSM_FRMAT_TRANSPOSE on a handle created without MSM_FRMAT_WITH_TRANSPOSE, x_len == cols
 * (rows with TRANSPOSE), y_len >= rows (cols with TRANSPOSE) and <= 2^26, device pointers 16-byte aligned, x and y apart.  Every element of x
 * that is READ is compared with r by the lane that reads it: one that is not below r makes the call return MSM_HIP_ERR_NONCANONICAL (y is
 * then unspecified; the next call is unaffected).  An element of x whose column no entry references is not read, and so not checked.
 *
 * The product.  y[i] = sum_j M[i][j] x[j], i < rows; y[rows .. y_len) is written as ZERO, so that a y_len that is a power of two is a sumcheck
 * table without a second call.  Nothing is assumed of what y held before.  With MSM_FRMAT_TRANSPOSE: y[j] = sum_i M[i][j] x[i], j < cols.  One
 * x per call: three matrices over one z are three calls into three rows of one buffer.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5), Grumpkin (1), Pallas (2), Vesta (3),
 * BLS12-381 (4 and 6).
 *
 * Ordering: msm_frmat_mul_device enqueues on `stream` (a hipStream_t; NULL: a stream of the library's own) and returns after that stream has
 * completed, so that the error word can be reported -- it comes back in ONE device-to-host copy through one pinned buffer per device.  Every
 * call runs on the handle's device and leaves the caller's current device as it found it.  Calls are serialised by the library.  msm_frmat_mul
 * stages x and y through device memory.
 *
 * How it runs (csrc/frmat_kernels.h).  Work is divided over the ENTRIES, not the rows: a workgroup owns 1024 consecutive
 * entries whatever rows they are of, so a constant-one column of 10^6 entries (a row of the transposed matrix) costs what 10^6 short rows cost.
 * A row that crosses workgroups is finished by a second, much smaller pass over the workgroups' partial sums (and so on: a third pass beyond
 * 2^19 partials).  A product is the fill of y and one launch per pass: 2 launches for a matrix without such rows, 3 up to 2^19 of them.  No
 * kernel waits for another workgroup and nothing is added into memory: the result is the same bytes on every run.
 */
#ifndef MSM_FRMAT_H
#define MSM_FRMAT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRMAT_MONT256 2u        /* mul: x and y are a * 2^256 mod r */
#define MSM_FRMAT_WITH_TRANSPOSE 4u /* create: also keep the transposed structure */
#define MSM_FRMAT_TRANSPOSE 8u      /* mul: y = M^T x (needs MSM_FRMAT_WITH_TRANSPOSE at create) */

typedef struct msm_frmat msm_frmat;

int msm_frmat_abi_version(void); /* 1 */

/* A handle for the rows x cols matrix in CSR form (HOST memory, read before the call returns).  flags: 0 or MSM_FRMAT_WITH_TRANSPOSE.  `device`
 * is where the products will run; it is not touched here. */
int msm_frmat_create(int curve, int device, size_t rows, size_t cols, size_t nnz, const uint32_t* row_ptr, const uint32_t* col_idx, const uint8_t* values, uint32_t flags,
                     msm_frmat** out);
/* what the handle was created with (any pointer may be NULL) */
int msm_frmat_info(const msm_frmat* m, size_t* rows, size_t* cols, size_t* nnz, uint32_t* flags);
/* frees the handle and its device memory (NULL: nothing) */
void msm_frmat_destroy(msm_frmat* m);

/* y = M x (MSM_FRMAT_TRANSPOSE: M^T x) for DEVICE memory x (x_len scalars) and y (y_len scalars).  flags: MSM_FRMAT_MONT256, MSM_FRMAT_TRANSPOSE. */
int msm_frmat_mul_device(const msm_frmat* m, void* stream, void* y, size_t y_len, const void* x, size_t x_len, uint32_t flags);
/* the host form: x and y are host memory, staged through device memory */
int msm_frmat_mul(const msm_frmat* m, uint8_t* y, size_t y_len, const uint8_t* x, size_t x_len, uint32_t flags);

/* frees the staging buffers of every device (they come back with the next call); the handles and their matrices stay */
void msm_frmat_release(void);

#define MSM_FRMAT_TEST_HOOKS 1
#ifdef MSM_FRMAT_TEST_HOOKS
/* shrinks the tile of the handles created FROM NOW ON to `entries` (a power of two, 2 .. 1024); 0 restores the design's 1024 */
int msm_frmat_test_tile(int entries);
/* shape of the last successful product: launches (the fill of y and one per level), and levels (1 where no row crosses tiles, 0 for nnz = 0) */
int msm_frmat_test_last(int* launches, int* levels);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRMAT_H */
