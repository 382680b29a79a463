/* libmsm_frmle.so -- the sumcheck over multilinear polynomials on the device (gfx950): binding a variable (fold), evaluation at a point (eval),
 * the eq(point, .) table (eq) and a round polynomial's values, optionally fused with the previous round's bind (round), over tables of
 * SCALAR-field elements.
 *
 * The fifth library of the engine, beside libmsm_hip.so (include/msm_hip.h: commitments), libmsm_fr.so (include/msm_fr.h: transforms),
 * libmsm_frvec.so (include/msm_frvec.h: vector arithmetic) and libmsm_frpoly.so (include/msm_frpoly.h: univariate openings): this one is the hot
 * loop between the commitments of a Nova / Spartan / HyperPlonk-style prover.  It shares no kernel, no constant and no host state with the other
 * four.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * Data.  A table is n = 2^k scalars, k >= 0, of 32 little-endian bytes, one after the other: canonical integers below r, or -- MSM_FRMLE_MONT256 --
 * a * 2^256 mod r; results are in the form of the input and canonical (below r).  Every input word is checked against r by the kernel that
 * first reads it: a value >= r makes the call return MSM_HIP_ERR_NONCANONICAL (the outputs are then unspecified; the next call is unaffected).
 * The constants handed over from the host (challenges, points, coefficients) are canonical integers below r in BOTH forms
 * (MSM_HIP_ERR_INVALID_ARG otherwise, before any device is touched); values_host receives values in the data's form.
 *
 * Rows.  `batch` rows start `stride` elements apart: stride >= n, batch * stride <= 2^26.  A sumcheck therefore runs in place in one
 * batch x N buffer, with n halving from N and the stride fixed at N.
 *
 * VARIABLE ORDER: point[0] / the first challenge binds the TOP bit of the index -- binding pairs element i with element i + n / 2, and the
 * variable x_j of a table is bit k - 1 - j of the index.  The value of a multilinear extension does not depend on the order in which its
 * variables are bound, so a table indexed with x_0 as the LEAST significant bit (arkworks) passes its point reversed to eval and eq.
 *
 * MSM_FRMLE_LOW_FIRST turns the order round for all four calls: the variable x_j is bit j of the index, and point[0] / the first challenge binds
 * bit 0 -- binding pairs element 2 i with element 2 i + 1, the order of arkworks' DenseMultilinearExtension::fix_variables and ml_sumcheck, of
 * HyperPlonk and Jolt built on it, and of the multilinear-to-univariate folds of Gemini, HyperKZG and Zeromorph.  A round polynomial depends on
 * which variable its round binds, so this is not a matter of reversing a point: under the flag
 *   fold   out[row][i] = a[row][2 i] + c (a[row][2 i + 1] - a[row][2 i]), i < n / 2.  Apart from a, only those n / 2 elements of every row of out
 *          are written.  IN PLACE (out == a) the first n / 2 elements of every row hold the result, the elements [n / 2, n) of the row are
 *          UNSPECIFIED afterwards and the elements [n, stride) are untouched -- unlike the top-first fold, which leaves everything behind the
 *          result as it was: a low-first bind stores output i on a slot that output i / 2 reads, so part of the row passes through scratch
 *          memory and the row's upper half is not kept out of it.
 *   eval   the value with point[j] at bit j (the top-first value at the reversed point);
 *   eq     out[i] = c prod_j (bit_j(i) ? point[j] : 1 - point[j]);
 *   round  g(t) = sum_{i < n / 2} sum_terms coeff prod_f (a[rows[f]][2 i] + t (a[rows[f]][2 i + 1] - a[rows[f]][2 i])); with fold_by the call
 *          first binds the LOWEST variable of all rows in place, exactly as the in-place fold above (the same unspecified [n / 2, n)), and returns
 *          the round values of the folded tables of n / 2 elements.
 * Checks, error codes, the check of every word read against r, the one copy, ordering and serialisation are the same in both orders; without the
 * flag every call does what it did before the flag existed.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5), Grumpkin (1), Pallas (2), Vesta (3),
 * BLS12-381 (4 and 6).  Grumpkin's scalar field (BN254's base field, 2-adicity 1) is offered here and by no other scalar-field library: the
 * sumcheck needs no root of unity.
 *
 * What the host checks before a device is asked for (MSM_HIP_ERR_INVALID_ARG): n a power of two within the call's range; batch, stride and the
 * flags; device pointers 16-byte aligned; the constants below r; the rows of a term below batch, its degree in 1 .. MSM_FRMLE_MAX_DEGREE, the
 * number of terms in 1 .. MSM_FRMLE_MAX_TERMS, batch <= MSM_FRMLE_MAX_ROWS for round; an output (fold) that overlaps its input in part.
 *
 * Ordering: the *_device calls enqueue on `stream` (a hipStream_t; NULL: a stream of the library's own) and return after that stream has
 * completed, so that the values and the error word can be reported -- both come back in ONE device-to-host copy through one pinned buffer per
 * device.  Every call runs on `device` and leaves the caller's current device as it found it.  Calls are serialised by the library.  The host
 * forms stage their tables through device memory.
 *
 * How it runs (csrc/frmle_kernels.h).  fold and eq are one launch.  eval and round work on tiles of 1024 elements
 * (pairs), level by level: 1 launch up to 2^10, 2 up to 2^20, 3 beyond (of n for eval, of n / 2 -- n / 4 with fold_by -- for round).  No kernel
 * waits for another workgroup.
 *
 * Low first, the same kernels run; eval, eq, the fold apart from its input and the round without fold_by take the launches and levels above.
 * The two in-place binds are split so that no launch stores where one of its own lanes reads -- correct for every order in which lanes and
 * workgroups run -- and what msm_frmle_test_last reports for them is:
 *   fold in place        n = 2: 1 launch.  n >= 4: 2 launches -- the outputs [0, n / 4) of every row into the library's scratch, then the outputs
 *                        [n / 4, n / 2) in place -- and one device-to-device copy of the scratch rows to the head of the rows (a copy, not a
 *                        launch: not counted).  1 level.
 *   round with fold_by   n = 4: 1 launch, 1 level.  n >= 8: the n / 4 pairs of the folded tables run as two launches of n / 8 pairs -- the first
 *                        folds into scratch, the second in place --, each over its own T = ceil(n / (4 tile)) tiles of tile / 2 pairs (half
 *                        the pairs to a launch, half the tile: the workgroups of the one top-first launch), then the same copy; the 2 T
 *                        partial sums per point are summed level by level as ever, over tiles of `tile`: levels = 1 + the levels of 2 T
 *                        values (2 up to n = 2 tile^2 -- 2^21 at the design's tile --, 3 beyond), launches = levels + 1.
 */
#ifndef MSM_FRMLE_H
#define MSM_FRMLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRMLE_MONT256 2u   /* the data are a * 2^256 mod r; checked against r like canonical data, not otherwise */
#define MSM_FRMLE_LOW_FIRST 8u /* the variable x_j is bit j of the index: VARIABLE ORDER above.  May be combined with MSM_FRMLE_MONT256 only */
#define MSM_FRMLE_MAX_DEGREE 4 /* round: the most factors of a term */
#define MSM_FRMLE_MAX_TERMS 8  /* round: the most terms */
#define MSM_FRMLE_MAX_ROWS 16  /* round: the most rows */

/* a term of a round polynomial: coeff * prod_{f < degree} row[rows[f]]; a row may repeat */
typedef struct msm_frmle_term {
  uint8_t coeff[32]; /* canonical, below r, in both data forms */
  uint32_t degree;   /* 1 .. MSM_FRMLE_MAX_DEGREE */
  uint32_t rows[4];  /* the first `degree` are read: each < batch */
} msm_frmle_term;

int msm_frmle_abi_version(void); /* 1 */

/* out[row][i] = a[row][i] + c (a[row][i + n / 2] - a[row][i]), i < n / 2, for every row: the top variable bound to c.  n >= 2.  out has the
 * stride of a and may be a itself (the elements at i >= n / 2 are then left as they were) or lie apart from it.  flags: MSM_FRMLE_MONT256,
 * MSM_FRMLE_LOW_FIRST (pairs 2 i and 2 i + 1; in place the elements [n / 2, n) of every row are unspecified afterwards: VARIABLE ORDER above). */
int msm_frmle_fold_device(int curve, int device, void* stream, void* out, const void* a, size_t n, size_t batch, size_t stride, const uint8_t* c, uint32_t flags);

/* values_host[row] = the multilinear extension of row `row` at `point` (log2(n) x 32 bytes of HOST memory; none are read for n = 1):
 * batch * 32 bytes of HOST memory.  Reads a once and writes no table.  MSM_FRMLE_LOW_FIRST: point[j] is the variable at bit j. */
int msm_frmle_eval_device(int curve, int device, void* stream, const void* a, size_t n, size_t batch, size_t stride, const uint8_t* point, uint32_t flags,
                          uint8_t* values_host);

/* out[i] = c prod_j (bit_(k-1-j)(i) ? point[j] : 1 - point[j]), i < n = 2^k <= 2^26: the table of eq(point, .) scaled by c.  No table input.
 * flags: MSM_FRMLE_MONT256 (the form of out), MSM_FRMLE_LOW_FIRST (bit_j(i) in place of bit_(k-1-j)(i)). */
int msm_frmle_eq_device(int curve, int device, void* stream, void* out, size_t n, const uint8_t* point, const uint8_t* c, uint32_t flags);

/* The values g(t), t = 0 .. D, D the largest degree among the terms, of
 *   g(t) = sum_{i < n / 2} sum_terms coeff prod_f (a[rows[f]][i] + t (a[rows[f]][i + n / 2] - a[rows[f]][i]))
 * into values_host ((D + 1) * 32 bytes of HOST memory).  fold_by == NULL: n >= 2, a is only read.  fold_by != NULL (32 bytes, below r): n >= 4;
 * the call first binds the top variable of ALL batch rows to that challenge, in place -- row[i] = row[i] + fold_by (row[i + n / 2] - row[i]),
 * i < n / 2; the elements behind stay as they were -- and returns the round values of the folded tables, of n / 2 elements: one pass over the
 * data per sumcheck round.  batch <= MSM_FRMLE_MAX_ROWS.  MSM_FRMLE_LOW_FIRST: the pairs are 2 i and 2 i + 1, fold_by binds the lowest variable
 * and leaves the elements [n / 2, n) of every row unspecified (VARIABLE ORDER above). */
int msm_frmle_round_device(int curve, int device, void* stream, void* a, size_t n, size_t batch, size_t stride, const msm_frmle_term* terms, size_t num_terms,
                           const uint8_t* fold_by, uint32_t flags, uint8_t* values_host);

/* the host forms: every table is host memory, staged through device memory (fold: out receives what the device form leaves in out, the first
 * n / 2 elements of every row, at the stride of a; round with fold_by: a is folded in place) */
int msm_frmle_fold(int curve, int device, uint8_t* out, const uint8_t* a, size_t n, size_t batch, size_t stride, const uint8_t* c, uint32_t flags);
int msm_frmle_eval(int curve, int device, const uint8_t* a, size_t n, size_t batch, size_t stride, const uint8_t* point, uint32_t flags, uint8_t* values_host);
int msm_frmle_eq(int curve, int device, uint8_t* out, size_t n, const uint8_t* point, const uint8_t* c, uint32_t flags);
int msm_frmle_round(int curve, int device, uint8_t* a, size_t n, size_t batch, size_t stride, const msm_frmle_term* terms, size_t num_terms, const uint8_t* fold_by,
                    uint32_t flags, uint8_t* values_host);

/* frees the scratch, the constants and the staging buffers of every device (they come back with the next call) */
void msm_frmle_release(void);

#define MSM_FRMLE_TEST_HOOKS 1
#ifdef MSM_FRMLE_TEST_HOOKS
/* shrinks the tile of eval and round to `elements` (a power of two, 2 .. 1024); 0 restores the design's 1024 */
int msm_frmle_test_tile(int elements);
/* shape of the last successful call: kernel launches, and levels of the hierarchy (1 for fold and eq); low first: "How it runs" above */
int msm_frmle_test_last(int* launches, int* levels);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRMLE_H */
