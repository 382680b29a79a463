/* libmsm_frlook.so -- lookup arguments over the SCALAR field on the device (gfx950): the multiplicity column of a logUp / plookup-style lookup,
 * m[j] = #{(row, i) : f[row][i] = t[j]}, and the table index of every looked-up value, for a table that is handed over once and stays resident.
 * It is the step before the logUp sum  sum_i 1 / (beta + f[i]) = sum_j m[j] / (beta + t[j])  that libmsm_frvec.so (include/msm_frvec.h) takes.
 *
 * The eighth library of the engine, beside libmsm_hip.so (include/msm_hip.h: commitments), libmsm_fr.so (include/msm_fr.h: transforms),
 * libmsm_frvec.so (include/msm_frvec.h: vector arithmetic), libmsm_frpoly.so (include/msm_frpoly.h: univariate openings), libmsm_frmle.so
 * (include/msm_frmle.h: the sumcheck), libmsm_frmat.so (include/msm_frmat.h: R1CS products) and libmsm_frgate.so (include/msm_frgate.h: the
 * quotient's numerator): this one fills the place between "quotient" and "commit".  It is the one step of a prover that is no field arithmetic --
 * matching 256-bit keys -- and shares no kernel, no constant and no host state with the other seven.  Error codes are those of msm_hip.h
 * (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * Data.  A scalar is 32 little-endian bytes: a canonical integer below r, or -- MSM_FRLOOK_MONT256 -- a * 2^256 mod r.  The flag is given at
 * create and belongs to the handle: a count whose flags differ in it returns MSM_HIP_ERR_INVALID_ARG.  Keys are compared AS STORED (both forms
 * are bijections of the field), so nothing is converted.  1 <= n_t <= 2^24 table entries; the looked-up values are `batch` rows of n scalars,
 * `stride` scalars apart: 1 <= n <= stride, batch * stride <= 2^26; n need not be a power of two.  Element i of row `row` is
 * f[row * stride + i]; the elements between n and stride are not read.
 *
 * The table may hold a value more than once: all matches are credited to its LOWEST index j; the later copies get m = 0 and are never an idx.
 * `distinct` (msm_frlook_info) is the number of different values.  The handle keeps its own copy of the keys: the caller's buffer is free when
 * create returns.
 *
 * A count writes any of: m_out (n_t scalars in the data's form, canonical: the count k, or k * 2^256 mod r under MONT256), counts_out (n_t
 * words) and idx_out (batch * n words, row-major WITHOUT stride: idx_out[row * n + i]); all three NULL is a pure membership check.  A looked-up
 * value that is not in the table is no error code: its idx is 0xFFFFFFFF (MSM_FRLOOK_MISSING), *missing is the number of such elements,
 * *first_missing the lowest flat index row * n + i among them (UINT64_MAX where there are none), and m counts only the elements found.
 * `missing` and `first_missing` are HOST words and may be NULL.  Integer adds commute: the result is the same bytes on every run.
 *
 * Checks.  Before any device is asked for (MSM_HIP_ERR_INVALID_ARG): the curve, the ranges above, the flags, the handle, device pointers of
 * scalars 16-byte aligned and of words 4-byte aligned, every output apart from f and from the other outputs.  Every element of the table and
 * every element of f that is read is compared with r by the lane that reads it: a value that is not below r makes the call return
 * MSM_HIP_ERR_NONCANONICAL (the outputs are then unspecified, a handle is not made; the next call is unaffected).  The host forms make that
 * comparison on the host first, before a device is asked for.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5), Grumpkin (1), Pallas (2), Vesta (3),
 * BLS12-381 (4 and 6).
 *
 * Ordering: msm_frlook_create_device and msm_frlook_count_device enqueue on `stream` (a hipStream_t; NULL: a stream of the library's own) and
 * return after that stream has completed, so that the error word, `distinct`, `missing` and `first_missing` can be reported -- they come back
 * in ONE device-to-host copy through one pinned buffer per device.  Every call runs on the handle's device and leaves the caller's current
 * device as it found it.  Calls are serialised by the library.  msm_frlook_create (HOST memory) checks the keys and counts the distinct ones on
 * the host and touches no device: the keys go to `device` when the handle is first used.  msm_frlook_count stages f and the outputs through
 * device memory.
 *
 * How it runs (csrc/frlook_kernels.h).  An open-addressing hash table of 2 * 2^ceil(log2 n_t) words that hold TABLE
 * INDICES (load <= 1/2, linear probing, a hash that mixes all eight words of a key).  Build: one lane per entry claims a slot with a compare-
 * and-swap, or -- the occupant has the same 32 bytes -- lowers it to the smaller index with an atomic minimum.  Count: one lane per looked-up
 * element probes with plain loads, the wave adds up the lanes that found the same j and its leader makes ONE atomic add per distinct j, so a
 * padding-heavy column costs one atomic per wave.  Finish: one lane per entry turns its count into a scalar.  No kernel waits for another.
 */
#ifndef MSM_FRLOOK_H
#define MSM_FRLOOK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRLOOK_MONT256 2u           /* create and count: the scalars are a * 2^256 mod r */
#define MSM_FRLOOK_MISSING 0xFFFFFFFFu  /* idx_out: the value is not in the table */
#define MSM_FRLOOK_MAX_TABLE (1u << 24)
#define MSM_FRLOOK_MAX_ELEMENTS (1u << 26)

typedef struct msm_frlook msm_frlook;

int msm_frlook_abi_version(void); /* 1 */

/* A handle for the n_t keys at `table` in DEVICE memory (a table folded with a challenge is new in every proof and never leaves the device);
 * copied on `stream` before the call returns.  flags: 0 or MSM_FRLOOK_MONT256. */
int msm_frlook_create_device(int curve, int device, void* stream, const void* table, size_t n_t, uint32_t flags, msm_frlook** out);
/* the same for HOST memory (read before the call returns); `device` is where the counts will run and is not touched here */
int msm_frlook_create(int curve, int device, const uint8_t* table, size_t n_t, uint32_t flags, msm_frlook** out);
/* what the handle holds (any pointer may be NULL) */
int msm_frlook_info(const msm_frlook* t, size_t* n_t, size_t* distinct, uint32_t* flags);
/* frees the handle and its device memory (NULL: nothing) */
void msm_frlook_destroy(msm_frlook* t);

/* Looks up the batch x n scalars of DEVICE memory f in the table.  m_out, counts_out, idx_out: device memory or NULL.  flags: the handle's. */
int msm_frlook_count_device(const msm_frlook* t, void* stream, void* m_out, uint32_t* counts_out, uint32_t* idx_out, const void* f, size_t n, size_t batch, size_t stride,
                            uint32_t flags, uint64_t* missing, uint64_t* first_missing);
/* the host form: f and the three outputs are host memory, staged through device memory */
int msm_frlook_count(const msm_frlook* t, uint8_t* m_out, uint32_t* counts_out, uint32_t* idx_out, const uint8_t* f, size_t n, size_t batch, size_t stride, uint32_t flags,
                     uint64_t* missing, uint64_t* first_missing);

/* frees the staging buffers of every device (they come back with the next call); the handles and their tables stay */
void msm_frlook_release(void);

#define MSM_FRLOOK_TEST_HOOKS 1
#ifdef MSM_FRLOOK_TEST_HOOKS
/* the handles created FROM NOW ON keep only the low `bits` (1 .. 32) of the hash; 0 restores the design's 32.  With 1 bit every key starts
 * probing at slot 0 or 1: a table of 65 keys then has chains longer than a wave. */
int msm_frlook_test_hash_bits(int bits);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRLOOK_H */
