/* libmsm_frcol.so -- the columns of a lookup argument from its counts, on the device (gfx950): halo2's permuted pair A', S' and plookup's sorted
 * vector s = (f, t) sorted by t.  Neither argument fixes the order of the runs -- any grouping of equal values satisfies the constraints -- so
 * both columns follow from the table t and the counts c[j] = #{i : f[i] = t[j]} that libmsm_frlook.so writes (include/msm_frlook.h: counts_out),
 * without a sort of 256-bit values: an integer prefix sum, a run expansion and a compaction.
 *
 * A library of its own beside libmsm_hip.so and the eight scalar-field libraries; it shares no kernel and no host state with them.  It moves
 * 32-byte scalars AS STORED: no field arithmetic, no comparison with r -- its inputs come from calls that have checked them --, so there is no
 * `curve` argument and no flag for the data's form.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * msm_frcol_expand.  With w[j] = counts[j] + bias, bias 0 or 1: out is t[0] w[0] times, then t[1] w[1] times, and so on.  1 <= n_t <= 2^24,
 * 1 <= n_out <= 2^26.  The sum of the w[j] is formed in 64 bits and returned in *total (a HOST word, may be NULL); where it is not n_out the
 * call returns MSM_HIP_ERR_INVALID_ARG and out is untouched (the counts are untrusted words: a sum that wraps in 32 bits is refused like any
 * other).  bias = 0 over a count's counts_out is halo2's A'; bias = 1 with n_out = n + n_t is plookup's s: every adjacent pair of s is an
 * equal pair or a pair (t[j], t[j + 1]).
 *
 * msm_frcol_pair.  halo2's two columns in one call; it requires n = n_t and sum counts = n.  With off[j] the exclusive prefix sum of counts,
 * r[j] = #{j' < j : counts[j'] > 0} and z the ascending list of the j with counts[j] = 0: for k = off[j] + d, d < counts[j],
 *     a_out[k] = t[j];      s_out[k] = t[j] if d = 0, else t[z[k - r[j] - 1]].
 * So A' is a permutation of the looked-up column, S' a permutation of the table as a multiset, A'[0] = S'[0], and for every i > 0
 * A'[i] is S'[i] or A'[i - 1].  (libmsm_frlook.so credits a repeated table value to its lowest index: the later copies have count 0 and are
 * fillers.)  *total: the sum of the counts; *used: the number of entries with counts > 0 (HOST words, may be NULL).  A sum that is not n:
 * MSM_HIP_ERR_INVALID_ARG, both outputs untouched.
 *
 * msm_frcol_gather.  out[i] = a[idx[i]], i < n; idx[i] = 0xFFFFFFFF (a count's MSM_FRLOOK_MISSING) gives 32 zero bytes.  Any other
 * idx[i] >= n_a makes the call return MSM_HIP_ERR_INVALID_ARG; that element is written as zero, the others as usual.  1 <= n_a, n <= 2^26.
 * What a vector lookup does after the count: it fetches the other columns of the matched rows.
 *
 * Checks, before any device is asked for (MSM_HIP_ERR_INVALID_ARG): the ranges above, bias, no NULL pointer among the data, device pointers of
 * scalars 16-byte aligned, pointers of words 4-byte aligned, every output apart from every input and from the other outputs.
 *
 * Ordering: the _device forms enqueue on `stream` (a hipStream_t; NULL: a stream of the library's own) and return after that stream has
 * completed; the error word and the totals come back in ONE device-to-host copy through one pinned buffer per device.  Every call runs on
 * `device` and leaves the caller's current device as it found it.  Calls are serialised by the library.  The host forms stage their operands
 * through device memory; a refused call copies nothing back.  The bytes are the same on every run: no atomics.
 *
 * How it runs (csrc/frcol_kernels.h): the prefix sums level by level over tiles of 1024 entries with 64-bit tile sums,
 * then one lane per OUTPUT, which finds its run by two binary searches -- the tile bases, then the offsets inside the tile.  One entry repeated
 * n times, n entries once each and a table of mostly zero counts cost the same.  No kernel waits for another workgroup.
 */
#ifndef MSM_FRCOL_H
#define MSM_FRCOL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRCOL_MISSING 0xFFFFFFFFu /* gather: idx of 32 zero bytes */
#define MSM_FRCOL_MAX_TABLE (1u << 24)
#define MSM_FRCOL_MAX_ELEMENTS (1u << 26)

int msm_frcol_abi_version(void); /* 1 */

/* DEVICE memory: out n_out scalars, t n_t scalars, counts n_t words */
int msm_frcol_expand_device(int device, void* stream, void* out, const void* t, const uint32_t* counts, size_t n_t, uint32_t bias, size_t n_out, uint64_t* total);
/* the same for HOST memory, staged through device memory */
int msm_frcol_expand(int device, uint8_t* out, const uint8_t* t, const uint32_t* counts, size_t n_t, uint32_t bias, size_t n_out, uint64_t* total);

/* DEVICE memory: a_out, s_out and t n scalars each, counts n words */
int msm_frcol_pair_device(int device, void* stream, void* a_out, void* s_out, const void* t, const uint32_t* counts, size_t n, uint64_t* total, uint64_t* used);
int msm_frcol_pair(int device, uint8_t* a_out, uint8_t* s_out, const uint8_t* t, const uint32_t* counts, size_t n, uint64_t* total, uint64_t* used);

/* DEVICE memory: out n scalars, a n_a scalars, idx n words */
int msm_frcol_gather_device(int device, void* stream, void* out, const void* a, size_t n_a, const uint32_t* idx, size_t n);
int msm_frcol_gather(int device, uint8_t* out, const uint8_t* a, size_t n_a, const uint32_t* idx, size_t n);

/* frees the scratch and staging buffers of every device (they come back with the next call) */
void msm_frcol_release(void);

#define MSM_FRCOL_TEST_HOOKS 1
#ifdef MSM_FRCOL_TEST_HOOKS
/* the calls FROM NOW ON scan over tiles of `entries` entries (2 .. 1024); 0 restores the design's 1024.  With 64 a table of 4097 entries
 * takes three levels (4097 entries, 65 tile sums, 2 sums of those). */
int msm_frcol_test_tile(int entries);
/* the kernel launches and the scan levels of the last expand or pair of this process */
int msm_frcol_test_last(int* launches, int* levels);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRCOL_H */
