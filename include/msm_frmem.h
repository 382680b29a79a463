/* libmsm_frmem.so -- the columns of a memory argument on the device (gfx950): a STABLE argsort of integer keys and, from it, the access counters
 * of offline memory checking.  Spartan's Spark, Lasso, Jolt's memories and the RAM of most zkVMs need, for every access i to an address,
 * rank[i] = #{j < i : addr[j] = addr[i]} and the final count per address; the memory and register arguments of halo2- and PLONK-style zkVMs need
 * the whole trace in (address, time) order.  A lookup argument leaves the order of equal values free (include/msm_frcol.h avoids a sort for that
 * reason); a memory argument does not.
 *
 * A library of its own beside libmsm_hip.so, the eight scalar-field libraries and libmsm_frcol.so; it shares no kernel and no host state with
 * them.  It is field-neutral: integer keys, no `curve` argument, no scalar form.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * Keys.  n unsigned words of key_bytes = 4 or 8, 1 <= n <= 2^26.  The caller declares key_bits in 1 .. 8 * key_bytes; the sort runs
 * ceil(key_bits / 8) passes.  Keys are untrusted: a key >= 2^key_bits makes the call return MSM_HIP_ERR_INVALID_ARG and NO output is written --
 * the first pass sees every key before any output exists, and every later launch reads its error word first.
 *
 * msm_frmem_sort.  perm_out[k] is the index of the k-th smallest key; equal keys appear in ascending index order (a stable ascending argsort).
 * keys_out, the sorted keys in the input's width, may be NULL.
 *
 * msm_frmem_access.  With keys[i] the address of access i:
 *     rank_out[i]   = #{j < i : keys[j] = keys[i]}
 *     prev_out[i]   = max{j < i : keys[j] = keys[i]}, or MSM_FRMEM_MISSING where there is none
 *     counts_out[a] = #{i : keys[i] = a}                     for a < n_t
 *     last_out[a]   = max{i : keys[i] = a}, or MSM_FRMEM_MISSING
 *     *distinct     = the number of distinct keys (a HOST word, may be NULL)
 * Any output may be NULL, but not all of them.  Where counts_out or last_out is given, 1 <= n_t <= 2^26 and every key must be < n_t: otherwise
 * MSM_HIP_ERR_INVALID_ARG and nothing is written.  Without them n_t is ignored.
 *
 * Checks, before any device is asked for (MSM_HIP_ERR_INVALID_ARG): the ranges above, key_bytes, key_bits, no NULL keys, no NULL perm_out, keys
 * and keys_out aligned to key_bytes, words to 4 bytes, every output apart from every input and from every other output.
 *
 * Ordering: the _device forms enqueue on `stream` (a hipStream_t; NULL: a stream of the library's own) and return after that stream has
 * completed; the error word and *distinct come back in ONE device-to-host copy through one pinned buffer per device.  Every call runs on
 * `device` and leaves the caller's current device as it found it.  Calls are serialised by the library.  The host forms stage their operands
 * through device memory; a refused call copies nothing back.  The bytes are the same on every run: no atomics.
 *
 * How it runs (csrc/frmem_kernels.h): a least-significant-digit radix sort, 8 bits per pass, with the 32-bit index as
 * payload; per pass a digit count per tile of 1024 keys, an exclusive scan of those counts level by level, and a scatter whose rank inside the
 * tile comes from wave ballots and wave totals in wave order.  access adds one max-scan of the runs' heads over the sorted keys and one lane
 * per sorted position.  No kernel waits for another workgroup.
 */
#ifndef MSM_FRMEM_H
#define MSM_FRMEM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRMEM_MISSING 0xFFFFFFFFu /* prev_out, last_out: no such access */
#define MSM_FRMEM_MAX_ELEMENTS (1u << 26)

int msm_frmem_abi_version(void); /* 1 */

/* DEVICE memory: perm_out n words, keys_out (or NULL) and keys n words of key_bytes */
int msm_frmem_sort_device(int device, void* stream, uint32_t* perm_out, void* keys_out, const void* keys, size_t key_bytes, uint32_t key_bits, size_t n);
/* the same for HOST memory, staged through device memory */
int msm_frmem_sort(int device, uint32_t* perm_out, void* keys_out, const void* keys, size_t key_bytes, uint32_t key_bits, size_t n);

/* DEVICE memory: rank_out and prev_out n words, counts_out and last_out n_t words (each or NULL), keys n words of key_bytes */
int msm_frmem_access_device(int device, void* stream, uint32_t* rank_out, uint32_t* prev_out, uint32_t* counts_out, uint32_t* last_out, size_t n_t, const void* keys,
                            size_t key_bytes, uint32_t key_bits, size_t n, uint64_t* distinct);
int msm_frmem_access(int device, uint32_t* rank_out, uint32_t* prev_out, uint32_t* counts_out, uint32_t* last_out, size_t n_t, const void* keys, size_t key_bytes,
                     uint32_t key_bits, size_t n, uint64_t* distinct);

/* frees the scratch and staging buffers of every device (they come back with the next call) */
void msm_frmem_release(void);

#define MSM_FRMEM_TEST_HOOKS 1
#ifdef MSM_FRMEM_TEST_HOOKS
/* the calls FROM NOW ON work over tiles of `entries` entries (2 .. 1024); 0 restores the design's 1024.  With 64, 4097 keys have 65 * 256 digit
 * counts per pass, which take three scan levels: four levels with the keys.  While a tile is set, a call whose 256 * ceil(n / entries) digit
 * counts do not fit 32 bits (entries <= 4 with n near 2^26) returns MSM_HIP_ERR_INVALID_ARG. */
int msm_frmem_test_tile(int entries);
/* the kernel launches and the levels of the last sort or access of this process */
int msm_frmem_test_last(int* launches, int* levels);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRMEM_H */
