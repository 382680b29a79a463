/* libmsm_frhash.so -- algebraic hashing over the SCALAR field on the device (gfx950): batches of Poseidon permutations, a sponge per row of
 * scalars, and whole Merkle trees, for parameters that are handed over once and stay resident.  It is the step of a prover that commits to a
 * vector by a Merkle root rather than by an MSM, hashes a row of evaluations to a leaf, or plays the random oracle of a folding scheme.
 *
 * The ninth library of the engine, beside libmsm_hip.so (include/msm_hip.h: commitments), libmsm_fr.so (include/msm_fr.h: transforms),
 * libmsm_frvec.so (include/msm_frvec.h: vector arithmetic), libmsm_frpoly.so (include/msm_frpoly.h: univariate openings), libmsm_frmle.so
 * (include/msm_frmle.h: the sumcheck), libmsm_frmat.so (include/msm_frmat.h: R1CS products), libmsm_frgate.so (include/msm_frgate.h: the
 * quotient's numerator) and libmsm_frlook.so (include/msm_frlook.h: lookups).  It shares no kernel, no constant and no host state with the
 * other eight.  Error codes are those of msm_hip.h (MSM_HIP_OK, MSM_HIP_ERR_*).
 *
 * The permutation.  Width t, R_F full rounds (even), R_P partial rounds, S-box x^5, round constants rc[(R_F + R_P) t], matrix M[t][t]
 * (row-major).  For round k = 0 .. R_F + R_P - 1:  s[i] += rc[k t + i] for all i;  s[i] = s[i]^5 for all i where k < R_F / 2 or
 * k >= R_F / 2 + R_P, else for i = 0 alone;  s'[i] = sum_j M[i][j] s[j].  x^5 permutes all five fields (gcd(5, r - 1) = 1), x^3 none of
 * them, so `alpha` is carried and 5 is the one value accepted.  The library is PARAMETER-AGNOSTIC: constants and matrix are the caller's
 * (msm_webgpu_amd.api.poseidon_parameters generates the Poseidon paper's); nothing is built in.
 *
 * Poseidon2 (Grassi, Khovratovich, Schofnegger 2023) is the second permutation, chosen with MSM_FRHASH_POSEIDON2 when the handle is created and
 * served by every call below unchanged: sponge, tree, both data forms, the five fields, the check against r.  Width t in {2, 3, 4, 8, 12} and no
 * other, R_F even and R_P within the limits above, S-box x^5, round constants rc[R_F t + R_P] in the order of their use -- t for each of the
 * first R_F / 2 external rounds, then one for each internal round, then t for each of the last R_F / 2 --, and a vector mu[t]:
 *     s = M_E s                                                                      (the initial linear layer)
 *     R_F / 2 times:  s[i] += rc[..] for all i;  s[i] = s[i]^5 for all i;  s = M_E s
 *     R_P times:      s[0] += rc[..];  s[0] = s[0]^5;  s[i] = mu[i] s[i] + sum_j s[j]  (the sum taken before any s[i] changes)
 *     R_F / 2 times:  as the first R_F / 2
 * M_E: for t = 2 and t = 3, out[i] = s[i] + sum_j s[j], that is circ(2, 1) and circ(2, 1, 1).  For t = 4 it is
 * M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]].  For t = 8 and t = 12, M4 is applied to every block of four and then the sum,
 * over all blocks, of the elements at position i mod 4 is added to element i: circ(2 M4, M4, ..).  The internal layer is M_I = J + diag(mu), J
 * the all-ones matrix.  NOTE WHAT mu IS: the internal matrix's diagonal MINUS ONE -- what HorizenLabs' parameter files call
 * mat_internal_diag_m_1 and Barretenberg internal_matrix_diagonal; the matrix's true diagonal is mu[i] + 1.  Handing over the true diagonal
 * computes another permutation and no check can tell.  Constants are the caller's here too: no published set is built in, and none is generated.
 * Barretenberg's sponge is the convention (L * 2^64, t - 1, 0) below.  The feed-forward compression P(x) + x is not offered.
 *
 * Data.  A scalar is 32 little-endian bytes: a canonical integer below r, or -- MSM_FRHASH_MONT256 -- a * 2^256 mod r; results are in the form
 * of the input and canonical.  THE HASH IS OF THE VALUES: a canonical vector and its a * 2^256 mod r image hash to each other's images.
 * Round constants, matrix and `capacity` are canonical integers below r in BOTH forms.  Every element a lane reads is compared with r by
 * that lane: a value >= r makes the call return MSM_HIP_ERR_NONCANONICAL (the output is then unspecified; the next call is unaffected).
 * Elements between len and stride of a row are not read.
 *
 * The sponge (msm_frhash_hash*): rate t - 1.  The state starts as zero with `capacity` at position capacity_at < t (NULL: 0).  The row's
 * len >= 1 elements are added, t - 1 at a time, onto the OTHER positions in index order, with a permutation after each block; a short last
 * block adds only what is there.  out[row] = state[out_at] after the last permutation.  For len <= t - 1 this is the one-permutation
 * compression of a Merkle node.  The length is the caller's to encode in `capacity`; the library pads with nothing.  (capacity,
 * capacity_at, out_at) is (0, 0, 0) for circomlib's poseidon(inputs), (L * 2^64, t - 1, 0) for halo2's ConstantLength<L>, and
 * (2^arity - 1, 0, 1) for neptune's.
 *
 * The tree (msm_frhash_merkle*): arity A = t - 1, n_leaves = A^k with k >= 1, at most 2^26.  `nodes` receives (n_leaves - 1) / (A - 1)
 * elements -- for A = 1 (t = 2) k elements, n_leaves being 1 and k then given in its place (see below) --, the level above the leaves first
 * and the root last.  Node j of a level is the sponge, with len = A, of elements [A j, A j + A) of the level below.
 *
 * Fields: `curve` is a MSM_HIP_CURVE_* id and selects that curve's scalar field -- BN254 (ids 0 and 5), Grumpkin (1), Pallas (2), Vesta (3),
 * BLS12-381 (4 and 6).  No root of unity is needed, so Grumpkin's scalar field is offered.
 *
 * What the host checks before a device is asked for (MSM_HIP_ERR_INVALID_ARG): the curve; 2 <= t <= MSM_FRHASH_MAX_WIDTH, full_rounds even
 * with 2 <= full_rounds <= MSM_FRHASH_MAX_FULL_ROUNDS, partial_rounds <= MSM_FRHASH_MAX_PARTIAL_ROUNDS, alpha == 5, under MSM_FRHASH_POSEIDON2 t in {2, 3, 4, 8, 12}; the flags; the handle;
 * the ranges given with each call; capacity_at and out_at below t; device pointers 16-byte aligned; the outputs apart from the inputs as
 * each call states.  A round constant, a matrix entry or a `capacity` that is not below r: MSM_HIP_ERR_NONCANONICAL, also before any device.
 *
 * Ordering: msm_frhash_create takes HOST pointers (the tables are tiny), converts them once to the kernel's representation and touches no
 * device; the tables go to `device` with the handle's first call and stay there.  The _device calls enqueue on `stream` (a hipStream_t;
 * NULL: a stream of the library's own) and return after that stream has completed, so that the error word can be reported -- it comes
 * back in ONE device-to-host copy through one pinned buffer per device.  Every call runs on the handle's device and leaves the caller's
 * current device as it found it.  Calls are serialised by the library.  The host forms stage their vectors through device memory.  The
 * library reads no environment setting.
 *
 * How it runs (csrc/frhash_kernels.h): one lane per permutation, its state in a slab of LDS of its own (Poseidon2:
 * one copy of it, both linear layers in place), 64 lanes to a workgroup; a tree is one launch per level.  No kernel waits for another workgroup.
 */
#ifndef MSM_FRHASH_H
#define MSM_FRHASH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_FRHASH_MONT256 2u              /* the data are a * 2^256 mod r; checked against r like canonical data */
#define MSM_FRHASH_POSEIDON2 16u           /* msm_frhash_create alone: the handle is a Poseidon2 permutation (see above) */
#define MSM_FRHASH_MAX_WIDTH 12            /* the largest t */
#define MSM_FRHASH_MAX_FULL_ROUNDS 16      /* the largest R_F */
#define MSM_FRHASH_MAX_PARTIAL_ROUNDS 128  /* the largest R_P */
#define MSM_FRHASH_MAX_ELEMENTS (1u << 26) /* the most scalars a call reads */
#define MSM_FRHASH_MAX_LEVELS 64           /* the most levels of a tree of arity 1 (a chain) */

typedef struct msm_frhash msm_frhash;

int msm_frhash_abi_version(void); /* 1 */

/* A handle for one permutation over one field.  round_constants: (full_rounds + partial_rounds) * t canonical scalars; mds: t * t canonical
 * scalars, row-major; both HOST memory, read before the call returns.  `device` is where the calls will run and is not touched here.
 * flags: 0 or MSM_FRHASH_MONT256, without effect (the tables are canonical integers in both forms, and a call names its own form), and
 * MSM_FRHASH_POSEIDON2: t is one of 2, 3, 4, 8, 12 (another: MSM_HIP_ERR_INVALID_ARG), round_constants holds full_rounds * t + partial_rounds
 * scalars in the order of their use, and mds holds the t scalars of mu -- the internal matrix's diagonal minus one. */
int msm_frhash_create(int curve, int device, uint32_t t, uint32_t full_rounds, uint32_t partial_rounds, uint32_t alpha, const uint8_t* round_constants,
                      const uint8_t* mds, uint32_t flags, msm_frhash** out);
/* what the handle holds (any pointer may be NULL) */
int msm_frhash_info(const msm_frhash* h, uint32_t* t, uint32_t* full_rounds, uint32_t* partial_rounds);
/* frees the handle and its device memory (NULL: nothing) */
void msm_frhash_destroy(msm_frhash* h);

/* n states of t consecutive elements, state i at elements [i t, (i + 1) t) of DEVICE memory: out = permutation(state).  out == state is
 * allowed (in place); otherwise the two are disjoint.  1 <= n, n * t <= 2^26.  flags: MSM_FRHASH_MONT256. */
int msm_frhash_permute_device(const msm_frhash* h, void* stream, void* out, const void* state, size_t n, uint32_t flags);
/* the host form: out and state are host memory */
int msm_frhash_permute(const msm_frhash* h, uint8_t* out, const uint8_t* state, size_t n, uint32_t flags);

/* out[row] = the sponge of a[row * stride .. row * stride + len), row < rows.  1 <= len <= stride, (rows - 1) * stride + len <= 2^26;
 * `out` (rows elements) is disjoint from a[0 .. (rows - 1) * stride + len).  capacity: 32 HOST bytes or NULL.  flags: MSM_FRHASH_MONT256. */
int msm_frhash_hash_device(const msm_frhash* h, void* stream, void* out, const void* a, size_t rows, size_t len, size_t stride, const uint8_t* capacity,
                           uint32_t capacity_at, uint32_t out_at, uint32_t flags);
/* the host form: out and a are host memory */
int msm_frhash_hash(const msm_frhash* h, uint8_t* out, const uint8_t* a, size_t rows, size_t len, size_t stride, const uint8_t* capacity, uint32_t capacity_at,
                    uint32_t out_at, uint32_t flags);

/* The levels of the tree over n_leaves = A^k leaves in DEVICE memory, A = t - 1: `nodes`, disjoint from the leaves, receives the
 * (n_leaves - 1) / (A - 1) elements above them.  For A = 1 the tree is a chain over ONE leaf and n_leaves is the number k of its levels,
 * 1 <= k <= MSM_FRHASH_MAX_LEVELS: nodes[0] = hash(leaf), nodes[j] = hash(nodes[j - 1]).  flags: MSM_FRHASH_MONT256. */
int msm_frhash_merkle_device(const msm_frhash* h, void* stream, void* nodes, const void* leaves, size_t n_leaves, const uint8_t* capacity, uint32_t capacity_at,
                             uint32_t out_at, uint32_t flags);
/* the host form: nodes and leaves are host memory */
int msm_frhash_merkle(const msm_frhash* h, uint8_t* nodes, const uint8_t* leaves, size_t n_leaves, const uint8_t* capacity, uint32_t capacity_at, uint32_t out_at,
                      uint32_t flags);

/* frees the staging buffers of every device (they come back with the next call); the handles and their tables stay */
void msm_frhash_release(void);

#define MSM_FRHASH_TEST_HOOKS 1
#ifdef MSM_FRHASH_TEST_HOOKS
/* only the first `lanes` (1 .. 64) lanes of a workgroup take a permutation, so that n = 65 states span 17 workgroups at lanes = 4; 0 restores
 * the design's 64.  Anything else: MSM_HIP_ERR_INVALID_ARG. */
int msm_frhash_test_tile(int lanes);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MSM_FRHASH_H */
