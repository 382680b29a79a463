// Layout constants of the MSM pipeline that no field enters: window and bucket-grid sizes, the sort's bin structure, the shapes of the scratch
// arrays the host allocates and the kernels index, and the bits of the device error word.  Included by the host code (msm_plan.h), by the
// curve-neutral recode and sort (recode.h, sort_kernels.h) and by every curve unit (msm_kernels.h).  No kernel and no device object lives here.
// Sizes that follow a unit's field (CW, REC_WORDS, XYZZ_WORDS, BPR_USE_W256, the *_WAVES_PER_SIMD values) stay in msm_kernels.h and reach the
// host through CurveOps (curve_ops.h).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else  // plain C++: the launch planner on the CPU (msm_plan.h under tests/host_harness/msm_plan_harness.cpp)
#define __host__
#define __device__
#endif

#include <cstddef>
#include <cstdint>

// Sparse launches (msm_hip_launch_sparse_device): entry j of the launch is the pair (scalar j, base idx[j]).  The recode and sort passes that
// read scalars take it as ONE trailing argument -- a kernel's `Sparse...` pack holds SparseIdx or nothing, and the dense instantiations, with
// nothing, keep their argument layout and code.  Only the record number an entry carries changes (the scatter passes: idx[j] where the dense
// pass writes the position j); everything behind the scatter never sees positions.  Curve-neutral: no field constant enters the mapping.
struct SparseIdx {
  const uint32_t* idx;  // nnz base indices: any order, repeats allowed
  uint32_t n_bases;     // points per base set; an entry whose index is not below it reads as a zero scalar and sets ERRBIT_BAD_INDEX
  uint32_t* err;        // the slot's error word (for the count passes that have none of their own)
};

namespace msm_layout {
// ---- windows
constexpr int WBITS = 16;   // the reference's window (chunk_size, src/cuzk/msm.rs:79) and the unit of the window-sharding API
constexpr int NWIN = 16;
constexpr int MAXLW = 64;  // local windows one launch may carry: (scalar vectors of the launch) x (windows of each)
constexpr int HALF = 1 << (WBITS - 1);  // 32768 bucket slots per window at 16 bits (the largest window supported)
// windows of a scalar at `bits`-bit signed digits (recode.h: WinCfg has the same as template constants)
__host__ __device__ constexpr int nwin_of(int bits, bool halves = false) { return ((halves ? 127 : 254) + bits) / bits; }
__host__ __device__ constexpr int narrow_nwin_of(int bits, int nb) { return (8 * nb + bits) / bits; }  // windows of an nb-byte narrow scalar
// The NB parameter of the kernels that load narrow scalars: +w for w-byte unsigned integers, -w for w-byte two's-complement ones
__host__ __device__ constexpr int narrow_width(int nb) { return nb < 0 ? -nb : nb; }
// wide fixed-base tables (sort_kernels.h: k_count_wide): tables and virtual windows of 2^15 slots at `bits`-bit digits
__host__ __device__ constexpr int wide_tables_of(int bits) { return (254 + bits) / bits; }
__host__ __device__ constexpr int wide_vwin_of(int bits) { return 1 << (bits - WBITS); }

// ---- the two-level sort (sort_kernels.h)
constexpr int NCOARSE = 128;       // coarse bins per window
constexpr int FINE = HALF / NCOARSE;  // 256 slots per coarse bin
constexpr int FINE_SPLIT = 8;          // workgroups that share a coarse bin of more than FINE_BIG entries (k_sort_fine)
constexpr uint32_t FINE_BIG = 32768;   // (a multiple of the fine sort's staging chunk)
constexpr uint32_t HUGE_BIN_MEANS = 4;  // a bin beyond FINE_BIG is reported as skew when it holds more than this many mean bins of its window
constexpr int LIST_SUB = 2048;          // scalars per sub-tile of the compact lists of wide-table shares (k_count_wide_list)
constexpr int WIDE_SHARE_VWIN_MAX = 4;  // shares of more virtual windows than this run the whole-MSM shape of the two passes
// byte windows (k_byte_count ...): counts[lw][tile][256] and bin_total[lw][256] in the arrays of the coarse sort, which hold BYTE_MAXLW windows of 256 bins
constexpr int BYTE_BINS = 256;
constexpr int BYTE_MAXLW = MAXLW * NCOARSE / BYTE_BINS;  // local windows a byte-window launch may carry (32)

// ---- SMVP chunks (msm_kernels.h: k_smvp_chunks; msm_plan.h: chunk_len_for; sort_kernels.h: smvp_chunk_len)
constexpr int SMVP_CHUNK_MIN_ENTRIES = 8;
constexpr int SMVP_CHUNK_MIN = SMVP_CHUNK_MIN_ENTRIES;
constexpr int SMVP_CHUNK_MAX = 1024;
constexpr int SMVP_TARGET_LANES = 9 << 16;  // three rounds of 3 waves per SIMD (1024 SIMDs x 64 lanes).  Round 3 sweep (profiles/r03_lanes_sweep.txt): against two
                                             // rounds the kernel itself is 3 % faster (shorter chunks even out the SIMDs' finishing times), the stitch has 1.5 x the pieces to
                                             // add, and the step is equal or up to 2 % shorter (2^18, plain bases, window shares); four rounds and more lose to the stitch

// ---- stitch (msm_kernels.h: k_smvp_stitch, k_smvp_stitch_big).  big_queue layout (words): [0] count, [1 .. CAP] items, [BIGQ_CHUNK_LEN] the
// launch's SMVP chunk length, [BIGQ_COUNTERS ..] 256 arrival counters (zero between launches), [BIGQ_SCRATCH ..] 256 bucket records
constexpr uint32_t STITCH_BIG_CAP = 1 << 15;  // queue capacity; more big buckets than this fall back to the serial walk
constexpr int STITCH_BLOCKS = 256;  // grid of k_smvp_stitch_big
constexpr size_t BIGQ_CHUNK_LEN = STITCH_BIG_CAP + 1;
constexpr size_t BIGQ_COUNTERS = STITCH_BIG_CAP + 4;
constexpr size_t BIGQ_SCRATCH = BIGQ_COUNTERS + STITCH_BLOCKS;

// ---- bucket reduce (msm_kernels.h: k_bpr_rowcol, k_bpr_planes)
constexpr int BPR_ROWS = 256, BPR_COLS = 128;
constexpr int PLANES_PER_WINDOW = 16;
// grid of k_bpr_rowcol<LOG_R, LOG_ROWS>: workgroups that sum rows, then workgroups that sum columns
template <int LOG_R, int LOG_ROWS>
constexpr int bpr_rowcol_blocks() {
  constexpr int R = 1 << LOG_R, ROWS = 1 << LOG_ROWS;
  constexpr int rpb = 256 / (BPR_COLS / R), cpb = 256 / (ROWS / R);
  return (ROWS + rpb - 1) / rpb + (BPR_COLS + cpb - 1) / cpb;
}

// ---- error bits written to the context's device error word
constexpr uint32_t ERRBIT_NONCANONICAL = 1u;
constexpr uint32_t ERRBIT_NOT_ON_CURVE = 2u;
constexpr uint32_t ERRBIT_SCALAR_CARRY = 4u;
constexpr uint32_t ERRBIT_BAD_INDEX = 8u;  // a sparse launch's base index was not below the number of resident bases (SparseIdx)
constexpr uint32_t INFOBIT_HUGE_BIN = 0x100u;  // not an error: the fine sort met a coarse bin beyond FINE_BIG and beyond HUGE_BIN_MEANS mean bins (skewed scalars) -- the host's cue to run k_fine_hist
}  // namespace msm_layout
