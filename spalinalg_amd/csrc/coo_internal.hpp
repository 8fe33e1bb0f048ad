// coo_internal.hpp -- what crosses the seams between the COO sources (not installed): spal_coo_sort.hip (scan, radix
// sort, group offsets), spal_coo_group.hip (the group kernel), spal_coo_assemble.hip (workspace, the assembly),
// spal_transpose.hip (CSR <-> CSC) and spal_coo.hip (handle, C ABI).
#pragma once

#include "spal_ops.hpp"

namespace spal {

// ---- device helpers of the sort kernels and the group kernel --------------------------------------------------------
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems;  // 2048

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v += t;
    }
    return v;
}

// Counters in LDS that the lanes of ONE wave hand to each other between two rounds of a ranking loop (the lowest lane of
// a digit publishes the new count, the next round's lanes read it).  The compiler must re-read them every round; declared
// `volatile` it did -- but through FLAT instructions (address-space inference leaves volatile accesses alone), each followed
// by s_waitcnt vmcnt(0): 32 serialised flat round trips per tile in radix_scatter, and in the group kernel a wait for every
// load in flight.  Relaxed atomics at wavefront scope are plain ds_read / ds_write, re-read every time, and LDS
// instructions of one wave execute in order.
__device__ __forceinline__ uint32_t lds_peek(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void lds_poke(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// block-wide exclusive scan of one value per thread (256 threads); returns the
// exclusive prefix, *total receives the block sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < kScanThreads / 64; ++i) {
        const uint32_t s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// ---- the radix sort (spal_coo_sort.hip) -----------------------------------------------------------------------------
// The digit counts of a pass and what the scatter derives its offsets from (round 4: no scan over all 256 x tiles counts --
// three launches and 24 us per pass at config 5 -- any more):
//   raw[d * stride + t]   keys of tile t with digit d, as counted (stride = tiles rounded up to whole groups of 16);
//   gt[d * groups + g]    the total of digit d over group g's 16 tiles; after digit_scan: the digit's keys in the groups
//                         BEFORE g (exclusive, inside the digit);
//   dt[d]                 all keys with digit d.
// Where tile t's keys with digit d go:  (sum of dt over smaller digits: 256 values, scanned by the scatter workgroup itself)
//   + gt[d][t / 16] + the raw counts of the tiles of t's group before t (at most 15 words of one 64-byte line).
struct PassCounts {
    uint32_t *raw = nullptr, *gt = nullptr, *dt = nullptr;
};
constexpr int kHistGroup = 16;   // tiles a radix_hist workgroup counts (see there)

template <typename T>
struct SortBuffers {
    uint32_t *key[2] = {nullptr, nullptr};
    uint32_t *aux[2] = {nullptr, nullptr};
    T *val[2] = {nullptr, nullptr};
    PassCounts counts;           // raw 256 * stride, gt 256 * groups, dt 256
    PassCounts counts2;          // the same again: the second pass's, when the first pass's counts must survive it
    uint32_t *sums = nullptr;    // scan scratch (general route)
};
// tiles of kSortTile entries, groups of kHistGroup tiles, and tiles rounded up to whole groups (the SPAL_SORT_* geometry
// stays in spal_coo_sort.hip)
uint32_t sort_tiles(uint64_t len);
uint32_t sort_groups(uint64_t len);
uint32_t sort_stride(uint64_t len);
inline uint32_t bits_for(uint64_t n) {  // bits needed for values in [0, n)
    uint32_t b = 0;
    while (b < 64 && (1ull << b) < n) ++b;
    return b ? b : 1;
}

// out[i] = sum in[0..i); *d_total (device, may be NULL) = sum of all; with
// `closing`, out must have n + 1 entries and out[n] = the total.  `sums` must
// hold ceil(n / kScanTile) u32.  in == out allowed.
hipError_t exclusive_scan_u32(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t *sums,
                              uint32_t *d_total, hipStream_t st, bool closing = false);
// Sorts by bits [lo_bit, lo_bit + nbits) of key, stably.  The first pass reads
// (k_in, a_in, v_in) when given (the caller's arrays, left untouched), else
// buffer set `cur`; `cur` is updated to the set that holds the result.
// `two_counts`: the second pass counts into b.counts2, so that the first pass's scanned counts (the digit buckets'
// starts) are still there afterwards.  `pack_bits` >= 0: the LAST pass writes the packed payload (radix_scatter<T, true>)
// and no keys.
template <typename T>
hipError_t radix_sort_bits(SortBuffers<T> &b, uint64_t len, uint32_t lo_bit, uint32_t nbits,
                           int &cur, hipStream_t st, const uint32_t *k_in = nullptr,
                           const uint32_t *a_in = nullptr, const T *v_in = nullptr,
                           bool two_counts = false, int pack_bits = -1);
// start[] of a sorted key array: the streaming pass, unless rows outnumber entries
// so much that one thread of it would fill long stretches of empty rows
void launch_row_starts(const uint32_t *sorted_row, uint32_t n, uint32_t nrows, uint32_t *start,
                       hipStream_t st, uint32_t shift = 0);
// After a sort by the row bits above gbits that left its result in set `cur`: gstart[0 .. ngroups] = the first sorted
// entry of every group of 2^gbits rows -- `two_pass`: from the two passes' counts (group_offsets), else by one streaming
// pass over the sorted keys -- and *fullest = max(*fullest, entries of the fullest group).
template <typename T>
void launch_group_starts(const SortBuffers<T> &b, int cur, bool two_pass, uint64_t len, uint32_t gbits,
                         uint32_t ngroups, uint32_t *gstart, uint32_t *fullest, hipStream_t st);

// ---- the group kernel (spal_coo_group.hip) --------------------------------------------------------------------------
constexpr int kGroupCap = 2048;  // entries a group of rows may hold for the LDS local sort
constexpr uint32_t kLookbackSpins = 1u << 21;   // (seconds: a bound, so that every wave reaches its exit; SPAL_COO_LOOKBACK_SPINS overrides)
constexpr uint32_t kTicketClasses = 8;
extern const uint32_t kTailWords;   // words of the state[] tail behind the groups' look-back words (laid out beside the kernel)
// coo_group_sort's arguments, in its order
template <typename T>
struct GroupSortArgs {
    const uint32_t *gstart, *sorted_row, *cols;
    const T *vals;
    uint32_t nrows, gbits, ngroups;
    unsigned long long *state;
    uint32_t *err, *tickets;
    uint32_t ticket_classes, spin_bound;
    uint32_t *rowptr, *out_col;
    T *out_val;
    uint2 *gwin;
};
// One launch of coo_group_sort<T, cap, packed, row_sort> over a.ngroups workgroups; cap is 512, 1024, 1536 or kGroupCap.
template <typename T>
int launch_group_sort(int cap, bool packed, bool row_sort, const GroupSortArgs<T> &a, hipStream_t st);

// ---- the assembly (spal_coo_assemble.hip) ---------------------------------------------------------------------------
// One allocation for everything the assembly needs besides its output, made
// when the COO matrix is uploaded (setup, not the timed path).
struct CooWorkspace {
    size_t bytes = 0;
    size_t off_key[2], off_aux[2], off_val[2], off_raw[2], off_gt[2], off_dt[2], off_sums, off_state, off_total, off_gstart;
};
CooWorkspace coo_workspace_layout(uint64_t len, uint64_t nrows, size_t elem);
// the sort buffers, both passes' counts and the scan scratch of a workspace block laid out by coo_workspace_layout
template <typename T>
SortBuffers<T> coo_workspace_sort_buffers(char *wb, const CooWorkspace &ws);

// Environment knobs of the assembly: read once per assembly call (never cached: the tests change them between calls).
struct CooKnobs {
    uint32_t lookback_spins = kLookbackSpins;   // SPAL_COO_LOOKBACK_SPINS: the look-back's spin bound (tests: 0 forces the backstop)
    int ticket_mode = 8;     // SPAL_COO_TICKET: 0 = blockIdx, 1 = one counter (round 3), anything else = the 8 class counters (tests, lab)
    bool no_offsets = false; // SPAL_COO_NO_OFFSETS: the groups' offsets from the sorted keys, not from the passes' counts (tests)
    bool no_pack = false;    // SPAL_COO_NO_PACK: key + column instead of the packed payload (tests, lab)
    bool loop_ranks = false; // SPAL_COO_LOOP_RANKS: the group kernel's loop-rank form from the first launch (lab)
    bool debug = false;      // SPAL_COO_DEBUG: one line per group-kernel launch on stderr (lab)
    bool eager_plan = false; // SPAL_COO_EAGER_PLAN=1: spal_coo_assemble_csr plans the products inside the call (lab)
};
CooKnobs coo_read_knobs();

// The assembly on (major, minor): for CSR major = rows, for CSC major = columns
// (`From<&CooMatrix> for CscMatrix`, src/csc/conv/coo.rs:4-115, is the same code
// with the two exchanged).  Produces the compressed arrays; the caller wraps
// them in a handle.  Invariant: cap >= nnz + kStreamPad, the stream kernels' over-read margin (ind and val hold cap entries,
// zeros behind the nnz-th), for the empty matrix too.
struct Assembled : OpArrays {   // (ptr, ind, val, nnz, cap: owned here until a handle adopts them)
    // {first, one past last} minor index of every group of 2^gwin_bits majors of the result, still on the device, when
    // the local sort produced it on the way (saves the CSR planner its own pass over the matrix; ownership passes to
    // whoever takes the result)
    uint2 *d_gwin = nullptr;
    uint32_t gwin_n = 0, gwin_bits = 0;
};
int coo_assemble(spal_coo *c, bool by_cols, hipStream_t st, const CooKnobs &knobs, Assembled &res);

}  // namespace spal
