// spal_coo_sort.hip -- the generic two-level exclusive scan and the stable LSD radix sort (histogram, digit scan,
// scatter) that the COO assembly and the CSR <-> CSC transpose are built on, and what follows a sort by rows: the
// groups' offsets, row starts, the fullest group.
#include "coo_internal.hpp"

namespace spal {

// --------------------------------------------------------------------------
// exclusive scan of u32 (generic, two levels)
// --------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void scan_tile_sums(const uint32_t *__restrict__ in,
                                                               uint64_t n,
                                                               uint32_t *__restrict__ sums) {
    const uint64_t t0 = (uint64_t)blockIdx.x * kScanTile;
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        const uint64_t i = t0 + (uint64_t)j * kScanThreads + threadIdx.x;
        if (i < n) acc += in[i];
    }
    uint32_t total;
    (void)block_exclusive_scan(acc, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// single workgroup: exclusive scan of `sums` in place; total -> *grand (may be NULL)
__global__ __launch_bounds__(kScanThreads) void scan_sums_inplace(uint32_t *sums, uint32_t m,
                                                                  uint32_t *grand) {
    uint32_t carry = 0;
    for (uint32_t b = 0; b < m; b += kScanThreads) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < m ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, &total);
        if (i < m) sums[i] = carry + ex;
        carry += total;
    }
    if (grand && threadIdx.x == 0) *grand = carry;
}

// out[i] = prefix; when `closing` is set out[n] = grand total as well
__global__ __launch_bounds__(kScanThreads) void scan_apply(const uint32_t *__restrict__ in,
                                                           uint32_t *__restrict__ out, uint64_t n,
                                                           const uint32_t *__restrict__ sums,
                                                           int closing) {
    // thread owns kScanItems CONSECUTIVE elements so the scan order is the array order
    const uint64_t t0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems];
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = (t0 + j < n) ? in[t0 + j] : 0u;
        acc += v[j];
    }
    uint32_t total;
    uint32_t ex = block_exclusive_scan(acc, &total) + sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (t0 + j < n) out[t0 + j] = ex;
        ex += v[j];
        if (closing && t0 + j + 1 == n) out[n] = ex;
    }
}

hipError_t exclusive_scan_u32(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t *sums,
                              uint32_t *d_total, hipStream_t st, bool closing) {
    if (n == 0) {
        hipError_t e = hipSuccess;
        if (d_total) e = hipMemsetAsync(d_total, 0, sizeof(uint32_t), st);
        if (e == hipSuccess && closing) e = hipMemsetAsync(out, 0, sizeof(uint32_t), st);
        return e;
    }
    const uint32_t tiles = (uint32_t)((n + kScanTile - 1) / kScanTile);
    hipLaunchKernelGGL(scan_tile_sums, dim3(tiles), dim3(kScanThreads), 0, st, in, n, sums);
    hipLaunchKernelGGL(scan_sums_inplace, dim3(1), dim3(kScanThreads), 0, st, sums, tiles, d_total);
    hipLaunchKernelGGL(scan_apply, dim3(tiles), dim3(kScanThreads), 0, st, in, out, n, sums,
                       closing ? 1 : 0);
    return hipGetLastError();
}

// --------------------------------------------------------------------------
// stable LSD radix sort: (u32 key, u32 aux, T value), 8 bits per pass
// --------------------------------------------------------------------------
#ifndef SPAL_SORT_THREADS
#define SPAL_SORT_THREADS 256
#endif
#ifndef SPAL_SORT_XCD
#define SPAL_SORT_XCD 1
#endif
#ifndef SPAL_SORT_ITEMS
#define SPAL_SORT_ITEMS 16
#endif
constexpr int kSortThreads = SPAL_SORT_THREADS;           // scatter workgroup
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortItems = SPAL_SORT_ITEMS;               // per thread
constexpr int kSortTile = kSortThreads * kSortItems;      // 4096 entries per workgroup
constexpr int kWaveChunk = 64 * kSortItems;               // consecutive entries per wave
constexpr int kHistThreads = 256;
constexpr int kHistItems = kSortTile / kHistThreads;

// radix_hist: the order inside a tile does not matter here: 16-byte loads, 4 keys per lane.  A workgroup counts kHistGroup
// consecutive tiles and writes, per digit, their counts as ONE run of kHistGroup words (one tile per workgroup wrote 107 MB
// for 12.5 MB of counts at config 5: profiles/r03/pmc_traffic.txt), and the run's total.
__global__ __launch_bounds__(kHistThreads) void radix_hist(const uint32_t *__restrict__ keys,
                                                           uint64_t len, uint32_t shift,
                                                           uint32_t *__restrict__ raw, uint32_t *__restrict__ gt,
                                                           uint32_t nblk, uint32_t stride, uint32_t groups) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    __shared__ uint32_t h[kHistGroup][257];   // (257: the transposed read below walks a column)
    for (int j = 0; j < kHistGroup; ++j) h[j][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t blk0 = blockIdx.x * kHistGroup;
    static_assert(kSortTile % (4 * kHistThreads) == 0, "tile = whole rounds of 4 keys per thread");
    for (int g = 0; g < kHistGroup; ++g) {   // uniform
        const uint32_t blk = blk0 + (uint32_t)g;
        if (blk >= nblk) break;
        const uint64_t t0 = (uint64_t)blk * kSortTile;  // multiple of 4: 16-byte aligned
        if (t0 + kSortTile <= len) {
            u32x4 k[kHistItems / 4];
#pragma unroll
            for (int j = 0; j < kHistItems / 4; ++j)
                k[j] = *reinterpret_cast<const u32x4 *>(keys + t0 + ((uint64_t)j * kHistThreads + threadIdx.x) * 4);
#pragma unroll
            for (int j = 0; j < kHistItems / 4; ++j) {
                atomicAdd(&h[g][(k[j].x >> shift) & 0xffu], 1u);
                atomicAdd(&h[g][(k[j].y >> shift) & 0xffu], 1u);
                atomicAdd(&h[g][(k[j].z >> shift) & 0xffu], 1u);
                atomicAdd(&h[g][(k[j].w >> shift) & 0xffu], 1u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < kHistItems; ++j) {
                const uint64_t i = t0 + (uint64_t)j * kHistThreads + threadIdx.x;
                if (i < len) atomicAdd(&h[g][(keys[i] >> shift) & 0xffu], 1u);
            }
        }
    }
    __syncthreads();
    // sixteen lanes write one digit's run of sixteen counts (64 contiguous, aligned bytes; zeros for tiles beyond the last),
    // a wave four digits' runs
    const uint32_t g = threadIdx.x % kHistGroup;
    for (uint32_t d = threadIdx.x / kHistGroup; d < 256; d += kHistThreads / kHistGroup)
        raw[(uint64_t)d * stride + blk0 + g] = h[g][d];
    {   // thread d: the group's total of digit d
        const uint32_t d = threadIdx.x;
        uint32_t tot = 0;
#pragma unroll
        for (int j = 0; j < kHistGroup; ++j) tot += h[j][d];
        gt[(uint64_t)d * groups + blockIdx.x] = tot;
    }
}

// Workgroup d: gt[d][.] -> its exclusive prefix in place (the digit's keys in earlier groups), dt[d] = the digit's total.
__global__ __launch_bounds__(256) void digit_scan(uint32_t *__restrict__ gt, uint32_t *__restrict__ dt, uint32_t groups) {
    uint32_t *row = gt + (uint64_t)blockIdx.x * groups;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < groups; b += 256) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < groups ? row[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, &total);
        if (i < groups) row[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) dt[blockIdx.x] = carry;
}

// Stable scatter of one tile.  Wave w owns the tile's entries [w*1024, (w+1)*1024)
// and walks them 64 at a time, so tile order = (wave, round, lane).  The rank
// of an entry among the tile's entries with the same digit is
//   entries of earlier waves + entries of earlier rounds of this wave +
//   earlier lanes of this round,
// computed from ballots and per-wave counters without atomics: deterministic
// and stable.  The tile is first written to LDS in digit order, then copied out
// linearly, so each digit leaves the workgroup as ONE contiguous run
// (coalesced stores) that starts at the scanned global offset of (digit, tile).
// PACK (the last pass before the group kernel, when the minor index and the row inside its group fit one word): the
// key is not written at all and the payload leaves as aux | (key & (2^pack_bits - 1)) << (32 - pack_bits) -- the group a
// sorted entry belongs to is its position, all the group kernel still needs of the row are its low bits: 12 instead of 16
// bytes per entry written here and read there.
template <typename T, bool PACK = false>
__global__ __launch_bounds__(kSortThreads) void radix_scatter(
    const uint32_t *__restrict__ kin, const uint32_t *__restrict__ ain, const T *__restrict__ vin,
    uint32_t *__restrict__ kout, uint32_t *__restrict__ aout, T *__restrict__ vout, uint64_t len,
    uint32_t shift, const uint32_t *__restrict__ raw, const uint32_t *__restrict__ gt, const uint32_t *__restrict__ dt,
    uint32_t nblk, uint32_t stride, uint32_t groups, uint32_t per_xcd, uint32_t pack_bits = 0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spal_sort_smem[];
    T *s_val = reinterpret_cast<T *>(spal_sort_smem);                       // kSortTile
    uint32_t *s_key = reinterpret_cast<uint32_t *>(s_val + kSortTile);      // kSortTile
    uint32_t *s_aux = s_key + kSortTile;                                    // kSortTile
    // lanes of a wave hand counts to each other through this array between two rounds (lds_peek / lds_poke)
    uint32_t *cnt = s_aux + kSortTile;                                       // [kSortWaves][256]
    uint32_t *s_start = cnt + kSortWaves * 256;                              // [256] tile-local digit start
    uint32_t *s_delta = s_start + 256;                                       // [256] global - local
    uint32_t *s_wsum = s_delta + 256;                                        // [4] + [4] digit-scan wave sums (tile-local starts, digit bases)

    // tiles that run side by side on one XCD are neighbours in tile order, so the
    // partial cache lines they leave at the end of each digit's run meet in one L2
#if SPAL_SORT_XCD
    const uint32_t tile = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
#else
    const uint32_t tile = blockIdx.x;
#endif
    if (tile >= nblk) return;  // block-uniform
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < kSortWaves * 256; i += kSortThreads) cnt[i] = 0;
    __syncthreads();

    const uint64_t tile0 = (uint64_t)tile * kSortTile;
    const uint64_t w0 = tile0 + (uint64_t)w * kWaveChunk;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t key[kSortItems], aux[kSortItems], rank[kSortItems];
    T val[kSortItems];
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint64_t i = w0 + (uint64_t)j * 64 + lane;
        const bool ok = i < len;
        key[j] = ok ? kin[i] : 0u;
        aux[j] = ok ? ain[i] : 0u;
        val[j] = ok ? vin[i] : T(0);
    }
    // thread d: where this tile's keys with digit d go, apart from the digits' bases (PassCounts) -- requested behind the
    // tile's entries, summed when the ranks are done (asked for first and summed at once they held the entries' loads back:
    // 379 instead of 351 us for the first pass at config 5)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    uint32_t my_dt = 0, my_gt = 0;
    u32x4 my_line[kHistGroup / 4];
    if (threadIdx.x < 256) {
        const uint32_t d = threadIdx.x, grp = tile / (uint32_t)kHistGroup;
        my_dt = dt[d];
        my_gt = gt[(uint64_t)d * groups + grp];
        const u32x4 *line = reinterpret_cast<const u32x4 *>(raw + (uint64_t)d * stride + (uint64_t)grp * kHistGroup);
#pragma unroll
        for (int q = 0; q < kHistGroup / 4; ++q) my_line[q] = line[q];
    }
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint64_t i = w0 + (uint64_t)j * 64 + lane;
        const bool ok = i < len;
        const uint32_t d = (key[j] >> shift) & 0xffu;
        // lanes of this round with the same digit (inactive tail lanes excluded)
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const uint32_t before = ok ? lds_peek(&cnt[w * 256 + d]) : 0u;
        rank[j] = before + (uint32_t)__popcll(peers & lt);
        // the lowest peer lane publishes the new count (one writer per digit)
        if (ok && (peers & lt) == 0) lds_poke(&cnt[w * 256 + d], before + (uint32_t)__popcll(peers));
    }
    __syncthreads();
    // per digit: exclusive prefix over the waves; tile-local start of the digit;
    // distance between the digit's global run and its place in the tile
    {
        const uint32_t d = threadIdx.x;  // the first 256 threads (whole waves) take the 256 digits
        uint32_t run = 0, inc = 0, inc_dt = 0;
        if (d < 256) {
#pragma unroll
            for (int ww = 0; ww < kSortWaves; ++ww) {
                const uint32_t c = cnt[ww * 256 + d];
                cnt[ww * 256 + d] = run;
                run += c;
            }
            inc = wave_inclusive_scan(run);
            inc_dt = wave_inclusive_scan(my_dt);
            if (lane == 63) { s_wsum[w] = inc; s_wsum[4 + w] = inc_dt; }
        }
        __syncthreads();
        if (d < 256) {
            uint32_t base = 0, base_dt = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (i < w) { base += s_wsum[i]; base_dt += s_wsum[4 + i]; }
            const uint32_t start = base + inc - run;
            s_start[d] = start;
            uint32_t my_before = my_gt;
            const uint32_t in_grp = tile % (uint32_t)kHistGroup;
#pragma unroll
            for (int q = 0; q < kHistGroup / 4; ++q)
                my_before += ((uint32_t)(4 * q) < in_grp ? my_line[q].x : 0u) + ((uint32_t)(4 * q + 1) < in_grp ? my_line[q].y : 0u) +
                             ((uint32_t)(4 * q + 2) < in_grp ? my_line[q].z : 0u) + ((uint32_t)(4 * q + 3) < in_grp ? my_line[q].w : 0u);
            s_delta[d] = (base_dt + inc_dt - my_dt) + my_before - start;   // keys with smaller digits + digit d's keys in earlier tiles
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint64_t i = w0 + (uint64_t)j * 64 + lane;
        if (i < len) {
            const uint32_t d = (key[j] >> shift) & 0xffu;
            const uint32_t lp = s_start[d] + cnt[w * 256 + d] + rank[j];
            s_key[lp] = key[j];
            s_aux[lp] = aux[j];
            s_val[lp] = val[j];
        }
    }
    __syncthreads();
    const uint32_t n_tile = (uint32_t)min((uint64_t)kSortTile, len - tile0);
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint32_t lp = j * kSortThreads + threadIdx.x;
        if (lp < n_tile) {
            const uint32_t k = s_key[lp];
            const uint32_t gp = s_delta[(k >> shift) & 0xffu] + lp;
            if (PACK) {
                aout[gp] = pack_bits ? (s_aux[lp] | ((k & ((1u << pack_bits) - 1u)) << (32u - pack_bits))) : s_aux[lp];
            } else {
                kout[gp] = k;
                aout[gp] = s_aux[lp];
            }
            vout[gp] = s_val[lp];
        }
    }
}

uint32_t sort_tiles(uint64_t len) { return (uint32_t)((len + kSortTile - 1) / kSortTile); }
uint32_t sort_groups(uint64_t len) { return (sort_tiles(len) + kHistGroup - 1) / kHistGroup; }
uint32_t sort_stride(uint64_t len) { return sort_groups(len) * kHistGroup; }

template <typename T>
static size_t sort_lds_bytes() {
    return (size_t)kSortTile * (sizeof(T) + 8) + (size_t)(kSortWaves * 256 + 512 + 8) * 4;
}

template <typename T>
hipError_t radix_sort_bits(SortBuffers<T> &b, uint64_t len, uint32_t lo_bit, uint32_t nbits, int &cur, hipStream_t st,
                           const uint32_t *k_in, const uint32_t *a_in, const T *v_in, bool two_counts, int pack_bits) {
    if (len == 0) return hipSuccess;
    const uint32_t nblk = sort_tiles(len), groups = sort_groups(len), stride = sort_stride(len);
    const size_t lds = sort_lds_bytes<T>();
    {  // > 64 KiB of dynamic LDS needs the cap raised (per device; cheap, so every call)
        hipError_t e = hipFuncSetAttribute((const void *)radix_scatter<T, false>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess && pack_bits >= 0)
            e = hipFuncSetAttribute((const void *)radix_scatter<T, true>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    int pass = 0;
    for (uint32_t shift = lo_bit; shift < lo_bit + nbits; shift += 8, ++pass) {
        const uint32_t *ki = k_in ? k_in : b.key[cur];
        const uint32_t *ai = k_in ? a_in : b.aux[cur];
        const T *vi = k_in ? v_in : b.val[cur];
        const int dst = k_in ? cur : (cur ^ 1);
        const PassCounts &pc = (two_counts && pass == 1) ? b.counts2 : b.counts;
        hipLaunchKernelGGL(radix_hist, dim3(groups), dim3(kHistThreads), 0, st, ki, len, shift, pc.raw, pc.gt, nblk, stride, groups);
        hipLaunchKernelGGL(digit_scan, dim3(256), dim3(256), 0, st, pc.gt, pc.dt, groups);
        const uint32_t per_xcd = (nblk + 7) / 8;
        const bool pack = shift + 8 >= lo_bit + nbits && pack_bits >= 0;   // the last pass, and the caller wants the packed payload
        hipLaunchKernelGGL((pack ? radix_scatter<T, true> : radix_scatter<T, false>), dim3(SPAL_SORT_XCD ? per_xcd * 8 : nblk),
                           dim3(kSortThreads), lds, st, ki, ai, vi, b.key[dst], b.aux[dst], b.val[dst], len, shift, pc.raw, pc.gt,
                           pc.dt, nblk, stride, groups, per_xcd, pack ? (uint32_t)pack_bits : 0u);
        cur = dst;
        k_in = nullptr;
    }
    return hipGetLastError();
}

// The groups' offsets after exactly TWO passes, from the passes' own counts (round 4; round 3 read all sorted keys once
// more for them, rows_boundaries: 206 MB and 45 us at config 5).  Group g = d2 << 8 | d1 (d1 = the first pass's digit, d2
// = the second's).  The second pass's input is ordered by d1: bucket d1 begins at B[d1] = the keys with a smaller first
// digit, inside tile t* = B[d1] / tile.  Entries ordered before group g in the result: every entry with a smaller d2, and
// of those with the same d2 the ones in buckets before d1 -- that is what the second pass's counts say about (d2, tiles
// before t*) (PassCounts) plus the entries with digit d2 inside tile t* that lie before B[d1], which workgroup d1 counts
// here (at most one tile of keys).
__global__ __launch_bounds__(256) void group_offsets(const uint32_t *__restrict__ dt1, const uint32_t *__restrict__ raw2,
                                                     const uint32_t *__restrict__ gt2, const uint32_t *__restrict__ dt2,
                                                     const uint32_t *__restrict__ keys1, uint32_t len, uint32_t nblk,
                                                     uint32_t stride, uint32_t groups, uint32_t shift2, uint32_t ngroups,
                                                     uint32_t *__restrict__ gstart) {
    __shared__ uint32_t h[256], s_b;
    const uint32_t d1 = blockIdx.x, t = threadIdx.x;
    h[t] = 0;
    uint32_t total;
    const uint32_t b_mine = block_exclusive_scan(dt1[t], &total);      // B[t]
    if (t == d1) s_b = b_mine;
    const uint32_t my_dt2 = dt2[t];
    const uint32_t base2 = block_exclusive_scan(my_dt2, &total);       // keys with a second digit below t (has barriers: s_b, h are set)
    const uint32_t b = s_b;
    const uint32_t tstar = b / (uint32_t)kSortTile, t0 = tstar * (uint32_t)kSortTile;
    for (uint32_t i = t0 + t; i < b; i += 256) atomicAdd(&h[(keys1[i] >> shift2) & 0xffu], 1u);
    __syncthreads();
    const uint32_t d2 = t, g = d2 << 8 | d1;
    if (g < ngroups) {
        uint32_t v = base2;
        if (tstar < nblk) {
            const uint32_t grp = tstar / (uint32_t)kHistGroup, in_grp = tstar % (uint32_t)kHistGroup;
            v += gt2[(uint64_t)d2 * groups + grp] + h[d2];
            for (uint32_t j = 0; j < in_grp; ++j) v += raw2[(uint64_t)d2 * stride + (uint64_t)grp * kHistGroup + j];
        } else {
            v += my_dt2;   // (the bucket begins at the very end: nothing of it exists, every key with this second digit lies before)
        }
        gstart[g] = v;
    }
    if (d1 == 0 && t == 0) gstart[ngroups] = len;
}

// --------------------------------------------------------------------------
// after the row sort
// --------------------------------------------------------------------------
// Row starts of an array of keys that is sorted by (key >> shift): with shift = 0
// rows, otherwise groups of 2^shift consecutive rows ("row" below = key >> shift).
// start[r] = first sorted entry whose row is >= r   (r in [0, nrows])
__global__ __launch_bounds__(256) void rows_lower_bound(const uint32_t *__restrict__ sorted_row,
                                                        uint32_t n, uint32_t nrows, uint32_t shift,
                                                        uint32_t *__restrict__ start) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)(sorted_row[mid] >> shift) < r) lo = mid + 1; else hi = mid;
    }
    start[r] = lo;
}

// start[r] = first sorted entry whose row is >= r, r in [0, nrows], by ONE
// streaming pass over the sorted keys: entry i with row[i] != row[i-1] is the
// first of its row and of every empty row in between.  (The binary search above
// costs 26 dependent loads per row; this reads every key once.)
__global__ __launch_bounds__(256) void rows_boundaries(const uint32_t *__restrict__ sorted_row,
                                                       uint32_t n, uint32_t nrows, uint32_t shift,
                                                       uint32_t *__restrict__ start) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    // four consecutive entries per thread (one 16-byte load) + the key before them
    const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 > n) return;
    // virtual row -1 before the first entry (0xffffffff + 1 == 0), nrows after the last one
    uint32_t prev = i0 == 0 ? 0xffffffffu : sorted_row[i0 - 1] >> shift;
    uint32_t k[4];
    if (i0 + 4 <= n) {
        const u32x4 q = *reinterpret_cast<const u32x4 *>(sorted_row + i0);
        k[0] = q.x >> shift; k[1] = q.y >> shift; k[2] = q.z >> shift; k[3] = q.w >> shift;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = (i0 + j < n) ? sorted_row[i0 + j] >> shift : nrows;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t i = i0 + j;
        if (i > n) break;
        // rows prev + 1 .. k[j] start at i (empty unless the row changes here)
        for (uint32_t r = prev + 1u; r <= k[j]; ++r) start[r] = (uint32_t)i;
        prev = k[j];
    }
}

void launch_row_starts(const uint32_t *sorted_row, uint32_t n, uint32_t nrows, uint32_t *start,
                       hipStream_t st, uint32_t shift) {
    if ((uint64_t)nrows > 8ull * n + 1024)
        hipLaunchKernelGGL(rows_lower_bound, dim3((uint32_t)(((uint64_t)nrows + 1 + 255) / 256)), dim3(256), 0,
                           st, sorted_row, n, nrows, shift, start);
    else
        hipLaunchKernelGGL(rows_boundaries, dim3((uint32_t)(((uint64_t)n / 4 + 1 + 255) / 256)), dim3(256), 0,
                           st, sorted_row, n, nrows, shift, start);
}

// *fullest = max(*fullest, entries of the fullest group): one atomicMax per workgroup (a few hundred at most -- thousands
// of waves raising one shared maximum would serialise on it)
__global__ __launch_bounds__(256) void groups_check(const uint32_t *__restrict__ gstart, uint32_t ngroups,
                                                    uint32_t *__restrict__ fullest) {
    __shared__ uint32_t s_max[4];
    uint32_t v = 0;
#pragma unroll 4
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (uint64_t)gridDim.x * 256)
        v = max(v, gstart[g + 1] - gstart[g]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(fullest, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
}

template <typename T>
void launch_group_starts(const SortBuffers<T> &b, int cur, bool two_pass, uint64_t len, uint32_t gbits,
                         uint32_t ngroups, uint32_t *gstart, uint32_t *fullest, hipStream_t st) {
    if (two_pass) {
        hipLaunchKernelGGL(group_offsets, dim3(256), dim3(256), 0, st, b.counts.dt, b.counts2.raw, b.counts2.gt, b.counts2.dt,
                           b.key[cur ^ 1], (uint32_t)len, sort_tiles(len), sort_stride(len), sort_groups(len), gbits + 8,
                           ngroups, gstart);
    } else {
        launch_row_starts(b.key[cur], (uint32_t)len, ngroups, gstart, st, gbits);   // (one streaming pass over the sorted keys)
    }
    hipLaunchKernelGGL(groups_check, dim3(std::max<uint32_t>(std::min<uint32_t>((ngroups + 255) / 256, 1024u), 1u)), dim3(256), 0, st,
                       gstart, ngroups, fullest);   // the fullest group (the kernel's capacity is a guess: see coo_group_sort)
}

template hipError_t radix_sort_bits<double>(SortBuffers<double> &, uint64_t, uint32_t, uint32_t, int &, hipStream_t,
                                            const uint32_t *, const uint32_t *, const double *, bool, int);
template hipError_t radix_sort_bits<float>(SortBuffers<float> &, uint64_t, uint32_t, uint32_t, int &, hipStream_t,
                                           const uint32_t *, const uint32_t *, const float *, bool, int);
template void launch_group_starts<double>(const SortBuffers<double> &, int, bool, uint64_t, uint32_t, uint32_t, uint32_t *,
                                          uint32_t *, hipStream_t);
template void launch_group_starts<float>(const SortBuffers<float> &, int, bool, uint64_t, uint32_t, uint32_t, uint32_t *,
                                         uint32_t *, hipStream_t);

}  // namespace spal
