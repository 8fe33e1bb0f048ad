// spal_csr_plan.hip -- the CSR planner: its device kernels (column windows, pages, 16-bit columns) and csr_plan_build,
// which chooses the kernel family and builds its tables.  The sliding kernel's plan is in spal_csr_slide.hip, the row
// split and its race against the block-window kernel in spal_csr_split.hip.
#include "csr_kernels.hpp"
#include "spal_internal.hpp"

namespace spal {

// ---- per-row-block column window ---------------------------------------------
// Columns are strictly increasing inside a row (src/csr.rs:152-156), so a
// row's first and last stored column bound it.  One workgroup per row block:
// out[b] = {min first column, max last column + 1}, {0xffffffff, 0} if the
// block stores nothing.
__global__ __launch_bounds__(256) void csr_block_windows(
    const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows,
    uint32_t R, uint2 *__restrict__ out) {
    __shared__ uint32_t s_min, s_max;
    if (threadIdx.x == 0) {
        s_min = 0xffffffffu;
        s_max = 0u;
    }
    __syncthreads();
    const uint32_t row0 = blockIdx.x * R;
    const uint32_t row1 = min(row0 + R, nrows);
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint32_t r = row0 + threadIdx.x; r < row1; r += 256) {
        const uint32_t a0 = rowptr[r], a1 = rowptr[r + 1];
        if (a0 < a1) {
            lo = min(lo, colind[a0]);
            hi = max(hi, colind[a1 - 1] + 1u);
        }
    }
    atomicMin(&s_min, lo);
    atomicMax(&s_max, hi);
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = make_uint2(s_min, s_max);
}

// ---- plan -------------------------------------------------------------------
// LDS budget for the x window of the vector kernel.  160 KiB per CU; 72 KiB per
// workgroup keeps two workgroups resident, smaller windows admit more.  (72 rather than 64: a band of 8192
// columns under 64 rows of 1500 entries is 66 KiB.)
static constexpr uint32_t kLdsBudgetBytes = 72 * 1024;
// stream kernel: 4 product strips (kStreamTileNnz each, 32 KiB f64) + a window of
// at most 48 KiB -> at most 80 KiB per workgroup, two workgroups per CU (skewed strips, 34 KiB: 44 KiB).
static constexpr uint32_t kStreamWindowBytes = 48 * 1024;
static constexpr uint32_t kStreamWindowBytesSkew = 44 * 1024;
// ... or one workgroup per CU with a window of up to 120 KiB (+ 32 / 34 KiB of strips), for matrices whose
// super-tiles touch more pages than 48 KiB hold: LDS gathers at half the occupancy still beat x through L2
// (band of 8192 columns, f64: 463 / 392 us against 722 us)
static constexpr uint32_t kStreamBigWindowBytes = 120 * 1024;

// One workgroup per super-tile: chk[b] = {skip bits, cost, entries, rows a multiple of 128 bytes long | ulen << 16},
// ulen = 1 + the length of every row of the super-tile when they are all equal (and below 4095), else 0.
//  - skip: a bit per tile that the stream kernels must leave to csr_spmv_overflow -- it holds more entries
//    than the product strip, or a row of more than row_max entries (the stream kernels sum a row per lane:
//    such a row keeps 63 lanes waiting, 25 cycles per entry);
//  - cost: what the super-tile's tiles cost at this tile height, in entries: a streamed tile as much as a
//    half-full one at least (its fixed work: 160 entries per 16-row tile ran 2.1 x slower than 400 per 64-row tile),
//    a skipped tile 1.5 per entry + 1000 (its own workgroup in the overflow kernel).  The planner takes the
//    tile height with the smallest sum (power-law rows, 10 per row on average: 64 / 32 / 16 rows per tile
//    predicted 1 : 1.37 : 2.1, measured 196 : 270 : 380 us).
constexpr uint32_t kTileFloorEntries = 512, kOverflowTileFixed = 1000;
__global__ __launch_bounds__(256) void csr_stream_check(const uint32_t *__restrict__ rowptr,
                                                        uint32_t nrows, uint32_t R, uint32_t rpt,
                                                        uint32_t row_max, uint32_t quantum,
                                                        uint4 *__restrict__ chk) {
    __shared__ uint32_t s_long[32];
    __shared__ uint32_t s_aligned, s_ragged;
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    const uint32_t row0 = b * R, row1 = min(row0 + R, nrows);
    if (t < 32) s_long[t] = 0u;
    if (t == 0) { s_aligned = 0u; s_ragged = 0u; }
    __syncthreads();
    const uint32_t len0 = rowptr[row0 + 1] - rowptr[row0];
    uint32_t aligned = 0;   // rows a non-zero multiple of `quantum` entries (128 bytes) long: see SKEW in csr_kernels.hpp
    for (uint32_t r = row0 + t; r < row1; r += 256) {
        const uint32_t len = rowptr[r + 1] - rowptr[r];
        if (len > row_max) s_long[(r - row0) / rpt] = 1u;   // (same value from every writer)
        if (len != len0) s_ragged = 1u;
        aligned += (len != 0u && len % quantum == 0u) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) aligned += (uint32_t)__shfl_xor((int)aligned, o, 64);
    if ((t & 63u) == 0 && aligned) atomicAdd(&s_aligned, aligned);
    __syncthreads();
    if (t < 64) {   // R / rpt <= 32 tiles
        const uint32_t r0 = row0 + t * rpt;
        bool bad = false;
        uint32_t cost = 0;
        if (t < R / rpt && r0 < row1) {
            const uint32_t rl = min(r0 + rpt, row1);
            const uint32_t e0 = rowptr[r0], e1 = rowptr[rl];
            bad = stream_tile_overflows(e0, e1) || s_long[t] != 0u;
            const uint32_t n = e1 - e0;
            cost = bad ? n + n / 2 + kOverflowTileFixed : max(n, kTileFloorEntries);
        }
        const uint64_t m = __ballot(bad);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cost += (uint32_t)__shfl_xor((int)cost, o, 64);
        if (t == 0) {
            const uint32_t ulen = (s_ragged == 0u && len0 < 4095u) ? len0 + 1u : 0u;
            chk[b] = make_uint4((uint32_t)m, cost, rowptr[row1] - rowptr[row0], s_aligned | (ulen << 16));
        }
    }
}

// Plan time: the first rows of the tiles the descriptors mark (in pieces of at most 64 rows), appended in any order.
__global__ __launch_bounds__(256) void csr_overflow_tiles(const uint4 *__restrict__ desc, uint32_t nrows,
                                                          uint32_t R, uint32_t rpt, uint32_t cap,
                                                          uint32_t *__restrict__ count,
                                                          uint32_t *__restrict__ tiles) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t r0 = i * rpt;
    if (r0 >= nrows) return;
    const uint4 d = desc[r0 / R];
    const uint32_t mode = desc_mode(d);
    if (mode != kModeStream && mode != kModeStreamGlobal) return;
    if (!((desc_skip_bits(d) >> (uint32_t)((r0 % R) / rpt)) & 1u)) return;
    for (uint64_t r = r0; r < min(r0 + rpt, (uint64_t)nrows); r += 64) {   // (csr_spmv_overflow takes up to 64 rows a piece)
        const uint32_t at = atomicAdd(count, 1u);
        if (at < cap) tiles[at] = (uint32_t)r;
    }
}

// ---- the pages a super-tile's rows touch ----------------------------------------------
// One workgroup per super-tile of R rows.  info[b] = {first column, one past the last
// column, number of pages or kNotPageable, 1 if the pages are the contiguous run that
// starts at page (first column >> kPageShift)}.  When the span holds at most `run_cap` pages
// the run is taken whole (a band); otherwise the columns are marked in an LDS bitmap
// (spans up to 16.7M columns), first for a sample of 2048 entries -- scattered columns
// are recognised and dropped there -- then for all of them, and the pages are listed in
// ascending order at pages[b * cap ...].
constexpr uint32_t kNotPageable = 0xffffffffu;
constexpr uint32_t kPageBitmapWords = 2048;   // 65536 pages
__global__ __launch_bounds__(256) void csr_block_pages(
    const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind, uint32_t nrows,
    uint32_t R, uint32_t cap, uint32_t run_cap, const uint2 *__restrict__ known_win,
    uint4 *__restrict__ info, uint32_t *__restrict__ pages) {
    __shared__ uint32_t s_bits[kPageBitmapWords];
    __shared__ uint32_t s_min, s_max, s_count, s_wsum[4];
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    if (t == 0) { s_min = 0xffffffffu; s_max = 0u; s_count = 0u; }
    __syncthreads();
    const uint32_t row0 = b * R, row1 = min(row0 + R, nrows);
    if (known_win) {   // the caller already knows {first column, one past the last} of this super-tile
        if (t == 0) { s_min = known_win[b].x; s_max = known_win[b].y; }
    } else {
        uint32_t lo = 0xffffffffu, hi = 0u;
        for (uint32_t r = row0 + t; r < row1; r += 256) {
            const uint32_t a0 = rowptr[r], a1 = rowptr[r + 1];
            if (a0 < a1) {   // columns ascend inside a row: its first and last entry bound it
                lo = min(lo, colind[a0]);
                hi = max(hi, colind[a1 - 1] + 1u);
            }
        }
        atomicMin(&s_min, lo);
        atomicMax(&s_max, hi);
    }
    __syncthreads();
    const uint32_t cmin = s_min, cmax = s_max;
    if (cmax == 0) {   // nothing stored
        if (t == 0) info[b] = make_uint4(0xffffffffu, 0u, 0u, 1u);
        return;
    }
    const uint32_t pmin = cmin >> kPageShift, span = ((cmax - 1u) >> kPageShift) - pmin + 1u;
    if (span <= run_cap) {   // (run_cap <= cap: the budget that keeps two workgroups per CU)
        if (t == 0) info[b] = make_uint4(cmin, cmax, span, 1u);
        return;
    }
    if (span > kPageBitmapWords * 32u) {
        if (t == 0) info[b] = make_uint4(cmin, cmax, kNotPageable, 0u);
        return;
    }
    const uint32_t words = (span + 31u) / 32u;
    for (uint32_t i = t; i < words; i += 256) s_bits[i] = 0u;
    __syncthreads();
    const uint32_t e0 = rowptr[row0], e1 = rowptr[row1];
    const uint32_t es = min(e0 + 2048u, e1);
    for (int pass = 0; pass < 2; ++pass) {
        const uint32_t a0 = pass ? es : e0, a1 = pass ? e1 : es;
        for (uint32_t e = a0 + t; e < a1; e += 256) {
            const uint32_t pg = (colind[e] >> kPageShift) - pmin;
            atomicOr(&s_bits[pg >> 5], 1u << (pg & 31u));
        }
        __syncthreads();
        uint32_t c = 0;
        for (uint32_t i = t; i < words; i += 256) c += (uint32_t)__popc(s_bits[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
        if ((t & 63u) == 0) s_wsum[t >> 6] = c;
        __syncthreads();
        const uint32_t count = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
        __syncthreads();
        if (count > cap) {   // block-uniform
            if (t == 0) info[b] = make_uint4(cmin, cmax, kNotPageable, 0u);
            return;
        }
        if (pass == 1 && t == 0) s_count = count;
    }
    // ascending page list: thread t owns the words [8t, 8t + 8)
    constexpr uint32_t kPer = kPageBitmapWords / 256;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
        const uint32_t w = t * kPer + q;
        if (w < words) mine += (uint32_t)__popc(s_bits[w]);
    }
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, o, 64);
        if ((t & 63u) >= (uint32_t)o) inc += v;
    }
    if ((t & 63u) == 63u) s_wsum[t >> 6] = inc;
    __syncthreads();
    uint32_t rank = inc - mine;
    for (uint32_t i = 0; i < (t >> 6); ++i) rank += s_wsum[i];
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
        const uint32_t w = t * kPer + q;
        if (w < words) {
            uint32_t bits = s_bits[w];
            while (bits) {
                const uint32_t bit = (uint32_t)__ffs((int)bits) - 1u;
                bits &= bits - 1u;
                pages[(size_t)b * cap + rank++] = pmin + w * 32u + bit;
            }
        }
    }
    if (t == 0) info[b] = make_uint4(cmin, cmax, s_count, s_count == span ? 1u : 0u);   // (every page of the span: a run after all)
}

// Vector plans with long rows: col16 = column - window base for the blocks (R rows) whose x window is in LDS.
__global__ __launch_bounds__(256) void csr_encode_col16_window(const uint32_t *__restrict__ rowptr,
                                                               const uint32_t *__restrict__ colind,
                                                               const uint4 *__restrict__ desc,
                                                               uint16_t *__restrict__ col16, uint32_t nrows,
                                                               uint32_t R) {
    const uint32_t b = blockIdx.x;
    const uint4 d = desc[b];
    if (d.z != kModeVectorLds) return;
    const uint32_t row0 = b * R, row1 = min(row0 + R, nrows);
    const uint32_t e0 = rowptr[row0], e1 = rowptr[row1];
    for (uint32_t e = e0 + threadIdx.x; e < e1; e += 256) col16[e] = (uint16_t)(colind[e] - d.x);
}

// One workgroup per super-tile: col16 = slot of the column's page * kPageCols + column
// inside the page (the slot by binary search in the super-tile's ascending page list).
__global__ __launch_bounds__(256) void csr_encode_col16(const uint32_t *__restrict__ rowptr,
                                                        const uint32_t *__restrict__ colind,
                                                        const uint4 *__restrict__ desc,
                                                        const uint32_t *__restrict__ pages,
                                                        uint16_t *__restrict__ col16,
                                                        uint32_t nrows, uint32_t R, uint32_t ring) {
    __shared__ uint32_t s_pg[64];
    uint4 d = desc[blockIdx.x];   // Stream: {first page / offset, npages | ulen << 8, mode, contiguous}
    if (desc_mode(d) != kModeStream) return;
    d.y &= 0xffu;
    const uint32_t row0 = blockIdx.x * R, row1 = min(row0 + R, nrows);
    const uint32_t p0 = rowptr[row0], p1 = rowptr[row1];
    if (d.w & 1u) {   // contiguous run of pages starting at page d.x
        if (ring) {   // the window is a ring: slot = page % ring (csr_slide.hpp)
            for (uint32_t p = p0 + threadIdx.x; p < p1; p += 256) {
                const uint32_t c = colind[p];
                col16[p] = (uint16_t)((((c >> kPageShift) % ring) << kPageShift) | (c & (kPageCols - 1u)));
            }
            return;
        }
        const uint32_t base = d.x << kPageShift;
        for (uint32_t p = p0 + threadIdx.x; p < p1; p += 256) col16[p] = (uint16_t)(colind[p] - base);
        return;
    }
    if (threadIdx.x < 64) s_pg[threadIdx.x] = threadIdx.x < d.y ? pages[d.x + threadIdx.x] : 0xffffffffu;
    __syncthreads();
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const uint32_t c = colind[p], pg = c >> kPageShift;
        uint32_t lo = 0, hi = d.y;   // the page is in the list: first slot with s_pg[slot] >= pg
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_pg[mid] < pg) lo = mid + 1; else hi = mid;
        }
        col16[p] = (uint16_t)(lo * kPageCols + (c & (kPageCols - 1u)));
    }
}

// Column-panel super-tiles (csr_panel.hpp): col16[p] = column - first column of the super-tile's span (at most 192
// pages = 49 152 columns: 16 bits).  One workgroup per listed super-tile.
__global__ __launch_bounds__(256) void csr_encode_col16_span(const uint32_t *__restrict__ rowptr,
                                                             const uint32_t *__restrict__ colind,
                                                             const uint32_t *__restrict__ ptiles,
                                                             const uint2 *__restrict__ pwin, uint16_t *__restrict__ col16,
                                                             uint32_t nrows, uint32_t R) {
    const uint32_t b = ptiles[blockIdx.x], c0 = pwin[blockIdx.x].x * kPageCols;
    const uint32_t e0 = rowptr[min(b * R, nrows)], e1 = rowptr[min(b * R + R, nrows)];
    for (uint32_t p = e0 + threadIdx.x; p < e1; p += 256) col16[p] = (uint16_t)(colind[p] - c0);
}

static int pick_lanes(double mean_row) {
    int L = 2;
    while (L < 64 && (double)L < mean_row) L <<= 1;
    return L;
}

// per-row-block column windows for block size R -> host vector {cmin, cmax + 1}
// ({0xffffffff, 0} for a block without entries).  The device pass runs once per
// matrix at 256-row granularity; every candidate R that is a multiple of 256 is
// derived from it on the host.

static int block_windows_device(spal_csr *a, uint32_t R, std::vector<uint2> &win) {
    const uint32_t nb = (uint32_t)((a->nrows + R - 1) / R);
    DevBuf d_win;   // (back to the allocator on every path out)
    SPAL_HIP_TRY(d_win.alloc((size_t)nb * sizeof(uint2)));
    hipLaunchKernelGGL(csr_block_windows, dim3(nb), dim3(256), 0, a->stream, a->d_rowptr,
                       a->d_colind, (uint32_t)a->nrows, R, d_win.as<uint2>());
    win.resize(nb);
    SPAL_HIP_TRY(hipMemcpyAsync(win.data(), d_win.p, (size_t)nb * sizeof(uint2), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    return SPAL_OK;
}

static int block_windows(spal_csr *a, uint32_t R, std::vector<uint2> &win) {
    if (R % kWinBase) return block_windows_device(a, R, win);
    if (a->win_base.empty()) SPAL_TRY(block_windows_device(a, kWinBase, a->win_base));
    const uint32_t k = R / kWinBase;
    const uint32_t nb = (uint32_t)((a->nrows + R - 1) / R);
    win.resize(nb);
    for (uint32_t b = 0; b < nb; ++b) {
        uint2 w = make_uint2(0xffffffffu, 0u);
        const size_t j1 = std::min<size_t>((size_t)(b + 1) * k, a->win_base.size());
        for (size_t j = (size_t)b * k; j < j1; ++j) {
            w.x = std::min(w.x, a->win_base[j].x);
            w.y = std::max(w.y, a->win_base[j].y);
        }
        win[b] = w;
    }
    return SPAL_OK;
}

// Stream plan: super-tiles of R rows; returns the fraction of rows
// that can be streamed and fills `desc`.
static int stream_plan(spal_csr *a, uint32_t R, uint32_t rpt, std::vector<uint4> &desc, uint32_t &cap,
                       double &frac, uint32_t **out_pages, uint32_t &n_over, std::vector<uint32_t> &skip,
                       double &cost, bool decide_skew, std::vector<uint2> &panel_win) {
    *out_pages = nullptr;
    n_over = 0;
    const uint32_t nb = (uint32_t)((a->nrows + R - 1) / R);
    // pages of 256 columns that fit the LDS budget: 24 (f64) / 48 (f32)
    // page budgets: `small` keeps two workgroups per CU, `page_cap` (<= 64: page ids travel in a wave's lanes) one
    const uint32_t page_bytes = kPageCols * (uint32_t)a->elem_size;
    const uint32_t page_cap = std::min<uint32_t>(64u, kStreamBigWindowBytes / page_bytes);
    auto small_pages = [&]() {
        return std::min<uint32_t>(page_cap, a->plan.skew ? (a->elem_size == 4 ? 62u : kStreamWindowBytesSkew / page_bytes)
                                                         : (a->elem_size == 4 ? 64u : kStreamWindowBytes / page_bytes));
    };
    uint32_t small_cap = small_pages();
    // temporaries of the plan: returned to the allocator on every path out of this function
    DevBuf b_pages, b_info, b_ok, b_win;
    SPAL_HIP_TRY(b_ok.alloc((size_t)nb * sizeof(uint4)));
    SPAL_HIP_TRY(b_info.alloc((size_t)nb * sizeof(uint4)));
    SPAL_HIP_TRY(b_pages.alloc((size_t)nb * page_cap * 4));
    uint32_t *d_pages = b_pages.as<uint32_t>();
    uint4 *d_info = b_info.as<uint4>(), *d_ok = b_ok.as<uint4>();
    hipLaunchKernelGGL(csr_stream_check, dim3(nb), dim3(256), 0, a->stream, a->d_rowptr, (uint32_t)a->nrows, R,
                       rpt, (uint32_t)a->plan.stream_row_max, 128u / (uint32_t)a->elem_size, d_ok);
    // column windows already known per 256 rows (e.g. handed over by the assembly): fold and pass them
    uint2 *d_win = nullptr;
    if (!a->win_base.empty() && R % kWinBase == 0) {
        std::vector<uint2> win;
        SPAL_TRY(block_windows(a, R, win));
        SPAL_HIP_TRY(b_win.alloc((size_t)nb * sizeof(uint2)));
        d_win = b_win.as<uint2>();
        SPAL_HIP_TRY(hipMemcpyAsync(d_win, win.data(), (size_t)nb * sizeof(uint2), hipMemcpyHostToDevice, a->stream));
        SPAL_HIP_TRY(hipStreamSynchronize(a->stream));   // `win` goes out of scope
    }
    hipLaunchKernelGGL(csr_block_pages, dim3(nb), dim3(256), 0, a->stream, a->d_rowptr, a->d_colind,
                       (uint32_t)a->nrows, R, page_cap,
                       a->plan.window_pages > 0 ? std::min<uint32_t>(page_cap, (uint32_t)a->plan.window_pages) : small_cap,
                       d_win, d_info, d_pages);
    std::vector<uint4> chk(nb);   // {a bit per tile that does not stream, cost of the tiles, entries, -}
    std::vector<uint4> info(nb);
    SPAL_HIP_TRY(hipMemcpyAsync(chk.data(), d_ok, (size_t)nb * sizeof(uint4), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipMemcpyAsync(info.data(), d_info, (size_t)nb * sizeof(uint4), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    (void)dev_free(b_ok.release());
    (void)dev_free(b_info.release());
    (void)dev_free(b_win.release());
    if (decide_skew) {   // skewed product strips when most rows are a multiple of 128 bytes long (16 f64 / 32 f32 entries)
        uint64_t aligned = 0;
        for (uint32_t b = 0; b < nb; ++b) aligned += chk[b].w & 0xffffu;
        a->plan.skew = 2 * aligned > a->nrows ? 1 : 0;
        small_cap = small_pages();   // (the page kernel above ran with the budget of the previous setting: at worst
                                     //  a super-tile of 23 or 24 pages gathers x through L2)
    }
    const uint32_t budget = kStreamWindowBytes / (uint32_t)a->elem_size;
    const uint32_t valign = 16u / (uint32_t)a->elem_size;
    // which page budget?  Rows weighted by what their mode costs per entry, from measurements on bands
    // (f64): LDS window at two workgroups per CU 1.0, at one workgroup per CU 1.35, x through L2 2.3
    uint32_t use_cap = small_cap;
    if (a->plan.window_pages > 0) {
        use_cap = std::min<uint32_t>(page_cap, (uint32_t)a->plan.window_pages);
    } else if (page_cap > small_cap) {
        // per super-tile, in bytes: its entries' stream (10 B each) plus the window's pages (staged through L2,
        // weighted 0.7); the 1.35 and 2.3 are measured on bands.  (A window as large as the entries it serves
        // does not pay: 256-row super-tiles of 10-entry rows spread over 10 000 columns ran 380 us with the
        // large window, 227 us with x through L2.)
        double cost_small = 0, cost_big = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            if (info[b].y == 0) continue;
            const double stream = 10.0 * (double)chk[b].z, gather = 2.3 * stream;
            const double window = 0.7 * (double)page_bytes * (double)info[b].z;
            const bool pageable = info[b].z != kNotPageable;
            cost_small += pageable && info[b].z <= small_cap ? stream + window : gather;
            cost_big += pageable ? 1.35 * (stream + window) : gather;
        }
        if (cost_big < 0.97 * cost_small) use_cap = page_cap;
    }
    desc.assign(nb, make_uint4(0, 0, kModeVectorGlobal, 0));
    panel_win.assign(nb, make_uint2(0u, 0u));
    cap = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint4 w = info[b];   // {first column, one past the last, pages or kNotPageable, contiguous}
        if (w.y == 0) {  // nothing stored: stream mode with one (arbitrary) page writes the zeros
            desc[b] = make_uint4(0, 1, kModeStream, 1);
            cap = std::max(cap, kPageCols);
            continue;
        }
        if (w.z != kNotPageable && w.z <= use_cap) {   // the pages its rows touch fit the LDS budget
            desc[b] = make_uint4(w.w ? (w.x >> kPageShift) : b * page_cap, w.z, kModeStream, w.w);
            cap = std::max(cap, w.z * kPageCols);
            continue;
        }
        if (a->plan.stream_global) {   // columns too scattered for LDS: x through L2 ...
            desc[b] = make_uint4(0, 0, kModeStreamGlobal, 0);
            // ... unless the column SPAN is a few LDS windows wide (a wide band): then the super-tile is taken in
            // column panels by csr_spmv_panel (csr_panel.hpp), desc.w bit 1
            const uint32_t p_first = w.x >> kPageShift, p_span = ((w.y - 1u) >> kPageShift) - p_first + 1u;
            if (a->plan.panel_pages > 0 && rpt <= 64u && a->plan.tiles_per_wave == 4 && !a->plan.skew &&
                p_span <= std::min<uint32_t>((uint32_t)a->plan.panel_pages, 255u)) {   // (span-relative columns are 16-bit: < 65 536)
                desc[b].w |= 2u;
                panel_win[b] = make_uint2(p_first, p_span);
            }
            continue;
        }
        // (stream_global switched off) vector rows, x window in LDS when the span fits
        const uint32_t cb = w.x & ~(valign - 1);
        const uint32_t len = w.y - cb;
        if (len <= budget) {
            desc[b] = make_uint4(cb, len, kModeVectorLds, 0);
            cap = std::max(cap, len);
        }
    }
    // super-tiles whose rows all have the same length: the kernels derive the row bounds and do not read rowptr
    if (a->plan.uniform_rows)
        for (uint32_t b = 0; b < nb; ++b)
            if (desc[b].z == kModeStream || desc[b].z == kModeStreamGlobal) desc[b].y |= (chk[b].w >> 16) << 8;
    // what the caller ranks tile heights by: the share of rows whose TILE streams (the marked tiles of a
    // super-tile in a stream mode are left to csr_spmv_overflow)
    {
        uint64_t rows_tiles = 0;
        skip.assign(nb, 0u);
        cost = 0.0;
        for (uint32_t b = 0; b < nb; ++b) {
            if (desc[b].z != kModeStream && desc[b].z != kModeStreamGlobal) {
                cost += 2.0 * (double)chk[b].z;   // (vector rows inside the stream kernel)
                continue;
            }
            skip[b] = chk[b].x;
            cost += (double)chk[b].y;
            const uint64_t rows = std::min<uint64_t>(R, a->nrows - (uint64_t)b * R);
            const uint32_t over = (uint32_t)__builtin_popcount(skip[b]);
            rows_tiles += rows - std::min<uint64_t>(rows, (uint64_t)over * rpt);
            n_over += over;
        }
        frac = a->nrows ? (double)rows_tiles / (double)a->nrows : 0.0;
    }
    *out_pages = (uint32_t *)b_pages.release();
    return SPAL_OK;
}

// Chooses the kernel and its parameters and builds the per-block tables.
// the assembly's per-group column spans -> win_base (per 256 rows), once
static int csr_fetch_group_windows(spal_csr *a) {
    if (!a->d_win_groups) return SPAL_OK;
    std::vector<uint2> g(a->win_groups);
    hipError_t e = hipMemcpy(g.data(), a->d_win_groups, (size_t)a->win_groups * sizeof(uint2), hipMemcpyDeviceToHost);
    (void)dev_free(a->d_win_groups);
    a->d_win_groups = nullptr;
    SPAL_HIP_TRY(e);
    const uint32_t per = 256u >> a->win_group_bits;
    a->win_base.assign(((size_t)a->nrows + 255) / 256, make_uint2(0xffffffffu, 0u));
    for (uint32_t i = 0; i < a->win_groups; ++i) {
        uint2 &w = a->win_base[i / per];
        w.x = std::min(w.x, g[i].x);
        w.y = std::max(w.y, g[i].y);
    }
    return SPAL_OK;
}

int csr_plan_build(spal_csr *a) {
    SPAL_TRY(csr_fetch_group_windows(a));
    blockwin_free(a);
    a->bw_us[0] = a->bw_us[1] = 0.f;
    if (a->plan.blockwin == 1 && !a->split_child) {   // asked for by name (tests): whenever the windows fit
        if (a->split_short) { csr_free(a->split_short); a->split_short = nullptr; }
        (void)dev_free(a->d_split_rows); a->d_split_rows = nullptr;
        a->split_nlong = 0;
        if (blockwin_plan(a) != SPAL_OK) { blockwin_free(a); (void)hipGetLastError(); }   // (an optional form: without it the plan below)
        if (a->bw_rows) { a->bw_on = 1; a->plan.kernel = 4; return SPAL_OK; }
    }
    {
        bool did = false;
        SPAL_TRY(csr_try_row_split(a, &did));
        if (did) {   // ("split": the products run through the short part's handle -- unless the block-window kernel beats it)
            a->plan.kernel = 3;
            if (a->plan.blockwin != 0) SPAL_TRY(csr_blockwin_or_split(a));
            return SPAL_OK;
        }
    }
    CsrPlan &p = a->plan;
    const double mean = a->nrows ? (double)a->nnz / (double)a->nrows : 0.0;
    // vector kernel geometry, from measurements (tools/lab.py ab): one lane per entry
    // up to 64 entries per row; longer rows loop in batches of 4 L entries per
    // lane group, which 16 lanes per row keep busiest (128/row: 65 %, L = 64: 38 %)
    // rows longer than a wave (tools/lab.py longrows, 70 ... 1500 entries per row): a whole wave per row,
    // one row group in flight, and few rows per workgroup (below) beat 16 lanes per row everywhere
    // (100/row 56 % against 37 %, 400/row 67 % against 17 %, 1500/row 54 % against 23 %)
    if (!p.user_lanes) p.lanes_per_row = mean > 85.0 ? 64 : mean > 64.0 ? 32 : pick_lanes(mean);
    p.long_rows = mean > 64.0 ? 1 : 0;   // (only the 16-lane instantiation has the batched rest-of-row loop)
    if (!p.user_unroll) p.unroll = mean > 64.0 ? 1 : 4;
    if (!p.user_threads) p.threads = 1024;
    if (a->d_desc) {
        SPAL_HIP_TRY(dev_free(a->d_desc));
        a->d_desc = nullptr;
    }
    p.stream_row_fraction = 0.0;
    p.vec_col16 = 0;
    p.slide = 0;
    p.rowrec = 0;
    p.valpack = 0;
    p.ring_pages = 0;
    if (a->nnz == 0) {
        cblock_free(a);
        p.kernel = 1;
        p.rows_per_block = 1024;
        p.nblocks = (uint32_t)((a->nrows + 1023) / 1024);
        p.lds_x = 0;
        return SPAL_OK;
    }
    const uint32_t valign = 16u / (uint32_t)a->elem_size;

    // ---- stream kernel: rows short enough that 64 / 32 / 24 / 16 / 12 / 8 of them fit a tile (auto: at least half
    // the rows in tiles that stream; fuller strips pay: 33/row 24 rows per tile 100 us vs 16 rows 109 us, 70/row
    // 12 rows 143 us vs 8 rows 159 us, 81/row 155 vs 187 us).  Measured against the vector kernel on bands (tools/lab.py rpt8): 54/row 82 % vs
    // 51 %, 63/row 84 % vs 47 %, 64/row 80 % (skewed strips) vs 50 %, 81/row 67 % vs 46 %, 100/row 71 % vs 54 %,
    // 120/row 68 % vs 56 %; 4-row tiles for 150 ... 250/row were level with or behind the vector kernel.
    if ((p.user_kernel == 0 && mean <= 120.0) || p.user_kernel == 2) {
        if (p.tiles_per_wave != 4 && p.tiles_per_wave != 8) p.tiles_per_wave = 4;
        const int rpt_all[] = {256, 128, 64, 32, 24, 16, 12, 8};   // (48 rows per tile measured behind 32: 20/row 124 vs 111 us)
        std::vector<int> rpts;
        if (p.user_rows_per_tile) rpts.push_back(p.rows_per_tile);
        else if (p.tiles_per_wave == 8) rpts.push_back(64);
        else rpts.assign(rpt_all + (mean <= 4.0 ? 0 : mean <= 8.0 ? 1 : 2), rpt_all + 8);   // (256 / 128 rows of more than 4 / 8 entries do not fit a tile)
        std::vector<uint4> desc, best_desc;
        uint32_t cap = 0, best_cap = 0;
        double frac = 0.0, best_frac = -1.0, best_cost = -1.0;
        int best_rpt = rpts[0];
        uint32_t *best_pages = nullptr;
        uint32_t n_over = 0, best_over = 0;
        std::vector<uint32_t> skip, best_skip;
        std::vector<uint2> pwin, best_pwin;
        if (a->d_pages) { SPAL_HIP_TRY(dev_free(a->d_pages)); a->d_pages = nullptr; }
        if (a->d_ovtiles) { SPAL_HIP_TRY(dev_free(a->d_ovtiles)); a->d_ovtiles = nullptr; }
        a->n_ovtiles = 0;
        for (int rpt : rpts) {
            const uint32_t R = (uint32_t)stream_rows(rpt > 128 ? 1 : rpt > 64 ? 2 : p.tiles_per_wave, rpt);   // (128 / 256-row tiles: two / one per wave, the same 1024 rows)
            uint32_t *pg = nullptr;
            double cost = 0.0;
            int st = stream_plan(a, R, (uint32_t)rpt, desc, cap, frac, &pg, n_over, skip, cost, !p.user_skew && rpt == rpts[0], pwin);
            if (st != SPAL_OK) { (void)dev_free(best_pages); return st; }
            if (best_cost < 0.0 || cost < 0.95 * best_cost) {  // a narrower tile must be estimated cheaper (see csr_stream_check)
                best_cost = cost;
                best_frac = frac; best_rpt = rpt; best_cap = cap; best_over = n_over; best_desc.swap(desc); best_skip.swap(skip);
                best_pwin.swap(pwin);
                (void)dev_free(best_pages);
                best_pages = pg;
            } else {
                (void)dev_free(pg);
            }
            if (best_cost <= 1.1 * (double)a->nnz) break;   // no tile height costs less than one per entry
        }
        if (!(p.user_kernel == 2 || best_frac >= 0.5)) (void)dev_free(best_pages);
        if (p.user_kernel == 2 || best_frac >= 0.5) {
            a->d_pages = best_pages;
            const uint32_t R = (uint32_t)stream_rows(best_rpt > 128 ? 1 : best_rpt > 64 ? 2 : p.tiles_per_wave, best_rpt);
            p.kernel = 2;
            p.rows_per_tile = best_rpt;
            p.rows_per_block = (int)R;
            p.threads = kStreamBlock;
            p.nblocks = (uint32_t)best_desc.size();
            p.lds_x = best_cap > 0;
            p.lds_entries = (std::max(best_cap, valign) + valign - 1) & ~(valign - 1);
            // one workgroup per CU (the large page budget): nothing else on the CU hides a workgroup's
            // cold start, the persistent form does (band of 8192 columns: 400 vs 460 us)
            if (!p.user_persistent)
                p.persistent = ((size_t)kStreamWaves * (p.skew ? stream_strip<true>() : stream_strip<false>()) + p.lds_entries) * a->elem_size > 80u * 1024u ? 1 : 0;
            p.stream_row_fraction = best_frac;
            uint64_t lds_rows = 0;
            for (uint32_t b = 0; b < p.nblocks; ++b)
                if (best_desc[b].z == kModeVectorLds || best_desc[b].z == kModeStream)
                    lds_rows += std::min<uint64_t>(R, a->nrows - (uint64_t)b * R);
            p.lds_row_fraction = (double)lds_rows / (double)a->nrows;
            uint64_t uni_rows = 0;
            for (uint32_t b = 0; b < p.nblocks; ++b)
                if ((best_desc[b].z == kModeStream || best_desc[b].z == kModeStreamGlobal) && (best_desc[b].y >> 8))
                    uni_rows += std::min<uint64_t>(R, a->nrows - (uint64_t)b * R);
            p.uniform_row_fraction = (double)uni_rows / (double)a->nrows;
            SPAL_HIP_TRY(dev_alloc((void **)&a->d_desc, (size_t)p.nblocks * sizeof(uint4)));
            std::vector<uint4> packed(best_desc);   // + the tiles to skip (see desc_skip_bits)
            for (uint32_t b = 0; b < p.nblocks; ++b) {
                packed[b].w |= (best_skip[b] & 0xffffu) << 16;
                packed[b].z |= best_skip[b] & 0xffff0000u;
            }
            SPAL_HIP_TRY(hipMemcpyAsync(a->d_desc, packed.data(), (size_t)p.nblocks * sizeof(uint4),
                                        hipMemcpyHostToDevice, a->stream));
            SPAL_HIP_TRY(hipStreamSynchronize(a->stream));   // `packed` goes out of scope
            // wide bands: the super-tiles csr_spmv_panel takes in column panels
            {
                if (a->d_ptiles) { SPAL_HIP_TRY(dev_free(a->d_ptiles)); a->d_ptiles = nullptr; }
                if (a->d_pwin) { SPAL_HIP_TRY(dev_free(a->d_pwin)); a->d_pwin = nullptr; }
                std::vector<uint32_t> ids;
                std::vector<uint2> wins;
                for (uint32_t b = 0; b < p.nblocks; ++b)
                    if (best_desc[b].z == kModeStreamGlobal && (best_desc[b].w & 2u)) { ids.push_back(b); wins.push_back(best_pwin[b]); }
                a->n_ptiles = (uint32_t)ids.size();
                if (a->n_ptiles) {
                    SPAL_HIP_TRY(dev_alloc((void **)&a->d_ptiles, ids.size() * sizeof(uint32_t)));
                    SPAL_HIP_TRY(dev_alloc((void **)&a->d_pwin, wins.size() * sizeof(uint2)));
                    SPAL_HIP_TRY(hipMemcpyAsync(a->d_ptiles, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
                    SPAL_HIP_TRY(hipMemcpyAsync(a->d_pwin, wins.data(), wins.size() * sizeof(uint2), hipMemcpyHostToDevice, a->stream));
                    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
                    // LDS: the panel window beside the strips (the one-super-tile kernels of this plan need none for these)
                    // a panel: 80 KB of LDS (two workgroups per CU), shared with the product strips; option
                    // "panel_window" sets it in pages (up to 156 KB: one workgroup per CU, fewer passes over the entries)
                    const uint32_t page_b = kPageCols * (uint32_t)a->elem_size;
                    uint32_t pp = (80u * 1024u) / page_b;
                    if (p.panel_window_user > 0) pp = std::min<uint32_t>((uint32_t)p.panel_window_user, (156u * 1024u) / page_b);
                    p.panel_window_pages = (int)pp;
                }
            }
            // bands and the like: the sliding-window kernel (csr_slide.hpp) and its ring-addressed window
            SPAL_TRY(slide_plan(a, (uint32_t)best_rpt, best_desc, best_skip, best_cap / kPageCols));
            if (p.ring_pages) p.lds_entries = (uint32_t)p.ring_pages * kPageCols;
            // 16-bit columns only where some super-tile reads them (a matrix whose columns are scattered
            // everywhere streams with the 32-bit ones: no 2 B/entry array to allocate and clear)
            bool any_stream = false;
            for (uint32_t b = 0; b < p.nblocks && !any_stream; ++b) any_stream = best_desc[b].z == kModeStream;
            if (any_stream || a->n_ptiles) {
                if (!a->d_col16) {
                    SPAL_HIP_TRY(dev_alloc((void **)&a->d_col16, (size_t)a->cap_entries * sizeof(uint16_t)));
                    SPAL_HIP_TRY(hipMemsetAsync(a->d_col16, 0, (size_t)a->cap_entries * sizeof(uint16_t), a->stream));
                }
                if (any_stream)
                    hipLaunchKernelGGL(csr_encode_col16, dim3(p.nblocks), dim3(256), 0, a->stream, a->d_rowptr,
                                       a->d_colind, a->d_desc, a->d_pages, a->d_col16, (uint32_t)a->nrows, R,
                                       (uint32_t)p.ring_pages);
                if (a->n_ptiles)   // the column-panel kernel's super-tiles: columns relative to the span's first column
                    hipLaunchKernelGGL(csr_encode_col16_span, dim3(a->n_ptiles), dim3(256), 0, a->stream, a->d_rowptr,
                                       a->d_colind, a->d_ptiles, a->d_pwin, a->d_col16, (uint32_t)a->nrows, R);
                SPAL_HIP_TRY(hipGetLastError());
            }
            // uniform short rows under the sliding kernel: one record per row instead of its col16 (csr_rowrec.hpp)
            SPAL_TRY(rowrec_plan(a));
            // ... and f64 values that share a quantum: one fixed-point block per row instead of its values (csr_valpack.hpp)
            SPAL_TRY(valpack_plan(a));
            if (best_over) {   // the tiles the stream kernels skip: listed for csr_spmv_overflow
                uint32_t *d_list = nullptr;   // [count][first rows]
                const uint32_t pieces = (uint32_t)std::max(1, best_rpt / 64) * best_over;   // (at most)
                SPAL_HIP_TRY(dev_alloc((void **)&d_list, ((size_t)pieces + 1) * 4));
                a->d_ovtiles = d_list;
                SPAL_HIP_TRY(hipMemsetAsync(d_list, 0, 4, a->stream));
                const uint64_t ntile = (a->nrows + (uint64_t)best_rpt - 1) / (uint64_t)best_rpt;
                hipLaunchKernelGGL(csr_overflow_tiles, dim3((uint32_t)((ntile + 255) / 256)), dim3(256), 0, a->stream,
                                   a->d_desc, (uint32_t)a->nrows, R, (uint32_t)best_rpt, pieces, d_list,
                                   d_list + 1);
                SPAL_HIP_TRY(hipGetLastError());
                uint32_t listed = 0;
                SPAL_HIP_TRY(hipMemcpyAsync(&listed, d_list, 4, hipMemcpyDeviceToHost, a->stream));
                SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
                if (listed > pieces || listed < best_over)   // (cannot happen: both count the same tiles)
                    return fail(SPAL_ERR_HIP, "csr plan: %u tiles listed for the overflow kernel, %u counted", listed, best_over);
                a->n_ovtiles = listed;
            }
            SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
            // columns anywhere (most rows sit in super-tiles that gather x from global memory over a span no panel
            // holds): the column-blocked kernel and its tiled copy of the matrix (csr_cblock.hpp)
            {
                uint64_t far_rows = 0;
                for (uint32_t b = 0; b < p.nblocks; ++b)
                    if (best_desc[b].z == kModeStreamGlobal && !(best_desc[b].w & 2u))
                        far_rows += std::min<uint64_t>(R, a->nrows - (uint64_t)b * R);
                p.nonlocal_row_fraction = (double)far_rows / (double)a->nrows;
                p.cblock_pending = 0;
                if (getenv("SPAL_CBLOCK_DEBUG"))
                    fprintf(stderr, "[spal cblock] plan: nonlocal rows %.3f, user %d, lazy %d\n", p.nonlocal_row_fraction, p.cblock_user, a->cblock_lazy);
                if (p.cblock_user == 1 || (p.cblock_user < 0 && p.nonlocal_row_fraction >= 0.5)) {
                    if (a->cblock_lazy && p.cblock_user < 0) { cblock_free(a); p.cblock_pending = 1; }   // built by the first product
                    else (void)cblock_plan(a, p.cblock_user == 1);   // (a failure: the stream kernels run, `cblock_failed`)
                } else {
                    cblock_free(a);
                }
            }
            return SPAL_OK;
        }
    }
    cblock_free(a);
    rowrec_free(a);
    valpack_free(a);

    // ---- vector kernel
    p.kernel = 1;
    if (p.threads != 512 && p.threads != 1024) p.threads = 1024;
    const uint32_t budget = kLdsBudgetBytes / (uint32_t)a->elem_size;  // elements
    const uint32_t cand_all[] = {4096, 2048, 1024, 512};
    std::vector<uint32_t> cands;
    if (p.user_rows_per_block) {
        cands.push_back((uint32_t)p.rows_per_block);
    } else if (mean > 64.0) {
        // long rows: about 100 000 entries per workgroup (1024 rows at 100/row ... 64 rows at 1500/row), so
        // that there are workgroups enough for 256 CUs -- 4096 rows of 400 entries were 61 workgroups
        uint32_t r0 = 1024;
        while (r0 > 64 && (double)r0 * mean > 131072.0) r0 >>= 1;
        // ... and a number of workgroups that fills whole rounds of the 512 the device holds at once (two of 1024
        // threads per CU): these launches are two or three rounds long, and 1250 workgroups (2.44 rounds) ran at
        // 60 ... 67 % where 980 (1.9 rounds) ran at 73 ... 78 % (tools/lab.py longrows threads).  R need not be
        // a power of two.
        if (p.threads == 1024) {
            const double want = std::max(1.0, (double)a->nnz / 100000.0);              // workgroups of ~100 000 entries
            const uint64_t rounds = std::max<uint64_t>(1, (uint64_t)(want / 512.0 + 0.5));
            // (98 % of the slots, rounded down by taking R up to a multiple of 16: a launch planned to the last slot
            // spills into one more round -- 200 entries per row: 947 ... 977 workgroups 213 ... 218 us, 1009 of them
            // 232 ... 240 us -- and an R that gives some waves one row more than others costs as much: 1500 per
            // row, R = 64: 162 ... 168 us, R = 68 or 72: 174 us)
            const uint64_t nb = rounds * 502;
            uint64_t R = (a->nrows + nb - 1) / nb;
            R = std::min<uint64_t>(4096, std::max<uint64_t>(16, (R + 15) / 16 * 16));   // 16 waves, the same number of rows each
            cands.push_back((uint32_t)R);
        }
        cands.push_back(r0);
        if (r0 > 64) cands.push_back(r0 >> 1);
    } else {
        cands.assign(cand_all, cand_all + 4);
    }

    std::vector<uint4> best_desc;
    uint32_t best_R = 0, best_cap = 0;
    double best_frac = -1.0;
    const bool want_lds = p.user_lds ? p.lds_x != 0 : true;
    for (uint32_t R : cands) {
        std::vector<uint2> win;
        SPAL_TRY(block_windows(a, R, win));
        const uint32_t nb = (uint32_t)win.size();
        std::vector<uint4> desc(nb, make_uint4(0, 0, kModeVectorGlobal, 0));
        uint64_t fit_rows = 0;
        uint32_t cap = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            const uint2 w = win[b];
            const uint64_t rows = std::min<uint64_t>(R, a->nrows - (uint64_t)b * R);
            if (w.y == 0) {  // block stores nothing: no window needed
                fit_rows += rows;
                continue;
            }
            const uint32_t cb = w.x & ~(valign - 1);
            const uint32_t len = w.y - cb;
            if (want_lds && len <= budget) {
                desc[b] = make_uint4(cb, len, kModeVectorLds, 0);
                cap = std::max(cap, len);
                fit_rows += rows;
            }
        }
        const double frac = (double)fit_rows / (double)a->nrows;
        // prefer the largest R whose blocks (nearly) all fit; otherwise the best coverage
        const bool good = frac >= 0.9;
        if (best_R == 0 || (good && best_frac < 0.9) || (!good && best_frac < 0.9 && frac > best_frac)) {
            best_R = R; best_frac = frac; best_cap = cap; best_desc.swap(desc);
        }
        if (good) break;
    }
    p.rows_per_block = (int)best_R;
    p.nblocks = (uint32_t)((a->nrows + best_R - 1) / best_R);
    p.lds_row_fraction = best_frac;
    // LDS only pays when most rows can use it; otherwise run without the
    // allocation so more workgroups fit per CU.
    const bool use_lds = want_lds && best_cap > 0 && (p.user_lds || best_frac >= 0.5);
    p.lds_x = use_lds ? 1 : 0;
    p.lds_entries = use_lds ? ((best_cap + valign - 1) & ~(valign - 1)) : 0;
    if (!use_lds)
        for (auto &d : best_desc) d = make_uint4(0, 0, kModeVectorGlobal, 0);
    SPAL_HIP_TRY(dev_alloc((void **)&a->d_desc, (size_t)p.nblocks * sizeof(uint4)));
    SPAL_HIP_TRY(hipMemcpy(a->d_desc, best_desc.data(), (size_t)p.nblocks * sizeof(uint4),
                           hipMemcpyHostToDevice));
    // long rows with LDS windows (at most 64 KiB: 16 bits address them): 2-byte columns for those blocks
    p.vec_col16 = (p.vec_col16_allowed && use_lds && p.long_rows && p.unroll == 1 &&
                   (p.lanes_per_row == 64 || p.lanes_per_row == 32) && best_cap <= 65536u) ? 1 : 0;
    if (p.vec_col16) {
        if (!a->d_col16) {
            SPAL_HIP_TRY(dev_alloc((void **)&a->d_col16, (size_t)a->cap_entries * sizeof(uint16_t)));
            SPAL_HIP_TRY(hipMemsetAsync(a->d_col16, 0, (size_t)a->cap_entries * sizeof(uint16_t), a->stream));
        }
        hipLaunchKernelGGL(csr_encode_col16_window, dim3(p.nblocks), dim3(256), 0, a->stream, a->d_rowptr,
                           a->d_colind, a->d_desc, a->d_col16, (uint32_t)a->nrows, best_R);
        SPAL_HIP_TRY(hipGetLastError());
        SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    }
    return SPAL_OK;
}

}  // namespace spal
