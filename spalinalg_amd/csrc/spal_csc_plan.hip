// spal_csc_plan.hip -- the plan of the column-tiled CSC scatter kernel (spal_csc_scatter.hip): per super-tile of columns
// its row window and mode, packed metadata for the LDS mode, cover lists for the two-phase flush, and whether the
// launch may hand rows from neighbour to neighbour instead of using atomics.
#include "csr_kernels.hpp"
#include "spal_internal.hpp"

namespace spal {

// ---- plan-time kernels ---------------------------------------------------------
// (rowind is strictly increasing inside a column, src/csc.rs:152-156: the first
// and last entry of a column bound its rows)
__global__ __launch_bounds__(256) void csc_block_windows(const uint32_t *__restrict__ colptr,
                                                         const uint32_t *__restrict__ rowind,
                                                         uint32_t ncols, uint32_t cols, uint2 *__restrict__ out) {
    __shared__ uint32_t s_min, s_max;
    if (threadIdx.x == 0) { s_min = 0xffffffffu; s_max = 0u; }
    __syncthreads();
    const uint32_t k0 = blockIdx.x * cols, k1 = min(k0 + cols, ncols);
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += 256) {
        const uint32_t a0 = colptr[k], a1 = colptr[k + 1];
        if (a0 < a1) {
            lo = min(lo, rowind[a0]);
            hi = max(hi, rowind[a1 - 1] + 1u);
        }
    }
    atomicMin(&s_min, lo);
    atomicMax(&s_max, hi);
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = make_uint2(s_min, s_max);
}

// *differs |= 1 when some column does not hold exactly `len` entries
__global__ __launch_bounds__(256) void csc_uniform_check(const uint32_t *__restrict__ colptr, uint32_t ncols, uint32_t len,
                                                         uint32_t *__restrict__ differs) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = k < ncols && colptr[k + 1] - colptr[k] != len;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(differs, 1u);
}

// meta[p] = (row - rbase) | (col - k0) << 16 for LDS-mode super-tiles
__global__ __launch_bounds__(256) void csc_encode_meta(const uint32_t *__restrict__ colptr,
                                                       const uint32_t *__restrict__ rowind,
                                                       const uint4 *__restrict__ desc,
                                                       uint32_t *__restrict__ meta, uint32_t ncols, uint32_t cols) {
    const uint4 d = desc[blockIdx.x];
    if (d.z != kCscModeLds) return;
    const uint32_t k0 = blockIdx.x * cols, k1 = min(k0 + cols, ncols);
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += 256)
        for (uint32_t p = colptr[k]; p < colptr[k + 1]; ++p)
            meta[p] = (rowind[p] - d.x) | ((k - k0) << 16);
}

// what the steps of csc_plan_build pass on
struct CscTiling {
    std::vector<uint4> desc;            // per super-tile {window base row, length, mode, offset of its window in d_windows}
    std::vector<uint32_t> cover_ptr;    // cover lists: chunk of kCscChunk rows -> LDS-mode super-tiles whose window overlaps it, ascending
    std::vector<uint32_t> cover;
    uint64_t slots = 0;                 // elements of d_windows
};

static int plan_reset(spal_csc *a) {
    for (void **p : {(void **)&a->d_desc, &a->d_windows, (void **)&a->d_chunk_ptr, (void **)&a->d_chunk_blk,
                     (void **)&a->d_prev_hi, (void **)&a->d_flags}) {
        SPAL_HIP_TRY(dev_free(*p));   // (nullptr is fine)
        *p = nullptr;
    }
    a->ordered = 0;
    a->epoch = 0;
    a->ticket_next = 0;
    a->ticket_auto = 0;
    a->spin_bound = 1u << 22;
    if (const char *e = getenv("SPAL_CSC_HANDOFF_SPINS")) a->spin_bound = (uint32_t)strtoul(e, nullptr, 10);   // (tests: 0 forces the backstop)
    a->windows_entries = 0;
    a->all_lds = 0;
    a->nchunks = 0;
    a->lds_entries = 0;
    a->lds_col_fraction = 0.0;
    a->cols_per_block = a->user_cols ? a->user_cols : 1024;
    a->nblocks = (uint32_t)((a->ncols + a->cols_per_block - 1) / a->cols_per_block);
    a->uniform_cols = 0;
    return SPAL_OK;
}

// every column the same length?  (then the kernel computes the column pointers)
static int plan_uniform_columns(spal_csc *a) {
    if (!a->nnz || a->nnz % a->ncols) return SPAL_OK;
    const uint32_t len = (uint32_t)(a->nnz / a->ncols);
    DevBuf differs;
    uint32_t f = 1;
    SPAL_HIP_TRY(differs.alloc(4));
    SPAL_HIP_TRY(hipMemsetAsync(differs.p, 0, 4, a->stream));
    hipLaunchKernelGGL(csc_uniform_check, dim3((uint32_t)((a->ncols + 255) / 256)), dim3(256), 0, a->stream,
                       a->d_colptr, (uint32_t)a->ncols, len, differs.as<uint32_t>());
    SPAL_HIP_TRY(hipMemcpyAsync(&f, differs.p, 4, hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    if (!f) a->uniform_cols = len + 1;
    return SPAL_OK;
}

// row windows per 1024 columns (one device pass); wider super-tiles are unions of those
static int plan_measure_windows(spal_csc *a, std::vector<uint2> &win1) {
    const uint32_t nb1 = (uint32_t)((a->ncols + 1023) / 1024);
    DevBuf d_win;
    SPAL_HIP_TRY(d_win.alloc((size_t)nb1 * sizeof(uint2)));
    hipLaunchKernelGGL(csc_block_windows, dim3(nb1), dim3(256), 0, a->stream, a->d_colptr,
                       a->d_rowind, (uint32_t)a->ncols, 1024u, d_win.as<uint2>());
    win1.resize(nb1);
    SPAL_HIP_TRY(hipMemcpyAsync(win1.data(), d_win.p, (size_t)nb1 * sizeof(uint2), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    return SPAL_OK;
}

// the windows of super-tiles of `cols` columns; returns the columns whose super-tile's window fits LDS
static uint64_t windows_for(const spal_csc *a, const std::vector<uint2> &win1, int cols, std::vector<uint2> &win) {
    const uint32_t nb1 = (uint32_t)win1.size();
    const uint32_t k = (uint32_t)cols / 1024u, nb = (uint32_t)((a->ncols + cols - 1) / cols);
    const uint32_t budget = csc_window_budget(a, cols);
    win.assign(nb, make_uint2(0xffffffffu, 0u));
    uint64_t fit_cols = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        for (uint32_t j = b * k; j < std::min(nb1, (b + 1) * k); ++j)
            if (win1[j].y) { win[b].x = std::min(win[b].x, win1[j].x); win[b].y = std::max(win[b].y, win1[j].y); }
        if (win[b].y == 0 || win[b].y - win[b].x <= budget)
            fit_cols += std::min<uint64_t>((uint64_t)cols, a->ncols - (uint64_t)b * cols);
    }
    return fit_cols;
}

// the widest super-tile whose windows fit as well as the 1024-column ones do (or the caller's width)
static void plan_choose_width(spal_csc *a, const std::vector<uint2> &win1, std::vector<uint2> &win) {
    const uint64_t fit1024 = windows_for(a, win1, 1024, win);
    if (a->user_cols) {
        (void)windows_for(a, win1, a->cols_per_block, win);
    } else {
        for (int cols : {4096, 2048}) {
            std::vector<uint2> w;
            if (windows_for(a, win1, cols, w) >= fit1024) { a->cols_per_block = cols; win.swap(w); break; }
        }
    }
    a->nblocks = (uint32_t)((a->ncols + a->cols_per_block - 1) / a->cols_per_block);
}

// descriptors (LDS mode where the window fits), slots of the two-phase flush's windows, cover lists
static void plan_tiles(spal_csc *a, const std::vector<uint2> &win, CscTiling &t) {
    t.desc.assign(a->nblocks, make_uint4(0, 0, kCscModeGlobal, 0));
    const uint32_t cols = (uint32_t)a->cols_per_block, budget = csc_window_budget(a, a->cols_per_block);
    uint64_t cols_lds = 0;
    bool all_lds = true;
    a->nchunks = (uint32_t)((a->nrows + kCscChunk - 1) / kCscChunk);
    t.cover_ptr.assign(a->nchunks + 1, 0);
    for (uint32_t b = 0; b < a->nblocks; ++b) {
        const uint2 w = win[b];
        if (w.y == 0) continue;  // no entries: the global path finds nothing to do
        const uint32_t len = w.y - w.x;
        if (len <= budget && t.slots + len < 0xffffffffull) {
            t.desc[b] = make_uint4(w.x, len, kCscModeLds, (uint32_t)t.slots);
            t.slots += (len + 1) & ~1ull;   // slots start on even elements
            a->lds_entries = std::max(a->lds_entries, len);
            cols_lds += std::min<uint64_t>(cols, a->ncols - (uint64_t)b * cols);
            for (uint32_t c = w.x / kCscChunk; c <= (w.y - 1) / kCscChunk; ++c) ++t.cover_ptr[c + 1];
        } else {
            all_lds = false;
        }
    }
    a->lds_col_fraction = (double)cols_lds / (double)a->ncols;
    a->all_lds = all_lds ? 1 : 0;
    for (uint32_t c = 0; c < a->nchunks; ++c) t.cover_ptr[c + 1] += t.cover_ptr[c];
    t.cover.resize(t.cover_ptr[a->nchunks]);
    std::vector<uint32_t> fill(t.cover_ptr.begin(), t.cover_ptr.end() - 1);
    for (uint32_t b = 0; b < a->nblocks; ++b) {
        if (t.desc[b].z != kCscModeLds) continue;
        for (uint32_t c = t.desc[b].x / kCscChunk; c <= (t.desc[b].x + t.desc[b].y - 1) / kCscChunk; ++c)
            t.cover[fill[c]++] = b;
    }
}

// Neighbour hand-off instead of atomics: every super-tile in LDS mode, windows ascending, and a window may
// overlap its neighbours' only (hi[b-1] <= lo[b+1]); rows no window covers are zero-filled by the next
// super-tile (the last one takes the tail), which must stay a small job.  A super-tile without entries
// becomes an empty window at the end of the previous one.
static int plan_handoff(spal_csc *a, std::vector<uint4> &desc) {
    if (!a->all_lds) return SPAL_OK;
    std::vector<uint32_t> prev_hi(a->nblocks, 0);
    bool ok = true;
    uint32_t lo1 = 0, hi1 = 0, hi2 = 0;     // window of b - 1, end of the window of b - 2
    const uint64_t fill_cap = 4ull * (uint32_t)a->cols_per_block;
    for (uint32_t b = 0; b < a->nblocks && ok; ++b) {
        if (desc[b].z != kCscModeLds) desc[b] = make_uint4(hi1, 0, kCscModeLds, 0);
        const uint32_t lo = desc[b].x, hi = lo + desc[b].y;
        prev_hi[b] = hi1;
        ok = lo >= lo1 && hi >= hi1 && lo >= hi2 && (lo <= hi1 || (uint64_t)(lo - hi1) <= fill_cap);
        hi2 = hi1; lo1 = lo; hi1 = hi;
    }
    if (!ok || a->nrows - hi1 > fill_cap) return SPAL_OK;
    SPAL_HIP_TRY(dev_alloc((void **)&a->d_prev_hi, (size_t)a->nblocks * 4));
    SPAL_HIP_TRY(dev_alloc((void **)&a->d_flags, ((size_t)a->nblocks + 2) * 4));   // flags, -, ticket counter
    SPAL_HIP_TRY(hipMemcpyAsync(a->d_prev_hi, prev_hi.data(), (size_t)a->nblocks * 4, hipMemcpyHostToDevice, a->stream));
    SPAL_HIP_TRY(hipMemsetAsync(a->d_flags, 0, ((size_t)a->nblocks + 2) * 4, a->stream));
    if (!a->h_gave_up) {   // one word of mapped host memory: the kernel's "gave up" report
        SPAL_HIP_TRY(hipHostMalloc((void **)&a->h_gave_up, 64, hipHostMallocMapped));
        *a->h_gave_up = 0;
        SPAL_HIP_TRY(hipHostGetDevicePointer((void **)&a->d_gave_up, a->h_gave_up, 0));
    }
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));   // prev_hi goes out of scope
    a->ordered = 1;
    // Which super-tile a workgroup takes: when the device holds ALL workgroups of the launch at once
    // (config 4: 245 workgroups, 256 CUs x 1), every one of them becomes resident whatever the dispatch
    // order and a waiting workgroup never keeps its predecessor off the device: blockIdx will do, and the
    // ticket's round trip at the start of every workgroup (+ 4 us of 39 at config 4) is saved.  Larger
    // launches take their super-tile from the start-order ticket (see csc_spmv_scatter).
    int dev_id = 0, cus = 0;
    (void)hipGetDevice(&dev_id);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id);
    const int per_cu = csc_scatter_per_cu(a);      // the runtime's occupancy of the compiled kernel; 0 = unknown: ticket
    a->ticket_auto = (per_cu <= 0 || (uint64_t)((a->nblocks + 7) / 8) * 8 > (uint64_t)cus * (uint64_t)per_cu) ? 1 : 0;
    return SPAL_OK;
}

// the windows of the two-phase flush with their cover lists, the descriptors, the packed metadata of the LDS-mode super-tiles
static int plan_upload(spal_csc *a, const CscTiling &t) {
    a->windows_entries = t.slots;
    if (t.slots) {
        SPAL_HIP_TRY(dev_alloc(&a->d_windows, (size_t)t.slots * a->elem_size));
        SPAL_HIP_TRY(dev_alloc((void **)&a->d_chunk_ptr, (size_t)(a->nchunks + 1) * 4));
        SPAL_HIP_TRY(dev_alloc((void **)&a->d_chunk_blk, std::max<size_t>(t.cover.size(), 1) * 4));
        SPAL_HIP_TRY(hipMemcpyAsync(a->d_chunk_ptr, t.cover_ptr.data(), (size_t)(a->nchunks + 1) * 4,
                                    hipMemcpyHostToDevice, a->stream));
        if (!t.cover.empty())
            SPAL_HIP_TRY(hipMemcpyAsync(a->d_chunk_blk, t.cover.data(), t.cover.size() * 4, hipMemcpyHostToDevice, a->stream));
        SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    }
    SPAL_HIP_TRY(dev_alloc((void **)&a->d_desc, (size_t)a->nblocks * sizeof(uint4)));
    SPAL_HIP_TRY(hipMemcpyAsync(a->d_desc, t.desc.data(), (size_t)a->nblocks * sizeof(uint4),
                                hipMemcpyHostToDevice, a->stream));
    if (a->lds_entries) {
        if (!a->d_meta) {
            SPAL_HIP_TRY(dev_alloc((void **)&a->d_meta, (size_t)(a->nnz + kStreamPad) * sizeof(uint32_t)));
            SPAL_HIP_TRY(hipMemsetAsync(a->d_meta, 0, (size_t)(a->nnz + kStreamPad) * sizeof(uint32_t), a->stream));
        }
        hipLaunchKernelGGL(csc_encode_meta, dim3(a->nblocks), dim3(256), 0, a->stream, a->d_colptr,
                           a->d_rowind, a->d_desc, a->d_meta, (uint32_t)a->ncols, (uint32_t)a->cols_per_block);
        SPAL_HIP_TRY(hipGetLastError());
    }
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));   // (the host vectors go out of scope)
    return SPAL_OK;
}

// Per-super-tile windows and modes; packed metadata for the LDS mode; then the row tiles.
int csc_plan_build(spal_csc *a) {
    SPAL_TRY(plan_reset(a));
    SPAL_TRY(plan_uniform_columns(a));
    CscTiling t;
    t.desc.assign(a->nblocks, make_uint4(0, 0, kCscModeGlobal, 0));
    if (a->nnz && a->use_lds) {
        std::vector<uint2> win1, win;
        SPAL_TRY(plan_measure_windows(a, win1));
        plan_choose_width(a, win1, win);
        plan_tiles(a, win, t);
        SPAL_TRY(plan_handoff(a, t.desc));
    }
    SPAL_TRY(plan_upload(a, t));
    return csc_rowtiles_plan(a);
}

}  // namespace spal
