// spal_csr.hip -- CSR handle: launchers of the product kernels, csr_launch, lifecycle (create / adopt / free / download),
// options and describe.  The planner is in spal_csr_plan.hip, the autotune and the placement walk in spal_csr_tune.hip.
// C ABI entry points documented in include/spal.h.
#include "csr_kernels.hpp"
#include "csr_slide.hpp"
#include "spal_ops.hpp"

namespace spal {

template <typename K>
static hipError_t raise_lds_cap(K kern, int device, size_t lds, std::atomic<uint64_t> &configured) {
    if (lds <= 48 * 1024) return hipSuccess;
    const uint64_t bit = 1ull << (device & 63);
    if (configured.load(std::memory_order_relaxed) & bit) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e == hipSuccess) configured.fetch_or(bit, std::memory_order_relaxed);
    return e;
}

template <typename T, int L, int U, bool LDSX, int BLOCK, int LB = 1>
static hipError_t launch_vec(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    const CsrPlan &p = a->plan;
    const uint32_t per_xcd = (p.nblocks + 7) / 8;
    const size_t lds = LDSX ? (size_t)p.lds_entries * sizeof(T) : 0;
    auto kern = csr_spmv_vector<T, L, U, LDSX, true, BLOCK, LB>;
    static std::atomic<uint64_t> configured{0};
    hipError_t e = raise_lds_cap(kern, a->device, lds, configured);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(BLOCK), lds, st, a->d_rowptr, a->d_colind,
                       (const T *)a->d_values, (const T *)x, (T *)y, a->d_desc, (uint32_t)a->nrows,
                       (uint32_t)a->nnz, (uint32_t)p.rows_per_block, p.nblocks, per_xcd);
    return hipGetLastError();
}

// long rows, x windows in LDS: the kernel that reads 16-bit window-relative columns (plan: vec_col16)
template <typename T, int L, int BLOCK>
static hipError_t launch_vec_col16(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    const CsrPlan &p = a->plan;
    const uint32_t per_xcd = (p.nblocks + 7) / 8;
    const size_t lds = (size_t)p.lds_entries * sizeof(T);
    auto kern = csr_spmv_vector_col16<T, L, BLOCK, 1>;   // (the batched rest-of-row loop, LB = 4, measured 10 ... 20 % slower here)
    static std::atomic<uint64_t> configured{0};
    hipError_t e = raise_lds_cap(kern, a->device, lds, configured);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(BLOCK), lds, st, a->d_rowptr, a->d_colind, a->d_col16,
                       (const T *)a->d_values, (const T *)x, (T *)y, a->d_desc, (uint32_t)a->nrows,
                       (uint32_t)a->nnz, (uint32_t)p.rows_per_block, p.nblocks, per_xcd);
    return hipGetLastError();
}

template <typename T, int L, int U, bool LDSX>
static hipError_t launch_vec_block(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    if constexpr ((L == 64 || L == 32) && U == 1 && LDSX) {
        if (a->plan.vec_col16)
            return a->plan.threads == 1024 ? launch_vec_col16<T, L, 1024>(a, x, y, st)
                                           : launch_vec_col16<T, L, 512>(a, x, y, st);
    }
    if constexpr (L == 16) {  // the long-row form exists for 16 lanes per row only (the planner's choice)
        if (a->plan.long_rows)
            return a->plan.threads == 1024 ? launch_vec<T, L, U, LDSX, 1024, 4>(a, x, y, st)
                                           : launch_vec<T, L, U, LDSX, 512, 4>(a, x, y, st);
    }
    return a->plan.threads == 1024 ? launch_vec<T, L, U, LDSX, 1024>(a, x, y, st)
                                   : launch_vec<T, L, U, LDSX, 512>(a, x, y, st);
}

template <typename T, int L, int U>
static hipError_t launch_vec_lds(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    return a->plan.lds_x ? launch_vec_block<T, L, U, true>(a, x, y, st)
                         : launch_vec_block<T, L, U, false>(a, x, y, st);
}

template <typename T, int L>
static hipError_t launch_vec_unroll(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    switch (a->plan.unroll) {
        case 1: return launch_vec_lds<T, L, 1>(a, x, y, st);
        case 2: return launch_vec_lds<T, L, 2>(a, x, y, st);
        case 4: return launch_vec_lds<T, L, 4>(a, x, y, st);
        default: return hipErrorInvalidValue;
    }
}

// the panel kernel takes the flagged super-tiles (its page loads are 16-byte vectors of x); otherwise the
// stream kernels gather x for them from global memory, as for any other super-tile wider than LDS
static bool panel_runs(const spal_csr *a, const void *x) {
    return a->plan.panel_on && (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
}

// stream kernel; its vector fallback for non-streamable super-tiles uses U = 2
template <typename T, int TPW, int RPT, bool SKEW = false, int PF = 1>
static hipError_t launch_stream_tpw(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    // the in-kernel vector fallback takes super-tiles with a tile of more than 1024 entries, i.e. with heavy
    // rows: a wave per row, four (colind, value) pairs per lane in flight (any geometry is correct)
    constexpr int L = 64;
    const CsrPlan &p = a->plan;
    // the 8 XCDs: one contiguous run of super-tiles each, or (option "xcd_chunk", default 32) interleaved in chunks
    const uint32_t C = (uint32_t)p.xcd_chunk;
    const uint32_t per_xcd = C ? (kXcdChunked | C) : (p.nblocks + 7) / 8;
    const uint32_t grid = C ? ((p.nblocks + 8 * C - 1) / (8 * C)) * 8 * C : ((p.nblocks + 7) / 8) * 8;
    const size_t lds = ((size_t)kStreamWaves * stream_strip<SKEW>() + p.lds_entries) * sizeof(T);
    auto kern = csr_spmv_stream<T, L, 1, true, TPW, RPT, SKEW, PF>;
    static std::atomic<uint64_t> configured{0};
    hipError_t e = raise_lds_cap(kern, a->device, lds, configured);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kStreamBlock), lds, st, a->d_rowptr, a->d_colind,
                       a->d_col16, (const T *)a->d_values, (const T *)x, (T *)y, a->d_desc, a->d_pages,
                       (uint32_t)a->nrows, (uint32_t)a->ncols, (uint32_t)a->nnz, p.nblocks, per_xcd,
                       (uint32_t)(p.nt_store == 1 ? 1 : 0) | ((a->n_ptiles && panel_runs(a, x)) ? 2u : 0u) | (uint32_t)p.diag,
                       (uint32_t)p.ring_pages);
    return hipGetLastError();
}

// persistent form: 2 workgroups per CU, contiguous chunks of each XCD's run
template <typename T, int TPW, int RPT, bool SKEW = false>
static hipError_t launch_stream_persistent(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    constexpr int L = 64;
    const CsrPlan &p = a->plan;
    const uint32_t per_xcd = (p.nblocks + 7) / 8;
    const size_t lds = ((size_t)kStreamWaves * stream_strip<SKEW>() + p.lds_entries) * sizeof(T);
    // grid: as many workgroups as the device holds at once -- 160 KiB of LDS per CU decide
    // (f64 band: 2 per CU = 512; f32, whose strips and window are half the size: 4 per CU)
    int grid = p.persistent_blocks;
    if (grid <= 0) {
        const int per_cu = (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / (lds + 1024)));
        grid = 256 * per_cu;
    }
    const uint32_t slots = (uint32_t)std::max(1, grid / 8);                   // workgroups per XCD
    const uint32_t chunk = (per_xcd + slots - 1) / slots;
    const uint32_t used = (per_xcd + chunk - 1) / chunk;                      // non-empty slots
    auto kern = csr_spmv_stream_persistent<T, L, 1, true, TPW, RPT, SKEW>;
    static std::atomic<uint64_t> configured{0};
    hipError_t e = raise_lds_cap(kern, a->device, lds, configured);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(used * 8), dim3(kStreamBlock), lds, st, a->d_rowptr, a->d_colind,
                       a->d_col16, (const T *)a->d_values, (const T *)x, (T *)y, a->d_desc, a->d_pages,
                       (uint32_t)a->nrows, (uint32_t)a->ncols, (uint32_t)a->nnz, p.nblocks, per_xcd, chunk,
                       (uint32_t)(p.nt_store == 1 ? 1 : 0) | ((a->n_ptiles && panel_runs(a, x)) ? 2u : 0u), (uint32_t)p.ring_pages);
    return hipGetLastError();
}

// rows of the tiles the stream kernels skipped (more than 1024 entries in one tile, or a very long row)
template <typename T>
static hipError_t launch_overflow(const spal_csr *a, const void *x, void *y, hipStream_t st, const uint32_t *tiles,
                                  uint32_t ntiles) {
    hipLaunchKernelGGL(csr_spmv_overflow<T>, dim3(ntiles), dim3(kStreamBlock), 0, st, a->d_rowptr,
                       a->d_colind, (const T *)a->d_values, (const T *)x, (T *)y, tiles,
                       ntiles, (uint32_t)std::min(a->plan.rows_per_tile, 64), (uint32_t)a->nrows);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_stream_main(const spal_csr *a, const void *x, void *y, hipStream_t st);

static bool slide_runs(const spal_csr *a, const void *x) {   // (its page loads are 16-byte vectors of x)
    return a->plan.slide && a->plan.slide_on && a->plan.slide_fill_ok && (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
}

template <typename T>
static hipError_t launch_stream(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    hipError_t e = launch_stream_main<T>(a, x, y, st);
    if (e == hipSuccess && a->n_ptiles && panel_runs(a, x)) e = launch_panel(a, x, y, st);
    // the sliding kernel keeps the tiles that fit the strip in halves: a shorter list is left over
    if (e == hipSuccess && slide_runs(a, x)) {
        if (a->n_ovtiles_slide) e = launch_overflow<T>(a, x, y, st, a->d_ovtiles_slide, a->n_ovtiles_slide);
    } else if (e == hipSuccess && a->n_ovtiles) {
        e = launch_overflow<T>(a, x, y, st, a->d_ovtiles + 1, a->n_ovtiles);
    }
    return e;
}

template <typename T>
static hipError_t launch_stream_main(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    const CsrPlan &p = a->plan;
    if (slide_runs(a, x)) return launch_slide(a, x, y, st);   // the sliding-window kernel
    if (p.tiles_per_wave == 8) return launch_stream_tpw<T, 8, 64>(a, x, y, st);  // (64-row tiles only)
    // two tiles of loads ahead: instantiated for the plain form of the 64- / 32- / 16-row tiles without skew
    if (p.prefetch == 2 && !p.persistent && !p.skew) {
        if (p.rows_per_tile == 64) return launch_stream_tpw<T, 4, 64, false, 2>(a, x, y, st);
        if (p.rows_per_tile == 32) return launch_stream_tpw<T, 4, 32, false, 2>(a, x, y, st);
        if (p.rows_per_tile == 16) return launch_stream_tpw<T, 4, 16, false, 2>(a, x, y, st);
    }
#define SPAL_STREAM_CASE(RPT, SKEW) \
    case RPT: return p.persistent ? launch_stream_persistent<T, (RPT > 128 ? 1 : RPT > 64 ? 2 : 4), RPT, SKEW>(a, x, y, st) \
                                  : launch_stream_tpw<T, (RPT > 128 ? 1 : RPT > 64 ? 2 : 4), RPT, SKEW>(a, x, y, st);
    if (p.skew) {
        switch (p.rows_per_tile) {
            SPAL_STREAM_CASE(256, true) SPAL_STREAM_CASE(128, true) SPAL_STREAM_CASE(64, true) SPAL_STREAM_CASE(32, true) SPAL_STREAM_CASE(24, true)
            SPAL_STREAM_CASE(16, true) SPAL_STREAM_CASE(12, true) SPAL_STREAM_CASE(8, true)
            default: return hipErrorInvalidValue;
        }
    }
    switch (p.rows_per_tile) {
        SPAL_STREAM_CASE(256, false) SPAL_STREAM_CASE(128, false) SPAL_STREAM_CASE(64, false) SPAL_STREAM_CASE(32, false) SPAL_STREAM_CASE(24, false)
        SPAL_STREAM_CASE(16, false) SPAL_STREAM_CASE(12, false) SPAL_STREAM_CASE(8, false)
        default: return hipErrorInvalidValue;
    }
#undef SPAL_STREAM_CASE
}

template <typename T>
static hipError_t launch_lanes(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    if (__atomic_load_n(&a->plan.cblock, __ATOMIC_ACQUIRE) && a->plan.cblock_on) return launch_cblock(a, x, y, st);   // columns anywhere: csr_cblock.hpp
    if (a->plan.kernel == 2) return launch_stream<T>(a, x, y, st);
    switch (a->plan.lanes_per_row) {
#define SPAL_LANES_CASE(LL) \
    case LL: return launch_vec_unroll<T, LL>(a, x, y, st);
        SPAL_LANES_CASE(2) SPAL_LANES_CASE(4) SPAL_LANES_CASE(8) SPAL_LANES_CASE(16)
        SPAL_LANES_CASE(32) SPAL_LANES_CASE(64)
#undef SPAL_LANES_CASE
        default: return hipErrorInvalidValue;
    }
}

// A handle assembled on the device (spal_coo_assemble_csr) is a complete CSR matrix the moment the assembly returns --
// shape, download, conversions work on its arrays -- but the plan of the PRODUCT kernels (tile heights, x windows, 16-bit
// columns, ...: csr_plan_build, a dozen small kernels and host round trips, ~0.3 ms at config 5) is not part of
// `CsrMatrix::from(&coo)` and is built when something first needs it: the first product, spal_csr_plan, set_option,
// autotune, alloc_vectors or describe.  Under mu_cb, pending until finished, like the column-blocked copy below.  The build
// never comes back here for the handle it is planning: what it launches, it launches through csr_launch_planned.
int csr_ensure_plan(spal_csr *a, hipStream_t launch_stream, bool from_launch) {
    if (!__atomic_load_n(&a->plan_pending, __ATOMIC_ACQUIRE)) return SPAL_OK;
    std::lock_guard<std::mutex> lock(a->mu_cb);
    if (!a->plan_pending) return SPAL_OK;
    if (from_launch) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(launch_stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "the first product of a device-assembled handle plans its kernels and cannot be "
                                                   "captured into a graph: call spal_csr_plan (or run one product) before the capture");
    }
    SPAL_TRY(csr_plan_build(a));
    __atomic_store_n(&a->plan_pending, 0, __ATOMIC_RELEASE);
    return SPAL_OK;
}

int csr_launch(spal_csr *a, const void *x_dev, void *y_dev, hipStream_t stream) {
    SPAL_TRY(csr_ensure_plan(a, stream, true));
    return csr_launch_planned(a, x_dev, y_dev, stream);
}

// The product of a handle whose plan exists or is being built by the caller: never looks at plan_pending, never takes mu_cb
// for the plan.  csr_plan_build times its candidate forms through this (csr_form1_faster) while csr_ensure_plan holds the
// non-recursive mu_cb with plan_pending still set; csr_launch above would lock it a second time on the same thread.  The
// parts of a row-block handle and the short part of a row split are planned before their parent can launch them.
int csr_launch_planned(spal_csr *a, const void *x_dev, void *y_dev, hipStream_t stream) {
    auto typed = [&](auto fn) { return a->elem_size == 8 ? fn(double()) : fn(float()); };   // fn(T()), T = the handle's element type
    if (!a->parts.empty()) {   // row blocks: each writes its own rows of y
        for (size_t b = 0; b < a->parts.size(); ++b)
            SPAL_TRY(csr_launch_planned(a->parts[b], x_dev, (char *)y_dev + a->part_row0[b] * (uint64_t)a->elem_size, stream));
        return SPAL_OK;
    }
    if (a->bw_on) {   // skewed rows, columns near the rows: the block-window kernel (spal_csr_blockwin.hip)
        SPAL_HIP_TRY(blockwin_launch(a, x_dev, y_dev, stream));
        return SPAL_OK;
    }
    if (a->split_short) {   // row split: the short rows' handle writes every row of y, the long rows are then overwritten
        SPAL_TRY(csr_launch_planned(a->split_short, x_dev, y_dev, stream));
        const uint32_t grid = a->split_nheavy + (a->split_nlong - a->split_nheavy + kStreamWaves - 1) / kStreamWaves;
        SPAL_HIP_TRY(typed([&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(csr_spmv_row_list<T>, dim3(grid), dim3(kStreamBlock), 0, stream, a->d_rowptr, a->d_colind,
                               (const T *)a->d_values, (const T *)x_dev, (T *)y_dev, a->d_split_rows, a->split_nlong, a->split_nheavy);
            return hipGetLastError();
        }));
        return SPAL_OK;
    }
    if (a->nnz == 0) {
        const uint64_t n = a->nrows;
        SPAL_HIP_TRY(typed([&](auto t) {
            hipLaunchKernelGGL(fill_zero<decltype(t)>, dim3((n + 255) / 256), dim3(256), 0, stream, (decltype(t) *)y_dev, n);
            return hipGetLastError();
        }));
        return SPAL_OK;
    }
    if (__atomic_load_n(&a->plan.cblock_pending, __ATOMIC_ACQUIRE)) {
        // a handle assembled on the device whose columns are anywhere: the tiled copy, built once by the first product.
        // `cblock_pending` stays set until the build has FINISHED, so every concurrent caller takes the lock and waits
        // for it (spal.h: products on one handle may run concurrently); the builder publishes plan.cblock last.
        std::lock_guard<std::mutex> lock(a->mu_cb);
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (a->plan.cblock_pending && hipStreamIsCapturing(stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
            (void)cblock_plan(a, false);    // a failure means "does not qualify": the stream kernels run
            __atomic_store_n(&a->plan.cblock_pending, 0, __ATOMIC_RELEASE);
        }
    }
    const hipError_t e = typed([&](auto t) { return launch_lanes<decltype(t)>(a, x_dev, y_dev, stream); });
    if (e != hipSuccess)
        return fail(SPAL_ERR_HIP, "csr spmv launch failed: %s", hipGetErrorString(e));
    return SPAL_OK;
}

void csr_free(spal_csr *a) {
    if (!a) return;
    for (spal_csr *part : a->parts) csr_free(part);
    (void)dev_free(a->d_rowptr);
    (void)dev_free(a->d_colind);
    (void)dev_free(a->d_values);
    (void)dev_free(a->d_desc);
    if (a->col16_placed) place_free(a->device, a->d_col16);
    else (void)dev_free(a->d_col16);
    rowrec_free(a);
    valpack_free(a);
    (void)dev_free(a->d_pages);
    (void)dev_free(a->d_ovtiles);
    (void)dev_free(a->d_sdesc);
    (void)dev_free(a->d_ovtiles_slide);
    (void)dev_free(a->d_ptiles);
    (void)dev_free(a->d_pwin);
    if (a->split_short) csr_free(a->split_short);
    (void)dev_free(a->d_split_rows);
    blockwin_free(a);
    if (a->d_vec_block && a->vec_block_owned) (void)hipFree(a->d_vec_block);
    else place_free(a->device, a->d_vec_block);
    (void)dev_free(a->d_win_groups);
    cblock_free(a);
    trsv_free(a);
    trsv_sweep_free(a);
    ordering_free(a->ops);
    (void)dev_free(a->d_x);
    (void)dev_free(a->d_y);
    stream_release(a->stream);
    delete a;
}

int csr_adopt_device(int device, int elem_size, uint64_t nrows, uint64_t ncols, uint64_t nnz,
                     uint64_t cap_entries, uint32_t *d_rowptr, uint32_t *d_colind, void *d_values,
                     spal_csr **out, bool eager_copies, bool lazy_plan,
                     uint2 *d_win_groups, uint32_t win_groups, uint32_t win_group_bits) {
    spal_csr *a = new spal_csr;
    if (d_win_groups && win_group_bits <= 8 && win_groups == (uint32_t)((nrows + (1ull << win_group_bits) - 1) >> win_group_bits)) {
        a->d_win_groups = d_win_groups; a->win_groups = win_groups; a->win_group_bits = win_group_bits;
    } else if (d_win_groups) {
        (void)dev_free(d_win_groups);
    }
    a->device = device;
    a->elem_size = elem_size;
    a->nrows = nrows; a->ncols = ncols; a->nnz = nnz;
    a->d_rowptr = d_rowptr; a->d_colind = d_colind; a->d_values = d_values;
    a->cap_entries = cap_entries;
    a->cblock_lazy = eager_copies ? 0 : 1;   // (a handle created from host arrays pays for its second copy at create time)
    auto bail = [&](int st) {
        // the caller keeps ownership of the arrays it passed in on failure
        if (a->d_rowptr == d_rowptr) a->d_rowptr = nullptr;
        if (a->d_colind == d_colind) a->d_colind = nullptr;
        if (a->d_values == d_values) a->d_values = nullptr;
        csr_free(a);
        return st;
    };
    hipError_t e = stream_acquire(&a->stream);
    if (e != hipSuccess) return bail(fail(SPAL_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    // the stream kernel reads whole 128-entry steps: keep kStreamPad spare entries
    const uint64_t need = nnz + kStreamPad;
    if (cap_entries < need) {
        uint32_t *ci = nullptr;
        void *va = nullptr;
        e = dev_alloc((void **)&ci, need * sizeof(uint32_t));
        if (e == hipSuccess) e = dev_alloc((void **)&va, need * (size_t)elem_size);
        if (e == hipSuccess) e = hipMemsetAsync(ci, 0, need * sizeof(uint32_t), a->stream);
        if (e == hipSuccess) e = hipMemsetAsync(va, 0, need * (size_t)elem_size, a->stream);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(ci, d_colind, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, a->stream);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(va, d_values, nnz * (size_t)elem_size, hipMemcpyDeviceToDevice, a->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
        if (e != hipSuccess) {
            (void)dev_free(ci); (void)dev_free(va);
            return bail(fail(e == hipErrorOutOfMemory ? SPAL_ERR_OUT_OF_MEMORY : SPAL_ERR_HIP,
                             "csr_adopt_device: %s", hipGetErrorString(e)));
        }
        a->d_colind = ci; a->d_values = va; a->cap_entries = need;
    }
    int st = SPAL_OK;
    if (lazy_plan && nnz != 0) a->plan_pending = 1;   // (csr_ensure_plan)
    else st = csr_plan_build(a);
    if (st != SPAL_OK) {
        const bool swapped = a->d_colind != d_colind;
        if (swapped) { (void)dev_free(a->d_colind); (void)dev_free(a->d_values); a->d_colind = d_colind; a->d_values = d_values; }
        return bail(st);
    }
    if (a->d_colind != d_colind) {  // the padded copies replaced the caller's arrays
        (void)dev_free(d_colind);
        (void)dev_free(d_values);
    }
    *out = a;
    return SPAL_OK;
}

// rows [r0, r1) of validated host arrays -> a handle whose offsets are relative to rowptr[r0]
template <typename T>
static int csr_create_rows(int device, uint64_t r0, uint64_t r1, uint64_t ncols, const uint64_t *rowptr,
                           const uint64_t *colind, const T *values, spal_csr **out) {
    const uint64_t nrows = r1 - r0, e0 = rowptr[r0], nnz = rowptr[r1] - e0;
    // narrow usize -> u32 on the host (threads), then one upload per array
    std::vector<uint32_t> rp32(nrows + 1), ci32(nnz);
    parallel_for(nrows + 1, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t i = b; i < e; ++i) rp32[i] = (uint32_t)(rowptr[r0 + i] - e0);
    });
    parallel_for(nnz, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t i = b; i < e; ++i) ci32[i] = (uint32_t)colind[e0 + i];
    });
    uint32_t *d_rp = nullptr, *d_ci = nullptr;
    void *d_v = nullptr;
    auto cleanup = [&] { (void)dev_free(d_rp); (void)dev_free(d_ci); (void)dev_free(d_v); };
    const uint64_t cap = nnz + kStreamPad;  // spare entries for the stream kernel's whole-step reads
    hipError_t e = dev_alloc((void **)&d_rp, (nrows + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = dev_alloc((void **)&d_ci, cap * sizeof(uint32_t));
    if (e == hipSuccess) e = dev_alloc((void **)&d_v, cap * sizeof(T));
    if (e == hipSuccess) e = hipMemset((char *)d_ci + nnz * sizeof(uint32_t), 0, kStreamPad * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset((char *)d_v + nnz * sizeof(T), 0, kStreamPad * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(d_rp, rp32.data(), (nrows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(d_ci, ci32.data(), nnz * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(d_v, values + e0, nnz * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        cleanup();
        return fail(e == hipErrorOutOfMemory ? SPAL_ERR_OUT_OF_MEMORY : SPAL_ERR_HIP,
                    "spal_csr_create: upload failed: %s", hipGetErrorString(e));
    }
    spal_csr *a = nullptr;
    int st = csr_adopt_device(device, (int)sizeof(T), nrows, ncols, nnz, cap, d_rp, d_ci, d_v, &a, true);
    if (st != SPAL_OK) { cleanup(); return st; }
    *out = a;
    return SPAL_OK;
}

// entries one set of 32-bit device offsets addresses; SPAL_CSR_PART_ENTRIES lowers it (tests of the row-block path)
static uint64_t csr_part_entries() {
    const char *s = getenv("SPAL_CSR_PART_ENTRIES");
    const uint64_t u = s ? strtoull(s, nullptr, 10) : 0;
    return u ? std::min<uint64_t>(u, kMaxEntries) : kMaxEntries;
}

template <typename T>
static int csr_create(int device, uint64_t nrows, uint64_t ncols, const uint64_t *rowptr,
                      uint64_t rowptr_len, const uint64_t *colind, uint64_t colind_len,
                      const T *values, uint64_t values_len, spal_csr_t *out) {
    if (!out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_create: out is NULL");
    *out = nullptr;
    if (!rowptr || (!colind && colind_len) || (!values && values_len))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_create: null array");
    int reason = 0;
    SPAL_TRY(spal_csr_validate(nrows, ncols, rowptr, rowptr_len, colind, colind_len, values_len, &reason));
    const uint64_t nnz = rowptr[nrows];
    if (nrows >= 0xffffffffull || ncols > 0xffffffffull)
        return fail(SPAL_ERR_UNSUPPORTED, "shape %llu x %llu does not fit 32-bit device indices",
                    (unsigned long long)nrows, (unsigned long long)ncols);
    DeviceGuard guard(device);
    if (guard.status != SPAL_OK) return guard.status;
    const uint64_t limit = csr_part_entries();
    if (nnz <= limit) return csr_create_rows<T>(device, 0, nrows, ncols, rowptr, colind, values, out);

    // more entries than 32-bit offsets address: row blocks of at most `limit` entries, cut at multiples of 1024
    // rows (super-tiles stay whole) where that leaves a block non-empty
    spal_csr *a = new spal_csr;
    a->device = device;
    a->elem_size = (int)sizeof(T);
    a->nrows = nrows; a->ncols = ncols; a->nnz = nnz;
    hipError_t e = stream_acquire(&a->stream);
    if (e != hipSuccess) { csr_free(a); return fail(SPAL_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    for (uint64_t r0 = 0; r0 < nrows;) {
        // largest r1 with rowptr[r1] - rowptr[r0] <= limit
        uint64_t r1 = (uint64_t)(std::upper_bound(rowptr + r0, rowptr + nrows + 1, rowptr[r0] + limit) - rowptr) - 1;
        if (r1 <= r0) {   // (one row above the limit: impossible while columns are < 2^32 and strictly increasing)
            csr_free(a);
            return fail(SPAL_ERR_UNSUPPORTED, "row %llu alone holds more than %llu entries", (unsigned long long)r0,
                        (unsigned long long)limit);
        }
        if (r1 < nrows && (r1 & ~1023ull) > r0) r1 &= ~1023ull;
        spal_csr *part = nullptr;
        const int st = csr_create_rows<T>(device, r0, r1, ncols, rowptr, colind, values, &part);
        if (st != SPAL_OK) { csr_free(a); return st; }
        a->parts.push_back(part);
        a->part_row0.push_back(r0);
        a->part_entry0.push_back(rowptr[r0]);
        r0 = r1;
    }
    a->part_row0.push_back(nrows);
    a->part_entry0.push_back(nnz);
    *out = a;
    return SPAL_OK;
}

template <typename T>
static int csr_spmv_host(spal_csr_t a, const T *x, uint64_t x_len, T *y, uint64_t y_len) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_spmv: handle is NULL");
    if (a->elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_spmv: handle holds %s values",
                    a->elem_size == 8 ? "f64" : "f32");
    if (x_len != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT,
                    "dimension mismatch: x.len() = %llu but ncols = %llu (assert_eq!, csr/ops/mul.rs:9)",
                    (unsigned long long)x_len, (unsigned long long)a->ncols);
    if (y_len != a->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "y.len() = %llu but nrows = %llu",
                    (unsigned long long)y_len, (unsigned long long)a->nrows);
    if (!x || !y) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_spmv: null vector");
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::lock_guard<std::mutex> lock(a->mu);
    if (!a->d_x) SPAL_HIP_TRY(dev_alloc((void **)&a->d_x, a->ncols * sizeof(T)));
    if (!a->d_y) SPAL_HIP_TRY(dev_alloc((void **)&a->d_y, a->nrows * sizeof(T)));
    SPAL_HIP_TRY(hipMemcpyAsync(a->d_x, x, a->ncols * sizeof(T), hipMemcpyHostToDevice, a->stream));
    SPAL_TRY(csr_launch(a, a->d_x, a->d_y, a->stream));
    SPAL_HIP_TRY(hipMemcpyAsync(y, a->d_y, a->nrows * sizeof(T), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    return SPAL_OK;
}

template <typename T>
static int csr_spmv_dev(spal_csr_t a, const T *x_dev, T *y_dev, void *stream) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_spmv_dev: handle is NULL");
    if (a->elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_spmv_dev: handle holds %s values",
                    a->elem_size == 8 ? "f64" : "f32");
    if (!x_dev || !y_dev) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_spmv_dev: null vector");
    int cur = -1;
    SPAL_HIP_TRY(hipGetDevice(&cur));
    if (cur != a->device) {
        DeviceGuard guard(a->device);
        if (guard.status != SPAL_OK) return guard.status;
        return csr_launch(a, x_dev, y_dev, (hipStream_t)stream);
    }
    return csr_launch(a, x_dev, y_dev, (hipStream_t)stream);
}

template <typename T>
static int csr_download(spal_csr_t a, uint64_t *rowptr, uint64_t *colind, T *values) {
    if (!a || !rowptr) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_download: null argument");
    if (a->elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_download: handle holds %s values",
                    a->elem_size == 8 ? "f64" : "f32");
    if (a->nnz && (!colind || !values))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_download: null array");
    if (!a->parts.empty()) {   // row blocks: each fills its slices; offsets become absolute again
        for (size_t b = 0; b < a->parts.size(); ++b) {
            const uint64_t r0 = a->part_row0[b], e0 = a->part_entry0[b];
            SPAL_TRY(csr_download<T>(a->parts[b], rowptr + r0, colind ? colind + e0 : nullptr, values ? values + e0 : nullptr));
            for (uint64_t i = r0; i <= a->part_row0[b + 1]; ++i) rowptr[i] += e0;
        }
        return SPAL_OK;
    }
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::vector<uint32_t> rp(a->nrows + 1), ci(a->nnz);
    SPAL_HIP_TRY(hipMemcpy(rp.data(), a->d_rowptr, rp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (a->nnz) {
        SPAL_HIP_TRY(hipMemcpy(ci.data(), a->d_colind, ci.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        SPAL_HIP_TRY(hipMemcpy(values, a->d_values, a->nnz * sizeof(T), hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i <= a->nrows; ++i) rowptr[i] = rp[i];
    for (uint64_t i = 0; i < a->nnz; ++i) colind[i] = ci[i];
    return SPAL_OK;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_create_f64(int device, uint64_t nrows, uint64_t ncols, const uint64_t *rowptr,
                        uint64_t rowptr_len, const uint64_t *colind, uint64_t colind_len,
                        const double *values, uint64_t values_len, spal_csr_t *out) {
    return csr_create<double>(device, nrows, ncols, rowptr, rowptr_len, colind, colind_len, values,
                              values_len, out);
}
int spal_csr_create_f32(int device, uint64_t nrows, uint64_t ncols, const uint64_t *rowptr,
                        uint64_t rowptr_len, const uint64_t *colind, uint64_t colind_len,
                        const float *values, uint64_t values_len, spal_csr_t *out) {
    return csr_create<float>(device, nrows, ncols, rowptr, rowptr_len, colind, colind_len, values,
                             values_len, out);
}

int spal_csr_destroy(spal_csr_t a) {
    if (!a) return SPAL_OK;
    DeviceGuard guard(a->device);
    csr_free(a);
    return SPAL_OK;
}

int spal_csr_shape(spal_csr_t a, uint64_t *nrows, uint64_t *ncols, uint64_t *nnz, int *elem_size) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_shape: handle is NULL");
    if (nrows) *nrows = a->nrows;
    if (ncols) *ncols = a->ncols;
    if (nnz) *nnz = a->nnz;
    if (elem_size) *elem_size = a->elem_size;
    return SPAL_OK;
}

int spal_csr_spmv_f64(spal_csr_t a, const double *x, uint64_t x_len, double *y, uint64_t y_len) {
    return csr_spmv_host<double>(a, x, x_len, y, y_len);
}
int spal_csr_spmv_f32(spal_csr_t a, const float *x, uint64_t x_len, float *y, uint64_t y_len) {
    return csr_spmv_host<float>(a, x, x_len, y, y_len);
}
int spal_csr_spmv_dev_f64(spal_csr_t a, const double *x_dev, double *y_dev, void *stream) {
    return csr_spmv_dev<double>(a, x_dev, y_dev, stream);
}
int spal_csr_spmv_dev_f32(spal_csr_t a, const float *x_dev, float *y_dev, void *stream) {
    return csr_spmv_dev<float>(a, x_dev, y_dev, stream);
}
int spal_csr_download_f64(spal_csr_t a, uint64_t *rowptr, uint64_t *colind, double *values) {
    return csr_download<double>(a, rowptr, colind, values);
}
int spal_csr_download_f32(spal_csr_t a, uint64_t *rowptr, uint64_t *colind, float *values) {
    return csr_download<float>(a, rowptr, colind, values);
}

// Options that only store a checked integer in one field of the plan; spal_csr_set_option then rebuilds the plan (or restores
// the saved one).  A value is taken when it lies in [lo, hi] and `also` (if any) agrees; otherwise `message` is the error.
struct PlanIntOption {
    const char *key;
    int CsrPlan::*field;
    int64_t lo, hi;
    bool (*also)(int64_t);
    const char *message;
};
static const PlanIntOption kPlanIntOptions[] = {
    {"stream_global", &CsrPlan::stream_global, 0, 1, nullptr, "stream_global must be 0 or 1"},
    // stream kernel: LDS budget of a super-tile in 256-column pages; 0 = automatic (24 f64 pages
    // at two workgroups per CU, or up to 60 at one when that is estimated to pay)
    {"window_pages", &CsrPlan::window_pages, 0, 64, nullptr, "window_pages must be in [0, 64]"},
    // vector kernel, long rows: 16-bit window-relative columns for blocks whose x window is in LDS
    {"col16", &CsrPlan::vec_col16_allowed, 0, 1, nullptr, "col16 must be 0 or 1"},
    // stream kernel: a tile with a row longer than this is left to the overflow kernel
    {"stream_row_max", &CsrPlan::stream_row_max, 1, 1024, nullptr, "stream_row_max must be in [1, 1024]"},
    {"nt_store", &CsrPlan::nt_store, 0, 1, nullptr, "nt_store must be 0 or 1"},
    {"persistent_blocks", &CsrPlan::persistent_blocks, 0, 4096, [](int64_t v) { return v == 0 || (v >= 8 && v % 8 == 0); },
     "persistent_blocks must be 0 (auto) or a multiple of 8 in [8, 4096]"},
    // the sliding-window kernel for band-like plans: -1 = use it where the plan allows (default), 0 = never
    // (the plan then keeps the window-relative col16 of the one-super-tile-per-workgroup kernels), 1 = as -1;
    // "slide_on" 0 keeps the ring plan but launches the one-super-tile-per-workgroup kernels on it (A/B)
    {"slide", &CsrPlan::slide_user, -1, 1, nullptr, "slide must be -1 (auto), 0 or 1"},
    // super-tiles whose column span is at most this many 256-column pages (and wider than the LDS window) are
    // taken in column panels by csr_spmv_panel; 0 = never (x through L2)
    {"panel_pages", &CsrPlan::panel_pages, 0, 255, nullptr, "panel_pages must be in [0, 255]"},
    {"panel_window", &CsrPlan::panel_window_user, 0, 624, nullptr, "panel_window must be in [0, 624] pages"},
    {"panel_on", &CsrPlan::panel_on, 0, 1, nullptr, "panel_on must be 0 or 1"},
    // sliding kernel: steps (of 4 tiles) per run; runs are dealt round-robin to an XCD's workgroups (0 = one run each)
    {"slide_run", &CsrPlan::slide_run, 0, 65535, nullptr, "slide_run must be in [0, 65535]"},
    // sliding kernel, one run per workgroup: steps split evenly over all workgroups of an XCD (default 1) or runs of ceil(steps / workgroups)
    {"slide_even", &CsrPlan::slide_even, 0, 1, nullptr, "slide_even must be 0 or 1"},
    // sliding kernel, matrices whose rows ALL have one length: tile bounds computed (r * length) instead of loaded (default 1)
    {"arith_bounds", &CsrPlan::arith_bounds, 0, 1, nullptr, "arith_bounds must be 0 or 1"},
    // sliding kernel: tiles above 1024 entries whose two halves fit the strip are computed in two passes (1,
    // default) or left to the overflow kernel like every other skipped tile (0)
    {"split_tiles", &CsrPlan::split_tiles_on, 0, 1, nullptr, "split_tiles must be 0 or 1"},
    // sliding kernel, rows of one even length in [12, 16]: one Elias-Fano record per row instead of its col16
    // (csr_rowrec.hpp): -1 = where the plan qualifies (default), 0 = never, 1 = as -1; "rowrec_on" 0 keeps the records
    // but streams col16 on the same plan (A/B, as "slide_on")
    {"rowrec", &CsrPlan::rowrec_user, -1, 1, nullptr, "rowrec must be -1 (auto), 0 or 1"},
    {"rowrec_on", &CsrPlan::rowrec_on, 0, 1, nullptr, "rowrec_on must be 0 or 1"},
    // record form, f64 values that are all multiples of one power of two: one fixed-point block per row instead of its values
    // (csr_valpack.hpp): -1 = where the plan qualifies (default), 0 = never, 1 = as -1; "valpack_on" 0 keeps the blocks but
    // streams the values on the same plan (A/B, as "rowrec_on")
    {"valpack", &CsrPlan::valpack_user, -1, 1, nullptr, "valpack must be -1 (auto), 0 or 1"},
    {"valpack_on", &CsrPlan::valpack_on, 0, 1, nullptr, "valpack_on must be 0 or 1"},
    // autotune: blocks of 1 GiB the 16-bit columns are tried in (0 = leave them where they are)
    {"place_tries", &CsrPlan::place_tries, 0, 16, nullptr, "place_tries must be in [0, 16]"},
    // stream kernel: super-tiles whose rows all have one length do not read rowptr (default 1)
    {"uniform_rows", &CsrPlan::uniform_rows, 0, 1, nullptr, "uniform_rows must be 0 or 1"},
    // stream kernel: tiles of loads ahead of the one being summed
    {"prefetch", &CsrPlan::prefetch, 1, 2, nullptr, "prefetch must be 1 or 2"},
    // one-super-tile stream kernel: super-tiles dealt to the 8 XCDs in chunks of this many (0 = one contiguous run per XCD)
    {"xcd_chunk", &CsrPlan::xcd_chunk, 0, 4096, nullptr, "xcd_chunk must be in [0, 4096]"},
    {"cblock_rows", &CsrPlan::cblock_rows_user, 0, 8192, nullptr,
     "cblock_rows (rows of a row block of the column-blocked kernel) must be 0 (auto) or in [1, 8192]"},
    {"cblock_shift", &CsrPlan::cblock_shift_user, 0, 24, [](int64_t v) { return v == 0 || v >= 8; },
     "cblock_shift (log2 of the columns of a column block) must be 0 (auto: 2 MB of x) or in [8, 24]"},
    // -1 = by the entries per run, 0 = entry-parallel kernel, 1 = rows form (rows of a row block: 256 ... 4096, a power of two)
    {"cblock_form", &CsrPlan::cblock_form_user, -1, 1, nullptr, "cblock_form must be -1 (auto), 0 (entry-parallel) or 1 (rows form)"},
};

int spal_csr_set_option(spal_csr_t a, const char *key, int64_t value) {
    if (!a || !key) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_set_option: null argument");
    {   // options of the sparse operations (this handle as their left operand): no plan involved
        int st = SPAL_OK;
        if (ops_set_option(a->ops, a, key, value, &st)) return st;
    }
    if (!a->parts.empty()) {   // row blocks: every block takes the option (each plans for its own rows)
        for (spal_csr *part : a->parts) SPAL_TRY(spal_csr_set_option(part, key, value));
        return SPAL_OK;
    }
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    SPAL_TRY(csr_ensure_plan(a, nullptr, false));
    if (!strcmp(key, "blockwin")) {
        // the block-window kernel (spal_csr_blockwin.hip): -1 = timed against the row split where that is built, 0 = never,
        // 1 = whenever the matrix's windows fit LDS
        if (value < -1 || value > 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "blockwin must be -1 (auto), 0 or 1");
        std::lock_guard<std::mutex> lock(a->mu);
        a->plan.blockwin = (int)value;
        return a->split_child ? SPAL_OK : csr_plan_build(a);
    }
    if (!strcmp(key, "row_split") || !strcmp(key, "row_split_threshold")) {
        // skewed row lengths: rows above the threshold multiplied apart from the rest (csr_try_row_split): -1 = when they keep
        // a tenth of the 64-row tiles from streaming, 0 = never, 1 = whenever there is such a row
        std::lock_guard<std::mutex> lock(a->mu);
        if (!strcmp(key, "row_split")) {
            if (value < -1 || value > 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "row_split must be -1 (auto), 0 or 1");
            a->plan.row_split = (int)value;
        } else {
            if (value < 1 || value > 4096) return fail(SPAL_ERR_INVALID_ARGUMENT, "row_split_threshold must be in [1, 4096]");
            a->plan.split_threshold = (int)value;
        }
        return a->split_child ? SPAL_OK : csr_plan_build(a);
    }
    if (a->split_short) return spal_csr_set_option(a->split_short, key, value);   // every other option concerns the short part's kernels
    if (a->bw_on) return SPAL_OK;   // (the block-window kernel has no options of its own; the stream kernels' do not concern it)
    std::lock_guard<std::mutex> lock(a->mu);
    CsrPlan saved = a->plan;
    CsrPlan &p = a->plan;
    const PlanIntOption *opt = nullptr;
    for (const PlanIntOption &o : kPlanIntOptions)
        if (!strcmp(key, o.key)) opt = &o;
    if (opt) {
        if (value < opt->lo || value > opt->hi || (opt->also && !opt->also(value)))
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s", opt->message);
        p.*(opt->field) = (int)value;
    } else if (!strcmp(key, "kernel")) {
        if (value < 0 || value > 2)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "kernel must be 0 (auto), 1 (vector) or 2 (stream)");
        p.user_kernel = (int)value;
        if (value == 0) {
            p.user_rows_per_block = p.user_lanes = p.user_lds = p.user_unroll = p.user_threads = false;
            p.user_rows_per_tile = false;
        }
    } else if (!strcmp(key, "rows_per_block")) {
        if (value == 0) p.user_rows_per_block = false;
        else if (value < 16 || value > 65536 || (value % 16))
            return fail(SPAL_ERR_INVALID_ARGUMENT, "rows_per_block must be a multiple of 16 in [16, 65536]");
        else { p.rows_per_block = (int)value; p.user_rows_per_block = true; }
    } else if (!strcmp(key, "lanes_per_row")) {
        if (value == 0) p.user_lanes = false;
        else if (value < 2 || value > 64 || (value & (value - 1)))
            return fail(SPAL_ERR_INVALID_ARGUMENT, "lanes_per_row must be one of 2,4,8,16,32,64");
        else { p.lanes_per_row = (int)value; p.user_lanes = true; }
    } else if (!strcmp(key, "lds_x")) {
        if (value < -1 || value > 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "lds_x must be -1 (auto), 0 or 1");
        if (value < 0) p.user_lds = false;
        else { p.lds_x = (int)value; p.user_lds = true; }
    } else if (!strcmp(key, "unroll")) {
        if (value == 0) p.user_unroll = false;
        else if (value != 1 && value != 2 && value != 4)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "unroll must be 1, 2 or 4");
        else { p.unroll = (int)value; p.user_unroll = true; }
    } else if (!strcmp(key, "skew")) {
        // stream kernel: skewed product strips (-1 = automatic: when most rows are a multiple of 128 bytes long)
        if (value < -1 || value > 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "skew must be -1 (auto), 0 or 1");
        p.user_skew = value >= 0;
        if (value >= 0) p.skew = (int)value;
    } else if (!strcmp(key, "persistent")) {
        if (value != 0 && value != 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "persistent must be 0 or 1");
        p.persistent = (int)value;
        p.user_persistent = true;
    } else if (!strcmp(key, "rows_per_tile")) {
        if (value == 0) p.user_rows_per_tile = false;
        else if (value != 256 && value != 128 && value != 64 && value != 32 && value != 24 && value != 16 && value != 12 && value != 8)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "rows_per_tile must be 0 (auto), 256, 128, 64, 32, 24, 16, 12 or 8");
        else if (p.tiles_per_wave == 8 && value != 64)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "rows_per_tile must be 64 (or 0 = auto) while tiles_per_wave = 8");
        else { p.rows_per_tile = (int)value; p.user_rows_per_tile = true; }
    } else if (!strcmp(key, "tiles_per_wave")) {
        if (value != 4 && value != 8) return fail(SPAL_ERR_INVALID_ARGUMENT, "tiles_per_wave must be 4 or 8");
        // the 8-tile form exists for 64-row tiles only (launch_stream_main): a plan built for another tile height
        // and launched with it would read descriptors of other rows
        if (value == 8 && p.user_rows_per_tile && p.rows_per_tile != 64)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "tiles_per_wave = 8 needs rows_per_tile = 64 (or 0 = auto)");
        p.tiles_per_wave = (int)value;
    } else if (!strcmp(key, "slide_on")) {
        if (value != 0 && value != 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "slide_on must be 0 or 1");
        p.slide_on = (int)value;
        p.slide_fill_user = value ? 1 : -1;   // (asked for by name: also where the tiles are ragged)
        p.slide_fill_ok = value ? 1 : p.slide_fill_ok;
    } else if (!strcmp(key, "diag")) {
#ifdef SPAL_DIAG
        if (value < 0 || value > 0xffff || (value & 0xff)) return fail(SPAL_ERR_INVALID_ARGUMENT, "diag: bits 8 ... 15 only");
        p.diag = (int)value;
#else
        return fail(SPAL_ERR_INVALID_ARGUMENT, "diag: this library is not an ablation build (-DSPAL_DIAG)");
#endif
    } else if (!strcmp(key, "walk_blocks")) {
        // spal_csr_alloc_vectors: blocks of 1 GiB the placement walk probes at most (1 = the first block, no search)
        if (value < 1 || value > 128) return fail(SPAL_ERR_INVALID_ARGUMENT, "walk_blocks must be in [1, 128]");
        a->walk_max = (int)value;
        return SPAL_OK;
    } else if (!strcmp(key, "cblock")) {
        // the column-blocked kernel (csr_cblock.hpp): -1 = when most rows gather x from beyond L2, 0 = never, 1 = always
        if (value < -1 || value > 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "cblock must be -1 (auto), 0 or 1");
        p.cblock_user = (int)value;
        p.cblock_on = 1;
    } else if (!strcmp(key, "threads")) {
        if (value == 0) p.user_threads = false;
        else if (value != 512 && value != 1024)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "threads must be 512 or 1024");
        else { p.threads = (int)value; p.user_threads = true; }
    } else {
        return fail(SPAL_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
    }
    int st = csr_plan_build(a);
    if (st != SPAL_OK) { a->plan = saved; (void)csr_plan_build(a); }
    return st;
}

int spal_csr_plan(spal_csr_t a) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_plan: handle is NULL");
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return csr_ensure_plan(a, nullptr, false);
}
static int csr_describe_plan(spal_csr_t a, char *buf, size_t buf_len) {
    if (!a->parts.empty()) {   // row blocks: the shape of the whole, the cuts, and the first block's plan
        std::string rows = "[";
        for (size_t b = 0; b < a->part_row0.size(); ++b) rows += (b ? ", " : "") + std::to_string(a->part_row0[b]);
        rows += "]";
        std::vector<char> first(buf_len);
        SPAL_TRY(spal_csr_describe(a->parts[0], first.data(), first.size()));
        snprintf(buf, buf_len,
                 "{\"format\": \"csr\", \"dtype\": \"%s\", \"nrows\": %llu, \"ncols\": %llu, \"nnz\": %llu, "
                 "\"kernel\": \"row_blocks\", \"parts\": %zu, \"part_rows\": %s, \"part0\": %s}",
                 a->elem_size == 8 ? "f64" : "f32", (unsigned long long)a->nrows, (unsigned long long)a->ncols,
                 (unsigned long long)a->nnz, a->parts.size(), rows.c_str(), first.data());
        return SPAL_OK;
    }
    {   // (describing the plan of a device-assembled handle builds it: what is printed is what the products will run)
        DeviceGuard guard(a->device);
        if (guard.status != SPAL_OK) return guard.status;
        SPAL_TRY(csr_ensure_plan(a, nullptr, false));
    }
    if (a->bw_on) {
        snprintf(buf, buf_len,
                 "{\"format\": \"csr\", \"dtype\": \"%s\", \"nrows\": %llu, \"ncols\": %llu, \"nnz\": %llu, \"kernel\": \"blockwin\", "
                 "\"index_bits\": 32, \"block_rows\": %u, \"blocks\": %u, \"window_columns\": %u, \"threads_per_block\": 1024, "
                 "\"pass_entries\": 4096, \"thread_rows_up_to\": 32, \"setup_us\": [%.1f, %.1f]}",
                 a->elem_size == 8 ? "f64" : "f32", (unsigned long long)a->nrows, (unsigned long long)a->ncols,
                 (unsigned long long)a->nnz, a->bw_rows, a->bw_blocks, a->bw_cols, a->bw_us[0], a->bw_us[1]);
        return SPAL_OK;
    }
    if (a->split_short) {   // row split: the whole, what was split off, and the short part's plan
        std::vector<char> part(buf_len);
        SPAL_TRY(spal_csr_describe(a->split_short, part.data(), part.size()));
        snprintf(buf, buf_len,
                 "{\"format\": \"csr\", \"dtype\": \"%s\", \"nrows\": %llu, \"ncols\": %llu, \"nnz\": %llu, \"kernel\": \"split\", "
                 "\"split_threshold\": %d, \"split_long_rows\": %u, \"split_long_entries\": %llu, \"short_part\": %s}",
                 a->elem_size == 8 ? "f64" : "f32", (unsigned long long)a->nrows, (unsigned long long)a->ncols,
                 (unsigned long long)a->nnz, a->plan.split_threshold, a->split_nlong, (unsigned long long)a->split_long_entries, part.data());
        return SPAL_OK;
    }
    const CsrPlan &p = a->plan;
    snprintf(buf, buf_len,
             "{\"format\": \"csr\", \"dtype\": \"%s\", \"nrows\": %llu, \"ncols\": %llu, \"nnz\": %llu, "
             "\"index_bits\": %d, \"kernel\": \"%s\", \"lanes_per_row\": %d, \"unroll\": %d, "
             "\"rows_per_block\": %d, \"rows_per_tile\": %d, \"blocks\": %u, \"threads_per_block\": %d, \"lds_x\": %d, "
             "\"lds_window_bytes\": %llu, \"lds_row_fraction\": %.4f, \"stream_row_fraction\": %.4f, "
             "\"overflow_tiles\": %u, \"skew\": %d, \"persistent\": %d, \"nt_store\": %d, \"uniform_row_fraction\": %.4f, "
             "\"prefetch\": %d, \"slide\": %d, \"ring_pages\": %d, \"tile_steps\": %d, \"split_tiles\": %u, \"panel_tiles\": %u, \"autotune_us\": [%.1f, %.1f, %.1f, %.1f], \"placement_us\": [%.1f, %.1f], \"placement_tries\": %d, \"addr\": [\"%llx\", \"%llx\", \"%llx\"], "
             "\"vectors_walk_us\": [%.1f, %.1f], \"vectors_walk_blocks\": %d, \"vectors_probes\": %d, \"placement_blocks\": %d, \"placement_free_bytes\": %llu, "
             "\"nonlocal_row_fraction\": %.4f, \"cblock\": %d, \"cblock_pending\": %d, \"cblock_rows\": %d, \"cblock_form\": \"%s\", \"cblock_run\": %.2f, \"cblock_cols\": %llu, \"cblock_col_blocks\": %d, \"cblock_row_blocks\": %u, \"cblock_us\": [%.1f, %.1f], \"cblock_failed\": %d}",
             a->elem_size == 8 ? "f64" : "f32", (unsigned long long)a->nrows,
             (unsigned long long)a->ncols, (unsigned long long)a->nnz, (p.kernel == 2 || p.vec_col16) ? 16 : 32,
             (p.cblock && p.cblock_on) ? "cblock" : p.kernel == 2 ? "stream" : "vector", p.lanes_per_row, p.kernel == 2 ? 2 : p.unroll,
             p.rows_per_block, p.kernel == 2 ? p.rows_per_tile : 0, p.nblocks, p.threads, p.lds_x,
             (unsigned long long)p.lds_entries * (unsigned long long)a->elem_size, p.lds_row_fraction,
             p.stream_row_fraction,
             p.kernel == 2 ? ((p.slide && p.slide_on) ? a->n_ovtiles_slide : a->n_ovtiles) : 0u,   // (tiles the overflow kernel runs)
             (p.kernel == 2 && p.skew) ? 1 : 0,
             (p.kernel == 2 && p.persistent && p.tiles_per_wave == 4) ? 1 : 0,
             p.kernel == 2 ? p.nt_store : 0, p.kernel == 2 ? p.uniform_row_fraction : 0.0,
             p.kernel == 2 ? p.prefetch : 0, (p.kernel == 2 && p.slide && p.slide_on && p.slide_fill_ok) ? 1 : 0,
             p.kernel == 2 ? p.ring_pages : 0, (p.kernel == 2 && p.slide) ? p.slide_S : 0,
             (p.kernel == 2 && p.slide && p.slide_on) ? a->n_split_tiles : 0u,
             (p.kernel == 2 && p.panel_on) ? a->n_ptiles : 0u,
             (double)a->tuned_us[0], (double)a->tuned_us[1],
             (double)a->tuned_us[2], (double)a->tuned_us[3], (double)a->place_us[0], (double)a->place_us[1],
             a->place_tried, (unsigned long long)(uintptr_t)a->d_values,
             (unsigned long long)(uintptr_t)a->d_col16, (unsigned long long)(uintptr_t)a->d_rowptr,
             (double)a->walk_us[0], (double)a->walk_us[1], a->walk_blocks, a->walk_probes, place_block_count(a->device),
             (unsigned long long)place_free_bytes(a->device),
             p.kernel == 2 ? p.nonlocal_row_fraction : 0.0, (p.cblock && p.cblock_on) ? 1 : 0, p.cblock_pending, p.cblock ? p.cblock_rows : 0, !p.cblock ? "" : p.cblock_form ? "rows" : "entry", p.cblock ? (double)p.cblock_run : 0.0,
             p.cblock ? (1ull << p.cblock_shift) : 0ull, p.cblock ? p.cblock_nbc : 0, p.cblock ? p.cblock_nrb : 0u,
             (double)a->cblock_us[0], (double)a->cblock_us[1], a->cblock_failed);
    // row records (csr_rowrec.hpp), where the plan has the sliding kernel they ride on: built, launched, their size, the
    // widest row they hold under this plan's ring, the autotune's {col16, records} per launch.  (Plans without it say nothing:
    // a caller's buffer that held the line of a small matrix still does.)
    if (p.kernel == 2 && p.slide) {
        const bool rr = p.rowrec && a->d_rowrec;
        const int rr_len = p.slide_uniform - 1;
        SPAL_TRY(describe_append(buf, buf_len, "rowrec", rr ? "1" : "0"));
        SPAL_TRY(describe_append(buf, buf_len, "rowrec_on", (rr && p.rowrec_on && p.slide_on && p.slide_fill_ok) ? "1" : "0"));
        SPAL_TRY(describe_append(buf, buf_len, "rowrec_bytes_per_row", std::to_string(rr ? 4 * rowrec_dwords(p.rowrec) : 0)));
        SPAL_TRY(describe_append(buf, buf_len, "rowrec_max_span",
                                 std::to_string(rowrec_length_ok(rr_len) ? rowrec_max_span(rr_len, (uint32_t)p.ring_pages * kPageCols) : 0u)));
        SPAL_TRY(describe_append(buf, buf_len, "rowrec_failed", std::to_string(p.rowrec_failed)));
        char us[64];
        snprintf(us, sizeof(us), "[%.1f, %.1f]", (double)a->rowrec_us[0], (double)a->rowrec_us[1]);
        SPAL_TRY(describe_append(buf, buf_len, "rowrec_us", us));
        // packed values (csr_valpack.hpp), f64 handles only: built, launched, the bits of the widest k and the quantum's
        // exponent, the block's size, the autotune's {values, packed} per launch, what the scan, builder and verify pass took
        if (a->elem_size == 8) {
            const bool vp = rr && p.valpack && a->d_valpack;
            SPAL_TRY(describe_append(buf, buf_len, "valpack", vp ? "1" : "0"));
            SPAL_TRY(describe_append(buf, buf_len, "valpack_on",
                                     (vp && p.valpack_on && p.rowrec_on && p.slide_on && p.slide_fill_ok) ? "1" : "0"));
            SPAL_TRY(describe_append(buf, buf_len, "valpack_bits", std::to_string(vp ? p.valpack_bits : 0)));
            SPAL_TRY(describe_append(buf, buf_len, "valpack_exp", std::to_string(vp ? p.valpack_exp : 0)));
            SPAL_TRY(describe_append(buf, buf_len, "valpack_bytes_per_row", std::to_string(vp ? 4 * valpack_dwords(p.valpack) : 0)));
            SPAL_TRY(describe_append(buf, buf_len, "valpack_failed", std::to_string(p.valpack_failed)));
            snprintf(us, sizeof(us), "[%.1f, %.1f]", (double)a->valpack_us[0], (double)a->valpack_us[1]);
            SPAL_TRY(describe_append(buf, buf_len, "valpack_us", us));
            snprintf(us, sizeof(us), "%.3f", (double)a->valpack_build_ms);
            SPAL_TRY(describe_append(buf, buf_len, "valpack_build_ms", us));
        }
    }
    return SPAL_OK;
}
int spal_csr_describe(spal_csr_t a, char *buf, size_t buf_len) {
    if (!a || !buf || !buf_len) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_describe: null argument");
    SPAL_TRY(csr_describe_plan(a, buf, buf_len));
    return ops_describe_append(buf, buf_len, a->ops, a);   // "spgemm", "spadd", "spmm", "trsv", "ilu0": those that apply
}

}  // extern "C"
