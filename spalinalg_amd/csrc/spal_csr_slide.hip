// spal_csr_slide.hip -- instantiations, launch and plan of the sliding-window CSR kernel (csr_slide.hpp); a
// translation unit of its own so that the build compiles it beside spal_csr.hip.
#include <chrono>

#include "csr_panel.hpp"
#include "csr_slide.hpp"
#include "spal_internal.hpp"

namespace spal {

// LDS, grid and runs of a launch of the sliding kernel, whatever its form
struct SlideGrid { size_t lds; uint32_t per_xcd, chunk, used; bool even; };
static SlideGrid slide_grid(const spal_csr *a, size_t elem) {
    const CsrPlan &p = a->plan;
    SlideGrid g;
    g.lds = ((size_t)kStreamWaves * stream_strip<false>() + (size_t)p.ring_pages * kPageCols) * elem;
    // as many workgroups as the device holds at once (160 KB of LDS per CU decide), each a contiguous chunk of
    // its XCD's run of steps
    const int per_cu = (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / (g.lds + 512)));
    const uint32_t grid = p.persistent_blocks > 0 ? (uint32_t)p.persistent_blocks : 256u * (uint32_t)per_cu;
    g.per_xcd = (p.slide_steps + 7u) / 8u;
    const uint32_t slots = std::max(1u, grid / 8u);
    // steps per run: one run per workgroup, or what the plan says ("slide_run": shorter runs dealt round-robin)
    const uint32_t one_run = (g.per_xcd + slots - 1u) / slots;
    g.chunk = p.slide_run > 0 ? std::min<uint32_t>((uint32_t)p.slide_run, one_run) : one_run;
    g.even = p.slide_run <= 0 && p.slide_even;        // one run per workgroup: the steps split evenly (csr_slide.hpp)
    g.used = g.even ? std::min(slots, g.per_xcd) : std::min(slots, (g.per_xcd + g.chunk - 1u) / g.chunk);
    return g;
}

template <typename T, int RPT, int S, bool UNI, int REC = 0>
static hipError_t launch_slide_inst(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    constexpr int PF = 2;
    const CsrPlan &p = a->plan;
    const SlideGrid g = slide_grid(a, sizeof(T));
    const size_t lds = g.lds;
    const uint32_t per_xcd = g.per_xcd, chunk = g.chunk, used = g.used;
    const bool even = g.even;
    auto kern = csr_spmv_slide<T, RPT, S, UNI, PF, REC>;
    // (the record form streams the records where the others stream col16)
    const uint16_t *cols = REC != 0 ? reinterpret_cast<const uint16_t *>(a->d_rowrec) : a->d_col16;
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (a->device & 63);
    if (lds > 48 * 1024 && !(configured.load(std::memory_order_relaxed) & bit)) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        configured.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(used * 8u), dim3(kStreamBlock), lds, st, a->d_rowptr, cols,
                       (const T *)a->d_values, (const T *)x, (T *)y, a->d_sdesc, (uint32_t)a->nrows, (uint32_t)a->ncols,
                       p.slide_steps, per_xcd, chunk, (uint32_t)p.ring_pages, (uint32_t)p.slide_uniform,
                       (uint32_t)(p.nt_store ? 1 : 0) | (uint32_t)p.diag | ((UNI && p.all_rows_uniform && p.arith_bounds) ? 4u : 0u) | (even ? 8u : 0u));
    return hipGetLastError();
}

template <typename T, int RPT, bool UNI>
static hipError_t launch_slide_steps(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    // every tile issues S loads per array; S = 4 serves the plans whose tiles are smaller still
    switch (std::max(4, a->plan.slide_S)) {
        case 4: return launch_slide_inst<T, RPT, 4, UNI>(a, x, y, st);
        case 5: return launch_slide_inst<T, RPT, 5, UNI>(a, x, y, st);
        case 6: return launch_slide_inst<T, RPT, 6, UNI>(a, x, y, st);
        case 7: return launch_slide_inst<T, RPT, 7, UNI>(a, x, y, st);
        case 8: return launch_slide_inst<T, RPT, 8, UNI>(a, x, y, st);
        default: return hipErrorInvalidValue;
    }
}

template <typename T, int RPT>
static hipError_t launch_slide_uni(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    return (a->plan.slide_uniform && a->plan.uniform_rows) ? launch_slide_steps<T, RPT, true>(a, x, y, st)
                                                          : launch_slide_steps<T, RPT, false>(a, x, y, st);
}

template <typename T>
static hipError_t launch_slide_rpt(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    switch (a->plan.rows_per_tile) {
        case 64: return launch_slide_uni<T, 64>(a, x, y, st);
        case 32: return launch_slide_uni<T, 32>(a, x, y, st);
        case 24: return launch_slide_uni<T, 24>(a, x, y, st);
        case 16: return launch_slide_uni<T, 16>(a, x, y, st);
        case 12: return launch_slide_uni<T, 12>(a, x, y, st);
        case 8: return launch_slide_uni<T, 8>(a, x, y, st);
        default: return hipErrorInvalidValue;
    }
}

// the row-record form (csr_rowrec.hpp): a kernel of its own per row length, no branch in the others
template <typename T>
static hipError_t launch_slide_rowrec(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    switch (a->plan.rowrec) {
        case 12: return launch_slide_inst<T, 64, 6, true, 12>(a, x, y, st);
        case 14: return launch_slide_inst<T, 64, 7, true, 14>(a, x, y, st);
        case 16: return launch_slide_inst<T, 64, 8, true, 16>(a, x, y, st);
        default: return hipErrorInvalidValue;
    }
}

// the packed-value form (csr_valpack.hpp): the record form's grid and runs, the row blocks in place of the values
template <int L>
static hipError_t launch_slide_valpack_inst(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    constexpr int PF = 2;
    const CsrPlan &p = a->plan;
    const SlideGrid g = slide_grid(a, sizeof(double));
    auto kern = csr_spmv_slide_valpack<L, PF>;
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (a->device & 63);
    if (g.lds > 48 * 1024 && !(configured.load(std::memory_order_relaxed) & bit)) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        configured.fetch_or(bit, std::memory_order_relaxed);
    }
    // (flag 4: the tiles' bounds are arithmetic -- the plan packs under no other -- and rowptr is not passed)
    hipLaunchKernelGGL(kern, dim3(g.used * 8u), dim3(kStreamBlock), g.lds, st, (const uint32_t *)a->d_rowrec,
                       (const valpack_chunk_t *)a->d_valpack, valpack_scale(p.valpack_exp), (const double *)x, (double *)y,
                       a->d_sdesc, (uint32_t)a->nrows, (uint32_t)a->ncols, p.slide_steps, g.per_xcd, g.chunk,
                       (uint32_t)p.ring_pages, (uint32_t)(p.nt_store ? 1 : 0) | (uint32_t)p.diag | 4u | (g.even ? 8u : 0u));
    return hipGetLastError();
}

static hipError_t launch_slide_valpack(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    switch (a->plan.valpack) {
        case 12: return launch_slide_valpack_inst<12>(a, x, y, st);
        case 14: return launch_slide_valpack_inst<14>(a, x, y, st);
        case 16: return launch_slide_valpack_inst<16>(a, x, y, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_slide(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    if (valpack_runs(a)) return launch_slide_valpack(a, x, y, st);
    if (rowrec_runs(a)) return a->elem_size == 8 ? launch_slide_rowrec<double>(a, x, y, st) : launch_slide_rowrec<float>(a, x, y, st);
    return a->elem_size == 8 ? launch_slide_rpt<double>(a, x, y, st) : launch_slide_rpt<float>(a, x, y, st);
}

template <typename T, int RPT>
static hipError_t launch_panel_inst(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    const CsrPlan &p = a->plan;
    // the panel window; the strips reuse it after the last panel
    const size_t lds = std::max((size_t)kStreamWaves * stream_strip<false>(), (size_t)p.panel_window_pages * kPageCols) * sizeof(T);
    auto kern = csr_spmv_panel<T, RPT>;
    static std::atomic<uint64_t> configured{0};
    const uint64_t bit = 1ull << (a->device & 63);
    if (lds > 48 * 1024 && !(configured.load(std::memory_order_relaxed) & bit)) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        configured.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(a->n_ptiles), dim3(kStreamBlock), lds, st, a->d_rowptr, a->d_col16,
                       (const T *)a->d_values, (const T *)x, (T *)y, a->d_ptiles, a->d_pwin, a->d_desc, a->n_ptiles,
                       (uint32_t)a->nrows, (uint32_t)a->ncols, (uint32_t)p.panel_window_pages,
                       (uint32_t)(p.nt_store == 1 ? 1 : 0));
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_panel_rpt(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    switch (a->plan.rows_per_tile) {
        case 64: return launch_panel_inst<T, 64>(a, x, y, st);
        case 32: return launch_panel_inst<T, 32>(a, x, y, st);
        case 24: return launch_panel_inst<T, 24>(a, x, y, st);
        case 16: return launch_panel_inst<T, 16>(a, x, y, st);
        case 12: return launch_panel_inst<T, 12>(a, x, y, st);
        case 8: return launch_panel_inst<T, 8>(a, x, y, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_panel(const spal_csr *a, const void *x, void *y, hipStream_t st) {
    return a->elem_size == 8 ? launch_panel_rpt<double>(a, x, y, st) : launch_panel_rpt<float>(a, x, y, st);
}


// ---- plan of the sliding-window kernel (csr_slide.hpp) -----------------------------------------------------
// One workgroup per STEP of SR = 4 * rpt rows (SR <= 256: a row per thread): out[i] = {first column, one past the
// last column (0: the step stores nothing), 1 + the length of every row if they are all equal else 0, the most
// 128-entry steps one of its four tiles needs | a bit per tile << 8 that can go through the strip in two HALVES}.
// A tile above the strip's 1024 entries whose halves (rpt / 2 rows each) both fit and that holds no row longer
// than row_max is such a tile: the sliding kernel takes it in two passes instead of leaving it to
// csr_spmv_overflow (rows of 1 ... 27 entries: 2 % of the 64-row tiles).  Its halves count for the step number,
// a tile that is left to the overflow kernel does not.
__global__ __launch_bounds__(256) void csr_slide_scan(const uint32_t *__restrict__ rowptr,
                                                      const uint32_t *__restrict__ colind, uint32_t nrows,
                                                      uint32_t rpt, uint32_t row_max, uint4 *__restrict__ out) {
    __shared__ uint32_t s_min, s_max, s_ragged, s_steps, s_long, s_split;
    const uint32_t t = threadIdx.x, SR = 4u * rpt;
    if (t == 0) { s_min = 0xffffffffu; s_max = 0u; s_ragged = 0u; s_steps = 0u; s_long = 0u; s_split = 0u; }
    __syncthreads();
    const uint32_t row0 = blockIdx.x * SR, row1 = min(row0 + SR, nrows);
    const uint32_t len0 = rowptr[row0 + 1] - rowptr[row0];
    if (row0 + t < row1 && t < SR) {
        const uint32_t a0 = rowptr[row0 + t], a1 = rowptr[row0 + t + 1];
        if (a0 < a1) {
            atomicMin(&s_min, colind[a0]);
            atomicMax(&s_max, colind[a1 - 1] + 1u);
        }
        if (a1 - a0 != len0) s_ragged = 1u;
        if (a1 - a0 > row_max) atomicOr(&s_long, 1u << (t / rpt));
    }
    __syncthreads();
    if (t < 4u && row0 + t * rpt < row1) {
        const uint32_t rb = row0 + t * rpt, re = min(rb + rpt, row1), rm = min(rb + rpt / 2u, re);
        const uint32_t b = rowptr[rb], m = rowptr[rm], e = rowptr[re];
        uint32_t steps = (e - (b & ~1u) + 127u) >> 7;
        if (stream_tile_overflows(b, e)) {
            const bool halves = rpt >= 2u && !((s_long >> t) & 1u) && !stream_tile_overflows(b, m) && !stream_tile_overflows(m, e);
            steps = halves ? max((m - (b & ~1u) + 127u) >> 7, (e - (m & ~1u) + 127u) >> 7) : 0u;
            if (halves) atomicOr(&s_split, 1u << t);
        }
        atomicMax(&s_steps, steps);
    }
    __syncthreads();
    if (t == 0)
        out[blockIdx.x] = make_uint4(s_min, s_max, (s_ragged == 0u && len0 < 4095u) ? len0 + 1u : 0u, s_steps | (s_split << 8));
}

// Decides whether the sliding kernel can run this stream plan and, if so, builds its step descriptors.
// desc / skip: the chosen stream plan's super-tiles (16 tiles of rpt rows each); super_pages: the most
// pages one of them stages (the one-super-tile-per-workgroup kernels read the same ring).
int slide_plan(spal_csr *a, uint32_t rpt, const std::vector<uint4> &desc,
                      const std::vector<uint32_t> &skip, uint32_t super_pages) {
    CsrPlan &p = a->plan;
    p.slide = 0;
    p.ring_pages = 0;
    if (a->d_sdesc) { SPAL_HIP_TRY(dev_free(a->d_sdesc)); a->d_sdesc = nullptr; }
    if (a->d_ovtiles_slide) { SPAL_HIP_TRY(dev_free(a->d_ovtiles_slide)); a->d_ovtiles_slide = nullptr; }
    a->n_ovtiles_slide = 0;
    a->n_split_tiles = 0;
    const uint32_t V = 16u / (uint32_t)a->elem_size;
    if (p.slide_user == 0 || p.tiles_per_wave != 4 || rpt > 64u || p.skew || a->ncols < kPageCols || a->nnz == 0) return SPAL_OK;
    for (const uint4 &d : desc)
        if (d.z != kModeStream || !(d.w & 1u)) return SPAL_OK;   // a page list, x through L2, vector rows: not a band
    const uint32_t SR = 4u * rpt;
    const uint32_t nsteps = (uint32_t)((a->nrows + SR - 1) / SR);
    DevBuf d_scan;   // (back to the allocator on every path out)
    SPAL_HIP_TRY(d_scan.alloc((size_t)nsteps * sizeof(uint4)));
    hipLaunchKernelGGL(csr_slide_scan, dim3(nsteps), dim3(256), 0, a->stream, a->d_rowptr, a->d_colind,
                       (uint32_t)a->nrows, rpt, (uint32_t)p.stream_row_max, d_scan.as<uint4>());
    std::vector<uint4> scan(nsteps);
    SPAL_HIP_TRY(hipMemcpyAsync(scan.data(), d_scan.p, (size_t)nsteps * sizeof(uint4), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    // windows: a step that stores nothing keeps its predecessor's window (nothing enters)
    std::vector<uint2> sd(nsteps);
    std::vector<uint32_t> left_over;     // first rows of the tiles csr_spmv_overflow computes when the sliding kernel runs
    uint32_t n_split = 0;
    uint32_t S = 1, ulen = scan[0].z;
    bool uni = true;
    uint32_t pf = 0, pn = 1;
    for (uint32_t i = 0; i < nsteps; ++i) {
        if (scan[i].y) {
            pf = scan[i].x >> kPageShift;
            pn = ((scan[i].y - 1u) >> kPageShift) - pf + 1u;
        }
        sd[i] = make_uint2(pf, pn);
        uni = uni && scan[i].z != 0u && scan[i].z == ulen;
        // tiles the stream kernels skip: those that fit the strip in two halves stay with the sliding kernel (split),
        // the others go to csr_spmv_overflow and do not bound S
        const uint32_t tile0 = i * 4u;
        uint32_t sk = 0;
        for (uint32_t w = 0; w < 4u; ++w) {
            const uint32_t tl = tile0 + w, b = tl / 16u;
            if (b < skip.size() && ((skip[b] >> (tl % 16u)) & 1u)) sk |= 1u << w;
        }
        const uint32_t sp = p.split_tiles_on ? (sk & ((scan[i].w >> 8) & 0xfu)) : 0u;
        sd[i].y |= (sk << 8) | (sp << 20);
        S = std::max(S, scan[i].w & 0xffu);
        for (uint32_t w = 0; w < 4u; ++w) {
            if ((sp >> w) & 1u) ++n_split;
            else if ((sk >> w) & 1u) left_over.push_back((tile0 + w) * rpt);
        }
    }
    if (S > (uint32_t)kStreamSteps) S = (uint32_t)kStreamSteps;   // (cannot be: the scan counts fitting tiles and halves only)
    // ring size: what the largest super-tile stages, and room for the pages that enter with the next step
    const uint32_t page_bytes = kPageCols * (uint32_t)a->elem_size;
    const uint32_t strips = (uint32_t)kStreamWaves * (uint32_t)stream_strip<false>() * (uint32_t)a->elem_size;
    const uint32_t cap2 = (80u * 1024u - strips) / page_bytes;            // two workgroups per CU
    const uint32_t cap1 = std::min<uint32_t>(255u, (160u * 1024u - strips) / page_bytes);   // one
    uint32_t want = super_pages;
    for (uint32_t i = 0; i + 1 < nsteps; ++i) {
        const uint32_t lo = std::min(sd[i].x, sd[i + 1].x);
        const uint32_t hi = std::max(sd[i].x + (sd[i].y & 0xffu), sd[i + 1].x + (sd[i + 1].y & 0xffu));
        want = std::max(want, hi - lo);
    }
    const uint32_t NP = want <= cap2 ? want : std::min(want, std::max(cap1, super_pages));
    if (NP < super_pages || NP > 255u) return SPAL_OK;   // (cannot be: super_pages fits the budget it was planned for)
    // which steps' entering pages are prefetched
    const uint32_t safe_cols = (uint32_t)(a->ncols / V) * V;   // below this column, x is made of whole 16-byte vectors
    const uint32_t VP = kPageCols / V;
    for (uint32_t i = 1; i < nsteps; ++i) {
        const uint32_t f0 = sd[i - 1].x, e0 = f0 + (sd[i - 1].y & 0xffu), f1 = sd[i].x, e1 = f1 + (sd[i].y & 0xffu);
        const uint32_t lo = std::min(f0, f1), hi = std::max(e0, e1);
        uint32_t entering = 0;
        if (f0 >= e1 || e0 <= f1) entering = e1 - f1;
        else entering = (f1 < f0 ? f0 - f1 : 0u) + (e1 > e0 ? e1 - e0 : 0u);
        const bool whole = (uint64_t)e1 * kPageCols <= safe_cols;
        if (hi - lo <= NP && entering * VP <= kSlideAsyncVecs * (uint32_t)kStreamBlock && whole) sd[i].y |= kSlideAsync;
    }
    SPAL_HIP_TRY(dev_alloc((void **)&a->d_sdesc, (size_t)nsteps * sizeof(uint2)));
    SPAL_HIP_TRY(hipMemcpyAsync(a->d_sdesc, sd.data(), (size_t)nsteps * sizeof(uint2), hipMemcpyHostToDevice, a->stream));
    a->n_ovtiles_slide = (uint32_t)left_over.size();
    a->n_split_tiles = n_split;
    if (!left_over.empty()) {
        SPAL_HIP_TRY(dev_alloc((void **)&a->d_ovtiles_slide, left_over.size() * 4));
        SPAL_HIP_TRY(hipMemcpyAsync(a->d_ovtiles_slide, left_over.data(), left_over.size() * 4, hipMemcpyHostToDevice, a->stream));
    }
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));   // `sd`, `left_over` go out of scope
    p.slide = 1;
    p.ring_pages = (int)NP;
    p.slide_steps = nsteps;
    p.slide_S = (int)S;
    p.slide_uniform = (uni && ulen != 0u) ? (int)ulen : 0;
    // every tile of the sliding kernel issues S loads per array (counted waits): where the tiles are on average less than
    // 60 % of the largest one -- ragged short rows, the short part of a row split: 4 of 8 steps -- half its loads are
    // re-reads, and the one-super-tile-per-workgroup kernel, which issues what a tile holds, is faster (power-law short
    // part: 104 -> 68 us); the autotune still times both
    {
        const double tiles = (double)nsteps * kStreamWaves;
        const double avg_steps = tiles > 0 ? (double)a->nnz / tiles / 128.0 : 0.0;
        p.slide_fill_ok = (p.slide_fill_user >= 0) ? p.slide_fill_user : (avg_steps >= 0.6 * (double)std::max(4u, S) ? 1 : 0);
    }
    // every row of the matrix that long: all steps stream (no tile left to the overflow kernel, none split) and the entries
    // add up
    p.all_rows_uniform = (p.slide_uniform && left_over.empty() && n_split == 0 &&
                          (uint64_t)a->nrows * (uint64_t)(ulen - 1u) == a->nnz) ? 1 : 0;
    return SPAL_OK;
}

// ---- row records (csr_rowrec.hpp) ---------------------------------------------------------------------------
// One thread per row of the 4 * slide_steps tiles: the record of a row of the matrix out of colind (every row holds L
// entries: row r's are colind[r * L ...]), the pad record for a row past the last.  flag[0]: a row is not ascending or
// not encodable (it keeps the pad record; the plan drops the records).
template <int L>
__global__ __launch_bounds__(256) void rowrec_build(const uint32_t *__restrict__ colind, uint32_t nrows, uint32_t rows_padded,
                                                    uint32_t R, uint32_t *__restrict__ rec, uint32_t *__restrict__ flag) {
    constexpr int NR = rowrec_dwords(L);
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= rows_padded) return;
    uint32_t w[kRowrecMaxDwords];
    rowrec_pad<L>(w);
    if (r < nrows) {
        uint32_t cols[L];
#pragma unroll
        for (int k = 0; k < L; ++k) cols[k] = colind[(size_t)r * L + k];
        if (!rowrec_encode<L>(cols, R, w)) atomicOr(&flag[0], 1u);
    }
    uint32_t *at = rec + (size_t)(r / 64u) * (NR * 64u) + r % 64u;
#pragma unroll
    for (int q = 0; q < NR; ++q) at[q * 64] = w[q];
}

// ... and every record decoded again and held against the row's col16.  flag[1]: one differs.
template <int L>
__global__ __launch_bounds__(256) void rowrec_verify(const uint32_t *__restrict__ rec, const uint16_t *__restrict__ col16,
                                                     uint32_t nrows, uint32_t R, uint32_t *__restrict__ flag) {
    constexpr int NR = rowrec_dwords(L);
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    uint32_t w[kRowrecMaxDwords] = {0u, 0u, 0u, 0u, 0u, 0u}, pos[L];
    const uint32_t *at = rec + (size_t)(r / 64u) * (NR * 64u) + r % 64u;
#pragma unroll
    for (int q = 0; q < NR; ++q) w[q] = at[q * 64];
    rowrec_decode<L>(w, R, pos);
    bool same = true;
#pragma unroll
    for (int k = 0; k < L; ++k) same = same && pos[k] == (uint32_t)col16[(size_t)r * L + k];
    if (!same) atomicOr(&flag[1], 1u);
}

// ---- packed values (csr_valpack.hpp) ------------------------------------------------------------------------
// One pass over the stored values: out[0] = the smallest exponent of a lowest set mantissa bit over the non-zero
// values, biased by 2048 (0xffffffff: there is none), out[1] = a value is NaN, Inf or -0.0, out[2 ... 3] = the largest
// |value| as its bit pattern.
__global__ __launch_bounds__(256) void valpack_scan(const double *__restrict__ vals, uint64_t n, uint32_t *__restrict__ out) {
    uint32_t emin = 0xffffffffu, bad = 0u;
    uint64_t amax = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t bits = valpack_bits_of(vals[i]);
        if (bits == 0ull) continue;
        uint64_t mant = 0;
        int ex = 0;
        if (!valpack_split(bits, &mant, &ex)) { bad = 1u; continue; }
        emin = min(emin, (uint32_t)(ex + __builtin_ctzll(mant) + 2048));
        const uint64_t mag = bits & ~(1ull << 63);
        amax = mag > amax ? mag : amax;
    }
    for (int o = 32; o > 0; o >>= 1) {   // (64-bit patterns travel and compare as integers, in two halves)
        emin = min(emin, (uint32_t)__shfl_xor((int)emin, o));
        bad |= (uint32_t)__shfl_xor((int)bad, o);
        const uint64_t other = (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)amax, o) |
                               ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(amax >> 32), o) << 32);
        amax = other > amax ? other : amax;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (emin != 0xffffffffu) atomicMin(&out[0], emin);
        if (bad) atomicOr(&out[1], 1u);
        if (amax) atomicMax(reinterpret_cast<unsigned long long *>(out + 2), (unsigned long long)amax);
    }
}

// One thread per row of the 4 * slide_steps tiles: the block of a row of the matrix out of its L values, a block of
// zeros for a row past the last.  flag[0]: a value is not encodable (the plan drops the array).
template <int L>
__global__ __launch_bounds__(256) void valpack_build(const double *__restrict__ vals, uint32_t nrows, uint32_t rows_padded,
                                                     int e, valpack_chunk_t *__restrict__ blocks, uint32_t *__restrict__ flag) {
    constexpr int NQ = valpack_chunks(L);
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= rows_padded) return;
    uint32_t w[4 * NQ];
#pragma unroll
    for (int q = 0; q < 4 * NQ; ++q) w[q] = 0u;
    if (r < nrows) {
        double v[L];
#pragma unroll
        for (int k = 0; k < L; ++k) v[k] = vals[(size_t)r * L + k];
        if (!valpack_encode<L>(v, e, w)) atomicOr(&flag[0], 1u);
    }
    valpack_chunk_t *at = blocks + (size_t)(r / 64u) * (NQ * 64u) + r % 64u;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        valpack_chunk_t c = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
        at[q * 64] = c;
    }
}

// ... and every block decoded again and held against the row's values, bit for bit.  flag[1]: one differs.
template <int L>
__global__ __launch_bounds__(256) void valpack_verify(const valpack_chunk_t *__restrict__ blocks, const double *__restrict__ vals,
                                                      uint32_t nrows, double scale, uint32_t *__restrict__ flag) {
    constexpr int NQ = valpack_chunks(L);
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    uint32_t w[4 * NQ];
    double v[L];
    const valpack_chunk_t *at = blocks + (size_t)(r / 64u) * (NQ * 64u) + r % 64u;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const valpack_chunk_t c = at[q * 64];
        w[4 * q] = c.x; w[4 * q + 1] = c.y; w[4 * q + 2] = c.z; w[4 * q + 3] = c.w;
    }
    valpack_decode<L>(w, scale, v);
    bool same = true;
#pragma unroll
    for (int k = 0; k < L; ++k) same = same && valpack_bits_of(v[k]) == valpack_bits_of(vals[(size_t)r * L + k]);
    if (!same) atomicOr(&flag[1], 1u);
}

void valpack_free(spal_csr *a) {
    (void)dev_free(a->d_valpack);
    a->d_valpack = nullptr;
    a->valpack_bytes = 0;
}

// Builds the row blocks where the plan has row records, the handle holds f64 and every value is k * 2^e with k inside
// the width for the rows' length.  Called after rowrec_plan, on the handle's stream.  The plain values stay resident:
// every other kernel, the download and the sparse operations read them.  An allocation of the right size is kept over
// a re-plan.
int valpack_plan(spal_csr *a) {
    CsrPlan &p = a->plan;
    p.valpack = 0;
    p.valpack_failed = 0;
    p.valpack_bits = 0;
    p.valpack_exp = 0;
    a->valpack_build_ms = 0.f;
    const int L = p.rowrec;
    if (p.valpack_user == 0 || a->elem_size != 8 || !p.rowrec || !a->d_rowrec || !valpack_length_ok(L)) {
        valpack_free(a);
        return SPAL_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    // 1. the quantum and the range
    DevBuf d_out;
    SPAL_HIP_TRY(d_out.alloc(6 * sizeof(uint32_t)));   // scan: {emin, bad, amax lo, amax hi}; build / verify: flag[0 ... 1]
    const uint32_t init[6] = {0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    SPAL_HIP_TRY(hipMemcpyAsync(d_out.p, init, sizeof(init), hipMemcpyHostToDevice, a->stream));
    const uint32_t scan_blocks = (uint32_t)std::min<uint64_t>(4096, (a->nnz + 255) / 256);
    hipLaunchKernelGGL(valpack_scan, dim3(scan_blocks), dim3(256), 0, a->stream, (const double *)a->d_values, (uint64_t)a->nnz,
                       d_out.as<uint32_t>());
    SPAL_HIP_TRY(hipGetLastError());
    uint32_t out[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    SPAL_HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(out), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));   // (`init` was read)
    const int e = out[0] == 0xffffffffu ? 0 : (int)out[0] - 2048;   // (stored zeros only: any quantum)
    const uint64_t amax = (uint64_t)out[2] | ((uint64_t)out[3] << 32);
    int bits = 1;   // of the widest k, sign included: 1 + the bits of the largest |k| (a negative power of two may need one fewer)
    if (amax) {
        uint64_t mant = 0;
        int ex = 0;
        (void)valpack_split(amax, &mant, &ex);
        bits = 1 + (ex + 64 - __builtin_clzll(mant)) - e;
    }
    p.valpack_bits = bits;
    p.valpack_exp = e;
    const int W = valpack_width(L);
    // (W + 1 bits: only -2^(W - 1) fits; the builder, which looks at every value, decides)
    if (out[1] || !valpack_exp_ok(e) || bits > W + 1) {
        valpack_free(a);
        return SPAL_OK;
    }
    // 2. the array
    const uint32_t rows_padded = p.slide_steps * 256u;
    const size_t bytes = (size_t)p.slide_steps * 4u * (size_t)valpack_chunks(L) * 64u * sizeof(valpack_chunk_t);
    if (a->d_valpack && a->valpack_bytes != bytes) valpack_free(a);
    if (!a->d_valpack) {
        if (dev_alloc((void **)&a->d_valpack, bytes) != hipSuccess) {   // no room: the plain values serve
            (void)hipGetLastError();
            a->d_valpack = nullptr;
            return SPAL_OK;
        }
        a->valpack_bytes = bytes;
    }
    uint32_t *d_flag = d_out.as<uint32_t>() + 4;
    const dim3 gb((rows_padded + 255u) / 256u), gv((uint32_t)((a->nrows + 255) / 256));
    auto run = [&](auto len) {
        constexpr int LL = decltype(len)::value;
        hipLaunchKernelGGL(valpack_build<LL>, gb, dim3(256), 0, a->stream, (const double *)a->d_values, (uint32_t)a->nrows,
                           rows_padded, e, (valpack_chunk_t *)a->d_valpack, d_flag);
        // 3. every block decoded and compared
        hipLaunchKernelGGL(valpack_verify<LL>, gv, dim3(256), 0, a->stream, (const valpack_chunk_t *)a->d_valpack,
                           (const double *)a->d_values, (uint32_t)a->nrows, valpack_scale(e), d_flag);
    };
    if (L == 12) run(std::integral_constant<int, 12>{});
    else if (L == 14) run(std::integral_constant<int, 14>{});
    else run(std::integral_constant<int, 16>{});
    SPAL_HIP_TRY(hipGetLastError());
    uint32_t flag[2] = {0u, 0u};
    SPAL_HIP_TRY(hipMemcpyAsync(flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    a->valpack_build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (flag[0] || flag[1]) {   // 4. not encodable after all, or (cannot be) a block that does not decode to its row
        valpack_free(a);
        p.valpack_failed = (!flag[0] && flag[1]) ? 1 : 0;
        return SPAL_OK;
    }
    p.valpack = L;
    return SPAL_OK;
}

void rowrec_free(spal_csr *a) {
    if (a->rowrec_placed) place_free(a->device, a->d_rowrec);
    else (void)dev_free(a->d_rowrec);
    a->d_rowrec = nullptr;
    a->rowrec_bytes = 0;
    a->rowrec_placed = 0;
}

// Builds the records where the plan qualifies: the sliding kernel, every row of the matrix L entries long with
// arithmetic tile bounds, 64-row tiles, L even in [12, 16], every row encodable.  Called once col16 is encoded, on the
// handle's stream.  An allocation of the right size is kept over a re-plan (it may be a placed piece).
int rowrec_plan(spal_csr *a) {
    CsrPlan &p = a->plan;
    p.rowrec = 0;
    p.rowrec_failed = 0;
    const int L = p.slide_uniform - 1;
    if (p.rowrec_user == 0 || !p.slide || !p.all_rows_uniform || !p.arith_bounds || p.rows_per_tile != 64 ||
        p.tiles_per_wave != 4 || !rowrec_length_ok(L) || p.slide_S != L / 2 || !a->d_col16) {
        rowrec_free(a);
        return SPAL_OK;
    }
    const uint32_t R = (uint32_t)p.ring_pages * kPageCols;
    const uint32_t rows_padded = p.slide_steps * 256u;
    const size_t bytes = (size_t)p.slide_steps * 4u * (size_t)rowrec_dwords(L) * 64u * sizeof(uint32_t);
    if (a->d_rowrec && a->rowrec_bytes != bytes) rowrec_free(a);
    if (!a->d_rowrec) {
        if (dev_alloc((void **)&a->d_rowrec, bytes) != hipSuccess) {   // no room: col16 serves
            (void)hipGetLastError();
            a->d_rowrec = nullptr;
            return SPAL_OK;
        }
        a->rowrec_bytes = bytes;
    }
    DevBuf d_flag;
    SPAL_HIP_TRY(d_flag.alloc(2 * sizeof(uint32_t)));
    SPAL_HIP_TRY(hipMemsetAsync(d_flag.p, 0, 2 * sizeof(uint32_t), a->stream));
    const dim3 gb((rows_padded + 255u) / 256u), gv((uint32_t)((a->nrows + 255) / 256));
    auto run = [&](auto len) {
        constexpr int LL = decltype(len)::value;
        hipLaunchKernelGGL(rowrec_build<LL>, gb, dim3(256), 0, a->stream, a->d_colind, (uint32_t)a->nrows, rows_padded, R,
                           a->d_rowrec, d_flag.as<uint32_t>());
        hipLaunchKernelGGL(rowrec_verify<LL>, gv, dim3(256), 0, a->stream, a->d_rowrec, a->d_col16, (uint32_t)a->nrows, R,
                           d_flag.as<uint32_t>());
    };
    if (L == 12) run(std::integral_constant<int, 12>{});
    else if (L == 14) run(std::integral_constant<int, 14>{});
    else run(std::integral_constant<int, 16>{});
    SPAL_HIP_TRY(hipGetLastError());
    uint32_t flag[2] = {0u, 0u};
    SPAL_HIP_TRY(hipMemcpyAsync(flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    if (flag[0] || flag[1]) {
        rowrec_free(a);
        p.rowrec_failed = (!flag[0] && flag[1]) ? 1 : 0;
        return SPAL_OK;
    }
    p.rowrec = L;
    return SPAL_OK;
}

}  // namespace spal
