// spal_csr_split.hip -- skewed row lengths: the ROW SPLIT (A = A_short + A_long) and, where both are built, its race
// against the block-window kernel (spal_csr_blockwin.hip).  Called by csr_plan_build; products are launched through
// csr_launch_planned (spal_csr.hip) only: the plan that csr_launch would ask for is the one being built here.
#include "csr_kernels.hpp"
#include "spal_internal.hpp"

namespace spal {

// setup: out = {rows longer than T, 64-row tiles that hold one, their entries (low, high word)} -- what decides whether the
// row split is worth building, before anything is copied to the host
__global__ __launch_bounds__(256) void csr_long_rows_scan(const uint32_t *__restrict__ rowptr, uint32_t nrows, uint32_t T,
                                                          unsigned long long *__restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t len = r < nrows ? rowptr[r + 1] - rowptr[r] : 0u;
    const bool lng = len > T;
    const uint64_t m = __ballot(lng);          // a wave = a 64-row tile
    unsigned long long entries = lng ? len : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) entries += __shfl_xor(entries, o);
    if ((threadIdx.x & 63) == 0 && m) {
        atomicAdd(&out[0], (unsigned long long)__popcll(m));
        atomicAdd(&out[1], 1ull);
        atomicAdd(&out[2], entries);
    }
}

// Setup time: two forms of h's product, switched by set_form(0 / 1), each timed on scratch vectors (x zeroed: the time of a
// product does not depend on the values) over 2 launches untimed and 5 timed.  us[] = microseconds per product of the two
// forms (0 where the measurement did not get that far); true when form 1 measured strictly faster.  Any failure says
// false: the second form is an optional one at both callers.  Both callers run under csr_plan_build, for a device-assembled
// handle inside csr_ensure_plan's lock: the launches are csr_launch_planned, which does not ask for the plan again.
template <typename F>
static bool csr_form1_faster(spal_csr *h, F &&set_form, float us[2]) {
    const size_t es = (size_t)h->elem_size;
    DevBuf sx, sy;
    SetupTimer timer;
    float ms[2] = {0.f, 0.f};
    bool ok = sx.alloc(std::max<uint64_t>(h->ncols, 2) * es) == hipSuccess &&
              sy.alloc(std::max<uint64_t>(h->nrows, 1) * es) == hipSuccess &&
              hipMemsetAsync(sx.p, 0, h->ncols * es, h->stream) == hipSuccess;
    for (int on = 0; on < 2 && ok; ++on) {
        set_form(on);
        ok = timer.run(h->stream, 2, 5, [&] { return csr_launch_planned(h, sx.p, sy.p, h->stream); }, &ms[on], "csr plan") == SPAL_OK;
    }
    us[0] = ms[0] * 200.f; us[1] = ms[1] * 200.f;   // (us per product: 5 launches)
    (void)hipGetLastError();
    return ok && ms[1] < ms[0];
}

// ROW SPLIT (round 4).  Power-law row lengths: 0.7 % of the rows are longer than the 128 entries a lane
// may sum, but a 64-row tile holds such a row with probability 36 % -- a third of the ROWS went to the overflow kernel, tile
// by tile, for the sake of those few (2M rows, 20M entries, columns within +-5000: 196 us = 0.18).  When long rows keep a
// tenth of the tiles and more from streaming, the handle multiplies as A = A_short + A_long instead: A_short is a compacted
// copy WITHOUT the long rows' entries (they are empty rows in it) with a complete plan of its own -- stream kernels, sliding
// window, column blocks, whatever its structure asks for --, the long rows are listed and taken a wave each out of the
// original arrays (csr_spmv_row_list).  Short rows stay bit-identical to the reference's order; long rows are tree sums, as
// they were in the overflow kernel (1e-10).  Built on the host side from a copy of rowptr (setup time).
int csr_try_row_split(spal_csr *a, bool *did) {
    CsrPlan &p = a->plan;
    *did = false;
    if (a->split_short) { csr_free(a->split_short); a->split_short = nullptr; }
    (void)dev_free(a->d_split_rows); a->d_split_rows = nullptr;
    a->split_nlong = 0; a->split_long_entries = 0;
    if (p.row_split == 0 || a->split_child || !a->parts.empty() || a->nnz == 0 || a->nrows < 2) return SPAL_OK;
    const uint32_t T = (uint32_t)std::max(1, p.split_threshold);
    {   // on the device first (one pass over rowptr, 24 bytes back): most matrices have no such rows, or too few
        unsigned long long cnt[3] = {0, 0, 0};
        DevBuf d_cnt;   // (back to the allocator on every path out of this block)
        SPAL_HIP_TRY(d_cnt.alloc(24));
        SPAL_HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 24, a->stream));
        hipLaunchKernelGGL(csr_long_rows_scan, dim3((uint32_t)((a->nrows + 255) / 256)), dim3(256), 0, a->stream, a->d_rowptr,
                           (uint32_t)a->nrows, T, d_cnt.as<unsigned long long>());
        SPAL_HIP_TRY(hipGetLastError());
        SPAL_HIP_TRY(hipMemcpyAsync(cnt, d_cnt.p, 24, hipMemcpyDeviceToHost, a->stream));
        SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
        const uint64_t ntiles0 = (a->nrows + 63) / 64, nnz_s0 = a->nnz - cnt[2];
        const bool wanted0 = p.row_split == 1 ? cnt[0] != 0
                                              : (cnt[1] * 10 >= ntiles0 && nnz_s0 >= a->nnz / 4 && (double)nnz_s0 / (double)a->nrows <= 64.0);
        if (!wanted0 || cnt[0] == 0 || nnz_s0 == 0) return SPAL_OK;
    }
    std::vector<uint32_t> rp((size_t)a->nrows + 1);
    SPAL_HIP_TRY(hipMemcpy(rp.data(), a->d_rowptr, rp.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> rows_long;
    uint64_t tiles_hit = 0, long_entries = 0, ntiles = (a->nrows + 63) / 64;
    for (uint64_t t = 0; t < ntiles; ++t) {
        bool hit = false;
        const uint64_t r1 = std::min<uint64_t>(a->nrows, (t + 1) * 64);
        for (uint64_t r = t * 64; r < r1; ++r) {
            const uint32_t len = rp[r + 1] - rp[r];
            if (len > T) { hit = true; rows_long.push_back((uint32_t)r); long_entries += len; }
        }
        tiles_hit += hit ? 1 : 0;
    }
    // longest first: the rows of more than 1024 entries get a workgroup each and start first (a row of 5000 entries by one
    // wave is 20 dependent trips, 80 us -- the launch's tail)
    std::stable_sort(rows_long.begin(), rows_long.end(), [&](uint32_t x, uint32_t y) { return rp[x + 1] - rp[x] > rp[y + 1] - rp[y]; });
    uint32_t n_heavy = 0;
    while (n_heavy < rows_long.size() && rp[rows_long[n_heavy] + 1] - rp[rows_long[n_heavy]] > 1024u) ++n_heavy;
    const uint64_t nnz_s = a->nnz - long_entries;
    const bool wanted = p.row_split == 1 ? !rows_long.empty()
                                         : (tiles_hit * 10 >= ntiles && nnz_s >= a->nnz / 4 &&       // a tenth of the tiles poisoned; the short part is worth a plan
                                            (double)nnz_s / (double)a->nrows <= 64.0);              // ... and streams
    if (!wanted || rows_long.empty() || nnz_s == 0) return SPAL_OK;
    // the short part's arrays
    std::vector<uint32_t> rps((size_t)a->nrows + 1);
    uint32_t run = 0;
    for (uint64_t r = 0; r < a->nrows; ++r) {
        rps[r] = run;
        const uint32_t len = rp[r + 1] - rp[r];
        if (len <= T) run += len;
    }
    rps[a->nrows] = run;
    const uint64_t cap = (uint64_t)nnz_s + kStreamPad;
    uint32_t *d_rps = nullptr, *d_cis = nullptr;
    void *d_vas = nullptr;
    hipError_t e = dev_alloc((void **)&d_rps, rps.size() * 4);
    if (e == hipSuccess) e = dev_alloc((void **)&d_cis, cap * 4);
    if (e == hipSuccess) e = dev_alloc(&d_vas, cap * (size_t)a->elem_size);
    std::vector<uint32_t> list(rows_long.size() * 3);   // {row, first entry, one past the last}
    for (size_t i = 0; i < rows_long.size(); ++i) {
        list[3 * i] = rows_long[i]; list[3 * i + 1] = rp[rows_long[i]]; list[3 * i + 2] = rp[rows_long[i] + 1];
    }
    if (e == hipSuccess) e = dev_alloc((void **)&a->d_split_rows, list.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_rps, rps.data(), rps.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a->d_split_rows, list.data(), list.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset((char *)d_cis + (size_t)nnz_s * 4, 0, kStreamPad * 4);
    if (e == hipSuccess) e = hipMemset((char *)d_vas + (size_t)nnz_s * a->elem_size, 0, kStreamPad * (size_t)a->elem_size);
    if (e == hipSuccess) {
        const uint32_t grid = (uint32_t)((a->nrows + 255) / 256);
        if (a->elem_size == 8)
            hipLaunchKernelGGL(csr_split_copy<double>, dim3(grid), dim3(256), 0, a->stream, a->d_rowptr, d_rps, a->d_colind,
                               (const double *)a->d_values, d_cis, (double *)d_vas, (uint32_t)a->nrows);
        else
            hipLaunchKernelGGL(csr_split_copy<float>, dim3(grid), dim3(256), 0, a->stream, a->d_rowptr, d_rps, a->d_colind,
                               (const float *)a->d_values, d_cis, (float *)d_vas, (uint32_t)a->nrows);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    spal_csr *child = nullptr;
    int st = e == hipSuccess ? SPAL_OK : SPAL_ERR_HIP;
    if (st == SPAL_OK) {
        // (a handle of its own: its plan is built here, eagerly, with this handle's user options that concern the stream kernels)
        st = csr_adopt_device(a->device, a->elem_size, a->nrows, a->ncols, nnz_s, cap, d_rps, d_cis, d_vas, &child, true, true);
        if (st == SPAL_OK) {
            child->split_child = 1;
            child->plan.row_split = 0;
            st = csr_ensure_plan(child, nullptr, false);
            if (st != SPAL_OK) { csr_free(child); child = nullptr; d_rps = nullptr; d_cis = nullptr; d_vas = nullptr; }
        }
    }
    if (st != SPAL_OK) {   // an optional form: without it the handle runs the kernels it always ran
        (void)dev_free(d_rps); (void)dev_free(d_cis); (void)dev_free(d_vas);
        (void)dev_free(a->d_split_rows); a->d_split_rows = nullptr;
        (void)hipGetLastError();
        return SPAL_OK;
    }
    // The short part of a skewed matrix is ragged short rows; where its super-tiles are too wide for an LDS window (they went
    // to the column panels) the column-blocked kernels may be the faster family (power-law rows, columns within +-5000: 93 us
    // in panels, 73 - 82 us column-blocked) -- or not (uniform rows in a band of 16 384: panels).  Setup time: both are timed
    // on scratch vectors, the faster stays.
    if (child->plan.kernel == 2 && child->n_ptiles * 2u > child->plan.nblocks && !child->plan.cblock && child->plan.cblock_user < 0) {
        (void)cblock_plan(child, true);
        if (child->plan.cblock) {
            const bool keep = csr_form1_faster(child, [&](int on) { child->plan.cblock_on = on; }, child->cblock_us);
            child->plan.cblock_on = 1;
            if (!keep) cblock_free(child);
        }
    }
    a->split_short = child;
    a->split_nheavy = n_heavy;
    a->split_nlong = (uint32_t)rows_long.size();
    a->split_long_entries = long_entries;
    *did = true;
    return SPAL_OK;
}

// Skewed matrices whose columns stay near their rows: the block-window kernel against the row split just built, both timed on
// scratch vectors (setup time); the faster form stays, the other is freed.
int csr_blockwin_or_split(spal_csr *a) {
    if (blockwin_plan(a) != SPAL_OK || !a->bw_rows) { blockwin_free(a); (void)hipGetLastError(); return SPAL_OK; }   // (optional form)
    float us[2];
    const bool keep = csr_form1_faster(a, [&](int on) { a->bw_on = on; }, us);
    if (keep) {
        a->bw_on = 1;
        if (a->split_short) { csr_free(a->split_short); a->split_short = nullptr; }
        (void)dev_free(a->d_split_rows); a->d_split_rows = nullptr;
        a->split_nlong = 0; a->split_nheavy = 0; a->split_long_entries = 0;
        a->plan.kernel = 4;
    } else {
        blockwin_free(a);
    }
    a->bw_us[0] = us[0]; a->bw_us[1] = us[1];
    return SPAL_OK;
}

}  // namespace spal
