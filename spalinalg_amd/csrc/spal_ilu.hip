// spal_ilu.hip -- ILU(0) of a CSR handle on the device.  The contract is a sequential loop over a copy F
// of A's values (A square, every row stores its diagonal, columns ascending; the structure never changes: no fill):
//   for i = 0 .. n-1:  for each stored (i, k), k < i, ascending k, at p:   w = F[p] / F[diag(k)];  F[p] = w;
//       for each stored (k, j), j > k, ascending j, u = F[(k, j)]:   if (i, j) is stored at q:  F[q] = F[q] - (w * u)
// with the product and the difference rounded separately.  Every entry's updates happen in the loop's order whatever
// runs in parallel, so the device returns those bits, f32 and f64.  The result holds L strictly below the diagonal
// (unit diagonal implied) and U on and above it.
//
// THE SCHEDULE IS THE LOWER SOLVE'S.  Row i needs exactly the rows k < i it stores, final: the dependency graph of
// L x = b.  The factorisation walks the lower TrsvPlan's launch list as spal_trsv.hip does: a wide level is one launch, a
// run of narrow levels one launch of one workgroup with __syncthreads() between levels.  Order between workgroups comes
// from stream order alone: no flags, no spins, no grid syncs.
//
// TWO FORMS, one per row (ilu_classify decides, from the row's work = the sum over its k of the entries of row k past
// the diagonal, against the option "ilu_wide_work"):
//   * row form: a thread owns the row and runs the loop as written, finding (i, j) by a two-pointer merge.
//   * wide form: a WAVE owns the row; k stays sequential, the lanes spread over row k's entries past the diagonal and
//     find (i, j) by binary search.  Columns of row k are distinct, so one lane touches an entry per k: the order of its
//     updates is the loop's.  Row i's columns and values are staged in LDS when it has at most kStage entries, else they
//     are updated in place in global memory; a workgroup-scope fence separates the k steps either way.
// A wave takes the row-form rows among its 64 rows first, a thread each, then its wide rows one after the other: loops
// that are uniform across the wave, nothing that waits for another wave inside a level.
// The factor's values are read and written by one kernel (other rows' final values, this row's running ones): the
// pointer is a plain T *, never const __restrict__.
#include "spal_ops.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr int kLevelThreads = 256;
constexpr int kChainThreads = 1024;
constexpr uint32_t kStage = 256;   // entries of a wide row that one wave stages in LDS

// diag[row] = position of the row's diagonal entry, from the plan's rows ordered by level
__global__ __launch_bounds__(256) void ilu_diag(const uint2 *__restrict__ rows, uint64_t n, uint32_t *__restrict__ diag) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint2 rd = rows[k];
    diag[rd.x] = rd.y;
}

// wide[i] = the row has an entry below the diagonal and at least `wide_work` updates to look for; *count = such rows
__global__ __launch_bounds__(256) void ilu_classify(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ colind,
                                                    const uint32_t *__restrict__ diag, uint64_t n, uint64_t wide_work,
                                                    uint8_t *__restrict__ wide, uint32_t *count) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool w = false;
    if (i < n) {
        const uint32_t p0 = rowptr[i], dp = diag[i];
        uint64_t work = 0;
        for (uint32_t p = p0; p < dp; ++p) {
            const uint32_t k = colind[p];
            work += rowptr[k + 1] - diag[k] - 1;
        }
        w = dp > p0 && work >= wide_work;
        wide[i] = w ? 1 : 0;
    }
    const uint64_t m = __ballot(w);
    if (m && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(count, (uint32_t)__popcll(m));
}

// what every row reads besides the factor's values
struct Structure {
    const uint32_t *__restrict__ rowptr;
    const uint32_t *__restrict__ colind;
    const uint32_t *__restrict__ diag;
    const uint8_t *__restrict__ wide;
};

// The loop as written, by one thread.
template <typename T>
__device__ __forceinline__ void ilu_row(uint32_t i, uint32_t dp, const Structure &s, T *f) {
    const uint32_t p1 = s.rowptr[i + 1];
    for (uint32_t p = s.rowptr[i]; p < dp; ++p) {
        const uint32_t k = s.colind[p];
        const uint32_t dk = s.diag[k], e1 = s.rowptr[k + 1];
        const T w = f[p] / f[dk];   // plain division: correctly rounded
        f[p] = w;
        uint32_t q = p + 1;
        for (uint32_t pu = dk + 1; pu < e1 && q < p1; ++pu) {
            const uint32_t j = s.colind[pu];
            while (q < p1 && s.colind[q] < j) ++q;
            if (q < p1 && s.colind[q] == j) {
                f[q] = f[q] - w * f[pu];
                ++q;
            }
        }
    }
}

// what a k step of the wide form stored is what the next step loads, by other lanes of the wave
__device__ __forceinline__ void wave_step_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One wave, all 64 lanes here, owns row i.  STAGED: the row's columns and values live in scol / sval (this wave's) for
// the duration; else both are read, and the values updated, where they are.
template <typename T, bool STAGED>
__device__ __forceinline__ void ilu_wide_row(uint32_t i, const Structure &s, T *f, uint32_t *scol, T *sval) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t p0 = s.rowptr[i], len = s.rowptr[i + 1] - p0, nl = s.diag[i] - p0;
    const uint32_t *col = STAGED ? scol : s.colind + p0;
    T *val = STAGED ? sval : f + p0;
    if (STAGED) {
        for (uint32_t x = lane; x < len; x += 64) {
            scol[x] = s.colind[p0 + x];
            sval[x] = f[p0 + x];
        }
        wave_step_fence();
    }
    for (uint32_t t = 0; t < nl; ++t) {
        const uint32_t k = col[t];
        const uint32_t dk = s.diag[k], e1 = s.rowptr[k + 1];
        const T w = val[t] / f[dk];
        for (uint32_t pu = dk + 1 + lane; pu < e1; pu += 64) {
            const uint32_t j = s.colind[pu];
            const T u = f[pu];
            uint32_t lo = t + 1, hi = len;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) / 2;
                if (col[mid] < j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < len && col[lo] == j) val[lo] = val[lo] - w * u;
        }
        if (lane == 0) val[t] = w;   // nothing reads it again before the row is done
        wave_step_fence();
    }
    if (STAGED) {
        for (uint32_t x = lane; x < len; x += 64) f[p0 + x] = sval[x];
        wave_step_fence();   // the next wide row of this wave stages over them
    }
}

// A wave's share of a level: row k of the ordered rows for each lane (`valid`: there is one).  Called by whole waves.
template <typename T>
__device__ __forceinline__ void ilu_wave_rows(const uint2 *__restrict__ rows, uint64_t k, bool valid, const Structure &s,
                                              T *f, uint32_t *scol, T *sval) {
    uint32_t row = 0;
    bool w = false;
    if (valid) {
        const uint2 rd = rows[k];
        row = rd.x;
        w = s.wide[row] != 0;
        if (!w) ilu_row<T>(row, rd.y, s, f);
    }
    uint64_t m = __ballot(w);
    while (m) {   // uniform across the wave
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint32_t i = __shfl(row, l, 64);
        if (s.rowptr[i + 1] - s.rowptr[i] <= kStage) ilu_wide_row<T, true>(i, s, f, scol, sval);
        else ilu_wide_row<T, false>(i, s, f, scol, sval);
    }
}

template <typename T>
__global__ __launch_bounds__(kLevelThreads) void ilu_level(const uint2 *__restrict__ rows, uint32_t k0, uint32_t k1,
                                                           Structure s, T *f) {
    __shared__ uint32_t scol[kLevelThreads / 64][kStage];
    __shared__ T sval[kLevelThreads / 64][kStage];
    const uint32_t wave = threadIdx.x / 64;
    const uint64_t k = (uint64_t)k0 + (uint64_t)blockIdx.x * kLevelThreads + threadIdx.x;
    ilu_wave_rows<T>(rows, k, k < k1, s, f, scol[wave], sval[wave]);
}

template <typename T>
__global__ __launch_bounds__(kChainThreads) void ilu_chain(const uint2 *__restrict__ rows,
                                                           const uint32_t *__restrict__ level_ptr, uint32_t l0, uint32_t l1,
                                                           Structure s, T *f) {
    __shared__ uint32_t scol[kChainThreads / 64][kStage];
    __shared__ T sval[kChainThreads / 64][kStage];
    const uint32_t wave = threadIdx.x / 64;
    for (uint32_t l = l0; l < l1; ++l) {
        const uint32_t a0 = level_ptr[l], a1 = level_ptr[l + 1];
        for (uint64_t base = a0; base < a1; base += kChainThreads) {   // a level wider than the workgroup is looped over
            const uint64_t k = base + threadIdx.x;
            ilu_wave_rows<T>(rows, k, k < a1, s, f, scol[wave], sval[wave]);
        }
        __syncthreads();   // level l's rows are final and visible to the workgroup before level l + 1 reads them
    }
}

// the lower plan's launch list, as run_list_t of spal_trsv.hip walks it
template <typename T>
hipError_t run_list(const TrsvPlan *p, const Structure &s, T *f, hipStream_t st) {
    for (const TrsvLaunch &ln : p->launches) {
        if (ln.chain) {
            hipLaunchKernelGGL(ilu_chain<T>, dim3(1), dim3(kChainThreads), 0, st, p->d_rows, p->d_level_ptr, ln.level0,
                               ln.level1, s, f);
        } else {
            const uint32_t k0 = p->level_ptr[ln.level0], k1 = p->level_ptr[ln.level1];
            hipLaunchKernelGGL(ilu_level<T>, dim3((k1 - k0 + kLevelThreads - 1) / kLevelThreads), dim3(kLevelThreads), 0, st,
                               p->d_rows, k0, k1, s, f);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void plan_release(TrsvPlan *p) {
    if (!p) return;
    (void)dev_free(p->d_rows);
    (void)dev_free(p->d_level_ptr);
    delete p;
}

// A copy of a plan for a handle of the same structure: device-to-device copies and the launch list.  The positions are
// identical because the structure is.
int plan_clone(const TrsvPlan *p, uint64_t n, hipStream_t st, TrsvPlan **out) {
    TrsvPlan *c = new TrsvPlan;
    c->levels = p->levels;
    c->max_level_rows = p->max_level_rows;
    c->first_missing_diag = p->first_missing_diag;
    c->level_ptr = p->level_ptr;
    c->launches = p->launches;
    c->chain_launches = p->chain_launches;
    c->analysis_ms = 0.0;   // nothing was analysed for it
    hipError_t e = dev_alloc((void **)&c->d_rows, std::max<uint64_t>(n, 1) * sizeof(uint2));
    if (e == hipSuccess) e = dev_alloc((void **)&c->d_level_ptr, p->level_ptr.size() * sizeof(uint32_t));
    if (e == hipSuccess && n) e = hipMemcpyAsync(c->d_rows, p->d_rows, n * sizeof(uint2), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->d_level_ptr, p->d_level_ptr, p->level_ptr.size() * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        plan_release(c);
        return fail(e == hipErrorOutOfMemory ? SPAL_ERR_OUT_OF_MEMORY : SPAL_ERR_HIP, "ilu0: copying the solve plan: %s",
                    hipGetErrorString(e));
    }
    *out = c;
    return SPAL_OK;
}

// The factor of `a` as three device arrays and a copy of a's lower plan, all the caller's until a handle adopts them.
struct Factor {
    OpArrays f;
    TrsvPlan *plan = nullptr;
    uint64_t levels = 0, launches = 0, chain_launches = 0, rows_wide = 0, rows_row = 0;
    int64_t wide_work = 0, chain_rows = 0;
    float kernel_ms = 0.f;
    Factor() = default;
    Factor(const Factor &) = delete;
    Factor &operator=(const Factor &) = delete;
    ~Factor() { plan_release(plan); }
};

// Called with a->mu held (the plan and its launch list are the handle's); synchronises `st`.
int factor_locked(const char *fn, spal_csr *a, hipStream_t st, Factor &out) {
    TrsvPlan *p = nullptr;
    SPAL_TRY(trsv_plan_get(fn, a, 0, 0, st, &p));   // row blocks, not square, a row without a diagonal: refused here
    const uint64_t n = a->nrows, nnz = a->nnz;
    const size_t es = (size_t)a->elem_size;
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(1));
    OpArrays &f = out.f;
    DevBuf diag, wide, cnt;
    SPAL_TRY(f.alloc(n, nnz, es, st));
    SPAL_HIP_TRY(diag.alloc(n * 4));
    SPAL_HIP_TRY(wide.alloc(n));
    SPAL_HIP_TRY(cnt.alloc(4));
    SPAL_HIP_TRY(hipMemcpyAsync(f.ptr, a->d_rowptr, (n + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (nnz) {
        SPAL_HIP_TRY(hipMemcpyAsync(f.ind, a->d_colind, nnz * 4, hipMemcpyDeviceToDevice, st));
        SPAL_HIP_TRY(hipMemcpyAsync(f.val, a->d_values, nnz * es, hipMemcpyDeviceToDevice, st));
    }
    SPAL_HIP_TRY(hipMemsetAsync(cnt.p, 0, 4, st));
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    if (n) {
        const unsigned grid = grid_of(n, 256);
        hipLaunchKernelGGL(ilu_diag, dim3(grid), dim3(256), 0, st, p->d_rows, n, diag.as<uint32_t>());
        hipLaunchKernelGGL(ilu_classify, dim3(grid), dim3(256), 0, st, a->d_rowptr, a->d_colind, diag.as<uint32_t>(), n,
                           (uint64_t)a->ilu_wide_work, wide.as<uint8_t>(), cnt.as<uint32_t>());
        SPAL_HIP_TRY(hipGetLastError());
        const Structure s{a->d_rowptr, a->d_colind, diag.as<uint32_t>(), wide.as<uint8_t>()};
        const hipError_t e = es == 8 ? run_list<double>(p, s, (double *)f.val, st) : run_list<float>(p, s, (float *)f.val, st);
        if (e != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    }
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    uint32_t nwide = 0;
    SPAL_HIP_TRY(hipMemcpyAsync(&nwide, cnt.p, 4, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    SPAL_HIP_TRY(ev.span(0, &out.kernel_ms));
    SPAL_TRY(plan_clone(p, n, st, &out.plan));
    out.levels = p->levels;
    out.launches = p->launches.size();
    out.chain_launches = p->chain_launches;
    out.rows_wide = nwide;
    out.rows_row = n - nwide;
    out.wide_work = a->ilu_wide_work;
    out.chain_rows = a->trsv_chain_rows;
    return SPAL_OK;
}

std::string info_json(const Factor &r, double call_ms) {
    char buf[512];
    snprintf(buf, sizeof buf,
             "{\"levels\": %llu, \"launches\": %llu, \"chain_launches\": %llu, \"rows_row_form\": %llu, "
             "\"rows_wide_form\": %llu, \"wide_work\": %lld, \"chain_rows\": %lld, \"lds_stage_entries\": %u, "
             "\"kernel_ms\": %.4f, \"call_ms\": %.3f}",
             (unsigned long long)r.levels, (unsigned long long)r.launches, (unsigned long long)r.chain_launches,
             (unsigned long long)r.rows_row, (unsigned long long)r.rows_wide, (long long)r.wide_work, (long long)r.chain_rows,
             kStage, (double)r.kernel_ms, call_ms);
    return buf;
}

// the result's handle takes the plan copy and the operand's schedule options (the copied launch list was recorded with them)
void give_plan(spal_csr *dst, Factor &r) {
    std::lock_guard<std::mutex> lock(dst->mu);
    dst->trsv_chain_rows = r.chain_rows;
    dst->ilu_wide_work = r.wide_work;
    dst->trsv[0] = r.plan;
    r.plan = nullptr;
}

// what both entry points end with: a handle of a's type around `arrays` (the factor, by rows or by columns), the plan
// copy handed to the CSR handle the solves will run on
template <typename H>
int adopt_factor(const H *a, OpArrays &arrays, Factor &r, std::chrono::steady_clock::time_point t0, H **out) {
    // nobody multiplies by L\U: the product plan is left to whoever asks for one
    SPAL_TRY(arrays.adopt(a->device, a->elem_size, a->nrows, a->ncols, out, false, true));
    give_plan(solve_handle(*out), r);
    (*out)->ops.ilu_info = info_json(r, ms_since(t0));
    return SPAL_OK;
}

}  // namespace

int ilu_option(spal_csr *a, const char *key, int64_t value, int *status) {
    if (strcmp(key, "ilu_wide_work")) return 0;
    if (value < 0) {
        *status = fail(SPAL_ERR_INVALID_ARGUMENT, "ilu_wide_work must be >= 0 (0: every row with an entry below the diagonal takes the wide form)");
        return 1;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    a->ilu_wide_work = value;
    *status = SPAL_OK;
    return 1;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_ilu0(spal_csr_t a, void *stream, spal_csr_t *out) {
    const char *fn = "spal_csr_ilu0";
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const auto t0 = std::chrono::steady_clock::now();
    Factor r;
    {
        std::lock_guard<std::mutex> lock(a->mu);
        SPAL_TRY(factor_locked(fn, a, (hipStream_t)stream, r));
    }
    return adopt_factor(a, r.f, r, t0, out);
}

int spal_csc_ilu0(spal_csc_t a, void *stream, spal_csc_t *out) {
    const char *fn = "spal_csc_ilu0";
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t st = (hipStream_t)stream;
    spal_csr *twin = a->as_csr;   // the same matrix as CSR
    Factor r;
    {
        std::lock_guard<std::mutex> lock(twin->mu);
        SPAL_TRY(factor_locked(fn, twin, st, r));
    }
    // the factor by columns (the existing transpose path), then a CSC handle around it; its constructor builds the twin,
    // which has the operand's twin's structure
    OpArrays bycol;
    SPAL_TRY(transpose_device(a->device, a->elem_size, a->nrows, a->ncols, a->nnz, r.f.ptr, r.f.ind, r.f.val, st, bycol));
    return adopt_factor(a, bycol, r, t0, out);
}

}  // extern "C"
