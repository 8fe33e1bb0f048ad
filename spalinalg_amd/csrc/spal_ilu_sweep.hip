// spal_ilu_sweep.hip -- ILU(0) by row sweeps: the factorisation's twin of spal_trsv_sweep.hip.  The
// contract (include/spal.h): F0 = A's values; for t = 1 .. s every row i, independently of the others, starts as a copy
// of A's row i and runs the body of ILU(0)'s loop on it -- for each stored (i, k), k < i, ascending: w = Ft[p] /
// F(t-1)[diag(k)]; Ft[p] = w; for each stored (k, j), j > k, ascending, u = F(t-1)[(k, j)]: if (i, j) is stored at q,
// Ft[q] = Ft[q] - (w * u), product and difference rounded separately.  Every read of ANOTHER row comes from the previous
// pass, the row's own running values are this pass's.  A row of level l holds ilu0's bits from pass l on, so
// s >= levels - 1 is spal_*_ilu0's factor bit for bit.
//
// ONE PASS IS ONE LAUNCH; ORDER BETWEEN PASSES IS STREAM ORDER ALONE: no atomics on values, no flags, nothing waits on
// another workgroup.  Three streams: A's values (read only), F(t-1) (read only within the launch: const __restrict__ is
// legitimate here, unlike in spal_ilu.hip) and Ft, every row of which is written by its owner alone.
//
// A workgroup owns kBlockRows consecutive rows, whose entries [rowptr[r0], rowptr[r1]) are contiguous.
//   PHASE 1, the row form.  A block of at most kStage entries is loaded, columns and A's values, coalesced into LDS; the
//   thread that owns a row runs the loop on the LDS copy (a two-pointer merge of row k's tail, gathered from F(t-1),
//   against its own row); the block goes back to Ft coalesced.  A block of more entries is copied A -> Ft coalesced and
//   its rows run in place on Ft in global memory: one long row costs its neighbours the stage, nothing else.
//   Either way every entry of the block is written, the wide rows' with A's values.
//   PHASE 2, the wide form, for rows whose work (ilu_sweep_classify: the sum over the row's k of the entries of row k
//   past its diagonal) is at least the option "ilu_wide_work".  A WAVE owns the row: k stays sequential, the lanes
//   spread over row k's tail and find (i, j) by binary search, as ilu_wide_row does.  The stage is free by now; each of
//   the workgroup's waves has kWideStage = kStage / waves entries of it, and a row of at most that many entries is
//   staged there, a longer one updated in place in Ft; a workgroup-scope fence separates the k steps either way.
// Columns of row k are distinct, so one lane touches an entry per k and the order of an entry's updates is the loop's
// in both forms: the bits do not depend on the threshold, the stage or the geometry.
// Every loop that contains a fence or a barrier is uniform across the wave or the workgroup.
//
// WHAT A HANDLE NEEDS is the diagonal's position per row: sweep_rows {dlo, dhi} of spal_trsv_sweep.hip, built once per
// handle under its lock (trsv_sweep_prepare).  No host analysis, no TrsvPlan; the operand is only read.
#include "spal_ops.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

// The geometry; -DSPAL_ILU_SWEEP_ROWS / -DSPAL_ILU_SWEEP_STAGE build the variants tools/bench_ilu_sweep.py compares.
#ifndef SPAL_ILU_SWEEP_ROWS
#define SPAL_ILU_SWEEP_ROWS 256
#endif
#ifndef SPAL_ILU_SWEEP_STAGE
#define SPAL_ILU_SWEEP_STAGE 4096
#endif
constexpr int kBlockRows = SPAL_ILU_SWEEP_ROWS;        // rows of a workgroup = its threads
constexpr uint32_t kWaves = kBlockRows / 64;
constexpr uint32_t kStage = SPAL_ILU_SWEEP_STAGE;      // entries of a block staged in LDS, 12 bytes each in f64
constexpr uint32_t kWideStage = kStage / kWaves;       // entries of a wide row that its wave stages
constexpr uint32_t kWalk = 8;                          // own entries a merge step walks over before it searches instead
constexpr int kAhead = 4;                              // entries of row k's tail a row's owner loads before it merges them
static_assert(kBlockRows % 64 == 0 && kBlockRows >= 64 && kBlockRows <= 1024 && kStage % kWaves == 0, "geometry");

// wide[i] = the row has an entry below the diagonal and at least `wide_work` updates to look for; *count = such rows
__global__ __launch_bounds__(256) void ilu_sweep_classify(uint32_t n, const uint32_t *__restrict__ rowptr,
                                                          const uint32_t *__restrict__ colind,
                                                          const uint2 *__restrict__ rows, uint64_t wide_work,
                                                          uint8_t *__restrict__ wide, uint32_t *count) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool w = false;
    if (i < n) {
        const uint32_t p0 = rowptr[i], dp = rows[i].x;
        uint64_t work = 0;
        for (uint32_t p = p0; p < dp; ++p) {
            const uint32_t k = colind[p];
            work += rowptr[k + 1] - rows[k].x - 1;
        }
        w = dp > p0 && work >= wide_work;
        wide[i] = w ? 1 : 0;
    }
    const uint64_t m = __ballot(w);
    if (m && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(count, (uint32_t)__popcll(m));
}

// what every row reads besides its own values
template <typename T>
struct Pass {
    const uint32_t *__restrict__ rowptr;
    const uint32_t *__restrict__ colind;
    const uint2 *__restrict__ rows;      // .x: the diagonal's position
    const T *__restrict__ prev;          // F(t-1)
};

// the first position in [lo, hi) whose column is >= j (columns ascend)
__device__ __forceinline__ uint32_t first_not_below(const uint32_t *col, uint32_t lo, uint32_t hi, uint32_t j) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (col[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The loop as written, by one thread, on the row's columns and running values at col / val [p0, p1) with the diagonal at
// dp (LDS, or global memory: the caller's pointers decide).
template <typename T>
__device__ __forceinline__ void sweep_row(const uint32_t *col, T *val, uint32_t p0, uint32_t dp, uint32_t p1,
                                          const Pass<T> &s) {
    if (p0 == dp) return;
    // The loads are what a row waits for, so they go out early: row k's bounds one k ahead, its tail kAhead entries at
    // a time before they are merged.  The order of the updates is the loop's.
    uint32_t k = col[p0];
    uint32_t dk = s.rows[k].x, e1 = s.rowptr[k + 1];
    for (uint32_t p = p0; p < dp; ++p) {
        uint32_t ndk = 0, ne1 = 0;
        if (p + 1 < dp) {
            k = col[p + 1];
            ndk = s.rows[k].x;
            ne1 = s.rowptr[k + 1];
        }
        const T w = val[p] / s.prev[dk];   // plain division: correctly rounded
        val[p] = w;
        uint32_t q = p + 1;
        for (uint32_t pu = dk + 1; pu < e1 && q < p1; pu += kAhead) {
            uint32_t j[kAhead];
            T u[kAhead];
#pragma unroll
            for (int x = 0; x < kAhead; ++x) {   // past the tail's end its last entry's addresses repeat
                const uint32_t at = min(pu + (uint32_t)x, e1 - 1);
                j[x] = s.colind[at];
                u[x] = s.prev[at];
            }
#pragma unroll
            for (int x = 0; x < kAhead; ++x) {
                if (pu + (uint32_t)x < e1) {
                    uint32_t walked = 0;
                    while (q < p1 && col[q] < j[x]) {   // to the first own entry with column >= j: a short walk, or
                        ++q;                             // a search when the row is long and row k's tail is sparse
                        if (++walked == kWalk) {
                            q = first_not_below(col, q, p1, j[x]);
                            break;
                        }
                    }
                    if (q < p1 && col[q] == j[x]) {
                        val[q] = val[q] - w * u[x];
                        ++q;
                    }
                }
            }
        }
        dk = ndk;
        e1 = ne1;
    }
}

// what a k step of the wide form stored is what the next step loads, by other lanes of the wave
__device__ __forceinline__ void wave_step_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One wave, all 64 lanes here, owns row i.  STAGED: the row's columns and A's values live in scol / sval (this wave's)
// for the duration; else the columns are read, and the values updated, where they are: in ft, which phase 1 filled
// with A's values.
template <typename T, bool STAGED>
__device__ __forceinline__ void sweep_wide_row(uint32_t i, const Pass<T> &s, const T *__restrict__ a, T *ft, uint32_t *scol,
                                               T *sval) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t p0 = s.rowptr[i], len = s.rowptr[i + 1] - p0, nl = s.rows[i].x - p0;
    const uint32_t *col = STAGED ? scol : s.colind + p0;
    T *val = STAGED ? sval : ft + p0;
    if (STAGED) {
        for (uint32_t x = lane; x < len; x += 64) {
            scol[x] = s.colind[p0 + x];
            sval[x] = a[p0 + x];
        }
        wave_step_fence();
    }
    for (uint32_t t = 0; t < nl; ++t) {
        const uint32_t k = col[t];
        const uint32_t dk = s.rows[k].x, e1 = s.rowptr[k + 1];
        const T w = val[t] / s.prev[dk];
        for (uint32_t pu = dk + 1 + lane; pu < e1; pu += 64) {
            const uint32_t j = s.colind[pu];
            const T u = s.prev[pu];
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
        for (uint32_t x = lane; x < len; x += 64) ft[p0 + x] = sval[x];
        wave_step_fence();   // the next wide row of this wave stages over them
    }
}

template <typename T>
__global__ __launch_bounds__(kBlockRows) void ilu_sweep_pass(uint32_t n, Pass<T> s, const uint8_t *__restrict__ wide,
                                                             const T *__restrict__ a, T *ft) {
    __shared__ uint32_t scol[kStage];
    __shared__ T sval[kStage];
    const uint32_t tid = threadIdx.x;
    const uint32_t r0 = blockIdx.x * kBlockRows;
    const uint32_t nr = min((uint32_t)kBlockRows, n - r0);   // rows of this block, >= 1
    const uint32_t e0 = s.rowptr[r0], e1 = s.rowptr[r0 + nr], cnt = e1 - e0;
    const bool mine = tid < nr;
    const uint32_t row = r0 + tid;
    uint32_t p0 = 0, dp = 0, p1 = 0;
    bool w = false;
    if (mine) {
        p0 = s.rowptr[row];
        p1 = s.rowptr[row + 1];
        dp = s.rows[row].x;
        w = wide[row] != 0;
    }
    // ---- phase 1 (the branch is uniform across the workgroup) ----
    if (cnt <= kStage) {
        for (uint32_t x = tid; x < cnt; x += kBlockRows) {
            scol[x] = s.colind[e0 + x];
            sval[x] = a[e0 + x];
        }
        __syncthreads();
        if (mine && !w) sweep_row<T>(scol, sval, p0 - e0, dp - e0, p1 - e0, s);
        __syncthreads();
        for (uint32_t x = tid; x < cnt; x += kBlockRows) ft[e0 + x] = sval[x];
    } else {
        for (uint32_t x = tid; x < cnt; x += kBlockRows) ft[e0 + x] = a[e0 + x];
        __syncthreads();   // (a fence at workgroup scope too: the copy is visible to the rows' owners)
        if (mine && !w) sweep_row<T>(s.colind, ft, p0, dp, p1, s);
    }
    // ---- phase 2: the wave's wide rows, one after the other ----
    if (!__syncthreads_or(w)) return;   // the stage is free and Ft holds A's values of the wide rows
    const uint32_t wave = tid / 64;
    uint32_t *wcol = scol + wave * kWideStage;
    T *wval = sval + wave * kWideStage;
    uint64_t m = __ballot(w);
    while (m) {   // uniform across the wave
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint32_t i = r0 + wave * 64 + (uint32_t)l;
        if (s.rowptr[i + 1] - s.rowptr[i] <= kWideStage) sweep_wide_row<T, true>(i, s, a, ft, wcol, wval);
        else sweep_wide_row<T, false>(i, s, a, ft, wcol, wval);
    }
}

// scratch of one call, taken from and returned to the runtime's stream-ordered allocator in stream order
struct StreamScratch {
    void *p = nullptr;
    hipStream_t st = nullptr;
    StreamScratch() = default;
    StreamScratch(const StreamScratch &) = delete;
    StreamScratch &operator=(const StreamScratch &) = delete;
    ~StreamScratch() {
        if (p) (void)hipFreeAsync(p, st);
    }
    hipError_t alloc(size_t bytes, hipStream_t stream) {
        st = stream;
        return hipMallocAsync(&p, bytes, stream);
    }
};

// The swept factor of `a` as three device arrays, the caller's until a handle adopts them.
struct SweepFactor {
    OpArrays f;
    uint64_t sweeps = 0, requested = 0, rows_wide = 0, rows_row = 0;
    int64_t wide_work = 0;
    float kernel_ms = 0.f;
};

template <typename T>
hipError_t run_passes(const spal_csr *a, uint64_t s, const uint8_t *wide, T *result, T *scratch, hipStream_t st) {
    const uint32_t n = (uint32_t)a->nrows;
    const T *values = (const T *)a->d_values;
    const T *prev = values;   // pass 1 reads A's array as F0
    for (uint64_t t = 1; t <= s; ++t) {
        T *out = (s - t) % 2 == 0 ? result : scratch;   // the last pass lands in the result
        const Pass<T> p{a->d_rowptr, a->d_colind, a->d_sweep_rows, prev};
        hipLaunchKernelGGL((ilu_sweep_pass<T>), dim3(grid_of(n, kBlockRows)), dim3(kBlockRows), 0, st, n, p, wide, values, out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        prev = out;
    }
    return hipSuccess;
}

// Takes a->mu for the preparation and the option only; synchronises `st`.
int factor(const char *fn, spal_csr *a, uint64_t requested, hipStream_t st, SweepFactor &out) {
    // row blocks, not square, a row without a diagonal: refused here, in ilu0's words
    SPAL_TRY(trsv_sweep_prepare(fn, a, 0, st));
    {
        std::lock_guard<std::mutex> lock(a->mu);
        out.wide_work = a->ilu_wide_work;
    }
    const uint64_t n = a->nrows, nnz = a->nnz;
    const size_t es = (size_t)a->elem_size;
    const uint64_t s = std::min<uint64_t>(requested, n ? n - 1 : 0);   // beyond n - 1 no bit changes
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(1));
    OpArrays &f = out.f;
    SPAL_TRY(f.alloc(n, nnz, es, st));
    SPAL_HIP_TRY(hipMemcpyAsync(f.ptr, a->d_rowptr, (n + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (nnz) SPAL_HIP_TRY(hipMemcpyAsync(f.ind, a->d_colind, nnz * 4, hipMemcpyDeviceToDevice, st));
    // one block: [the other side of the ping-pong, s >= 2][wide flags][their count]
    const size_t val_bytes = s >= 2 ? ((nnz * es + 255) & ~(size_t)255) : 0;
    const size_t flag_bytes = (n + 255) & ~(size_t)255;
    StreamScratch w;
    uint32_t nwide = 0;
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    if (s == 0) {
        if (nnz) SPAL_HIP_TRY(hipMemcpyAsync(f.val, a->d_values, nnz * es, hipMemcpyDeviceToDevice, st));
    } else {
        SPAL_HIP_TRY(w.alloc(val_bytes + flag_bytes + 256, st));
        uint8_t *wide = (uint8_t *)w.p + val_bytes;
        uint32_t *count = (uint32_t *)(wide + flag_bytes);
        SPAL_HIP_TRY(hipMemsetAsync(count, 0, 4, st));
        hipLaunchKernelGGL(ilu_sweep_classify, dim3(grid_of(n, 256)), dim3(256), 0, st, (uint32_t)n, a->d_rowptr, a->d_colind,
                           a->d_sweep_rows, (uint64_t)out.wide_work, wide, count);
        SPAL_HIP_TRY(hipGetLastError());
        const hipError_t e = es == 8 ? run_passes<double>(a, s, wide, (double *)f.val, (double *)w.p, st)
                                     : run_passes<float>(a, s, wide, (float *)f.val, (float *)w.p, st);
        if (e != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
        SPAL_HIP_TRY(hipMemcpyAsync(&nwide, count, 4, hipMemcpyDeviceToHost, st));
    }
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    SPAL_HIP_TRY(ev.span(0, &out.kernel_ms));
    out.sweeps = s;
    out.requested = requested;
    out.rows_wide = nwide;
    out.rows_row = n - nwide;
    return SPAL_OK;
}

std::string info_json(const SweepFactor &r, double call_ms) {
    char buf[512];
    snprintf(buf, sizeof buf,
             "{\"sweeps\": %llu, \"requested\": %llu, \"launches\": %llu, \"block_rows\": %d, \"stage_entries\": %u, "
             "\"wide_stage_entries\": %u, \"rows_row_form\": %llu, \"rows_wide_form\": %llu, \"wide_work\": %lld, "
             "\"kernel_ms\": %.4f, \"call_ms\": %.3f}",
             (unsigned long long)r.sweeps, (unsigned long long)r.requested, (unsigned long long)r.sweeps, kBlockRows, kStage,
             kWideStage, (unsigned long long)r.rows_row, (unsigned long long)r.rows_wide, (long long)r.wide_work,
             (double)r.kernel_ms, call_ms);
    return buf;
}

// what both entry points end with: a handle of a's type around `arrays` (the factor, by rows or by columns); nobody
// multiplies by L\U, so the product plan is left to whoever asks for one, and no solve plan is handed over
template <typename H>
int adopt_factor(const H *a, OpArrays &arrays, const SweepFactor &r, std::chrono::steady_clock::time_point t0, H **out) {
    SPAL_TRY(arrays.adopt(a->device, a->elem_size, a->nrows, a->ncols, out, false, true));
    (*out)->ops.ilu_sweep_info = info_json(r, ms_since(t0));
    return SPAL_OK;
}

}  // namespace
}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_ilu0_sweep(spal_csr_t a, uint64_t sweeps, void *stream, spal_csr_t *out) {
    const char *fn = "spal_csr_ilu0_sweep";
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const auto t0 = std::chrono::steady_clock::now();
    SweepFactor r;
    SPAL_TRY(factor(fn, a, sweeps, (hipStream_t)stream, r));
    return adopt_factor(a, r.f, r, t0, out);
}

int spal_csc_ilu0_sweep(spal_csc_t a, uint64_t sweeps, void *stream, spal_csc_t *out) {
    const char *fn = "spal_csc_ilu0_sweep";
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t st = (hipStream_t)stream;
    SweepFactor r;
    SPAL_TRY(factor(fn, a->as_csr, sweeps, st, r));   // the same matrix as CSR
    // the factor by columns (the existing transpose path), then a CSC handle around it
    OpArrays bycol;
    SPAL_TRY(transpose_device(a->device, a->elem_size, a->nrows, a->ncols, a->nnz, r.f.ptr, r.f.ind, r.f.val, st, bycol));
    return adopt_factor(a, bycol, r, t0, out);
}

}  // extern "C"
