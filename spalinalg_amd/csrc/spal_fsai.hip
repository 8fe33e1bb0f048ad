// spal_fsai.hip -- FSAI on the device: G ~ L^-1 on a prescribed lower-triangular pattern, M^-1 = Gt * G,
// applied by two SpMVs on planned handles.  The text is in include/spal.h; its Cholesky and back-substitution on one
// local system are fsai_host.hpp, which spal_fsai_row_* run on the host.
//
// SETUP, ORDERED BY THE STREAM ALONE (no flags, no spins, nothing another workgroup waits on):
//   count     a thread per row of the pattern S: the entries with column <= row (S's columns ascend: a bisection), the
//             first row without a stored diagonal (atomicMin), the rows of the wave form, the capped rows, the largest m;
//   scan      scan_exclusive over the counts: G's row offsets;
//   fill      G's columns, and the list of the rows the wave form takes (appended in any order, one atomic per wave);
//   factor    TWO FORMS, chosen per row by m = min(|Q|, cap), both returning the text's bits:
//             thread form, m <= kThreadMax: a thread per row.  The local system sits at the END of a kThreadMax x
//               kThreadMax triangle held in registers (every index is a constant after unrolling); the unused leading
//               part contributes products 0 * 0 = +0.0, and d - (+0.0) = d for every d, so the bits are the text's;
//             wave form, larger m: a workgroup of ONE wave per listed row.  B / C are a packed lower triangle in LDS (at
//               most 64 * 65 / 2 values).  A lane gathers one element of B at a time (a bisection in row P[s] of A), 64
//               side by side.  For column j lane r owns C[r, j] and runs its k loop in the text's order;
//               the pivot reaches every lane by one __shfl, so rejection is uniform.  The back-substitution has lane t
//               run the u loop of g[t], t descending, with a barrier between two t.
//   transpose Gt by transpose_device: the CSC arrays of G are the CSR arrays of Gt, values moved bit for bit;
//   plans     both factors are adopted as CSR handles and planned, so the first application pays nothing.
// APPLY: spmv(G, v) -> u, spmv(Gt, u) -> out through the handles' own entry points; no lock is held across a product.
#define SPAL_OPS_SCAN
#include "fsai_host.hpp"
#include "spal_ops.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr int kThreads = 256;       // rows of a workgroup in the count, fill and thread-form launches ("block_rows")
constexpr int kThreadMax = 8;       // the largest m of the thread form ("thread_form_max"): DESIGN 3.30 records the scratch read
constexpr int kWaveMax = (int)kFsaiCapMax;
constexpr int kTri = kWaveMax * (kWaveMax + 1) / 2;

struct Stats {
    uint32_t missing;    // the first pattern row without a stored diagonal (n: none)
    uint32_t nwave;      // rows of the wave form
    uint32_t capped;     // rows with more than cap entries
    uint32_t max_row;    // the largest m
    uint32_t listed;     // the fill's cursor into the wave list
    uint32_t rejected;
};

template <typename T>
__device__ __forceinline__ bool finite_of(T x) {
    return (x - x) == T(0);   // inf - inf and NaN - NaN are NaN
}
template <typename T>
__device__ __forceinline__ T reject_diag(T aii) {
    if (aii > T(0) && finite_of(aii)) {
        const T d = T(1) / sqrt(aii);
        if (finite_of(d)) return d;
    }
    return T(1);
}

// the stored entry (row, col) of A at or after position q of the row, +0.0 where there is none; *q = where to resume
template <typename T>
__device__ __forceinline__ T entry_of(const uint32_t *__restrict__ ind, const T *__restrict__ val, uint32_t *q, uint32_t e,
                                      uint32_t col) {
    uint32_t lo = *q, hi = e;
    while (lo < hi) {   // the first entry with column >= col
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ind[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    *q = lo;
    return (lo < e && ind[lo] == col) ? val[lo] : T(0);
}

// ---- structure ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_count(const uint32_t *__restrict__ sptr, const uint32_t *__restrict__ sind,
                                                    uint32_t n, uint32_t cap, uint32_t *__restrict__ cnt, Stats *stats) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool wave = false, capped = false;
    uint32_t m = 0;
    if (i64 < n) {
        const uint32_t i = (uint32_t)i64, s = sptr[i], e = sptr[i + 1];
        uint32_t lo = s, hi = e;
        while (lo < hi) {   // the first entry with column > i
            const uint32_t mid = lo + (hi - lo) / 2;
            if (sind[mid] <= i) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t c = lo - s;
        cnt[i] = c;
        if (c == 0 || sind[lo - 1] != i) atomicMin(&stats->missing, i);
        m = min(c, cap);
        capped = c > cap;
        wave = m > (uint32_t)kThreadMax;
    } else if (i64 == n) {
        cnt[n] = 0;   // closes the scan
    }
    const unsigned long long mw = __ballot(wave), mc = __ballot(capped);
    if ((threadIdx.x & 63) == 0) {
        if (mw) atomicAdd(&stats->nwave, (uint32_t)__popcll(mw));
        if (mc) atomicAdd(&stats->capped, (uint32_t)__popcll(mc));
    }
    if (m > __atomic_load_n(&stats->max_row, __ATOMIC_RELAXED)) atomicMax(&stats->max_row, m);
}

__global__ __launch_bounds__(kThreads) void k_fill(const uint32_t *__restrict__ sptr, const uint32_t *__restrict__ sind,
                                                   const uint32_t *__restrict__ gptr, uint32_t n, uint32_t cap,
                                                   uint32_t *__restrict__ gind, uint32_t *__restrict__ list, Stats *stats) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool wave = false;
    if (i64 < n) {
        const uint32_t i = (uint32_t)i64, s = sptr[i], g0 = gptr[i], c = gptr[i + 1] - g0;
        for (uint32_t k = 0; k < c; ++k) gind[g0 + k] = sind[s + k];
        wave = min(c, cap) > (uint32_t)kThreadMax;
    }
    const unsigned long long mw = __ballot(wave);   // appended in any order: one atomic per wave
    if (mw) {
        const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll(mw) - 1;
        uint32_t at = 0;
        if (lane == leader) at = atomicAdd(&stats->listed, (uint32_t)__popcll(mw));
        at = __shfl(at, (int)leader, 64);
        if (wave) list[at + (uint32_t)__popcll(mw & ((1ull << lane) - 1))] = (uint32_t)i64;
    }
}

// ---- the factor kernel: thread form ------------------------------------------------------------------------------------
constexpr int tri(int r, int c) { return r * (r + 1) / 2 + c; }

template <typename T>
__global__ __launch_bounds__(kThreads) void k_factor_thread(const uint32_t *__restrict__ aptr, const uint32_t *__restrict__ aind,
                                                            const T *__restrict__ aval, const uint32_t *__restrict__ gptr,
                                                            const uint32_t *__restrict__ gind, T *__restrict__ gval, uint32_t n,
                                                            uint32_t cap, Stats *stats) {
    constexpr int M = kThreadMax;
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t g0 = gptr[i64], g1 = gptr[i64 + 1];
    const uint32_t m = min(g1 - g0, cap);
    if (m > (uint32_t)M || m == 0) return;   // the wave form's row (m == 0: a row without a diagonal, refused by the host)
    const uint32_t p0 = g1 - m;              // P = gind[p0, g1)
    for (uint32_t q = g0; q < p0; ++q) gval[q] = T(0);
    const int off = M - (int)m;              // the local system is rows / columns off .. M - 1 of the triangle
    uint32_t P[M];
    T C[M * (M + 1) / 2], g[M];
#pragma unroll
    for (int s = 0; s < M; ++s) P[s] = s >= off ? gind[p0 + (uint32_t)(s - off)] : 0u;
#pragma unroll
    for (int s = 0; s < M; ++s) {
        uint32_t q = 0, e = 0;
        if (s >= off) {
            q = aptr[P[s]];
            e = aptr[P[s] + 1];
        }
#pragma unroll
        for (int t = 0; t <= s; ++t) C[tri(s, t)] = (s >= off && t >= off) ? entry_of<T>(aind, aval, &q, e, P[t]) : T(0);
    }
    const T aii = C[tri(M - 1, M - 1)];
    bool rejected = false;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        if (j < off) continue;
        T d = C[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - (C[tri(j, k)] * C[tri(j, k)]);
        if (!(d > T(0) && finite_of(d))) rejected = true;
        const T cjj = sqrt(d);
        C[tri(j, j)] = cjj;
#pragma unroll
        for (int r = j + 1; r < M; ++r) {
            T t = C[tri(r, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - (C[tri(r, k)] * C[tri(j, k)]);
            C[tri(r, j)] = t / cjj;
        }
    }
    g[M - 1] = T(1) / C[tri(M - 1, M - 1)];
#pragma unroll
    for (int t = M - 2; t >= 0; --t) {
        T s = T(0);
#pragma unroll
        for (int u = t + 1; u < M; ++u) s = s + (C[tri(u, t)] * g[u]);
        g[t] = (T(0) - s) / C[tri(t, t)];
    }
#pragma unroll
    for (int t = 0; t < M; ++t)
        if (t >= off && !finite_of(g[t])) rejected = true;
    if (rejected) atomicAdd(&stats->rejected, 1u);
    const T gd = rejected ? reject_diag<T>(aii) : g[M - 1];
#pragma unroll
    for (int t = 0; t < M - 1; ++t)
        if (t >= off) gval[p0 + (uint32_t)(t - off)] = rejected ? T(0) : g[t];
    gval[g1 - 1] = gd;
}

// ---- the factor kernel: wave form, one workgroup of one wave per listed row --------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_factor_wave(const uint32_t *__restrict__ aptr, const uint32_t *__restrict__ aind,
                                                    const T *__restrict__ aval, const uint32_t *__restrict__ gptr,
                                                    const uint32_t *__restrict__ gind, T *__restrict__ gval,
                                                    const uint32_t *__restrict__ list, uint32_t cap, Stats *stats) {
    __shared__ T C[kTri];
    __shared__ T gl[kWaveMax];
    __shared__ uint32_t P[kWaveMax];
    const uint32_t lane = threadIdx.x, i = list[blockIdx.x];
    const uint32_t g0 = gptr[i], g1 = gptr[i + 1];
    const uint32_t m = min(min(g1 - g0, cap), (uint32_t)kWaveMax);   // (cap <= 64: the last min changes nothing)
    const uint32_t p0 = g1 - m;
    for (uint32_t q = g0 + lane; q < p0; q += 64) gval[q] = T(0);
    if (lane < m) P[lane] = gind[p0 + lane];
    __syncthreads();
    // B: a lane per packed element (s, t), 64 bisections side by side.  (A lane per ROW of B, resuming its bisection
    // from entry to entry -- a chain of up to m dependent searches per lane -- measured 10.7 ms against 7.0 ms for the
    // whole kernel at m = 13 on 1M rows in f64, and 30.7 against 25.2 ms at m = 32: DESIGN 3.30.)
    for (uint32_t p = lane; p < m * (m + 1) / 2; p += 64) {
        uint32_t s = (uint32_t)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);   // p < 2080: off by one at most
        while (s * (s + 1) / 2 > p) --s;
        while ((s + 1) * (s + 2) / 2 <= p) ++s;
        const uint32_t t = p - s * (s + 1) / 2;
        uint32_t q = aptr[P[s]];
        C[p] = entry_of<T>(aind, aval, &q, aptr[P[s] + 1], P[t]);
    }
    __syncthreads();
    const T aii = C[(m - 1) * m / 2 + (m - 1)];
    bool rejected = false;
    const uint32_t rowbase = lane * (lane + 1) / 2;
    for (uint32_t j = 0; j < m; ++j) {   // uniform trips: m is the wave's
        T acc = T(0);
        if (lane >= j && lane < m) {
            acc = C[rowbase + j];
            const uint32_t jb = j * (j + 1) / 2;
            for (uint32_t k = 0; k < j; ++k) acc = acc - (C[rowbase + k] * C[jb + k]);
        }
        const T d = __shfl(acc, (int)j, 64);
        if (!(d > T(0) && finite_of(d))) {   // the same d in every lane
            rejected = true;
            break;
        }
        const T cjj = sqrt(d);
        if (lane >= j && lane < m) C[rowbase + j] = lane == j ? cjj : acc / cjj;
        __syncthreads();
    }
    if (!rejected) {
        T gt = T(0);
        for (uint32_t t = m; t-- > 0;) {
            if (lane == t) {
                if (t == m - 1) {
                    gt = T(1) / C[rowbase + t];
                } else {
                    T s = T(0);
                    for (uint32_t u = t + 1; u < m; ++u) s = s + (C[u * (u + 1) / 2 + t] * gl[u]);
                    gt = (T(0) - s) / C[rowbase + t];
                }
                gl[t] = gt;
            }
            __syncthreads();
        }
        rejected = __ballot(lane < m && !finite_of(gt)) != 0;
        if (!rejected && lane < m) gval[p0 + lane] = gt;
    }
    if (rejected) {
        if (lane == 0) atomicAdd(&stats->rejected, 1u);
        if (lane < m) gval[p0 + lane] = lane == m - 1 ? reject_diag<T>(aii) : T(0);
    }
}

}  // namespace
}  // namespace spal

struct spal_fsai {
    int device = 0, elem_size = 8;
    uint64_t n = 0, nnz = 0;
    int64_t cap = spal::kFsaiCapDefault;
    spal::Stats stats{};
    spal_csr *g = nullptr, *gt = nullptr;   // G and its transpose, planned
    double setup_ms = 0.0, structure_ms = 0.0, kernel_ms = 0.0, transpose_ms = 0.0, plan_ms = 0.0;
};

namespace spal {
namespace {

void fsai_free(spal_fsai *f) {
    if (!f) return;
    csr_free(f->g);
    csr_free(f->gt);
    delete f;
}
struct FsaiOwner {
    spal_fsai *f = nullptr;
    ~FsaiOwner() { fsai_free(f); }
    spal_fsai *release() { spal_fsai *p = f; f = nullptr; return p; }
};

template <typename T>
int setup_run(const char *fn, spal_csr *a, spal_csr *s, int64_t cap, hipStream_t st, spal_fsai *f) {
    const auto t_setup = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)a->nrows;
    f->device = a->device;
    f->elem_size = a->elem_size;
    f->n = n;
    f->cap = cap;
    const dim3 block(kThreads), grid_n(std::max(1u, grid_of(n, kThreads))), grid_n1(grid_of((uint64_t)n + 1, kThreads));
    // structure
    auto t0 = std::chrono::steady_clock::now();
    DevBuf cnt, dstats, list;
    OpArrays G;
    SPAL_HIP_TRY(cnt.alloc(((size_t)n + 1) * 4));
    SPAL_HIP_TRY(dstats.alloc(sizeof(Stats)));
    SPAL_HIP_TRY(dev_alloc((void **)&G.ptr, ((size_t)n + 1) * 4));
    Stats h{};
    h.missing = n;
    SPAL_HIP_TRY(hipMemcpyAsync(dstats.p, &h, sizeof h, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_count, grid_n1, block, 0, st, (const uint32_t *)s->d_rowptr, (const uint32_t *)s->d_colind, n,
                       (uint32_t)cap, cnt.as<uint32_t>(), dstats.as<Stats>());
    SPAL_HIP_TRY(hipGetLastError());
    SPAL_HIP_TRY(scan_exclusive<uint32_t>(cnt.as<uint32_t>(), G.ptr, (uint64_t)n + 1, st));
    uint32_t nnz = 0;
    SPAL_HIP_TRY(hipMemcpyAsync(&nnz, G.ptr + n, 4, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipMemcpyAsync(&h, dstats.p, sizeof h, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    if (h.missing < n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: row %u of the pattern stores no diagonal entry (every row of G ends in it)", fn,
                    h.missing);
    f->nnz = nnz;
    G.nnz = nnz;
    G.cap = (uint64_t)nnz + kStreamPad;
    SPAL_HIP_TRY(dev_alloc((void **)&G.ind, G.cap * 4));
    SPAL_HIP_TRY(dev_alloc(&G.val, G.cap * sizeof(T)));
    SPAL_HIP_TRY(hipMemsetAsync((char *)G.ind + (size_t)nnz * 4, 0, kStreamPad * 4, st));
    SPAL_HIP_TRY(hipMemsetAsync((char *)G.val + (size_t)nnz * sizeof(T), 0, kStreamPad * sizeof(T), st));
    SPAL_HIP_TRY(list.alloc((size_t)h.nwave * 4));
    if (n) {
        hipLaunchKernelGGL(k_fill, grid_n, block, 0, st, (const uint32_t *)s->d_rowptr, (const uint32_t *)s->d_colind,
                           (const uint32_t *)G.ptr, n, (uint32_t)cap, G.ind, list.as<uint32_t>(), dstats.as<Stats>());
        SPAL_HIP_TRY(hipGetLastError());
    }
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    f->structure_ms = ms_since(t0);
    // the factor kernel, timed on the device
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(1));
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    if (n) {
        hipLaunchKernelGGL(k_factor_thread<T>, grid_n, block, 0, st, (const uint32_t *)a->d_rowptr, (const uint32_t *)a->d_colind,
                           (const T *)a->d_values, (const uint32_t *)G.ptr, (const uint32_t *)G.ind, (T *)G.val, n, (uint32_t)cap,
                           dstats.as<Stats>());
        SPAL_HIP_TRY(hipGetLastError());
    }
    if (h.nwave) {
        hipLaunchKernelGGL(k_factor_wave<T>, dim3(h.nwave), dim3(64), 0, st, (const uint32_t *)a->d_rowptr,
                           (const uint32_t *)a->d_colind, (const T *)a->d_values, (const uint32_t *)G.ptr, (const uint32_t *)G.ind,
                           (T *)G.val, (const uint32_t *)list.p, (uint32_t)cap, dstats.as<Stats>());
        SPAL_HIP_TRY(hipGetLastError());
    }
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipMemcpyAsync(&h, dstats.p, sizeof h, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    f->stats = h;
    f->kernel_ms = (double)ev.ms(1);
    // Gt: the CSC arrays of G are the CSR arrays of its transpose
    t0 = std::chrono::steady_clock::now();
    OpArrays Gt;
    SPAL_TRY(transpose_device(f->device, f->elem_size, n, n, nnz, G.ptr, G.ind, G.val, st, Gt));
    f->transpose_ms = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    SPAL_TRY(G.adopt(f->device, f->elem_size, n, n, &f->g));
    SPAL_TRY(Gt.adopt(f->device, f->elem_size, n, n, &f->gt));
    SPAL_TRY(spal_csr_plan(f->g));
    SPAL_TRY(spal_csr_plan(f->gt));
    f->plan_ms = ms_since(t0);
    f->setup_ms = ms_since(t_setup);
    return SPAL_OK;
}

template <typename H>
int setup_entry(const char *fn, H *a, H *pattern, void *stream, spal_fsai_t *out) {
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    H *s = pattern ? pattern : a;
    if (row_blocks(a) || row_blocks(s)) return refuse_row_blocks(fn);
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    if (s->nrows != a->nrows || s->ncols != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the pattern is %llu x %llu but the matrix %llu x %llu", fn,
                    (unsigned long long)s->nrows, (unsigned long long)s->ncols, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    SPAL_TRY(check_same_device_and_dtype(fn, a, s));
    spal_csr *csr = solve_handle(a), *scsr = solve_handle(s);   // a CSC handle: its CSR twin
    int64_t cap;
    {
        std::lock_guard<std::mutex> lock(csr->mu);
        cap = a->ops.fsai_max_row;
    }
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    SPAL_TRY(refuse_capture(fn, st, "the call allocates and synchronises"));
    FsaiOwner own;
    own.f = new spal_fsai;
    SPAL_TRY(a->elem_size == 8 ? setup_run<double>(fn, csr, scsr, cap, st, own.f) : setup_run<float>(fn, csr, scsr, cap, st, own.f));
    *out = own.release();
    return SPAL_OK;
}

template <typename T>
int apply_checks(const char *fn, spal_fsai *f, const T *b, const T *x) {
    if (!f) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    if (!b || !x) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null vector", fn);
    SPAL_TRY(check_dtype<T>(fn, f->elem_size));
    if (b == x) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x == b (the second product reads what the first wrote, not b)", fn);
    return SPAL_OK;
}

template <typename T>
int apply_dev(const char *fn, spal_fsai *f, const T *b, T *x, void *stream) {
    SPAL_TRY(apply_checks<T>(fn, f, b, x));
    DeviceGuard guard(f->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    StreamWork work;   // u: the stream's own scratch block
    SPAL_TRY(work.take(fn, st, (size_t)f->n * sizeof(T)));
    return fsai_apply_enqueue(fn, f, b, work.p, x, st);
}

template <typename T>
int apply_host(const char *fn, spal_fsai *f, const T *b, uint64_t b_len, T *x, uint64_t x_len) {
    SPAL_TRY(apply_checks<T>(fn, f, b, x));
    const uint64_t n = f->n;
    if (b_len != n || x_len != n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: b.len() = %llu and x.len() = %llu but the factor has %llu rows", fn,
                    (unsigned long long)b_len, (unsigned long long)x_len, (unsigned long long)n);
    DeviceGuard guard(f->device);
    if (guard.status != SPAL_OK) return guard.status;
    DevBuf db, du, dx;
    hipStream_t s = nullptr;
    SPAL_HIP_TRY(db.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(du.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(dx.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(stream_acquire(&s));
    struct Release {
        hipStream_t s;
        ~Release() { stream_release(s); }
    } release{s};
    SPAL_HIP_TRY(hipMemcpyAsync(db.p, b, n * sizeof(T), hipMemcpyHostToDevice, s));
    SPAL_TRY(fsai_apply_enqueue(fn, f, db.p, du.p, dx.p, s));
    SPAL_HIP_TRY(hipMemcpyAsync(x, dx.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
    SPAL_HIP_TRY(hipStreamSynchronize(s));
    return SPAL_OK;
}

template <typename T>
int row_entry(const char *fn, uint64_t m, const T *b_lower, T *g, int *rejected) {
    if (!b_lower || !g || !rejected) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (m < 1 || m > (uint64_t)kFsaiCapMax)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: m = %llu must be 1 .. %lld", fn, (unsigned long long)m, (long long)kFsaiCapMax);
    std::vector<T> c(b_lower, b_lower + m * (m + 1) / 2);
    *rejected = fsai_row_host<T>((size_t)m, c.data(), c.data(), g);
    return SPAL_OK;
}

}  // namespace

// ---- what spal_krylov.hip calls (spal_ops.hpp) -------------------------------------------------------------------------
int fsai_check_match(const char *fn, const spal_fsai *f, uint64_t nrows, int device, int elem_size) {
    if (!f) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument (the FSAI factor)", fn);
    if (f->device != device) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: operands on devices %d and %d", fn, device, f->device);
    if (f->elem_size != elem_size)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: operands of element sizes %d and %d", fn, elem_size, f->elem_size);
    if (f->n != nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the FSAI factor has %llu rows but the matrix %llu", fn, (unsigned long long)f->n,
                    (unsigned long long)nrows);
    return SPAL_OK;
}
int fsai_apply_enqueue(const char *fn, spal_fsai *f, const void *b, void *u, void *x, hipStream_t st) {
    (void)fn;
    if (f->elem_size == 8) {
        SPAL_TRY(spal_csr_spmv_dev_f64(f->g, (const double *)b, (double *)u, st));
        return spal_csr_spmv_dev_f64(f->gt, (const double *)u, (double *)x, st);
    }
    SPAL_TRY(spal_csr_spmv_dev_f32(f->g, (const float *)b, (float *)u, st));
    return spal_csr_spmv_dev_f32(f->gt, (const float *)u, (float *)x, st);
}

int fsai_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status) {
    if (strcmp(key, "fsai_max_row")) return 0;
    if (!fsai_cap_valid(value)) {
        *status = fail(SPAL_ERR_INVALID_ARGUMENT, "fsai_max_row must be 1 .. 64 (the largest local system of a row of G)");
        return 1;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    s.fsai_max_row = value;
    *status = SPAL_OK;
    return 1;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_fsai_setup(spal_csr_t a, spal_csr_t pattern, void *stream, spal_fsai_t *out) {
    return setup_entry("spal_csr_fsai_setup", a, pattern, stream, out);
}
int spal_csc_fsai_setup(spal_csc_t a, spal_csc_t pattern, void *stream, spal_fsai_t *out) {
    return setup_entry("spal_csc_fsai_setup", a, pattern, stream, out);
}

int spal_fsai_destroy(spal_fsai_t f) {
    if (!f) return SPAL_OK;
    DeviceGuard guard(f->device);
    fsai_free(f);
    return SPAL_OK;
}

int spal_fsai_describe(spal_fsai_t f, char *buf, size_t buf_len) {
    const char *fn = "spal_fsai_describe";
    if (!f || !buf || !buf_len) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    char tmp[768];
    const int len = snprintf(
        tmp, sizeof tmp,
        "{\"dtype\": \"%s\", \"rows\": %llu, \"nnz\": %llu, \"cap\": %lld, \"max_row\": %u, \"capped_rows\": %u, \"rejected\": %u, "
        "\"rows_thread_form\": %llu, \"rows_wave_form\": %u, \"block_rows\": %d, \"thread_form_max\": %d, \"setup_ms\": %.4f, "
        "\"structure_ms\": %.4f, \"kernel_ms\": %.4f, \"transpose_ms\": %.4f, \"plan_ms\": %.4f}",
        f->elem_size == 8 ? "f64" : "f32", (unsigned long long)f->n, (unsigned long long)f->nnz, (long long)f->cap, f->stats.max_row,
        f->stats.capped, f->stats.rejected, (unsigned long long)(f->n - f->stats.nwave), f->stats.nwave, kThreads, kThreadMax,
        f->setup_ms, f->structure_ms, f->kernel_ms, f->transpose_ms, f->plan_ms);
    if (len < 0 || (size_t)len + 1 > buf_len || (size_t)len + 1 > sizeof tmp)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the buffer holds %zu bytes, %d are needed", fn, buf_len, len + 1);
    memcpy(buf, tmp, (size_t)len + 1);
    return SPAL_OK;
}

int spal_fsai_factor_csr(spal_fsai_t f, int transposed, spal_csr_t *copy) {
    const char *fn = "spal_fsai_factor_csr";
    if (!f || !copy) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *copy = nullptr;
    if (transposed != 0 && transposed != 1)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: transposed = %d must be 0 (G) or 1 (Gt)", fn, transposed);
    DeviceGuard guard(f->device);
    if (guard.status != SPAL_OK) return guard.status;
    const spal_csr *src = transposed ? f->gt : f->g;
    OpArrays o;
    SPAL_TRY(o.alloc(f->n, f->nnz, (size_t)f->elem_size, nullptr));
    SPAL_HIP_TRY(hipMemcpyAsync(o.ptr, src->d_rowptr, ((size_t)f->n + 1) * 4, hipMemcpyDeviceToDevice, nullptr));
    if (f->nnz) {
        SPAL_HIP_TRY(hipMemcpyAsync(o.ind, src->d_colind, (size_t)f->nnz * 4, hipMemcpyDeviceToDevice, nullptr));
        SPAL_HIP_TRY(hipMemcpyAsync(o.val, src->d_values, (size_t)f->nnz * f->elem_size, hipMemcpyDeviceToDevice, nullptr));
    }
    SPAL_HIP_TRY(hipStreamSynchronize(nullptr));
    return o.adopt(f->device, f->elem_size, f->n, f->n, copy);
}

int spal_fsai_apply_f64(spal_fsai_t f, const double *b, uint64_t b_len, double *x, uint64_t x_len) {
    return apply_host<double>("spal_fsai_apply", f, b, b_len, x, x_len);
}
int spal_fsai_apply_f32(spal_fsai_t f, const float *b, uint64_t b_len, float *x, uint64_t x_len) {
    return apply_host<float>("spal_fsai_apply", f, b, b_len, x, x_len);
}
int spal_fsai_apply_dev_f64(spal_fsai_t f, const double *b_dev, double *x_dev, void *stream) {
    return apply_dev<double>("spal_fsai_apply_dev", f, b_dev, x_dev, stream);
}
int spal_fsai_apply_dev_f32(spal_fsai_t f, const float *b_dev, float *x_dev, void *stream) {
    return apply_dev<float>("spal_fsai_apply_dev", f, b_dev, x_dev, stream);
}

int spal_fsai_row_f64(uint64_t m, const double *b_lower, double *g, int *rejected) {
    return row_entry<double>("spal_fsai_row", m, b_lower, g, rejected);
}
int spal_fsai_row_f32(uint64_t m, const float *b_lower, float *g, int *rejected) {
    return row_entry<float>("spal_fsai_row", m, b_lower, g, rejected);
}

}  // extern "C"
