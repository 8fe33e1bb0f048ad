// spal_cheb.hip -- the Chebyshev filter's device half: one recurrence step per launch,
//     out[r] = (alpha * (rowsum(y, r) - (cT * y[r]))) - (beta * x[r]),
// the same kernel without the epilogue (q = rowsum(x): filtered eigsh's true residuals), Gershgorin's enclosure, and the
// entry points spal_*_cheb_apply_* and spal_*_gershgorin.  The contract is the sequential text in include/spal.h: rowsum
// adds a row's rounded products in storage order onto +0.0, whatever the handle's plan is.
//
// THE STEP STREAMS THE MATRIX.  A workgroup of 256 threads owns 256 consecutive rows, a thread one row.  The rows' entries
// are one contiguous range of `values` / `colind`; the workgroup walks it in chunks (16 KiB of products: 2048 f64 or 4096
// f32 entries).  Per chunk every lane loads its entries' values and columns COALESCED (non-temporal: the matrix is read
// once per launch and should not push y out of the caches), gathers y, and writes the ROUNDED product to LDS; after a
// barrier each thread adds the products of its own row that lie in the chunk, in order, onto an accumulator that it
// carries from chunk to chunk.  So a row of any length, across any number of chunk boundaries, is the text's sum.  A
// thread per row reading its own entries from global memory (spal_amg.hip's k_step) makes a wave touch 64 rows x 14
// entries scattered over 7 KiB for every load; here every global load of the matrix is a whole line.
//   * 16 KiB of LDS and 256 threads: eight workgroups per CU (128 of 160 KiB, 32 waves), the CU's wave limit.
//   * NO LONG-ROW ROUTE: spal_amg.hip's ordered_sum hands a long row to its wave so that 64 products are FORMED in
//     parallel; its additions stay one chain through readlane.  Here all products of a chunk are formed by 256 lanes
//     whatever the rows' lengths are, and the owner's chain of additions reads LDS instead: the same serial work, no
//     second path, no threshold.
//   * The d launches of a filter application are ordered by the stream alone, the coefficients are kernel arguments,
//     nothing waits on another workgroup and nothing is polled.
//   * `out` may be `x` (a thread reads x[r] before it writes out[r], and nobody else touches element r) but never `y`,
//     which other workgroups gather.  cheb_apply_enqueue rotates two buffers on that: t_i overwrites t_{i-2}.
// Option "cheb_chunk" on `a`: entries per chunk (0 = the default above, else 256, 512, 1024, 2048 or 4096).  It moves
// the chunk boundaries and nothing else: the bits do not depend on it.
//
// THE SERIES: s = sum_i k_i t_i over the unscaled recurrence, spal_*_cheb_series_*, is the same step with the
// accumulation in its epilogue (cheb_series_step), d launches for degree d; spal_cheb_delta_coefficients is host only.
// Option "cheb_series_form" on `a`: 0 = automatic = 1 = that fused step; 2 = the recurrence step and a separate
// accumulation launch, the same bits (DESIGN 3.28 measured the fused form faster on both bench matrices).
#include "krylov_kernels.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr int kChebThreads = 256;          // = the rows of a workgroup
constexpr unsigned kChebChunkBytes = 16 * 1024;
constexpr unsigned kChebLoads = 4;         // entries a lane has in flight per batch

enum ChebMode { CHEB_PLAIN = 0, CHEB_FIRST = 1, CHEB_STEP = 2 };

// rowsum(y, row) of the workgroup's 256 rows, row = blockIdx.x * 256 + threadIdx.x (+0.0 for a row >= n): the streaming
// walk described above.  Every thread of the workgroup calls it (it holds barriers).
template <typename T>
__device__ __forceinline__ T cheb_rowsum(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ ind,
                                         const T *__restrict__ val, uint64_t n, const T *y, uint32_t chunk, T *prod) {
    const uint32_t t = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * kChebThreads, row = row0 + t;
    const uint64_t rend = row0 + kChebThreads < n ? row0 + kChebThreads : n;
    const uint32_t e0 = ptr[row0], e1 = ptr[rend];      // row0 < n: the grid has ceil(n / 256) workgroups
    uint32_t s = 0, e = 0;
    if (row < n) {
        s = ptr[row];
        e = ptr[row + 1];
    }
    T acc = T(0);
    for (uint32_t c0 = e0; c0 < e1; c0 += chunk) {      // uniform in the workgroup; c0 + chunk < 2^32 (kMaxEntries)
        const uint32_t cend = e1 - c0 < chunk ? e1 : c0 + chunk;
        for (uint32_t q0 = c0 + t; q0 < cend; q0 += kChebLoads * kChebThreads) {
            T a[kChebLoads], g[kChebLoads];
            uint32_t col[kChebLoads];
#pragma unroll
            for (unsigned u = 0; u < kChebLoads; ++u) {
                const uint32_t q = q0 + u * kChebThreads;
                if (q < cend) {
                    a[u] = __builtin_nontemporal_load(val + q);
                    col[u] = __builtin_nontemporal_load(ind + q);
                }
            }
#pragma unroll
            for (unsigned u = 0; u < kChebLoads; ++u)
                if (q0 + u * kChebThreads < cend) g[u] = y[col[u]];
#pragma unroll
            for (unsigned u = 0; u < kChebLoads; ++u) {
                const uint32_t q = q0 + u * kChebThreads;
                if (q < cend) prod[q - c0] = a[u] * g[u];
            }
        }
        __syncthreads();
        const uint32_t lo = s > c0 ? s : c0, hi = e < cend ? e : cend;
        for (uint32_t q = lo; q < hi; ++q) acc = acc + prod[q - c0];
        __syncthreads();
    }
    return acc;
}

// MODE PLAIN: out[r] = rowsum(y, r).  FIRST: out[r] = alpha * (rowsum(y, r) - (cT * y[r])).  STEP: the full step.
// The variants are separate code, not arguments: beta = 0 would turn a -0.0 into +0.0 and 0 * inf into NaN.
template <typename T, int MODE>
__global__ __launch_bounds__(kChebThreads) void cheb_step(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ ind,
                                                          const T *__restrict__ val, uint64_t n, const T *y, const T *x, T *out,
                                                          T alpha, T beta, T cT, uint32_t chunk) {
    extern __shared__ __align__(16) unsigned char cheb_raw[];
    const T acc = cheb_rowsum<T>(ptr, ind, val, n, y, chunk, reinterpret_cast<T *>(cheb_raw));
    const uint64_t row = (uint64_t)blockIdx.x * kChebThreads + threadIdx.x;
    if (row >= n) return;
    if (MODE == CHEB_PLAIN) {
        out[row] = acc;
    } else if (MODE == CHEB_FIRST) {
        out[row] = alpha * (acc - (cT * y[row]));
    } else {
        out[row] = (alpha * (acc - (cT * y[row]))) - (beta * x[row]);
    }
}

// THE SERIES STEP: the step above on the UNSCALED recurrence, with the accumulation s += k_i * t_i in its
// epilogue -- the row's thread holds t_i[r], so the series costs one read and one write of s[r] more per step and no
// launch of its own.  FIRST: t[r] = a * (rowsum(y, r) - (cT*y[r])) and s[r] = (k0*y[r]) + (k*t[r]).  STEP: t[r] =
// (a * (rowsum(y, r) - (cT*y[r]))) - x[r] and s[r] = s[r] + (k*t[r]).  Separate kernels from cheb_step, whose
// instantiations and launches stay what they were.  `t` may be `x`, as out may above; s is touched by its row's thread alone.
enum ChebSeriesMode { SERIES_FIRST = 0, SERIES_STEP = 1 };

template <typename T, int MODE>
__global__ __launch_bounds__(kChebThreads) void cheb_series_step(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ ind,
                                                                 const T *__restrict__ val, uint64_t n, const T *y, const T *x, T *t,
                                                                 T *s, T a, T cT, T k0, T k, uint32_t chunk) {
    extern __shared__ __align__(16) unsigned char cheb_raw[];
    const T acc = cheb_rowsum<T>(ptr, ind, val, n, y, chunk, reinterpret_cast<T *>(cheb_raw));
    const uint64_t row = (uint64_t)blockIdx.x * kChebThreads + threadIdx.x;
    if (row >= n) return;
    if (MODE == SERIES_FIRST) {
        const T yr = y[row];
        const T ti = a * (acc - (cT * yr));
        t[row] = ti;
        s[row] = (k0 * yr) + (k * ti);
    } else {
        const T ti = (a * (acc - (cT * y[row]))) - x[row];
        t[row] = ti;
        s[row] = s[row] + (k * ti);
    }
}

// The unfused form's accumulation: s[r] = (k0 * x[r]) + (k * t[r]) when FIRST, else s[r] = s[r] + (k * t[r]).
template <typename T, bool FIRST>
__global__ __launch_bounds__(kChebThreads) void cheb_series_accumulate(uint64_t n, const T *x, const T *t, T *s, T k0, T k) {
    const uint64_t row = (uint64_t)blockIdx.x * kChebThreads + threadIdx.x;
    if (row >= n) return;
    s[row] = FIRST ? (k0 * x[row]) + (k * t[row]) : s[row] + (k * t[row]);
}

// Gershgorin: per row d = the stored diagonal (0 without one), sum = the |off-diagonal entries| in storage order onto
// +0.0, in double; part[2 * block] = the block's min(d - sum), part[2 * block + 1] = its max(d + sum); *bad != 0 when a
// row's value is not finite.  min and max do not depend on the order they are taken in.
template <typename T>
__global__ __launch_bounds__(kChebThreads) void gershgorin_rows(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ ind,
                                                               const T *__restrict__ val, uint64_t n, double *part, unsigned *bad) {
    __shared__ double lo_s[kChebThreads], hi_s[kChebThreads];
    const unsigned t = threadIdx.x;
    const uint64_t row = (uint64_t)blockIdx.x * kChebThreads + t;
    double lo = INFINITY, hi = -INFINITY;
    if (row < n) {
        double d = 0.0, sum = 0.0;
        for (uint32_t q = ptr[row], e = ptr[row + 1]; q < e; ++q) {
            const double v = (double)val[q];
            if (ind[q] == row) d = v;
            else sum = sum + fabs(v);
        }
        lo = d - sum;
        hi = d + sum;
        if (!isfinite(lo) || !isfinite(hi)) atomicOr(bad, 1u);
    }
    lo_s[t] = lo;
    hi_s[t] = hi;
    __syncthreads();
    for (unsigned h = kChebThreads / 2; h >= 1; h >>= 1) {
        if (t < h) {
            lo_s[t] = fmin(lo_s[t], lo_s[t + h]);
            hi_s[t] = fmax(hi_s[t], hi_s[t + h]);
        }
        __syncthreads();
    }
    if (t == 0) {
        part[2 * (uint64_t)blockIdx.x] = lo_s[0];
        part[2 * (uint64_t)blockIdx.x + 1] = hi_s[0];
    }
}

unsigned chunk_entries(unsigned option, size_t elem) { return option ? option : (unsigned)(kChebChunkBytes / elem); }

template <typename T, int MODE>
int launch_step(const char *fn, const spal_csr *a, const T *y, const T *x, T *out, T alpha, T beta, T cT, unsigned chunk_opt,
                hipStream_t st) {
    if (a->nrows == 0) return SPAL_OK;
    const unsigned chunk = chunk_entries(chunk_opt, sizeof(T));
    hipLaunchKernelGGL((cheb_step<T, MODE>), dim3(grid_of(a->nrows, kChebThreads)), dim3(kChebThreads), (size_t)chunk * sizeof(T), st,
                       (const uint32_t *)a->d_rowptr, (const uint32_t *)a->d_colind, (const T *)a->d_values, a->nrows, y, x, out, alpha,
                       beta, cT, chunk);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(le));
    return SPAL_OK;
}

bool overlap(const void *p, const void *q, size_t bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + bytes && b < a + bytes;
}

// ---- the refusals that need no device ----------------------------------------------------------------------------------
template <typename T, typename H>
int apply_check(const char *fn, H *a, const T *x, T *out, uint64_t degree, double lo, double hi, double a0) {
    if (!a || !x || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    const ChebRefusal r = cheb_check(degree, lo, hi, a0);
    if (r != CHEB_OK)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: %s (degree = %llu, lo = %g, hi = %g, a0 = %g)", fn, cheb_refusal_text(r),
                    (unsigned long long)degree, lo, hi, a0);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    if (row_blocks(a)) return refuse_row_blocks(fn);
    if (overlap(x, out, (size_t)std::max<uint64_t>(a->nrows, 1) * sizeof(T)))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: out overlaps x (every step gathers the previous one)", fn);
    return SPAL_OK;
}

template <typename H>
unsigned chunk_option_of(H *a) {
    std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
    return (unsigned)a->ops.cheb_chunk;
}

template <typename T, typename H>
int apply_dev(const char *fn, H *a, const T *x_dev, T *out_dev, uint64_t degree, double lo, double hi, double a0, void *stream) {
    SPAL_TRY((apply_check<T, H>(fn, a, x_dev, out_dev, degree, lo, hi, a0)));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    SPAL_TRY(refuse_capture(fn, st, "the call takes its work vector from the stream's scratch"));
    const ChebCoeffs<T> k = cheb_coefficients<T>(degree, lo, hi, a0);
    StreamWork work;
    if (degree >= 2) SPAL_TRY(work.take(fn, st, (size_t)std::max<uint64_t>(a->nrows, 1) * sizeof(T)));
    return cheb_apply_enqueue<T>(fn, solve_handle(a), k, x_dev, out_dev, work.as<T>(), chunk_option_of(a), st);
}

template <typename T, typename H>
int apply_host(const char *fn, H *a, const T *x, uint64_t x_len, T *out, uint64_t out_len, uint64_t degree, double lo, double hi,
               double a0) {
    SPAL_TRY((apply_check<T, H>(fn, a, x, out, degree, lo, hi, a0)));
    const uint64_t n = a->nrows;
    if (x_len != n || out_len != n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x.len() = %llu and out.len() = %llu but the matrix has %llu rows", fn,
                    (unsigned long long)x_len, (unsigned long long)out_len, (unsigned long long)n);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const ChebCoeffs<T> k = cheb_coefficients<T>(degree, lo, hi, a0);
    DevBuf vecs;
    PooledStream ps;
    const uint64_t stride = (n + 63) & ~(uint64_t)63;
    SPAL_HIP_TRY(vecs.alloc((size_t)std::max<uint64_t>(3 * stride, 1) * sizeof(T)));
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    T *dx = vecs.as<T>(), *dout = dx + stride, *dwork = dout + stride;
    SPAL_HIP_TRY(hipMemcpyAsync(dx, x, n * sizeof(T), hipMemcpyHostToDevice, ps.s));
    SPAL_TRY(cheb_apply_enqueue<T>(fn, solve_handle(a), k, dx, dout, dwork, chunk_option_of(a), ps.s));
    SPAL_HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(T), hipMemcpyDeviceToHost, ps.s));
    SPAL_HIP_TRY(hipStreamSynchronize(ps.s));
    return SPAL_OK;
}

// ---- the series ------------------------------------------------------------------------------------------
template <typename T, int MODE>
int launch_series_step(const char *fn, const spal_csr *a, const T *y, const T *x, T *t, T *s, T alpha, T cT, T k0, T k,
                       unsigned chunk_opt, hipStream_t st) {
    const unsigned chunk = chunk_entries(chunk_opt, sizeof(T));
    hipLaunchKernelGGL((cheb_series_step<T, MODE>), dim3(grid_of(a->nrows, kChebThreads)), dim3(kChebThreads), (size_t)chunk * sizeof(T),
                       st, (const uint32_t *)a->d_rowptr, (const uint32_t *)a->d_colind, (const T *)a->d_values, a->nrows, y, x, t, s,
                       alpha, cT, k0, k, chunk);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(le));
    return SPAL_OK;
}

template <typename T, bool FIRST>
int launch_series_accumulate(const char *fn, const spal_csr *a, const T *x, const T *t, T *s, T k0, T k, hipStream_t st) {
    hipLaunchKernelGGL((cheb_series_accumulate<T, FIRST>), dim3(grid_of(a->nrows, kChebThreads)), dim3(kChebThreads), 0, st, a->nrows, x,
                       t, s, k0, k);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(le));
    return SPAL_OK;
}

// the refusals that need no device
template <typename T, typename H>
int series_check(const char *fn, H *a, const T *x, T *out, uint64_t degree, double lo, double hi, const double *coef,
                 uint64_t coef_len) {
    if (!a || !x || !out || !coef) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    const ChebSeriesRefusal r = cheb_series_check(degree, lo, hi, coef, coef_len);
    if (r != CHEB_SERIES_OK)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: %s (degree = %llu, coef_len = %llu, lo = %g, hi = %g)", fn,
                    cheb_series_refusal_text(r), (unsigned long long)degree, (unsigned long long)coef_len, lo, hi);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    if (row_blocks(a)) return refuse_row_blocks(fn);
    if (overlap(x, out, (size_t)std::max<uint64_t>(a->nrows, 1) * sizeof(T)))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: out overlaps x (every step gathers the previous one)", fn);
    return SPAL_OK;
}

template <typename H>
void series_options_of(H *a, unsigned *chunk, int *form) {
    std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
    *chunk = (unsigned)a->ops.cheb_chunk;
    *form = a->ops.cheb_series_form;
}

template <typename T, typename H>
int series_dev(const char *fn, H *a, const T *x_dev, T *out_dev, uint64_t degree, double lo, double hi, const double *coef,
               uint64_t coef_len, void *stream) {
    SPAL_TRY((series_check<T, H>(fn, a, x_dev, out_dev, degree, lo, hi, coef, coef_len)));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    SPAL_TRY(refuse_capture(fn, st, "the call takes its work vectors from the stream's scratch"));
    const ChebSeries<T> k = cheb_series_scalars<T>(lo, hi, coef, coef_len);
    const uint64_t stride = (std::max<uint64_t>(a->nrows, 1) + 63) & ~(uint64_t)63;
    StreamWork work;
    SPAL_TRY(work.take(fn, st, (size_t)(2 * stride) * sizeof(T)));
    unsigned chunk = 0;
    int form = 0;
    series_options_of(a, &chunk, &form);
    return cheb_series_enqueue<T>(fn, solve_handle(a), k, x_dev, out_dev, work.as<T>(), work.as<T>() + stride, chunk, form, st);
}

template <typename T, typename H>
int series_host(const char *fn, H *a, const T *x, uint64_t x_len, T *out, uint64_t out_len, uint64_t degree, double lo, double hi,
                const double *coef, uint64_t coef_len) {
    SPAL_TRY((series_check<T, H>(fn, a, x, out, degree, lo, hi, coef, coef_len)));
    const uint64_t n = a->nrows;
    if (x_len != n || out_len != n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x.len() = %llu and out.len() = %llu but the matrix has %llu rows", fn,
                    (unsigned long long)x_len, (unsigned long long)out_len, (unsigned long long)n);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const ChebSeries<T> k = cheb_series_scalars<T>(lo, hi, coef, coef_len);
    DevBuf vecs;
    PooledStream ps;
    const uint64_t stride = (n + 63) & ~(uint64_t)63;
    SPAL_HIP_TRY(vecs.alloc((size_t)std::max<uint64_t>(4 * stride, 1) * sizeof(T)));
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    T *dx = vecs.as<T>(), *dout = dx + stride, *dw1 = dout + stride, *dw2 = dw1 + stride;
    unsigned chunk = 0;
    int form = 0;
    series_options_of(a, &chunk, &form);
    SPAL_HIP_TRY(hipMemcpyAsync(dx, x, n * sizeof(T), hipMemcpyHostToDevice, ps.s));
    SPAL_TRY(cheb_series_enqueue<T>(fn, solve_handle(a), k, dx, dout, dw1, dw2, chunk, form, ps.s));
    SPAL_HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(T), hipMemcpyDeviceToHost, ps.s));
    SPAL_HIP_TRY(hipStreamSynchronize(ps.s));
    return SPAL_OK;
}

template <typename H>
int gershgorin_entry(const char *fn, H *a, double *glo, double *ghi) {
    if (!a || !glo || !ghi) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    if (a->nrows == 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix has no rows", fn);
    if (row_blocks(a)) return refuse_row_blocks(fn);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    PooledStream ps;
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    return gershgorin_run(fn, solve_handle(a), ps.s, glo, ghi);
}

}  // namespace

// out = rowsum(y) on `st`
template <typename T>
int cheb_rowsum_enqueue(const char *fn, spal_csr *a, const T *y, T *out, unsigned chunk, hipStream_t st) {
    return launch_step<T, CHEB_PLAIN>(fn, a, y, nullptr, out, T(0), T(0), T(0), chunk, st);
}

// out = t_d on `st`: degree launches.  t_i lands in `out` when degree - i is even and in `work` when it is odd, so t_i
// overwrites t_{i-2} (except t_2, whose t_0 is the caller's x) and t_d is in `out`.  work: n elements, unused at degree 1.
template <typename T>
int cheb_apply_enqueue(const char *fn, spal_csr *a, const ChebCoeffs<T> &k, const T *x, T *out, T *work, unsigned chunk,
                       hipStream_t st) {
    const uint64_t d = k.alpha.size();
    auto buf = [&](uint64_t i) { return (d - i) % 2 == 0 ? out : work; };
    SPAL_TRY((launch_step<T, CHEB_FIRST>(fn, a, x, nullptr, buf(1), k.alpha[0], T(0), k.cT, chunk, st)));
    for (uint64_t i = 2; i <= d; ++i)
        SPAL_TRY((launch_step<T, CHEB_STEP>(fn, a, (const T *)buf(i - 1), i == 2 ? x : (const T *)buf(i), buf(i), k.alpha[i - 1],
                                            k.beta[i - 1], k.cT, chunk, st)));
    return SPAL_OK;
}
template int cheb_rowsum_enqueue<double>(const char *, spal_csr *, const double *, double *, unsigned, hipStream_t);
template int cheb_rowsum_enqueue<float>(const char *, spal_csr *, const float *, float *, unsigned, hipStream_t);
template int cheb_apply_enqueue<double>(const char *, spal_csr *, const ChebCoeffs<double> &, const double *, double *, double *,
                                        unsigned, hipStream_t);
template int cheb_apply_enqueue<float>(const char *, spal_csr *, const ChebCoeffs<float> &, const float *, float *, float *, unsigned,
                                       hipStream_t);

// s = cheb_series(x) on `st`: d launches in the fused form (form 0 or 1), 2 d in the unfused one (form 2), the same bits.
// t_i lands in w1 for odd i and in w2 for even i, so t_i overwrites t_{i-2} (except t_2, whose t_0 is the caller's x,
// which is only read).  x, s, w1 and w2 are distinct vectors of n elements.
template <typename T>
int cheb_series_enqueue(const char *fn, spal_csr *a, const ChebSeries<T> &k, const T *x, T *s, T *w1, T *w2, unsigned chunk,
                        int form, hipStream_t st) {
    if (a->nrows == 0) return SPAL_OK;
    const uint64_t d = k.k.size() - 1;
    auto buf = [&](uint64_t i) { return i % 2 ? w1 : w2; };
    if (form == 2) {
        SPAL_TRY((launch_step<T, CHEB_FIRST>(fn, a, x, nullptr, w1, k.a1, T(0), k.cT, chunk, st)));
        SPAL_TRY((launch_series_accumulate<T, true>(fn, a, x, (const T *)w1, s, k.k[0], k.k[1], st)));
        for (uint64_t i = 2; i <= d; ++i) {
            SPAL_TRY((launch_step<T, CHEB_STEP>(fn, a, (const T *)buf(i - 1), i == 2 ? x : (const T *)buf(i), buf(i), k.a2, T(1), k.cT,
                                                chunk, st)));   // 1 * t_{i-2} is t_{i-2}: the unscaled recurrence
            SPAL_TRY((launch_series_accumulate<T, false>(fn, a, nullptr, (const T *)buf(i), s, T(0), k.k[i], st)));
        }
        return SPAL_OK;
    }
    SPAL_TRY((launch_series_step<T, SERIES_FIRST>(fn, a, x, nullptr, w1, s, k.a1, k.cT, k.k[0], k.k[1], chunk, st)));
    for (uint64_t i = 2; i <= d; ++i)
        SPAL_TRY((launch_series_step<T, SERIES_STEP>(fn, a, (const T *)buf(i - 1), i == 2 ? x : (const T *)buf(i), buf(i), s, k.a2, k.cT,
                                                     T(0), k.k[i], chunk, st)));
    return SPAL_OK;
}
template int cheb_series_enqueue<double>(const char *, spal_csr *, const ChebSeries<double> &, const double *, double *, double *,
                                         double *, unsigned, int, hipStream_t);
template int cheb_series_enqueue<float>(const char *, spal_csr *, const ChebSeries<float> &, const float *, float *, float *, float *,
                                        unsigned, int, hipStream_t);

// (glo, ghi) of a square matrix with rows; synchronises `st`.  Both are NaN when a row's value is not finite.
int gershgorin_run(const char *fn, spal_csr *a, hipStream_t st, double *glo, double *ghi) {
    const uint64_t n = a->nrows;
    const unsigned blocks = grid_of(n, kChebThreads);
    DevBuf part;
    SPAL_HIP_TRY(part.alloc((size_t)blocks * 2 * sizeof(double) + sizeof(unsigned)));
    double *d_part = part.as<double>();
    unsigned *d_bad = reinterpret_cast<unsigned *>(d_part + (size_t)blocks * 2);
    SPAL_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned), st));
    if (a->elem_size == 8)
        hipLaunchKernelGGL((gershgorin_rows<double>), dim3(blocks), dim3(kChebThreads), 0, st, (const uint32_t *)a->d_rowptr,
                           (const uint32_t *)a->d_colind, (const double *)a->d_values, n, d_part, d_bad);
    else
        hipLaunchKernelGGL((gershgorin_rows<float>), dim3(blocks), dim3(kChebThreads), 0, st, (const uint32_t *)a->d_rowptr,
                           (const uint32_t *)a->d_colind, (const float *)a->d_values, n, d_part, d_bad);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(le));
    std::vector<double> h((size_t)blocks * 2 + 1);
    SPAL_HIP_TRY(hipMemcpyAsync(h.data(), d_part, (size_t)blocks * 2 * sizeof(double) + sizeof(unsigned), hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    unsigned bad = 0;
    memcpy(&bad, &h[(size_t)blocks * 2], sizeof bad);
    double lo = INFINITY, hi = -INFINITY;
    for (unsigned b = 0; b < blocks; ++b) {
        lo = std::fmin(lo, h[2 * (size_t)b]);
        hi = std::fmax(hi, h[2 * (size_t)b + 1]);
    }
    *glo = bad ? (double)NAN : lo;
    *ghi = bad ? (double)NAN : hi;
    return SPAL_OK;
}

int cheb_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status) {
    if (!strcmp(key, "cheb_series_form")) {
        if (value < 0 || value > 2) {
            *status = fail(SPAL_ERR_INVALID_ARGUMENT, "cheb_series_form must be 0 (automatic), 1 (fused step) or 2 (step and a separate accumulation)");
            return 1;
        }
        std::lock_guard<std::mutex> lock(a->mu);
        s.cheb_series_form = (int)value;
        *status = SPAL_OK;
        return 1;
    }
    if (strcmp(key, "cheb_chunk")) return 0;
    if (value != 0 && value != 256 && value != 512 && value != 1024 && value != 2048 && value != 4096) {
        *status = fail(SPAL_ERR_INVALID_ARGUMENT, "cheb_chunk must be 0 (16 KiB of products) or 256, 512, 1024, 2048 or 4096 entries");
        return 1;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    s.cheb_chunk = (int)value;
    *status = SPAL_OK;
    return 1;
}

}  // namespace spal

using namespace spal;

extern "C" {

#define SPAL_CHEB_ENTRIES(kind, sfx, T)                                                                                  \
    int spal_##kind##_cheb_apply_##sfx(spal_##kind##_t a, const T *x, uint64_t x_len, T *out, uint64_t out_len,           \
                                       uint64_t degree, double lo, double hi, double a0) {                                \
        return apply_host<T, spal_##kind>("spal_" #kind "_cheb_apply", a, x, x_len, out, out_len, degree, lo, hi, a0);    \
    }                                                                                                                     \
    int spal_##kind##_cheb_apply_dev_##sfx(spal_##kind##_t a, const T *x_dev, T *out_dev, uint64_t degree, double lo,     \
                                           double hi, double a0, void *stream) {                                          \
        return apply_dev<T, spal_##kind>("spal_" #kind "_cheb_apply_dev", a, x_dev, out_dev, degree, lo, hi, a0, stream); \
    }
SPAL_CHEB_ENTRIES(csr, f64, double)
SPAL_CHEB_ENTRIES(csr, f32, float)
SPAL_CHEB_ENTRIES(csc, f64, double)
SPAL_CHEB_ENTRIES(csc, f32, float)
#undef SPAL_CHEB_ENTRIES

#define SPAL_CHEB_SERIES_ENTRIES(kind, sfx, T)                                                                            \
    int spal_##kind##_cheb_series_##sfx(spal_##kind##_t a, const T *x, uint64_t x_len, T *out, uint64_t out_len,            \
                                        uint64_t degree, double lo, double hi, const double *coef, uint64_t coef_len) {     \
        return series_host<T, spal_##kind>("spal_" #kind "_cheb_series", a, x, x_len, out, out_len, degree, lo, hi, coef,   \
                                           coef_len);                                                                       \
    }                                                                                                                       \
    int spal_##kind##_cheb_series_dev_##sfx(spal_##kind##_t a, const T *x_dev, T *out_dev, uint64_t degree, double lo,      \
                                            double hi, const double *coef, uint64_t coef_len, void *stream) {               \
        return series_dev<T, spal_##kind>("spal_" #kind "_cheb_series_dev", a, x_dev, out_dev, degree, lo, hi, coef,        \
                                          coef_len, stream);                                                                \
    }
SPAL_CHEB_SERIES_ENTRIES(csr, f64, double)
SPAL_CHEB_SERIES_ENTRIES(csr, f32, float)
SPAL_CHEB_SERIES_ENTRIES(csc, f64, double)
SPAL_CHEB_SERIES_ENTRIES(csc, f32, float)
#undef SPAL_CHEB_SERIES_ENTRIES

int spal_cheb_delta_coefficients(uint64_t degree, double gamma, double *coef, uint64_t coef_len) {
    const char *fn = "spal_cheb_delta_coefficients";
    if (!coef) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    ChebSeriesRefusal r = degree < 1 || degree > kChebSeriesMaxDegree ? CHEB_SERIES_DEGREE
                          : coef_len != degree + 1                   ? CHEB_SERIES_LEN
                                                                     : CHEB_SERIES_OK;
    std::vector<double> c;
    if (r == CHEB_SERIES_OK) {
        c.resize(degree + 1);
        r = cheb_delta_coefficients(degree, gamma, c.data());
    }
    if (r != CHEB_SERIES_OK)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: %s (degree = %llu, coef_len = %llu, gamma = %.17g)", fn,
                    cheb_series_refusal_text(r), (unsigned long long)degree, (unsigned long long)coef_len, gamma);
    std::copy(c.begin(), c.end(), coef);
    return SPAL_OK;
}

int spal_csr_gershgorin(spal_csr_t a, double *glo, double *ghi) { return gershgorin_entry("spal_csr_gershgorin", a, glo, ghi); }
int spal_csc_gershgorin(spal_csc_t a, double *glo, double *ghi) { return gershgorin_entry("spal_csc_gershgorin", a, glo, ghi); }

}  // extern "C"
