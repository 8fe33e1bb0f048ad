// spal_spmm.hip -- Y = A * X for a dense row-major block X of k vectors: `&A * &X` of src/csr/ops/mul.rs with
// every entry of X stored.  Y[i, j] is row i's stored entries in ascending column, the first product assigned, every
// later one added, multiply and add rounded separately -- bit for bit the reference, whatever k, the leading dimensions
// or the column tile are.  CSC handles run the same kernel on their CSR twin.
//
// ONE KERNEL, ONE PASS OVER THE MATRIX.  A workgroup of 256 threads owns a tile of R consecutive rows (R a power of two
// <= 256, picked from the mean row length so that a tile's entries fit the LDS strip).  It loads the tile's row bounds,
// then the tile's whole entry range rowptr[r0] .. rowptr[r0 + R) -- columns and values -- coalesced into LDS, once, for
// all k columns of X.  Then one thread owns one (row, column j) pair: the 256 threads are 256 / KT lane groups of KT
// lanes, lane group g walks rows g, g + 256 / KT, ... of the tile and, per row, the column tiles j0 = 0, KT, 2 KT, ...
// of X (the last one partial: lanes with j0 + j >= k sit it out).  The KT lanes of a group read the same entry from
// LDS (a broadcast) and gather X[col * ldx + j0 .. j0 + KT), one contiguous segment; their stores of Y[row * ldy + j0 ..)
// are one contiguous segment too, merged by the memory pipeline from per-lane stores, so no alignment of ldx / ldy is
// assumed anywhere.  Workgroups are dealt to the 8 XCDs in turn; consecutive tiles are given to ONE XCD's workgroups.
//   * a tile whose entries exceed the strip (skewed row lengths) walks its rows straight from global memory instead;
//   * rows of more than kLong entries are left out of both walks and listed in LDS: afterwards each wave of the
//     workgroup takes (long row, 64 columns of X) items -- 64 entries loaded coalesced into registers, handed round by
//     readlane, lane j adding for column j.  The order inside the row stays the stored order: the row's sum is never
//     split, only given to other lanes.
// Nothing is read from CsrPlan and nothing is written to the handle or to scratch memory: the launch is safe on a
// handle whose SpMV plan is still pending, under graph capture, and from several threads at once.
#include "spal_ops.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kCap = 2048;        // entries of a tile's LDS strip
constexpr uint32_t kLong = 512;        // rows above it are walked by a whole wave
constexpr uint32_t kTileRowsMax = 256; // R <= kThreads: one thread looks at one row's length
constexpr int kTiles[] = {1, 2, 4, 8, 16, 32};   // the instantiated column tiles

__device__ __forceinline__ uint32_t lane_bcast(uint32_t v, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}
__device__ __forceinline__ float lane_bcast(float v, uint32_t src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)src));
}
__device__ __forceinline__ double lane_bcast(double v, uint32_t src) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)b >> 32), (int)src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One (row, column of X) pair: entries [b, e) of `col` / `val` (the LDS strip or the global arrays), e > b.  The row is
// taken kBatch entries at a time: all gathers of a batch are issued before the first add (a row of up to kBatch entries
// waits for memory once), past the row's end they repeat its last entry's address and their products are dropped.
constexpr uint32_t kBatch = 16;
template <typename T>
__device__ __forceinline__ T spmm_row_sum(const uint32_t *col, const T *val, uint32_t b, uint32_t e,
                                          const T *__restrict__ xj, uint64_t ldx) {
    T acc = T(0);
    for (uint32_t p = b; p < e; p += kBatch) {
        T x[kBatch], v[kBatch];
#pragma unroll
        for (uint32_t u = 0; u < kBatch; ++u) {
            const uint32_t q = min(p + u, e - 1);
            x[u] = xj[(uint64_t)col[q] * ldx];
            v[u] = val[q];
        }
        const T first = v[0] * x[0];
        acc = p == b ? first : acc + first;   // the row's first product is assigned (-0.0 stays -0.0)
#pragma unroll
        for (uint32_t u = 1; u < kBatch; ++u)
            if (p + u < e) acc = acc + v[u] * x[u];
    }
    return acc;
}

// The lane groups' walk over the tile's rows; `col` / `val` are indexed by (entry - base).
template <typename T, int KT>
__device__ __forceinline__ void spmm_walk(const uint32_t *s_rp, const uint32_t *col, const T *val, uint32_t base,
                                          uint32_t r0, uint32_t nr, uint32_t k, const T *__restrict__ X, uint64_t ldx,
                                          T *__restrict__ Y, uint64_t ldy) {
    constexpr uint32_t G = kThreads / KT;
    const uint32_t g = threadIdx.x / KT, j = threadIdx.x % KT;
    for (uint32_t lr = g; lr < nr; lr += G) {
        const uint32_t b = s_rp[lr] - base, e = s_rp[lr + 1] - base;
        if (e - b > kLong) continue;   // a wave takes it afterwards
        T *yrow = Y + (uint64_t)(r0 + lr) * ldy;
        for (uint32_t jc = j; jc < k; jc += KT)   // column tiles of X, the last one partial
            yrow[jc] = e == b ? T(0) : spmm_row_sum<T>(col, val, b, e, X + jc, ldx);
    }
}

template <typename T, int KT>
__global__ __launch_bounds__(kThreads) void spmm_csr_tile(const uint32_t *__restrict__ rowptr,
                                                          const uint32_t *__restrict__ colind,
                                                          const T *__restrict__ values, uint32_t nrows, uint32_t R,
                                                          uint32_t k, const T *__restrict__ X, uint64_t ldx,
                                                          T *__restrict__ Y, uint64_t ldy) {
    __shared__ uint32_t s_rp[kTileRowsMax + 1];
    __shared__ uint32_t s_long[kTileRowsMax];
    __shared__ uint32_t s_nlong;
    __shared__ uint32_t s_col[kCap];
    __shared__ T s_val[kCap];
    const uint32_t tid = threadIdx.x;
    // consecutive tiles go to one XCD (workgroups are dealt to the 8 XCDs in turn): its L2 then holds one stretch of X
    const uint32_t per_xcd = gridDim.x / 8;
    const uint32_t tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if ((uint64_t)tile * R >= nrows) return;
    const uint32_t r0 = tile * R;
    const uint32_t nr = min(R, nrows - r0);
    for (uint32_t i = tid; i <= nr; i += kThreads) s_rp[i] = rowptr[r0 + i];
    if (tid == 0) s_nlong = 0;
    __syncthreads();
    const uint32_t e0 = s_rp[0], n = s_rp[nr] - e0;
    const bool staged = n <= kCap;
    if (staged) {   // the tile's entries, coalesced, all loads issued before the first LDS store
        constexpr int U = kCap / kThreads;
        uint32_t c[U] = {};
        T v[U] = {};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = tid + u * kThreads;
            if (i < n) { c[u] = colind[e0 + i]; v[u] = values[e0 + i]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = tid + u * kThreads;
            if (i < n) { s_col[i] = c[u]; s_val[i] = v[u]; }
        }
    }
    if (tid < nr && s_rp[tid + 1] - s_rp[tid] > kLong) s_long[atomicAdd(&s_nlong, 1u)] = tid;
    __syncthreads();
    if (staged) spmm_walk<T, KT>(s_rp, s_col, s_val, e0, r0, nr, k, X, ldx, Y, ldy);
    else spmm_walk<T, KT>(s_rp, colind, values, 0u, r0, nr, k, X, ldx, Y, ldy);

    const uint32_t nlong = s_nlong;
    if (nlong == 0) return;
    // long rows: a wave per (row, 64 columns of X); the listing order does not matter, every item is a row of its own
    const uint32_t wave = tid / 64, lane = tid % 64, cchunks = (k + 63) / 64;
    for (uint32_t item = wave; item < nlong * cchunks; item += kThreads / 64) {
        const uint32_t lr = s_long[item / cchunks];
        const uint32_t jc = (item % cchunks) * 64 + lane;
        const T *xj = X + min(jc, k - 1);   // lanes past k compute a copy of column k - 1 and store nothing
        const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_rp[lr]);
        const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_rp[lr + 1]);
        T acc = T(0);
        for (uint32_t p = b; p < e; p += 64) {
            const uint32_t q = p + lane;
            const uint32_t mc = q < e ? colind[q] : 0u;
            const T mv = q < e ? values[q] : T(0);
            const uint32_t m = min(64u, e - p);
            uint32_t u = 0;
            if (p == b) {   // the row's first product is assigned
                acc = lane_bcast(mv, 0u) * xj[(uint64_t)lane_bcast(mc, 0u) * ldx];
                u = 1;
            }
            for (; u + 8 <= m; u += 8) {   // eight gathers in flight, then the adds in stored order
                T x[8];
#pragma unroll
                for (uint32_t w = 0; w < 8; ++w) x[w] = xj[(uint64_t)lane_bcast(mc, u + w) * ldx];
#pragma unroll
                for (uint32_t w = 0; w < 8; ++w) acc = acc + lane_bcast(mv, u + w) * x[w];
            }
            for (; u < m; ++u) acc = acc + lane_bcast(mv, u) * xj[(uint64_t)lane_bcast(mc, u) * ldx];
        }
        if (jc < k) Y[(uint64_t)(r0 + lr) * ldy + jc] = acc;
    }
}

// rows of more than kLong entries (describe)
__global__ __launch_bounds__(256) void spmm_count_long(const uint32_t *__restrict__ rowptr, uint32_t nrows,
                                                       uint32_t *__restrict__ count) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool is_long = r < nrows && rowptr[r + 1] - rowptr[r] > kLong;
    const uint32_t n = (uint32_t)__popcll(__ballot(is_long));
    if (n && threadIdx.x % 64 == 0) atomicAdd(count, n);
}

bool tile_instantiated(int64_t t) {
    for (int v : kTiles)
        if (t == v) return true;
    return false;
}

// automatic column tile: the narrowest instantiated tile that holds k (measured, DESIGN 3.10: a tile wider than k
// idles lanes, a narrower one gathers X in more and shorter segments, and the gathers are what costs)
int auto_tile(uint64_t k) {
    int t = 1;
    while (t < 32 && (uint64_t)t < k) t *= 2;
    return t;
}

// rows of a tile: the largest power of two whose entries fit the strip with a tenth to spare
uint32_t tile_rows(const spal_csr *a) {
    const double mean = a->nrows ? (double)a->nnz / (double)a->nrows : 0.0;
    uint32_t R = kTileRowsMax;
    while (R > 8 && (double)R * mean * 1.1 > (double)kCap) R /= 2;
    return R;
}

template <typename T, int KT>
hipError_t launch_t(const spal_csr *a, uint32_t R, uint64_t k, const void *x, uint64_t ldx, void *y, uint64_t ldy,
                    hipStream_t st) {
    const uint32_t grid = (uint32_t)(((a->nrows + R - 1) / R + 7) / 8 * 8);   // a multiple of the 8 XCDs
    hipLaunchKernelGGL((spmm_csr_tile<T, KT>), dim3(grid), dim3(kThreads), 0, st, a->d_rowptr, a->d_colind,
                       (const T *)a->d_values, (uint32_t)a->nrows, R, (uint32_t)k, (const T *)x, ldx, (T *)y, ldy);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_tile(const spal_csr *a, int tile, uint32_t R, uint64_t k, const void *x, uint64_t ldx, void *y,
                       uint64_t ldy, hipStream_t st) {
    switch (tile) {
    case 1: return launch_t<T, 1>(a, R, k, x, ldx, y, ldy, st);
    case 2: return launch_t<T, 2>(a, R, k, x, ldx, y, ldy, st);
    case 4: return launch_t<T, 4>(a, R, k, x, ldx, y, ldy, st);
    case 8: return launch_t<T, 8>(a, R, k, x, ldx, y, ldy, st);
    case 16: return launch_t<T, 16>(a, R, k, x, ldx, y, ldy, st);
    default: return launch_t<T, 32>(a, R, k, x, ldx, y, ldy, st);
    }
}

int count_long_rows(const spal_csr *a, hipStream_t st, uint64_t *out) {
    if (!a->parts.empty()) {
        for (const spal_csr *part : a->parts) SPAL_TRY(count_long_rows(part, st, out));
        return SPAL_OK;
    }
    if (a->nrows == 0) return SPAL_OK;
    DevBuf cnt;
    SPAL_HIP_TRY(cnt.alloc(sizeof(uint32_t)));
    SPAL_HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(spmm_count_long, dim3((uint32_t)((a->nrows + 255) / 256)), dim3(256), 0, st, a->d_rowptr,
                       (uint32_t)a->nrows, cnt.as<uint32_t>());
    SPAL_HIP_TRY(hipGetLastError());
    uint32_t h = 0;
    SPAL_HIP_TRY(hipMemcpyAsync(&h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    *out += h;
    return SPAL_OK;
}

int launch_rows(const spal_csr *a, int tile, uint64_t k, const void *x, uint64_t ldx, void *y, uint64_t ldy,
                hipStream_t st) {
    if (!a->parts.empty()) {   // row blocks: block b writes rows part_row0[b] ... of Y
        for (size_t b = 0; b < a->parts.size(); ++b)
            SPAL_TRY(launch_rows(a->parts[b], tile, k, x, ldx,
                                 (char *)y + a->part_row0[b] * ldy * (uint64_t)a->elem_size, ldy, st));
        return SPAL_OK;
    }
    if (a->nrows == 0) return SPAL_OK;
    const uint32_t R = tile_rows(a);
    SPAL_HIP_TRY(a->elem_size == 8 ? launch_tile<double>(a, tile, R, k, x, ldx, y, ldy, st)
                                   : launch_tile<float>(a, tile, R, k, x, ldx, y, ldy, st));
    return SPAL_OK;
}

template <typename T>
int check_common(const char *fn, const void *a, int elem_size, uint64_t k, const void *x, uint64_t ldx, const void *y,
                 uint64_t ldy) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    SPAL_TRY(check_dtype<T>(fn, elem_size));
    if (!x || !y) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null block of vectors", fn);
    if (k == 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: k = 0 (X and Y need at least one column)", fn);
    if (k > 0xffffffffull) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: k = %llu does not fit 32 bits", fn, (unsigned long long)k);
    if (ldx < k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ldx = %llu is less than k = %llu", fn, (unsigned long long)ldx,
                    (unsigned long long)k);
    if (ldy < k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ldy = %llu is less than k = %llu", fn, (unsigned long long)ldy,
                    (unsigned long long)k);
    return SPAL_OK;
}

int check_rows(const char *fn, uint64_t nrows, uint64_t ncols, uint64_t x_rows, uint64_t y_rows) {
    if (x_rows != ncols)   // assert_eq!(self.ncols(), rhs.nrows())  mul.rs:9
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: assertion failed: ncols == rhs.nrows (left: %llu, right: %llu)", fn,
                    (unsigned long long)ncols, (unsigned long long)x_rows);
    if (y_rows != nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: Y has %llu rows but nrows = %llu", fn, (unsigned long long)y_rows,
                    (unsigned long long)nrows);
    return SPAL_OK;
}

// host arrays: X packed to ld = k on the way up, Y's k columns copied back into the caller's rows (padding untouched)
template <typename T>
int spmm_host(spal_csr *a, int tile, hipStream_t st, uint64_t k, const T *x, uint64_t ldx, T *y, uint64_t ldy) {
    DevBuf dx, dy;
    const size_t row = (size_t)k * sizeof(T);
    SPAL_HIP_TRY(dx.alloc(a->ncols * row));
    SPAL_HIP_TRY(dy.alloc(a->nrows * row));
    if (a->ncols)
        SPAL_HIP_TRY(hipMemcpy2DAsync(dx.p, row, x, (size_t)ldx * sizeof(T), row, a->ncols, hipMemcpyHostToDevice, st));
    SPAL_TRY(spmm_launch(a, tile, k, dx.p, k, dy.p, k, st));
    if (a->nrows)
        SPAL_HIP_TRY(hipMemcpy2DAsync(y, (size_t)ldy * sizeof(T), dy.p, row, row, a->nrows, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    return SPAL_OK;
}

// The entry points, for either handle type: the handle's own lock, stream and option; the product on solve_handle(a).
template <typename T, typename H>
int spmm_host_entry(const char *fn, H *a, uint64_t k, const T *x, uint64_t ldx, uint64_t x_rows, T *y, uint64_t ldy,
                    uint64_t y_rows) {
    SPAL_TRY(check_common<T>(fn, a, a ? a->elem_size : 0, k, x, ldx, y, ldy));
    SPAL_TRY(check_rows(fn, a->nrows, a->ncols, x_rows, y_rows));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::lock_guard<std::mutex> lock(a->mu);
    return spmm_host<T>(solve_handle(a), a->ops.spmm_tile, a->stream, k, x, ldx, y, ldy);
}

template <typename T, typename H>
int spmm_dev_entry(const char *fn, H *a, uint64_t k, const T *x, uint64_t ldx, T *y, uint64_t ldy, void *stream) {
    SPAL_TRY(check_common<T>(fn, a, a ? a->elem_size : 0, k, x, ldx, y, ldy));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return spmm_launch(solve_handle(a), a->ops.spmm_tile, k, x, ldx, y, ldy, (hipStream_t)stream);
}

}  // namespace

int spmm_launch(spal_csr *a, int tile, uint64_t k, const void *x_dev, uint64_t ldx, void *y_dev, uint64_t ldy,
                hipStream_t st) {
    if (tile == 0) tile = auto_tile(k);
    SPAL_TRY(launch_rows(a, tile, k, x_dev, ldx, y_dev, ldy, st));
    // what describe() reports: {tile, k} of the last call in one word (concurrent calls each store a consistent pair)
    __atomic_store_n(&a->spmm_last, ((uint64_t)tile << 32) | (uint64_t)(uint32_t)k, __ATOMIC_RELAXED);
    return SPAL_OK;
}

int spmm_option(const char *key, int64_t value, OpState &s, int *status) {
    if (strcmp(key, "spmm_tile")) return 0;
    *status = (value == 0 || tile_instantiated(value))
                  ? SPAL_OK
                  : fail(SPAL_ERR_INVALID_ARGUMENT, "spmm_tile must be 0 (automatic) or one of 1, 2, 4, 8, 16, 32");
    if (*status == SPAL_OK) s.spmm_tile = (int)value;
    return 1;
}

int spmm_describe_append(char *buf, size_t buf_len, const spal_csr *a) {
    const uint64_t last = a ? __atomic_load_n(&a->spmm_last, __ATOMIC_RELAXED) : 0;
    if (!last) return SPAL_OK;
    const uint32_t tile = (uint32_t)(last >> 32), k = (uint32_t)last;
    uint64_t nlong = 0;
    {
        DeviceGuard guard(a->device);
        if (guard.status != SPAL_OK) return guard.status;
        SPAL_TRY(count_long_rows(a, a->stream, &nlong));
    }
    const spal_csr *first = a->parts.empty() ? a : a->parts[0];
    char info[256];
    snprintf(info, sizeof info,
             "{\"tile\": %u, \"k\": %u, \"column_tiles\": %u, \"tile_rows\": %u, \"strip_entries\": %u, "
             "\"long_row_threshold\": %u, \"long_rows\": %llu}",
             tile, k, (k + tile - 1) / tile, tile_rows(first), kCap, kLong, (unsigned long long)nlong);
    return describe_append(buf, buf_len, "spmm", info);
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_spmm_f64(spal_csr_t a, uint64_t k, const double *x, uint64_t ldx, uint64_t x_rows, double *y, uint64_t ldy,
                      uint64_t y_rows) {
    return spmm_host_entry<double>("spal_csr_spmm", a, k, x, ldx, x_rows, y, ldy, y_rows);
}
int spal_csr_spmm_f32(spal_csr_t a, uint64_t k, const float *x, uint64_t ldx, uint64_t x_rows, float *y, uint64_t ldy,
                      uint64_t y_rows) {
    return spmm_host_entry<float>("spal_csr_spmm", a, k, x, ldx, x_rows, y, ldy, y_rows);
}
int spal_csr_spmm_dev_f64(spal_csr_t a, uint64_t k, const double *x_dev, uint64_t ldx, double *y_dev, uint64_t ldy,
                          void *stream) {
    return spmm_dev_entry<double>("spal_csr_spmm_dev", a, k, x_dev, ldx, y_dev, ldy, stream);
}
int spal_csr_spmm_dev_f32(spal_csr_t a, uint64_t k, const float *x_dev, uint64_t ldx, float *y_dev, uint64_t ldy,
                          void *stream) {
    return spmm_dev_entry<float>("spal_csr_spmm_dev", a, k, x_dev, ldx, y_dev, ldy, stream);
}
int spal_csc_spmm_f64(spal_csc_t a, uint64_t k, const double *x, uint64_t ldx, uint64_t x_rows, double *y, uint64_t ldy,
                      uint64_t y_rows) {
    return spmm_host_entry<double>("spal_csc_spmm", a, k, x, ldx, x_rows, y, ldy, y_rows);
}
int spal_csc_spmm_f32(spal_csc_t a, uint64_t k, const float *x, uint64_t ldx, uint64_t x_rows, float *y, uint64_t ldy,
                      uint64_t y_rows) {
    return spmm_host_entry<float>("spal_csc_spmm", a, k, x, ldx, x_rows, y, ldy, y_rows);
}
int spal_csc_spmm_dev_f64(spal_csc_t a, uint64_t k, const double *x_dev, uint64_t ldx, double *y_dev, uint64_t ldy,
                          void *stream) {
    return spmm_dev_entry<double>("spal_csc_spmm_dev", a, k, x_dev, ldx, y_dev, ldy, stream);
}
int spal_csc_spmm_dev_f32(spal_csc_t a, uint64_t k, const float *x_dev, uint64_t ldx, float *y_dev, uint64_t ldy,
                          void *stream) {
    return spmm_dev_entry<float>("spal_csc_spmm_dev", a, k, x_dev, ldx, y_dev, ldy, stream);
}

}  // extern "C"
