// spal_csc.hip -- the CSC handle: life cycle, the route of y = A*x, conversions, options, describe and the C ABI.
//
// Contract (reference src/csc/ops/mul.rs:26-46): for
// every stored entry (i, k): y[i] += values[p] * x[k]; rows never touched
// give 0.0.  Two routes: "kernel" 2 (default) multiplies with the handle's CSR twin -- the same matrix transposed once
// on the device by the constructor -- and the CSR kernels; "kernel" 1 scatters with LDS-privatised atomics, over row
// tiles where the plan built them (spal_csc_rowtiles.hip), else over column tiles (spal_csc_scatter.hip, planned by
// spal_csc_plan.hip).
#include "spal_ops.hpp"

namespace spal {

static int pick_lanes_csc(const spal_csc *a) {
    const double mean = a->ncols ? (double)a->nnz / (double)a->ncols : 0.0;
    int L = 2;
    while (L < 64 && (double)L < mean) L <<= 1;
    return L;
}

static int csc_launch(spal_csc *a, const void *x, void *y, hipStream_t st) {
    if (a->kernel == 2) return csr_launch(a->as_csr, x, y, st);   // the same matrix as CSR, stream / vector CSR kernel
    // row tiles where the plan built them: a workgroup owns rows of y outright -- no memset, no hand-off, no launch chain
    const bool row_tiles = a->rowtiles && a->rowtiles_user != 0 && a->flush == 0 && a->nnz;
    hipError_t e = row_tiles ? launch_csc_rowtiles(a, x, y, st) : launch_csc_scatter(a, x, y, st);
    if (e == hipErrorLaunchTimeOut)
        return fail(SPAL_ERR_HIP, "csc spmv: an earlier product of this handle gave up waiting in the neighbour hand-off "
                    "(spin bound reached): that product's y is invalid; nothing was launched now, and the handle flushes "
                    "with global atomics from here on");
    if (e != hipSuccess) return fail(SPAL_ERR_HIP, "csc spmv launch failed: %s", hipGetErrorString(e));
    return SPAL_OK;
}

// CSC -> CSR on the device (stable sort of the entries by row) into a new CSR handle; nothing is left behind on failure
static int csc_to_csr_arrays(spal_csc *a, spal_csr **out) {
    OpArrays t;
    SPAL_TRY(transpose_device(a->device, a->elem_size, a->ncols, a->nrows, a->nnz, a->d_colptr,
                              a->d_rowind, a->d_values, a->stream, t));
    return t.adopt(a->device, a->elem_size, a->nrows, a->ncols, out);
}

// what both constructors end with: the scatter plan, then the CSR twin (setup work, not the first product's)
static int csc_finish(spal_csc *a) {
    a->lanes_per_col = pick_lanes_csc(a);
    SPAL_TRY(csc_plan_build(a));
    return csc_to_csr_arrays(a, &a->as_csr);
}

static void csc_free(spal_csc *a) {
    if (!a) return;
    if (a->as_csr) (void)spal_csr_destroy(a->as_csr);
    (void)dev_free(a->d_colptr);
    (void)dev_free(a->d_rowind);
    (void)dev_free(a->d_values);
    (void)dev_free(a->d_meta);
    (void)dev_free(a->d_desc);
    (void)dev_free(a->d_windows);
    (void)dev_free(a->d_chunk_ptr);
    (void)dev_free(a->d_chunk_blk);
    (void)dev_free(a->d_prev_hi);
    (void)dev_free(a->d_flags);
    csc_rowtiles_free(a);
    ordering_free(a->ops);
    if (a->ev_last) (void)hipEventDestroy(a->ev_last);
    if (a->h_gave_up) (void)hipHostFree(a->h_gave_up);
    (void)dev_free(a->d_x);
    (void)dev_free(a->d_y);
    stream_release(a->stream);
    delete a;
}

int csc_adopt_device(int device, int elem_size, uint64_t nrows, uint64_t ncols, uint64_t nnz, uint64_t cap_entries,
                     uint32_t *d_colptr, uint32_t *d_rowind, void *d_values, spal_csc **out) {
    if (cap_entries < nnz + kStreamPad)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "csc_adopt_device: capacity %llu < nnz + pad = %llu",
                    (unsigned long long)cap_entries, (unsigned long long)(nnz + kStreamPad));
    spal_csc *a = new spal_csc;
    a->device = device;
    a->elem_size = elem_size;
    a->nrows = nrows; a->ncols = ncols; a->nnz = nnz;
    a->d_colptr = d_colptr; a->d_rowind = d_rowind; a->d_values = d_values;
    const hipError_t e = stream_acquire(&a->stream);
    const int st = e == hipSuccess ? csc_finish(a) : fail(SPAL_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    if (st != SPAL_OK) {
        a->d_colptr = nullptr; a->d_rowind = nullptr; a->d_values = nullptr;  // stay with the caller
        csc_free(a);
        return st;
    }
    *out = a;
    return SPAL_OK;
}

template <typename T>
static int csc_create(int device, uint64_t nrows, uint64_t ncols, const uint64_t *colptr,
                      uint64_t colptr_len, const uint64_t *rowind, uint64_t rowind_len,
                      const T *values, uint64_t values_len, spal_csc_t *out) {
    if (!out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_create: out is NULL");
    *out = nullptr;
    if (!colptr || (!rowind && rowind_len) || (!values && values_len))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_create: null array");
    int reason = 0;
    SPAL_TRY(spal_csc_validate(nrows, ncols, colptr, colptr_len, rowind, rowind_len, values_len, &reason));
    const uint64_t nnz = colptr[ncols];
    if (ncols >= 0xffffffffull || nrows > 0xffffffffull || nnz > kMaxEntries)
        return fail(SPAL_ERR_UNSUPPORTED,
                    "shape %llu x %llu with %llu entries does not fit 32-bit device indices",
                    (unsigned long long)nrows, (unsigned long long)ncols, (unsigned long long)nnz);
    DeviceGuard guard(device);
    if (guard.status != SPAL_OK) return guard.status;
    std::vector<uint32_t> cp32(ncols + 1), ri32(nnz);
    parallel_for(ncols + 1, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t i = b; i < e; ++i) cp32[i] = (uint32_t)colptr[i];
    });
    parallel_for(nnz, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t i = b; i < e; ++i) ri32[i] = (uint32_t)rowind[i];
    });
    spal_csc *a = new spal_csc;
    a->device = device;
    a->elem_size = (int)sizeof(T);
    a->nrows = nrows; a->ncols = ncols; a->nnz = nnz;
    const uint64_t cap = nnz + kStreamPad;  // whole-step reads of the LDS-mode stream
    hipError_t e = dev_alloc((void **)&a->d_colptr, (ncols + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = dev_alloc((void **)&a->d_rowind, cap * sizeof(uint32_t));
    if (e == hipSuccess) e = dev_alloc((void **)&a->d_values, cap * sizeof(T));
    if (e == hipSuccess) e = hipMemset((char *)a->d_values + nnz * sizeof(T), 0, kStreamPad * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(a->d_colptr, cp32.data(), (ncols + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(a->d_rowind, ri32.data(), nnz * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(a->d_values, values, nnz * sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = stream_acquire(&a->stream);
    if (e != hipSuccess) {
        csc_free(a);
        return fail(e == hipErrorOutOfMemory ? SPAL_ERR_OUT_OF_MEMORY : SPAL_ERR_HIP,
                    "spal_csc_create: upload failed: %s", hipGetErrorString(e));
    }
    const int st = csc_finish(a);
    if (st != SPAL_OK) { csc_free(a); return st; }
    *out = a;
    return SPAL_OK;
}

template <typename T>
static int csc_spmv_host(spal_csc_t a, const T *x, uint64_t x_len, T *y, uint64_t y_len) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_spmv: handle is NULL");
    if (a->elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_spmv: handle holds %s values",
                    a->elem_size == 8 ? "f64" : "f32");
    if (x_len != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT,
                    "dimension mismatch: x.len() = %llu but ncols = %llu (assert_eq!, csc/ops/mul.rs:9)",
                    (unsigned long long)x_len, (unsigned long long)a->ncols);
    if (y_len != a->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "y.len() = %llu but nrows = %llu",
                    (unsigned long long)y_len, (unsigned long long)a->nrows);
    if (!x || !y) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_spmv: null vector");
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::lock_guard<std::mutex> lock(a->mu);
    if (!a->d_x) SPAL_HIP_TRY(dev_alloc((void **)&a->d_x, a->ncols * sizeof(T)));
    if (!a->d_y) SPAL_HIP_TRY(dev_alloc((void **)&a->d_y, a->nrows * sizeof(T)));
    SPAL_HIP_TRY(hipMemcpyAsync(a->d_x, x, a->ncols * sizeof(T), hipMemcpyHostToDevice, a->stream));
    SPAL_TRY(csc_launch(a, a->d_x, a->d_y, a->stream));
    SPAL_HIP_TRY(hipMemcpyAsync(y, a->d_y, a->nrows * sizeof(T), hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    // neighbour hand-off: a super-tile hit its spin bound (the backstop; see csc_spmv_scatter) -- this handle keeps to
    // the atomics flush from now on and the product is repeated
    bool gave_up;
    {
        std::lock_guard<std::mutex> chain(a->mu_launch);
        gave_up = csc_gave_up_consume(a);
    }
    if (gave_up) {
        SPAL_TRY(csc_launch(a, a->d_x, a->d_y, a->stream));
        SPAL_HIP_TRY(hipMemcpyAsync(y, a->d_y, a->nrows * sizeof(T), hipMemcpyDeviceToHost, a->stream));
        SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    }
    return SPAL_OK;
}

template <typename T>
static int csc_spmv_dev(spal_csc_t a, const T *x_dev, T *y_dev, void *stream) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_spmv_dev: handle is NULL");
    if (a->elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_spmv_dev: handle holds %s values",
                    a->elem_size == 8 ? "f64" : "f32");
    if (!x_dev || !y_dev) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_spmv_dev: null vector");
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return csc_launch(a, x_dev, y_dev, (hipStream_t)stream);
}

template <typename T>
static int csc_download(spal_csc_t a, uint64_t *colptr, uint64_t *rowind, T *values) {
    if (!a || !colptr) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_download: null argument");
    if (a->elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_download: handle holds %s values",
                    a->elem_size == 8 ? "f64" : "f32");
    if (a->nnz && (!rowind || !values)) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_download: null array");
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::vector<uint32_t> cp(a->ncols + 1), ri(a->nnz);
    SPAL_HIP_TRY(hipMemcpy(cp.data(), a->d_colptr, cp.size() * 4, hipMemcpyDeviceToHost));
    if (a->nnz) {
        SPAL_HIP_TRY(hipMemcpy(ri.data(), a->d_rowind, ri.size() * 4, hipMemcpyDeviceToHost));
        SPAL_HIP_TRY(hipMemcpy(values, a->d_values, a->nnz * sizeof(T), hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i <= a->ncols; ++i) colptr[i] = cp[i];
    for (uint64_t i = 0; i < a->nnz; ++i) rowind[i] = ri[i];
    return SPAL_OK;
}
}  // namespace spal

using namespace spal;

extern "C" {

int spal_csc_create_f64(int device, uint64_t nrows, uint64_t ncols, const uint64_t *colptr,
                        uint64_t colptr_len, const uint64_t *rowind, uint64_t rowind_len,
                        const double *values, uint64_t values_len, spal_csc_t *out) {
    return csc_create<double>(device, nrows, ncols, colptr, colptr_len, rowind, rowind_len, values,
                              values_len, out);
}
int spal_csc_create_f32(int device, uint64_t nrows, uint64_t ncols, const uint64_t *colptr,
                        uint64_t colptr_len, const uint64_t *rowind, uint64_t rowind_len,
                        const float *values, uint64_t values_len, spal_csc_t *out) {
    return csc_create<float>(device, nrows, ncols, colptr, colptr_len, rowind, rowind_len, values,
                             values_len, out);
}
int spal_csc_destroy(spal_csc_t a) {
    if (!a) return SPAL_OK;
    DeviceGuard guard(a->device);
    csc_free(a);
    return SPAL_OK;
}
int spal_csc_shape(spal_csc_t a, uint64_t *nrows, uint64_t *ncols, uint64_t *nnz, int *elem_size) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_shape: handle is NULL");
    if (nrows) *nrows = a->nrows;
    if (ncols) *ncols = a->ncols;
    if (nnz) *nnz = a->nnz;
    if (elem_size) *elem_size = a->elem_size;
    return SPAL_OK;
}
int spal_csc_spmv_f64(spal_csc_t a, const double *x, uint64_t x_len, double *y, uint64_t y_len) {
    return csc_spmv_host<double>(a, x, x_len, y, y_len);
}
int spal_csc_spmv_f32(spal_csc_t a, const float *x, uint64_t x_len, float *y, uint64_t y_len) {
    return csc_spmv_host<float>(a, x, x_len, y, y_len);
}
int spal_csc_spmv_dev_f64(spal_csc_t a, const double *x_dev, double *y_dev, void *stream) {
    return csc_spmv_dev<double>(a, x_dev, y_dev, stream);
}
int spal_csc_spmv_dev_f32(spal_csc_t a, const float *x_dev, float *y_dev, void *stream) {
    return csc_spmv_dev<float>(a, x_dev, y_dev, stream);
}
int spal_csc_to_csr(spal_csc_t a, spal_csr_t *out) {
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_to_csr: null argument");
    *out = nullptr;
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::lock_guard<std::mutex> lock(a->mu);
    return csc_to_csr_arrays(a, out);
}

int spal_csr_to_csc(spal_csr_t a, spal_csc_t *out) {
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_to_csc: null argument");
    *out = nullptr;
    if (!a->parts.empty())
        return fail(SPAL_ERR_UNSUPPORTED, "spal_csr_to_csc: %llu entries do not fit one set of 32-bit device offsets "
                    "(a CSC handle is not split into blocks)", (unsigned long long)a->nnz);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::lock_guard<std::mutex> lock(a->mu);
    OpArrays t;
    SPAL_TRY(transpose_device(a->device, a->elem_size, a->nrows, a->ncols, a->nnz, a->d_rowptr,
                              a->d_colind, a->d_values, a->stream, t));
    return t.adopt(a->device, a->elem_size, a->nrows, a->ncols, out);
}

int spal_csc_download_f64(spal_csc_t a, uint64_t *colptr, uint64_t *rowind, double *values) {
    return csc_download<double>(a, colptr, rowind, values);
}
int spal_csc_download_f32(spal_csc_t a, uint64_t *colptr, uint64_t *rowind, float *values) {
    return csc_download<float>(a, colptr, rowind, values);
}

int spal_csc_autotune_f64(spal_csc_t a, const double *x_dev, double *y_dev, void *stream, int iters) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_autotune: handle is NULL");
    if (a->kernel != 2) return SPAL_OK;  // the scatter kernel has a single form
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return spal_csr_autotune_f64(a->as_csr, x_dev, y_dev, stream, iters);
}
int spal_csc_autotune_f32(spal_csc_t a, const float *x_dev, float *y_dev, void *stream, int iters) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_autotune: handle is NULL");
    if (a->kernel != 2) return SPAL_OK;
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return spal_csr_autotune_f32(a->as_csr, x_dev, y_dev, stream, iters);
}

int spal_csc_set_option(spal_csc_t a, const char *key, int64_t value) {
    if (!a || !key) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_set_option: null argument");
    {   // options of the sparse operations (this handle as their left operand): no plan involved
        int st = SPAL_OK;
        if (ops_set_option(a->ops, a->as_csr, key, value, &st)) return st;
    }
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::lock_guard<std::mutex> lock(a->mu);
    if (!strcmp(key, "lanes_per_col")) {
        if (value == 0) {
            a->lanes_per_col = pick_lanes_csc(a);
            return SPAL_OK;
        }
        if (value < 2 || value > 64 || (value & (value - 1)))
            return fail(SPAL_ERR_INVALID_ARGUMENT, "lanes_per_col must be one of 2,4,8,16,32,64");
        a->lanes_per_col = (int)value;
        return SPAL_OK;
    }
    if (!strcmp(key, "kernel")) {
        // 1 = atomic scatter (the path BASELINE config 4 names), 2 = transposed
        // (the CSR twin and the CSR kernels), 0 = auto = 2
        if (value < 0 || value > 2) return fail(SPAL_ERR_INVALID_ARGUMENT, "kernel must be 0, 1 or 2");
        a->kernel = value == 1 ? 1 : 2;
        if (a->kernel == 1 && !a->rowtiles) return csc_rowtiles_plan(a);   // the scatter path's row tiles: built when the path is selected
        return SPAL_OK;
    }
    if (!strcmp(key, "flush")) {
        // 0 (default) = window rows flushed with global atomics; 1 = LDS windows stored per super-tile,
        // then an ordered reduce (no global atomics; measured 89.6 vs 80.1 us at config 4: the LDS
        // atomics, not the flush, bound the kernel)
        // 2 = global atomics even where the plan allows the neighbour hand-off (0: hand-off when allowed)
        if (value < 0 || value > 2) return fail(SPAL_ERR_INVALID_ARGUMENT, "flush must be 0, 1 or 2");
        a->flush = (int)value;
        return SPAL_OK;
    }
    if (!strcmp(key, "cols_per_block")) {
        // columns of a super-tile of the scatter kernel: 0 = the widest of 4096 / 2048 / 1024 whose row windows fit LDS
        if (value != 0 && value != 1024 && value != 2048 && value != 4096)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "cols_per_block must be 0 (auto), 1024, 2048 or 4096");
        a->user_cols = (int)value;
        return csc_plan_build(a);
    }
    if (!strcmp(key, "ticket")) {
        // neighbour hand-off: 1 = a workgroup's super-tile is its start-order ticket, 0 = its blockIdx, -1 (default) =
        // the ticket unless the device holds all workgroups of the launch at once
        if (value < -1 || value > 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "ticket must be -1 (auto), 0 or 1");
        a->use_ticket = (int)value;
        return SPAL_OK;
    }
    if (!strcmp(key, "row_tiles")) {
        // the scatter path over row tiles (spal_csc_rowtiles.hip): -1 / 1 = where every tile's window of x fits LDS, 0 = never
        if (value < -1 || value > 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "row_tiles must be -1 (auto), 0 or 1");
        a->rowtiles_user = (int)value;
        return csc_rowtiles_plan(a);
    }
    if (!strcmp(key, "row_tile_rows")) {
        if (value != 0 && value != 1024 && value != 2048 && value != 4096)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "row_tile_rows must be 0 (auto), 1024, 2048 or 4096");
        a->rt_rows_user = (uint32_t)value;
        return csc_rowtiles_plan(a);
    }
    if (!strcmp(key, "lds")) {
        if (value != 0 && value != 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "lds must be 0 or 1");
        a->use_lds = (int)value;
        return csc_plan_build(a);
    }
    return fail(SPAL_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
}
int spal_csc_status(spal_csc_t a, int *invalid_products) {
    if (!a || !invalid_products) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_status: null argument");
    std::lock_guard<std::mutex> chain(a->mu_launch);
    *invalid_products = csc_invalid_products(a);
    return SPAL_OK;
}
int spal_csc_describe(spal_csc_t a, char *buf, size_t buf_len) {
    if (!a || !buf || !buf_len) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_describe: null argument");
    snprintf(buf, buf_len,
             "{\"format\": \"csc\", \"dtype\": \"%s\", \"nrows\": %llu, \"ncols\": %llu, \"nnz\": %llu, "
             "\"kernel\": \"%s\", \"cols_per_block\": %d, \"blocks\": %u, \"lanes_per_col\": %d, "
             "\"lds_window_bytes\": %llu, \"lds_col_fraction\": %.4f, \"flush\": \"%s\", "
             "\"window_store_bytes\": %llu, \"ticket\": %d, \"handoff_timeouts\": %d, \"uniform_columns\": %d, "
             "\"row_tiles\": %d, \"row_tile_rows\": %u, \"row_tile_count\": %u, \"row_tile_x_window\": %u, \"row_tiles_failed\": %d}",
             a->elem_size == 8 ? "f64" : "f32", (unsigned long long)a->nrows,
             (unsigned long long)a->ncols, (unsigned long long)a->nnz,
             a->kernel == 2 ? "transposed_csr" : a->lds_entries ? "lds_privatised_scatter" : "atomic_scatter",
             a->cols_per_block, a->nblocks,
             a->lanes_per_col, (unsigned long long)a->lds_entries * (unsigned long long)a->elem_size,
             a->lds_col_fraction, (a->flush == 1 && a->d_windows) ? "windows_then_reduce"
                                  : (a->flush == 0 && a->ordered) ? "neighbour_handoff" : "global_atomics",
             (unsigned long long)a->windows_entries * (unsigned long long)a->elem_size, a->use_ticket < 0 ? a->ticket_auto : a->use_ticket,
             csc_invalid_products(a),
             a->uniform_cols ? 1 : 0,
             (a->rowtiles && a->rowtiles_user != 0 && a->flush == 0) ? 1 : 0, a->rt_rows, a->rt_ntiles, a->rt_xcap, a->rowtiles_failed);
    return ops_describe_append(buf, buf_len, a->ops, a->as_csr);   // "spgemm", "spadd", "spmm", "trsv", "ilu0": those that apply
}

}  // extern "C"
