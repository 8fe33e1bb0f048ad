// spal_coo.hip -- the COO handle (upload, describe, destroy) and the spal_coo_* entry points; the assembly itself is
// spal_coo_assemble.hip.
#include "coo_internal.hpp"

namespace spal {

static void coo_free(spal_coo *c) {
    if (!c) return;
    if (c->h_back) (void)hipHostFree(c->h_back);
    (void)dev_free(c->d_work);
    (void)dev_free(c->d_rows);
    (void)dev_free(c->d_cols);
    (void)dev_free(c->d_vals);
    delete c;
}

template <typename T>
static int coo_upload(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                      const uint64_t *cols, const T *vals, spal_coo_t *out) {
    if (!out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_coo_upload: out is NULL");
    *out = nullptr;
    if (len && (!rows || !cols || !vals))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_coo_upload: null array");
    // CooMatrix::new asserts (src/coo.rs:105-106)
    if (!(nrows > 0)) return fail(SPAL_ERR_INVARIANT, "CooMatrix::new would panic: assertion failed: nrows > 0");
    if (!(ncols > 0)) return fail(SPAL_ERR_INVARIANT, "CooMatrix::new would panic: assertion failed: ncols > 0");
    // A COO handle assembles to CSR (pointer array over nrows + 1) and to CSC (over ncols + 1): whichever becomes
    // the MAJOR dimension needs dim + 1 to fit 32 bits, so both are bounded alike here (spal_csr_create / spal_csc_create
    // know their major dimension and allow the minor one to be exactly 2^32 - 1).
    if (nrows >= 0xffffffffull || ncols >= 0xffffffffull || len > kMaxEntries)
        return fail(SPAL_ERR_UNSUPPORTED, "COO shape does not fit 32-bit device indices (nrows, ncols < 2^32 - 1)");
    // every entry inside the matrix (push asserts, src/coo.rs:432-433)
    std::vector<uint32_t> r32(len), c32(len);
    std::vector<uint64_t> bad(host_threads(), UINT64_MAX);  // first offending entry of every thread's range
    parallel_for(len, [&](uint64_t b, uint64_t e, unsigned t) {
        for (uint64_t i = b; i < e; ++i) {
            if (rows[i] >= nrows || cols[i] >= ncols) { bad[t] = i; return; }
            r32[i] = (uint32_t)rows[i];
            c32[i] = (uint32_t)cols[i];
        }
    });
    uint64_t first_bad = UINT64_MAX;
    for (uint64_t f : bad) first_bad = std::min(first_bad, f);
    if (first_bad != UINT64_MAX) {  // the entry a sequence of push() calls would have panicked on (row is asserted first)
        const bool row_bad = rows[first_bad] >= nrows;
        return fail(SPAL_ERR_INDEX_OUT_OF_BOUNDS,
                    "CooMatrix::push would panic: assertion failed: %s (entry %llu: %s %llu)",
                    row_bad ? "row < nrows" : "col < ncols", (unsigned long long)first_bad, row_bad ? "row" : "col",
                    (unsigned long long)(row_bad ? rows[first_bad] : cols[first_bad]));
    }
    DeviceGuard guard(device);
    if (guard.status != SPAL_OK) return guard.status;
    spal_coo *c = new spal_coo;
    c->device = device; c->elem_size = (int)sizeof(T);
    c->nrows = nrows; c->ncols = ncols; c->len = len;
    hipError_t e = dev_alloc((void **)&c->d_rows, std::max<uint64_t>(len, 1) * 4);
    if (e == hipSuccess) e = dev_alloc((void **)&c->d_cols, std::max<uint64_t>(len, 1) * 4);
    if (e == hipSuccess) e = dev_alloc((void **)&c->d_vals, std::max<uint64_t>(len, 1) * sizeof(T));
    if (e == hipSuccess && len) e = hipMemcpy(c->d_rows, r32.data(), len * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && len) e = hipMemcpy(c->d_cols, c32.data(), len * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && len) e = hipMemcpy(c->d_vals, vals, len * sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess && len) {  // the assembly's workspace: setup, not the timed path
        c->work_bytes = coo_workspace_layout(len, nrows, sizeof(T)).bytes;
        e = dev_alloc((void **)&c->d_work, c->work_bytes);
    }
    if (e != hipSuccess) {
        coo_free(c);
        return fail(e == hipErrorOutOfMemory ? SPAL_ERR_OUT_OF_MEMORY : SPAL_ERR_HIP,
                    "spal_coo_upload: upload failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return SPAL_OK;
}

template <typename T>
static int coo_to_csr(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                      const uint64_t *cols, const T *vals, spal_csr_t *out) {
    if (!out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_coo_to_csr: out is NULL");
    *out = nullptr;
    spal_coo_t c = nullptr;
    SPAL_TRY(coo_upload<T>(device, nrows, ncols, len, rows, cols, vals, &c));
    int st = spal_coo_assemble_csr(c, nullptr, out);
    spal_coo_destroy(c);
    return st;
}

template <typename T>
static int coo_to_csc(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                      const uint64_t *cols, const T *vals, spal_csc_t *out) {
    if (!out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_coo_to_csc: out is NULL");
    *out = nullptr;
    spal_coo_t c = nullptr;
    SPAL_TRY(coo_upload<T>(device, nrows, ncols, len, rows, cols, vals, &c));
    int st = spal_coo_assemble_csc(c, nullptr, out);
    spal_coo_destroy(c);
    return st;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_coo_upload_f64(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                        const uint64_t *cols, const double *vals, spal_coo_t *out) {
    return coo_upload<double>(device, nrows, ncols, len, rows, cols, vals, out);
}
int spal_coo_upload_f32(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                        const uint64_t *cols, const float *vals, spal_coo_t *out) {
    return coo_upload<float>(device, nrows, ncols, len, rows, cols, vals, out);
}
int spal_coo_destroy(spal_coo_t c) {
    if (!c) return SPAL_OK;
    DeviceGuard guard(c->device);
    coo_free(c);
    return SPAL_OK;
}
int spal_coo_describe(spal_coo_t c, char *buf, size_t buf_len) {
    if (!c || !buf || !buf_len) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_coo_describe: null argument");
    snprintf(buf, buf_len,
             "{\"format\": \"coo\", \"dtype\": \"%s\", \"nrows\": %llu, \"ncols\": %llu, \"len\": %llu, "
             "\"last_route\": \"%s\", \"group_rows\": %d, \"group_cap\": %d, \"group_relaunches\": %d, "
             "\"lookback_gave_up\": %d, \"ticket_mode\": %d, \"packed_payload\": %d, \"offsets_from_counts\": %d, \"row_sort\": %d}",
             c->elem_size == 8 ? "f64" : "f32", (unsigned long long)c->nrows, (unsigned long long)c->ncols,
             (unsigned long long)c->len, c->last_group_rows ? "local_sort" : "general", c->last_group_rows,
             c->last_group_cap, c->last_relaunches, c->last_lookback_gave_up, c->last_ticket, c->last_packed, c->last_offsets, c->last_row_sort);
    return SPAL_OK;
}
int spal_coo_assemble_csr(spal_coo_t c, void *stream, spal_csr_t *out) {
    if (!c || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_coo_assemble_csr: null argument");
    *out = nullptr;
    DeviceGuard guard(c->device);
    if (guard.status != SPAL_OK) return guard.status;
    const CooKnobs knobs = coo_read_knobs();
    Assembled r;
    SPAL_TRY(coo_assemble(c, false, (hipStream_t)stream, knobs, r));
    return r.adopt(c->device, c->elem_size, c->nrows, c->ncols, out, false, !knobs.eager_plan,
                   r.d_gwin, r.gwin_n, r.gwin_bits);   // (takes the spans' block, also when it fails)
}
int spal_coo_assemble_csc(spal_coo_t c, void *stream, spal_csc_t *out) {
    if (!c || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_coo_assemble_csc: null argument");
    *out = nullptr;
    DeviceGuard guard(c->device);
    if (guard.status != SPAL_OK) return guard.status;
    Assembled r;
    SPAL_TRY(coo_assemble(c, true, (hipStream_t)stream, coo_read_knobs(), r));
    (void)dev_free(r.d_gwin);   // (the groups' ROW spans: the CSC planner has no use for them)
    r.d_gwin = nullptr;
    return r.adopt(c->device, c->elem_size, c->nrows, c->ncols, out);
}
int spal_coo_to_csr_f64(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                        const uint64_t *cols, const double *vals, spal_csr_t *out) {
    return coo_to_csr<double>(device, nrows, ncols, len, rows, cols, vals, out);
}
int spal_coo_to_csr_f32(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                        const uint64_t *cols, const float *vals, spal_csr_t *out) {
    return coo_to_csr<float>(device, nrows, ncols, len, rows, cols, vals, out);
}
int spal_coo_to_csc_f64(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                        const uint64_t *cols, const double *vals, spal_csc_t *out) {
    return coo_to_csc<double>(device, nrows, ncols, len, rows, cols, vals, out);
}
int spal_coo_to_csc_f32(int device, uint64_t nrows, uint64_t ncols, uint64_t len, const uint64_t *rows,
                        const uint64_t *cols, const float *vals, spal_csc_t *out) {
    return coo_to_csc<float>(device, nrows, ncols, len, rows, cols, vals, out);
}

}  // extern "C"
