// spal_ops.hpp -- the host layer the sparse operations share: spal_spgemm.hip, spal_spadd.hip,
// spal_spmm.hip, spal_trsv.hip, spal_trsv_sweep.hip, spal_trsm.hip, spal_ilu.hip, spal_ilu_sweep.hip, spal_krylov.hip, spal_krylov_block.hip, spal_gmres.hip, spal_gmres_block.hip, spal_eigsh.hip, spal_cheb.hip, spal_kpm.hip, spal_colour.hip, spal_amg.hip and spal_fsai.hip keep their kernels, their driver, their option's validation and their
// info JSON; what surrounds a launch the same way in each of them is here, once.  (Not installed.)
#pragma once

#include <chrono>

#ifdef SPAL_OPS_SCAN   // spgemm and spadd define it before the include: nobody else pays for rocprim's headers
#include <rocprim/device/device_scan.hpp>
#endif

#include "cheb_host.hpp"
#include "spal_internal.hpp"

namespace spal {

// ---- small helpers -------------------------------------------------------------------------------------------------
inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

inline unsigned grid_of(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// Device time of up to two spans of a stream's work: span i runs from event 2i to event 2i + 1 (what lies between two
// spans -- a read back, an allocation -- is not counted).
struct EventSpans {
    hipEvent_t e[4] = {};
    EventSpans() = default;
    EventSpans(const EventSpans &) = delete;
    EventSpans &operator=(const EventSpans &) = delete;
    ~EventSpans() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    hipError_t create(int spans) {
        hipError_t r = hipSuccess;
        for (int i = 0; i < 2 * spans && r == hipSuccess; ++i) r = hipEventCreate(&e[i]);
        return r;
    }
    hipError_t span(int i, float *ms) const { return hipEventElapsedTime(ms, e[2 * i], e[2 * i + 1]); }
    float ms(int spans) const {   // the first `spans` together; one that cannot be read counts as 0
        float sum = 0.f, v = 0.f;
        for (int i = 0; i < spans; ++i)
            if (span(i, &v) == hipSuccess) sum += v;
        return sum;
    }
};

#ifdef SPAL_OPS_SCAN
// rocprim's exclusive sum by its own convention: tmp == nullptr asks for the size of the temporary block
template <typename U>
hipError_t scan_step(void *tmp, size_t &bytes, const U *in, U *out, uint64_t n, hipStream_t st) {
    return rocprim::exclusive_scan(tmp, bytes, in, out, U(0), (size_t)n, rocprim::plus<U>(), st);
}
// ... and one whole scan; synchronises `st`
template <typename U>
hipError_t scan_exclusive(const U *in, U *out, uint64_t n, hipStream_t st) {
    size_t bytes = 0;
    DevBuf tmp;
    hipError_t e = scan_step<U>(nullptr, bytes, in, out, n, st);
    if (e == hipSuccess) e = tmp.alloc(bytes);
    if (e == hipSuccess) e = scan_step<U>(tmp.p, bytes, in, out, n, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // (tmp returns to the allocator on exit)
    return e;
}
#endif

// ---- checks several entry points make with the same words ----------------------------------------------------------
template <typename T>
int check_dtype(const char *fn, int elem_size) {
    if (elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle holds %s values", fn, elem_size == 8 ? "f64" : "f32");
    return SPAL_OK;
}

template <typename H>
int check_same_device_and_dtype(const char *fn, const H *a, const H *b) {
    if (a->device != b->device)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: operands on devices %d and %d", fn, a->device, b->device);
    if (a->elem_size != b->elem_size)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: operands of element sizes %d and %d", fn, a->elem_size, b->elem_size);
    return SPAL_OK;
}

// the exact solve's and the sweeps' flags, and what both refuse of a handle before they look at its entries
inline int check_uplo_unit(const char *fn, int uplo, int unit_diag) {
    if (uplo != 0 && uplo != 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: uplo = %d must be 0 (lower) or 1 (upper)", fn, uplo);
    if (unit_diag != 0 && unit_diag != 1)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: unit_diag = %d must be 0 or 1", fn, unit_diag);
    return SPAL_OK;
}
inline int check_solvable(const char *fn, const spal_csr *a) {
    if (!a->parts.empty())
        return fail(SPAL_ERR_UNSUPPORTED, "%s: handles held as row blocks (more than 2^32 - 65537 entries) have no solve", fn);
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn,
                    (unsigned long long)a->nrows, (unsigned long long)a->ncols);
    return SPAL_OK;
}

// ---- CSR and CSC through one body ----------------------------------------------------------------------------------
// Either handle type's arrays as an operand: CSC's (colptr, rowind) are the CSR arrays of the transpose.
struct Operand {
    uint64_t nmajor, nminor, nnz;
    const uint32_t *ptr, *ind;
    const void *val;
};
inline Operand operand_of(const spal_csr *a) { return {a->nrows, a->ncols, a->nnz, a->d_rowptr, a->d_colind, a->d_values}; }
inline Operand operand_of(const spal_csc *a) { return {a->ncols, a->nrows, a->nnz, a->d_colptr, a->d_rowind, a->d_values}; }
// the CSR handle SpMM, the triangular solve and ILU(0) run on, whose `mu` guards their options and plans
inline spal_csr *solve_handle(spal_csr *a) { return a; }
inline spal_csr *solve_handle(spal_csc *a) { return a->as_csr; }
// held as row blocks (a CSC handle never is): the operations on whole matrices refuse such an operand
inline bool row_blocks(const spal_csr *a) { return !a->parts.empty(); }
inline bool row_blocks(const spal_csc *) { return false; }
inline int refuse_row_blocks(const char *fn) {
    return fail(SPAL_ERR_UNSUPPORTED, "%s: an operand of more than 2^32 - 65537 entries (row blocks)", fn);
}

// ---- the three device arrays of a compressed result ----------------------------------------------------------------
// Owned here until a handle adopts them; whatever is still owned returns to the allocator on destruction, as a DevBuf.
struct OpArrays {
    uint32_t *ptr = nullptr, *ind = nullptr;
    void *val = nullptr;
    uint64_t nnz = 0, cap = 0;
    OpArrays() = default;
    OpArrays(const OpArrays &) = delete;
    OpArrays &operator=(const OpArrays &) = delete;
    ~OpArrays() {
        (void)dev_free(ptr);
        (void)dev_free(ind);
        (void)dev_free(val);
    }
    // nmajor + 1 offsets and nnz + kStreamPad entries (the padding contract), the pad zeroed on `st`
    int alloc(uint64_t nmajor, uint64_t entries, size_t elem_size, hipStream_t st) {
        nnz = entries;
        cap = entries + kStreamPad;
        SPAL_HIP_TRY(dev_alloc((void **)&ptr, (nmajor + 1) * 4));
        SPAL_HIP_TRY(dev_alloc((void **)&ind, cap * 4));
        SPAL_HIP_TRY(dev_alloc(&val, cap * elem_size));
        SPAL_HIP_TRY(hipMemsetAsync((char *)ind + nnz * 4, 0, kStreamPad * 4, st));
        SPAL_HIP_TRY(hipMemsetAsync((char *)val + nnz * elem_size, 0, kStreamPad * elem_size, st));
        return SPAL_OK;
    }
    // A handle around the arrays: they are the handle's when the call succeeds and stay here when it fails.  (A CSC
    // handle is always planned by its constructor; its overload takes the CSR one's two flags so that one body serves
    // both types, and ignores them.)
    int adopt(int device, int elem_size, uint64_t nrows, uint64_t ncols, spal_csr **out, bool eager_copies = false,
              bool lazy_plan = false, uint2 *d_win_groups = nullptr, uint32_t win_groups = 0, uint32_t win_group_bits = 0) {
        SPAL_TRY(csr_adopt_device(device, elem_size, nrows, ncols, nnz, cap, ptr, ind, val, out, eager_copies, lazy_plan,
                                  d_win_groups, win_groups, win_group_bits));
        ptr = ind = nullptr;
        val = nullptr;
        return SPAL_OK;
    }
    int adopt(int device, int elem_size, uint64_t nrows, uint64_t ncols, spal_csc **out, bool = false, bool = false) {
        SPAL_TRY(csc_adopt_device(device, elem_size, nrows, ncols, nnz, cap, ptr, ind, val, out));
        ptr = ind = nullptr;
        val = nullptr;
        return SPAL_OK;
    }
};

// implemented in spal_transpose.hip: stable sort of the entries by their minor index (compressed-by-major ->
// compressed-by-minor) into `out`
int transpose_device(int device, int elem_size, uint64_t nmajor, uint64_t nminor, uint64_t nnz, const uint32_t *d_ptr,
                     const uint32_t *d_ind, const void *d_val, hipStream_t st, OpArrays &out);

// ---- Jacobi sweeps on a triangle, for callers that bring their own scratch (spal_trsv_sweep.hip) --------
// Both take a->mu themselves.  prepare: builds the handle's sweep rows if it has none (synchronises `st`); refuses what
// the exact solve refuses, a row without a diagonal unless unit_diag.  Afterwards a->d_sweep_rows is there until the
// handle is freed and never changes: spal_ilu_sweep.hip reads the diagonals' positions from it without the lock.  enqueue: x = sweep(a, uplo, unit_diag, sweeps, b)
// on `st`, allocating and synchronising nothing on a prepared handle; b, x, w0, w1 are device vectors of a's element
// type, w0 is written when sweeps >= 1 and w1 when sweeps >= 2, x may be b.
int trsv_sweep_prepare(const char *fn, spal_csr *a, int unit_diag, hipStream_t st);
int trsv_sweep_enqueue(const char *fn, spal_csr *a, int uplo, int unit_diag, uint64_t sweeps, const void *b, void *x,
                       void *w0, void *w1, hipStream_t st);
int64_t trsv_sweeps_of(spal_csr *a);   // the option "trsv_sweeps" of a solve handle, read under its lock

// ---- the AMG hierarchy as a preconditioner (spal_amg.hip), for spal_krylov.hip -----------------------------
// match: g is there and agrees with a matrix of `nrows` rows in rows, device and element type.  enqueue: x = cycle(0, b)
// on `st` (x != b, device vectors of g's element type); takes g's lock, allocates and synchronises nothing.
int amg_check_match(const char *fn, const spal_amg *g, uint64_t nrows, int device, int elem_size);
int amg_apply_enqueue(const char *fn, spal_amg *g, const void *b, void *x, hipStream_t st);

// ---- the FSAI factor as a preconditioner (spal_fsai.hip), for spal_krylov.hip ------------------------------
// match: as amg_check_match.  enqueue: x = Gt * (G * b) on `st` through u (b, u and x distinct device vectors of f's
// element type): two products of planned handles; takes no lock of f, allocates and synchronises nothing.
int fsai_check_match(const char *fn, const spal_fsai *f, uint64_t nrows, int device, int elem_size);
int fsai_apply_enqueue(const char *fn, spal_fsai *f, const void *b, void *u, void *x, hipStream_t st);

// ---- the Chebyshev filter's launches (spal_cheb.hip), for spal_eigsh.hip -----------------------------------
// All on a solve handle's plain arrays, enqueued on `st`, allocating and synchronising nothing.  chunk: the option
// "cheb_chunk" (0 = default).  rowsum: out = rowsum(y), out != y.  apply: out = t_d through `work` (n elements, unused
// at degree 1); x, out and work are distinct.  gershgorin_run synchronises `st`.
template <typename T>
int cheb_rowsum_enqueue(const char *fn, spal_csr *a, const T *y, T *out, unsigned chunk, hipStream_t st);
template <typename T>
int cheb_apply_enqueue(const char *fn, spal_csr *a, const ChebCoeffs<T> &k, const T *x, T *out, T *work, unsigned chunk,
                       hipStream_t st);
int gershgorin_run(const char *fn, spal_csr *a, hipStream_t st, double *glo, double *ghi);
// series: s = cheb_series(x) through w1 and w2; x, s, w1 and w2 are distinct vectors of n elements, x is
// only read.  form: the option "cheb_series_form" (0 or 1 = the fused step, 2 = step and accumulation apart; the same bits).
template <typename T>
int cheb_series_enqueue(const char *fn, spal_csr *a, const ChebSeries<T> &k, const T *x, T *s, T *w1, T *w2, unsigned chunk,
                        int form, hipStream_t st);

// ---- per-operation state of a handle (spal_internal.hpp: OpState), set and described in one place -------------------
// Each operation file implements its own: 1 = the key is this operation's and *status says how setting it went, 0 =
// another key.  The solve's and ILU(0)'s options live on the solve handle, under its `mu`.
int spgemm_option(const char *key, int64_t value, OpState &s, int *status);   // "spgemm_route", "spgemm_lds_cap"
int spadd_option(const char *key, int64_t value, OpState &s, int *status);    // "spadd_tile"
int spmm_option(const char *key, int64_t value, OpState &s, int *status);     // "spmm_tile"
int trsv_option(spal_csr *a, const char *key, int64_t value, int *status);    // "trsv_chain_rows" (launch lists rebuilt)
int trsv_sweep_option(spal_csr *a, const char *key, int64_t value, int *status);   // "trsv_sweeps"
int trsm_option(spal_csr *a, const char *key, int64_t value, int *status);    // "trsm_tile"
int ilu_option(spal_csr *a, const char *key, int64_t value, int *status);     // "ilu_wide_work"
int krylov_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status);   // "krylov_check_every"
int krylov_block_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status);   // "krylov_tile"
int eigsh_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status);   // "eigsh_rotate"
int cheb_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status);    // "cheb_chunk", "cheb_series_form"
int kpm_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status);     // "kpm_tile", "kpm_form"
int fsai_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status);    // "fsai_max_row"
inline int ops_set_option(OpState &s, spal_csr *solve, const char *key, int64_t value, int *status) {
    return spgemm_option(key, value, s, status) || spadd_option(key, value, s, status) ||
           spmm_option(key, value, s, status) || trsv_option(solve, key, value, status) ||
           trsv_sweep_option(solve, key, value, status) || trsm_option(solve, key, value, status) ||
           ilu_option(solve, key, value, status) || krylov_option(solve, key, value, s, status) ||
           krylov_block_option(solve, key, value, s, status) || eigsh_option(solve, key, value, s, status) ||
           cheb_option(solve, key, value, s, status) || kpm_option(solve, key, value, s, status) ||
           fsai_option(solve, key, value, s, status);
}

// (describe_append itself is host code: spal_host.cpp, declared in spal_internal.hpp)
// the "spmm" / "trsv" objects of a handle an SpMM ran on / a triangle of which was analysed (spal_spmm.hip, spal_trsv.hip)
int spmm_describe_append(char *buf, size_t buf_len, const spal_csr *a);
int trsv_describe_append(char *buf, size_t buf_len, spal_csr *a);
// the "trsv_sweep" object of a handle prepared for Jacobi sweeps (spal_trsv_sweep.hip)
int trsv_sweep_describe_append(char *buf, size_t buf_len, spal_csr *a);
// the "trsm" object of a handle a block of right-hand sides was solved or swept on (spal_trsm.hip)
int trsm_describe_append(char *buf, size_t buf_len, spal_csr *a);
// the "krylov" object of a handle a solve ran with as A (spal_krylov.hip; the string is read under the solve handle's lock)
int krylov_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
// the "krylov_block" object of a handle spal_*_krylov_block_* ran with as A (spal_krylov_block.hip; the same lock)
int krylov_block_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
// the "gmres" object of a handle spal_*_gmres_* ran with as A (spal_gmres.hip; read under the same lock)
int gmres_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
// the "gmres_block" object of a handle spal_*_gmres_block_* ran with as A (spal_gmres_block.hip; the same lock)
int gmres_block_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
// the "eigsh" object of a handle spal_*_eigsh_* ran with as A (spal_eigsh.hip; the same lock)
int eigsh_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
// the "eigsh_filter" object of a handle spal_*_eigsh_filtered_* ran with as A (spal_eigsh.hip; the same lock)
int eigsh_filter_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
// the "eigsh_near" object of a handle spal_*_eigsh_near_* ran with as A (spal_eigsh.hip; the same lock)
int eigsh_near_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
// the "kpm" object of a handle spal_*_kpm_moments_* ran with as A (spal_kpm.hip; the same lock)
int kpm_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve);
inline int ops_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    SPAL_TRY(describe_append(buf, buf_len, "spgemm", s.spgemm_info));   // a product of spal_*_mul: how it was built
    SPAL_TRY(describe_append(buf, buf_len, "spadd", s.spadd_info));     // a result of spal_*_add / _sub / _neg
    SPAL_TRY(spmm_describe_append(buf, buf_len, solve));                // an SpMM ran on it
    SPAL_TRY(trsv_describe_append(buf, buf_len, solve));                // a triangle of it was analysed for a solve
    SPAL_TRY(trsv_sweep_describe_append(buf, buf_len, solve));          // it was prepared for sweeps on a triangle
    SPAL_TRY(trsm_describe_append(buf, buf_len, solve));                // a block of right-hand sides ran on it
    SPAL_TRY(describe_append(buf, buf_len, "ilu0", s.ilu_info));        // a factor of spal_*_ilu0: how it was built
    SPAL_TRY(describe_append(buf, buf_len, "ilu0_sweep", s.ilu_sweep_info));   // ... of spal_*_ilu0_sweep
    SPAL_TRY(krylov_describe_append(buf, buf_len, s, solve));           // spal_*_krylov_* ran with it as A: the last call
    SPAL_TRY(krylov_block_describe_append(buf, buf_len, s, solve));     // spal_*_krylov_block_* ran with it as A: the last call
    SPAL_TRY(gmres_describe_append(buf, buf_len, s, solve));            // spal_*_gmres_* ran with it as A: the last call
    SPAL_TRY(gmres_block_describe_append(buf, buf_len, s, solve));      // spal_*_gmres_block_* ran with it as A: the last call
    SPAL_TRY(eigsh_describe_append(buf, buf_len, s, solve));            // spal_*_eigsh_* ran with it as A: the last call
    SPAL_TRY(eigsh_filter_describe_append(buf, buf_len, s, solve));     // spal_*_eigsh_filtered_* ran with it as A: the last call
    SPAL_TRY(eigsh_near_describe_append(buf, buf_len, s, solve));       // spal_*_eigsh_near_* ran with it as A: the last call
    SPAL_TRY(kpm_describe_append(buf, buf_len, s, solve));              // spal_*_kpm_moments_* ran with it as A: the last call
    return describe_append(buf, buf_len, "ordering", s.ordering_info);  // a result of spal_*_permute / _multicolour
}

}  // namespace spal
