// krylov_kernels.hpp -- what spal_krylov.hip (the dot product, CG, BiCGStab: DESIGN 3.14), spal_krylov_block.hip (the
// same two loops on a block of right-hand sides: DESIGN 3.22), spal_gmres.hip (GMRES: DESIGN 3.17) and
// spal_gmres_block.hip (GMRES on a block: DESIGN 3.23) share: the tile sum and the upper levels of reduce(), the scalar
// block, the fused vector updates and the scalar steps of CG and BiCGStab (their names, and the two loops that enqueue
// them, are in krylov_loops.hpp), the sizes of a dot's scratch, the entry points a driver goes through by handle and
// element type, the preparation of the plans, M^-1, the refusals that need no device, and the frame of a call: the
// launch-and-check macro, SolveFrame (pinned heads, polls, device time), the locked store of a describe string and the
// staging of host vectors.  For the block drivers: the column tiles and their dispatch macro, column_tree, the routes
// to SpMM and trsm, M^-1 on a block, the refusals of k / ldb / ldx, the sweep scratch and the staging of host blocks.
// The contracts are written out in include/spal.h.  (Not installed.)
#pragma once

#include "krylov_loops.hpp"
#include "spal_ops.hpp"

#include <cmath>
#include <limits>

#pragma clang fp contract(off)

namespace spal {

constexpr uint64_t kTile = 1024;
constexpr int kThreads = 256;
constexpr unsigned kMaxGrid = 4096;   // first-level workgroups of a launch; each walks tiles blockIdx.x, + gridDim.x, ...

// The sum of one tile, valid in thread 0.  `lds` holds kThreads elements; ends with a barrier, so it can be reused.
template <typename T>
__device__ __forceinline__ T tile_sum(T v0, T v1, T v2, T v3, T *lds) {
    const unsigned t = threadIdx.x;
    T a = (v0 + v2) + (v1 + v3);                 // h = 512 (e[t], e[t + 256]), then h = 256
    lds[t] = a;
    __syncthreads();
    if (t < 128) {
        a = lds[t] + lds[t + 128];               // h = 128
        if (t >= 64) lds[t] = a;                 // (its own slot: nobody else read it)
    }
    __syncthreads();
    if (t < 64) {
        a = a + lds[t + 64];                     // h = 64
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) a = a + __shfl_down(a, h, 64);
    }
    __syncthreads();
    return a;
}

// `part` holds the c1 sums of the first level, then room for every further level; returns reduce()'s result.  The
// workgroup reads what it stored a level earlier: __syncthreads() orders that (workgroup scope), as in trsv_chain.
template <typename T>
__device__ T upper_levels(T *part, uint64_t c1, T *lds) {
    T *in = part;
    uint64_t m = c1;
    while (m > 1) {
        const uint64_t c = (m + kTile - 1) / kTile;
        T *out = in + m;
        for (uint64_t tile = 0; tile < c; ++tile) {
            const uint64_t i = tile * kTile + threadIdx.x;
            T v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = i + (uint64_t)k * kThreads < m ? in[i + (uint64_t)k * kThreads] : T(0);
            const T s = tile_sum<T>(v[0], v[1], v[2], v[3], lds);
            if (threadIdx.x == 0) out[tile] = s;
        }
        __syncthreads();
        in = out;
        m = c;
    }
    return in[0];
}

// ---- what the vector loops (spal_krylov.hip) and the block loops (spal_krylov_block.hip) share on the device ----------
// The scalars of one call -- of one column of a block call --, on the device; the host reads a copy in pinned memory
// when it polls.
template <typename T>
struct Scal {
    T rr, bb, thr, rz, alpha, beta, omega, rho;
    unsigned long long it;
    unsigned done, reason, half, pad;
    // MINRES (rr holds pp): the Lanczos and rotation state, then what the vector updates read
    T lbeta, oldb, dbar, epsln, cs, sn, phibar, alfa;
    T c1, c2, oldeps, delta, denom, phi, sinv;
};

// The scalars an update reads, loaded once per launch (per column of a block); `go`: the call has not stopped.
template <typename T>
struct Coef {
    T alpha, beta, omega, c3, c4;
    bool go;
};
// Whether update OP still runs: everything freezes at the stop, except the one update that the stop left behind --
// V_BI_HALF runs only then, V_MR_WX runs then too (without its last part).
template <typename T, int OP>
__device__ __forceinline__ bool op_live(const Scal<T> *s) {
    if (OP == V_BI_HALF) return s->half != 0;
    if (OP == V_MR_WX) return s->done == 0 || s->half != 0;
    return s->done == 0;
}
template <typename T, int OP>
__device__ __forceinline__ Coef<T> op_coef(const Scal<T> *s, T sg) {
    if (OP == V_MR_WX) return {s->oldeps, s->delta, s->denom, s->phi, s->sinv, s->done == 0};
    if (OP >= V_MR_R0) return {sg, s->c1, s->c2, s->sinv, T(0), true};
    return {s->alpha, s->beta, s->omega, T(0), T(0), true};
}

// (the updates by name, VecOp, and the scalar steps by name, FinOp: krylov_loops.hpp)
template <int OP> struct Dots {
    static constexpr int n = (OP == V_CG_P || OP == V_BI_P || OP == V_BI_HALF || OP == V_MR_V || OP == V_MR_T2_PRE || OP == V_MR_WX) ? 0
                             : (OP == V_DOT2 || OP == V_INIT || OP == V_MR_R0)                                                       ? 2
                                                                                                                                     : 1;
};

// What update OP reads and writes of an element, and its arithmetic on the values alone: x and y come in as loaded (or
// as anything, where OP does not read them) and go out as what OP stores.  p0 / p1: the element's products for d0 / d1.
// z is the third written operand, V_MR_WX's alone.
template <int OP> struct Reads {
    static constexpr bool c = OP == V_BI_XR || OP == V_MR_R0, d = OP == V_BI_XR;
    static constexpr bool x = OP == V_CG_XR || OP == V_BI_HALF || OP == V_BI_XR || OP == V_MR_WX;
    static constexpr bool y = OP == V_CG_XR || OP == V_CG_P || OP == V_BI_P || OP == V_MR_T1 || OP == V_MR_T2 || OP == V_MR_T2_PRE || OP == V_MR_WX;
    static constexpr bool b = OP != V_CG_P && OP != V_MR_V && OP != V_MR_T2 && OP != V_MR_T2_PRE;   // every OP reads a
    static constexpr bool z = OP == V_MR_WX;
};
template <int OP> struct Writes {
    static constexpr bool x = Reads<OP>::x;
    static constexpr bool y = OP != V_DOT && OP != V_DOT2;
    static constexpr bool z = Reads<OP>::z;
};
template <typename T, int OP>
__device__ __forceinline__ void vec_value(T a, T b, T c, T d, T &x, T &y, T &z, const Coef<T> &k, T &p0, T &p1) {
    const T alpha = k.alpha, beta = k.beta, omega = k.omega;
    if (OP == V_MR_R0) {
        y = a - (b - alpha * c);           // alpha: sg
        p0 = y * y;
        p1 = a * a;
    } else if (OP == V_MR_V) {
        y = a * k.c3;                      // c3: s
    } else if (OP == V_MR_T1) {
        y = (y - alpha * a) - beta * b;    // beta: c1
        p0 = a * y;
    } else if (OP == V_MR_T2 || OP == V_MR_T2_PRE) {
        y = y - omega * a;                 // omega: c2
        p0 = y * y;
    } else if (OP == V_MR_WX) {            // alpha, beta, omega, c3, c4: oldeps, delta, denom, phi, s
        y = ((z - alpha * y) - beta * b) * omega;
        x = x + k.c3 * y;
        if (k.go) z = a * k.c4;            // stopped: v stays
    } else if (OP == V_DOT) {
        p0 = a * b;
    } else if (OP == V_DOT2) {
        p0 = a * b;
        p1 = a * a;
    } else if (OP == V_INIT) {
        y = a - b;
        p0 = y * y;
        p1 = a * a;
    } else if (OP == V_COPY_DOT) {
        p0 = a * b;
        y = b;
    } else if (OP == V_CG_XR) {
        x = x + alpha * a;
        y = y - alpha * b;
        p0 = y * y;
    } else if (OP == V_CG_P) {
        y = a + beta * y;
    } else if (OP == V_BI_P) {
        y = a + beta * (y - omega * b);
    } else if (OP == V_BI_S) {
        y = a - alpha * b;
        p0 = y * y;
    } else if (OP == V_BI_HALF) {
        x = x + alpha * a;
        y = b;
    } else if (OP == V_BI_XR) {
        x = (x + alpha * a) + omega * b;
        y = c - omega * d;
        p0 = y * y;
    }
}

// One element of update OP through memory: every pointer is AT the element (of a vector, or of a column of a row-major
// block), and the ones OP does not name are never dereferenced.  Nothing is __restrict__, and nothing needs to be: two
// operands are either the same array (z is r, ph is p, sh is s -- all of them only read) or disjoint, and an element's
// update touches that element's index alone, so loading everything before the first store changes nothing.
template <typename T, int OP>
__device__ __forceinline__ void vec_update(const T *a, const T *b, const T *c, const T *d, T *x, T *y, T *z, const Coef<T> &k,
                                           T &p0, T &p1) {
    const T av = *a, bv = Reads<OP>::b ? *b : T(0), cv = Reads<OP>::c ? *c : T(0), dv = Reads<OP>::d ? *d : T(0);
    T xv = Reads<OP>::x ? *x : T(0), yv = Reads<OP>::y ? *y : T(0), zv = Reads<OP>::z ? *z : T(0);
    vec_value<T, OP>(av, bv, cv, dv, xv, yv, zv, k, p0, p1);
    if (Writes<OP>::x) *x = xv;
    if (Writes<OP>::y) *y = yv;
    if (Writes<OP>::z) *z = zv;
}

// ---- the scalar step that follows a dot: thread 0 of the launch that walked the upper levels --------------------------
template <typename T>
__device__ __forceinline__ void stop_test(Scal<T> *s, T rr, uint64_t maxit) {
    s->rr = rr;
    if (rr <= s->thr) {
        s->done = 1;
        s->reason = 0;
    } else if (!isfinite(rr)) {
        s->done = 1;
        s->reason = 2;
    } else if (s->it == maxit) {
        s->done = 1;
        s->reason = 1;
    }
}

// d0 / d1: the dots the launch finished; tol2 = T(tol * tol); unpreconditioned (F_TEST_CG): z is r, so rz1 = rr and beta
// follows here
template <typename T, int OP>
__device__ __forceinline__ void scalar_step(Scal<T> *s, T d0, T d1, T tol2, uint64_t maxit, int unpreconditioned) {
    if (OP == F_INIT) {
        s->bb = d1;
        s->thr = tol2 * d1;
        s->it = 0;
        s->rho = s->alpha = s->omega = T(1);
        stop_test<T>(s, d0, maxit);
    } else if (OP == F_RZ) {
        s->rz = d0;
    } else if (OP == F_ALPHA_CG) {
        s->alpha = s->rz / d0;
    } else if (OP == F_TEST_CG) {
        s->it += 1;
        stop_test<T>(s, d0, maxit);
        if (unpreconditioned && !s->done) {
            s->beta = d0 / s->rz;
            s->rz = d0;
        }
    } else if (OP == F_BETA) {
        s->beta = d0 / s->rz;
        s->rz = d0;
    } else if (OP == F_RHO) {
        s->beta = (d0 / s->rho) * (s->alpha / s->omega);
        s->rho = d0;
    } else if (OP == F_ALPHA_BI) {
        s->alpha = s->rho / d0;
    } else if (OP == F_HALF) {
        s->it += 1;
        const bool small = d0 <= s->thr;
        if (small || !isfinite(d0)) {
            s->rr = d0;
            s->reason = small ? 0 : 2;
            s->half = 1;
            s->done = 1;
        }
    } else if (OP == F_OMEGA) {
        s->omega = d0 / d1;
    } else if (OP == F_TEST_BI) {
        stop_test<T>(s, d0, maxit);
    } else if (OP == F_MR_BB) {
        s->bb = d0;
    } else if (OP == F_MR_INIT) {
        const T bb = unpreconditioned ? d1 : s->bb;
        s->bb = bb;
        s->thr = tol2 * bb;
        s->it = 0;
        const T beta = sqrt(d0);   // IEEE, correctly rounded, as is every / below
        s->lbeta = s->phibar = beta;
        s->oldb = s->dbar = s->epsln = s->sn = s->c1 = T(0);
        s->cs = T(-1);
        stop_test<T>(s, beta * beta, maxit);
        if (!s->done) s->sinv = T(1) / beta;
    } else if (OP == F_MR_ALFA) {
        s->alfa = d0;
        s->c2 = d0 / s->lbeta;
    } else if (OP == F_MR_ROT) {
        const T oldb = s->lbeta, beta = sqrt(d0), cs = s->cs, sn = s->sn, dbar = s->dbar, alfa = s->alfa;
        s->oldb = oldb;
        s->lbeta = beta;
        s->it += 1;
        s->oldeps = s->epsln;
        s->delta = (cs * dbar) + (sn * alfa);
        const T gbar = (sn * dbar) - (cs * alfa);
        s->epsln = sn * beta;
        s->dbar = -(cs * beta);
        const T gamma = sqrt((gbar * gbar) + (beta * beta));
        s->cs = gbar / gamma;
        s->sn = beta / gamma;
        s->phi = s->cs * s->phibar;
        s->phibar = s->sn * s->phibar;
        s->denom = T(1) / gamma;
        stop_test<T>(s, s->phibar * s->phibar, maxit);
        if (s->done) {
            s->half = 1;   // V_MR_WX behind this launch still applies this iteration's w and x
        } else {
            s->sinv = T(1) / beta;
            s->c1 = beta / oldb;   // the next iteration's: its beta / oldb are these
        }
    }
}

inline uint64_t tiles_of(uint64_t n) { return std::max<uint64_t>(1, (n + kTile - 1) / kTile); }
// elements of the scratch of ONE dot over n elements: the first level's sums and every level above
inline uint64_t scratch_elems(uint64_t n) {
    uint64_t m = tiles_of(n), total = m;
    while (m > 1) {
        m = (m + kTile - 1) / kTile;
        total += m;
    }
    return total;
}
inline unsigned first_level_grid(uint64_t n) { return (unsigned)std::min<uint64_t>(tiles_of(n), kMaxGrid); }

// ---- the entry points the driver goes through, by handle and element type -------------------------------------------
inline int mul_dev(spal_csr *a, const double *x, double *y, void *st) { return spal_csr_spmv_dev_f64(a, x, y, st); }
inline int mul_dev(spal_csr *a, const float *x, float *y, void *st) { return spal_csr_spmv_dev_f32(a, x, y, st); }
inline int mul_dev(spal_csc *a, const double *x, double *y, void *st) { return spal_csc_spmv_dev_f64(a, x, y, st); }
inline int mul_dev(spal_csc *a, const float *x, float *y, void *st) { return spal_csc_spmv_dev_f32(a, x, y, st); }
inline int solve_dev(spal_csr *m, int uplo, int unit, const double *b, double *x, void *st) { return spal_csr_trsv_dev_f64(m, uplo, unit, b, x, st); }
inline int solve_dev(spal_csr *m, int uplo, int unit, const float *b, float *x, void *st) { return spal_csr_trsv_dev_f32(m, uplo, unit, b, x, st); }
inline int solve_dev(spal_csc *m, int uplo, int unit, const double *b, double *x, void *st) { return spal_csc_trsv_dev_f64(m, uplo, unit, b, x, st); }
inline int solve_dev(spal_csc *m, int uplo, int unit, const float *b, float *x, void *st) { return spal_csc_trsv_dev_f32(m, uplo, unit, b, x, st); }
inline int analyse(spal_csr *m, int uplo, int unit, void *st) { return spal_csr_trsv_analyse(m, uplo, unit, st); }
inline int analyse(spal_csc *m, int uplo, int unit, void *st) { return spal_csc_trsv_analyse(m, uplo, unit, st); }
inline int product_plan(spal_csr *a) { return spal_csr_plan(a); }
inline int product_plan(spal_csc *) { return SPAL_OK; }   // planned, twin included, by its constructor

// ---- the frame of a solver call, the same in all four drivers ---------------------------------------------------------
// The helpers of this layer live in the four driver files alone: the library does not export them.
#define KRYLOV_LOCAL __attribute__((visibility("hidden")))

// Launch and check: `fn` and `st` are the caller's, and so is the `return`.
#define KRYLOV_LAUNCH(kernel, grid, ...)                                                                       \
    do {                                                                                                       \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, st, __VA_ARGS__);                             \
        const hipError_t le_ = hipGetLastError();                                                              \
        if (le_ != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(le_)); \
    } while (0)

// The `count` heads of a call (Scal or GHead: what the host polls) in pinned memory, the call's device time and its
// polls.  create() comes after the call's device allocations; begin .. end is the span that "solve_ms" reports.
template <typename Head>
struct KRYLOV_LOCAL SolveFrame {
    hipStream_t st = nullptr;
    const Head *dev = nullptr;
    Head *h = nullptr;
    size_t count = 0;
    uint64_t polls = 0;
    EventSpans ev;
    SolveFrame() = default;
    SolveFrame(const SolveFrame &) = delete;
    SolveFrame &operator=(const SolveFrame &) = delete;
    ~SolveFrame() { if (h) (void)hipHostFree(h); }

    int create(hipStream_t stream, size_t heads) {
        st = stream;
        count = heads;
        SPAL_HIP_TRY(hipHostMalloc((void **)&h, count * sizeof(Head), hipHostMallocDefault));
        SPAL_HIP_TRY(ev.create(1));
        return SPAL_OK;
    }
    // the heads are the first bytes of the scalars
    int begin(void *dev_scalars, size_t bytes_to_zero) {
        dev = (const Head *)dev_scalars;
        SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
        SPAL_HIP_TRY(hipMemsetAsync(dev_scalars, 0, bytes_to_zero, st));
        return SPAL_OK;
    }
    int poll() {
        SPAL_HIP_TRY(hipMemcpyAsync(h, dev, count * sizeof(Head), hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        ++polls;
        return SPAL_OK;
    }
    int end(float *ms) {
        SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        SPAL_HIP_TRY(ev.span(0, ms));
        return SPAL_OK;
    }
    void fill(spal_krylov_info *info, size_t j, float ms) const {
        info->iterations = h[j].it;
        info->reason = (int)h[j].reason;
        info->residual_sq = (double)h[j].rr;
        info->rhs_sq = (double)h[j].bb;
        info->solve_ms = (double)ms;
    }
};

// A call's describe string (OpState::krylov_info, ...) is stored and read under the lock of a's solve handle.
template <typename H>
KRYLOV_LOCAL void store_info(H *a, std::string OpState::*which, const std::string &json) {
    std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
    a->ops.*which = json;
}
KRYLOV_LOCAL inline int info_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve, const char *key,
                                std::string OpState::*which) {
    if (!solve) return SPAL_OK;
    std::string info;
    {
        std::lock_guard<std::mutex> lock(solve->mu);
        info = s.*which;
    }
    return describe_append(buf, buf_len, key, info);
}

struct PooledStream {
    hipStream_t s = nullptr;
    PooledStream() = default;
    PooledStream(const PooledStream &) = delete;
    PooledStream &operator=(const PooledStream &) = delete;
    ~PooledStream() { stream_release(s); }
};

// a's option "krylov_check_every", 0 (unset) resolved to the default: 1 with a preconditioner, 8 without
template <typename H>
int64_t krylov_check_every_of(H *a, bool preconditioned) {
    int64_t check_every;
    {
        std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
        check_every = a->ops.krylov_check_every;
    }
    return check_every ? check_every : (preconditioned ? 1 : 8);
}

// Plans first: nothing plans lazily once the iterations are being enqueued.  *sweeps = m's option "trsv_sweeps", -1
// without m.
template <typename H>
int krylov_prepare(const char *fn, H *a, H *m, hipStream_t st, int64_t *sweeps) {
    SPAL_TRY(product_plan(a));
    *sweeps = m ? trsv_sweeps_of(solve_handle(m)) : -1;
    if (m && *sweeps >= 0) {
        SPAL_TRY(trsv_sweep_prepare(fn, solve_handle(m), 0, st));   // no analysis; a row without a diagonal: the solve's own message
    } else if (m) {
        SPAL_TRY(analyse(m, 0, 1, st));
        SPAL_TRY(analyse(m, 1, 0, st));   // a row without a diagonal: the solve's own message
    }
    return SPAL_OK;
}

// out = M^-1 v (out != v): two exact solves, or `sweeps` >= 0 Jacobi sweeps per triangle through w0 / w1
template <typename T, typename H>
int prec_dev(const char *fn, H *m, int64_t sweeps, const T *v, T *out, T *w0, T *w1, hipStream_t st) {
    if (sweeps >= 0) {
        SPAL_TRY(trsv_sweep_enqueue(fn, solve_handle(m), 0, 1, (uint64_t)sweeps, v, out, w0, w1, st));
        return trsv_sweep_enqueue(fn, solve_handle(m), 1, 0, (uint64_t)sweeps, out, out, w0, w1, st);
    }
    SPAL_TRY(solve_dev(m, 0, 1, v, out, st));
    return solve_dev(m, 1, 0, out, out, st);
}

// every refusal of a solver that needs no device and is not about its own parameters
template <typename T, typename H>
int krylov_check_operands(const char *fn, H *a, H *m, double tol) {
    if (!(tol >= 0.0)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: tol = %g must be >= 0", fn, tol);
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    if (m) {
        SPAL_TRY(check_same_device_and_dtype(fn, a, m));
        if (m->nrows != a->nrows || m->ncols != a->ncols)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the preconditioner is %llu x %llu but the matrix %llu x %llu", fn,
                        (unsigned long long)m->nrows, (unsigned long long)m->ncols, (unsigned long long)a->nrows,
                        (unsigned long long)a->ncols);
    }
    if (row_blocks(a) || (m && row_blocks(m))) return refuse_row_blocks(fn);
    return SPAL_OK;
}

// A solve on host vectors, after the caller's own refusals: b and x0 go up, run(b_dev, x_dev, stream) solves, x comes back.
template <typename T, typename H, typename Solve>
KRYLOV_LOCAL int with_host_vectors(const char *fn, H *a, const T *b, uint64_t b_len, T *x, uint64_t x_len, Solve run) {
    const uint64_t n = a->nrows;
    if (b_len != n || x_len != n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: b.len() = %llu and x.len() = %llu but the matrix has %llu rows", fn,
                    (unsigned long long)b_len, (unsigned long long)x_len, (unsigned long long)n);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    DevBuf db, dx;
    PooledStream ps;   // a stream of the call's own: the handle's staging stream belongs to whoever holds its lock
    SPAL_HIP_TRY(db.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(dx.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    SPAL_HIP_TRY(hipMemcpyAsync(db.p, b, n * sizeof(T), hipMemcpyHostToDevice, ps.s));
    SPAL_HIP_TRY(hipMemcpyAsync(dx.p, x, n * sizeof(T), hipMemcpyHostToDevice, ps.s));
    SPAL_TRY(run((const T *)db.p, dx.as<T>(), ps.s));
    SPAL_HIP_TRY(hipMemcpyAsync(x, dx.p, n * sizeof(T), hipMemcpyDeviceToHost, ps.s));
    SPAL_HIP_TRY(hipStreamSynchronize(ps.s));
    return SPAL_OK;
}

// ---- what the block drivers (spal_krylov_block.hip, spal_gmres_block.hip) share --------------------------------------
constexpr unsigned kBlockMaxGrid = 1024;   // first-level workgroups along the rows; each walks tiles blockIdx.x, + gridDim.x, ...
constexpr unsigned kColumnGrid = 64;       // ... and along the column tiles (blockIdx.y)
constexpr unsigned kFinishGrid = 65535;    // finish workgroups; each walks columns blockIdx.x, + gridDim.x, ...
constexpr int kTiles[] = {1, 2, 4, 8, 16, 32};   // the instantiated column tiles

// A block operand: the pointer and its leading dimension.  Nothing is __restrict__: without a preconditioner z is r, ph
// is p and sh is s.
template <typename T>
struct Mat {
    T *p;
    uint64_t ld;
};

// The h < G levels of a column's tile: `a` is the sum over the thread's own rows; valid in threads 0 .. KT - 1.  `lds`
// holds kThreads elements; ends with a barrier, so it can be reused.
template <typename T, int KT>
__device__ __forceinline__ T column_tree(T a, T *lds) {
    const unsigned t = threadIdx.x;
    lds[t] = a;
    __syncthreads();
    if (t < 128) {
        a = lds[t] + lds[t + 128];               // h = 128 / KT
        if (t >= 64) lds[t] = a;                 // (its own slot: nobody else read it)
    }
    __syncthreads();
    if (t < 64) {
        a = a + lds[t + 64];                     // h = 64 / KT
#pragma unroll
        for (int h = 32; h >= KT; h >>= 1) a = a + __shfl_down(a, h, 64);
    }
    __syncthreads();
    return a;
}

inline bool tile_instantiated(int64_t t) {
    for (int v : kTiles)
        if (t == v) return true;
    return false;
}

// automatic column tile: the narrowest instantiated tile that holds k
inline int auto_tile(uint64_t k) {
    int t = 1;
    while (t < 32 && (uint64_t)t < k) t *= 2;
    return t;
}

// the entry points a block driver goes through, by handle and element type
#define SPAL_KB_ROUTES(kind, sfx, T)                                                                                   \
    inline int mul_block(spal_##kind *a, uint64_t k, const T *x, uint64_t ldx, T *y, uint64_t ldy, void *st) {         \
        return spal_##kind##_spmm_dev_##sfx(a, k, x, ldx, y, ldy, st);                                                 \
    }                                                                                                                  \
    inline int solve_block(spal_##kind *m, int uplo, int unit, uint64_t k, const T *b, uint64_t ldb, T *x,             \
                           uint64_t ldx, void *st) {                                                                   \
        return spal_##kind##_trsm_dev_##sfx(m, uplo, unit, k, b, ldb, x, ldx, st);                                     \
    }                                                                                                                  \
    inline int sweep_block(spal_##kind *m, int uplo, int unit, uint64_t s, uint64_t k, const T *b, uint64_t ldb, T *x, \
                           uint64_t ldx, void *st) {                                                                   \
        return spal_##kind##_trsm_sweep_dev_##sfx(m, uplo, unit, s, k, b, ldb, x, ldx, st);                            \
    }
SPAL_KB_ROUTES(csr, f64, double)
SPAL_KB_ROUTES(csr, f32, float)
SPAL_KB_ROUTES(csc, f64, double)
SPAL_KB_ROUTES(csc, f32, float)
#undef SPAL_KB_ROUTES

// a * b * c * d, or false when it does not fit half of size_t
inline bool bytes_of(uint64_t a, uint64_t b, uint64_t c, uint64_t d, size_t *out) {
    unsigned __int128 v = (unsigned __int128)a * b;
    if (v > std::numeric_limits<size_t>::max()) return false;
    v *= c;
    if (v > std::numeric_limits<size_t>::max()) return false;
    v *= d;
    if (v > std::numeric_limits<size_t>::max() / 2) return false;
    *out = (size_t)v;
    return true;
}

// out = M^-1 v for packed blocks of k columns (out != v): two exact block solves, or `sweeps` >= 0 sweeps per triangle
template <typename T, typename H>
KRYLOV_LOCAL int prec_block(H *m, int64_t sweeps, uint32_t k, const T *v, T *out, hipStream_t st) {
    if (sweeps >= 0) {
        SPAL_TRY(sweep_block(m, 0, 1, (uint64_t)sweeps, k, v, k, out, k, st));
        return sweep_block(m, 1, 0, (uint64_t)sweeps, k, out, k, out, k, st);
    }
    SPAL_TRY(solve_block(m, 0, 1, k, v, k, out, k, st));
    return solve_block(m, 1, 0, k, out, k, out, k, st);
}

// what a block call refuses of k, ldb and ldx: it needs nothing of the handles
KRYLOV_LOCAL inline int check_block_geometry(const char *who, uint64_t k, uint64_t ldb, uint64_t ldx) {
    if (k == 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: k = 0 (B and X need at least one column)", who);
    if (k > 0xffffffffull) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: k = %llu does not fit 32 bits", who, (unsigned long long)k);
    if (ldb < k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ldb = %llu is less than k = %llu", who, (unsigned long long)ldb,
                    (unsigned long long)k);
    if (ldx < k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ldx = %llu is less than k = %llu", who, (unsigned long long)ldx,
                    (unsigned long long)k);
    return SPAL_OK;
}

// a's option "krylov_tile", 0 (automatic) resolved for k columns
template <typename H>
KRYLOV_LOCAL int column_tile_of(H *a, uint64_t k) {
    int tile;
    {
        std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
        tile = a->ops.krylov_tile;
    }
    return tile ? tile : auto_tile(k);
}

// Runs `launch`, in which KT_ is the instantiated column tile that equals `tile`.
#define KRYLOV_BY_TILE(tile, launch)                  \
    switch (tile) {                                   \
    case 1: { constexpr int KT_ = 1; launch; } break;   \
    case 2: { constexpr int KT_ = 2; launch; } break;   \
    case 4: { constexpr int KT_ = 4; launch; } break;   \
    case 8: { constexpr int KT_ = 8; launch; } break;   \
    case 16: { constexpr int KT_ = 16; launch; } break; \
    default: { constexpr int KT_ = 32; launch; } break; \
    }

// From here on the stream's sweep scratch holds `bytes` (n x k per ping-pong block): the sweeps of M^-1 take it from there,
// so no iteration allocates.
template <typename H>
KRYLOV_LOCAL int grow_sweep_scratch(const char *fn, hipStream_t st, H *m, int64_t sweeps, uint64_t n, size_t bytes) {
    if (!m || sweeps < 1 || !n) return SPAL_OK;
    StreamWork grow;
    return grow.take(fn, st, bytes);
}

// A block solve on host blocks, after the caller's own refusals: B and X0 go up packed (leading dimension k),
// run(b_dev, x_dev, stream) solves, the k columns of X come back into the caller's rows.
template <typename T, typename H, typename Solve>
KRYLOV_LOCAL int with_host_block(const char *who, H *a, uint64_t k, const T *b, uint64_t ldb, uint64_t b_rows, T *x, uint64_t ldx,
                    uint64_t x_rows, Solve run) {
    const uint64_t n = a->nrows;
    if (b_rows != n || x_rows != n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: B has %llu rows and X has %llu rows but the matrix has %llu rows", who,
                    (unsigned long long)b_rows, (unsigned long long)x_rows, (unsigned long long)n);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    size_t bytes = 0;
    if (!bytes_of(n, k, sizeof(T), 1, &bytes))
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for blocks of %llu x %llu", who, (unsigned long long)n,
                    (unsigned long long)k);
    const size_t row = (size_t)k * sizeof(T);
    DevBuf db, dx;
    PooledStream ps;   // a stream of the call's own: the handle's staging stream belongs to whoever holds its lock
    SPAL_HIP_TRY(db.alloc(bytes));
    SPAL_HIP_TRY(dx.alloc(bytes));
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    if (n) {
        SPAL_HIP_TRY(hipMemcpy2DAsync(db.p, row, b, (size_t)ldb * sizeof(T), row, n, hipMemcpyHostToDevice, ps.s));
        SPAL_HIP_TRY(hipMemcpy2DAsync(dx.p, row, x, (size_t)ldx * sizeof(T), row, n, hipMemcpyHostToDevice, ps.s));
    }
    SPAL_TRY(run((const T *)db.p, dx.as<T>(), ps.s));
    if (n) SPAL_HIP_TRY(hipMemcpy2DAsync(x, (size_t)ldx * sizeof(T), dx.p, row, row, n, hipMemcpyDeviceToHost, ps.s));
    SPAL_HIP_TRY(hipStreamSynchronize(ps.s));
    return SPAL_OK;
}

}  // namespace spal
