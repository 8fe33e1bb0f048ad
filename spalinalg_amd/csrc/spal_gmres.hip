// spal_gmres.hip -- restarted, right-preconditioned GMRES on the device.  The contract is the sequential
// text in include/spal.h: two passes of classical Gram-Schmidt per step, Givens rotations on the Hessenberg column, a
// column-form back substitution at the end of a cycle; every dot is reduce() of the rounded products (krylov_kernels.hpp),
// so the device returns the text's bits in f32 and f64.
//
// THE ORTHOGONALISATION IS TWO STREAMING KERNELS.  `mdot` reads w ONCE for all j + 1 dot products of a pass: a thread
// keeps its four elements of w in registers and takes the basis vectors kDotBatch at a time -- all the batch's loads are
// issued before the first product, then one thread-local stage, one LDS stage [kDotBatch][256] and the shuffles serve the
// whole batch: three barriers per batch, not per vector.  Every single dot keeps reduce()'s operand order; batching only
// interleaves independent sums.  `mfinish` walks the upper levels with ONE WORKGROUP PER k.  `mupdate` subtracts the j + 1
// projections in the text's left-to-right order, batched the same way; the second one of a step also forms the first
// level of dot(w, w).  v_{j+1} = w / hn is a pass of its own (`scale`).
//
// THE SCALARS live in a block of device memory: a head (GHead) the host polls, then h, c, cs, sn, g, y and the
// Hessenberg matrix H, (restart + 1) x restart by columns.  One workgroup (`step_scalars`) finishes dot(w, w), adds c to
// h, applies the earlier rotations in thread 0, forms the new one, updates g, computes est and decides the end of the cycle.
//
// FREEZE.  `done`, `cyc_end` and `jj` in the head are written by a one-workgroup launch and only read -- never waited
// on -- by later launches.  Every kernel of inner step j returns before it writes unless the device is exactly there
// (!done, !cyc_end, jj == j); the kernels of a cycle's end read jj from the head and return unless the cycle has ended
// and the call has not; after `done` every kernel returns before it writes.  Products and solves enqueued past a stop
// still run, into work vectors nobody reads again.  So x, it, reason and rr do not depend on "krylov_check_every".
// ORDER BETWEEN LAUNCHES IS STREAM ORDER ALONE.  The driver holds no handle lock across a product or a solve.
//
// (The frame of the call -- KRYLOV_LAUNCH, SolveFrame with the pinned head, the polls and the device time, store_info,
// with_host_vectors -- is krylov_kernels.hpp's, shared with CG and BiCGStab; the cycle loop in gmres_run is this file's.)
#include "gmres_kernels.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

// (GHead, GBlock, block_elems and the three scalar steps are in gmres_kernels.hpp, shared with spal_gmres_block.hip; so
// are kDotBatch, Basis, load4, tile_sum_batch, scale, mdot, mfinish and mupdate, shared with spal_eigsh.hip.)

// ---- the head of a cycle --------------------------------------------------------------------------------------------
// r = b - q;  first levels of rr = dot(r, r) and bb = dot(b, b)
template <typename T>
__global__ __launch_bounds__(kThreads) void residual(const GHead<T> *s, const T *b, const T *q, T *r, T *part0, T *part1,
                                                     uint64_t n, uint64_t tiles) {
    __shared__ T lds[2][kThreads];
    if (s->done != 0) return;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T p[4], pb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t e = i + (uint64_t)k * kThreads;
            p[k] = pb[k] = T(0);
            if (e < n) {
                const T bv = b[e];
                const T rv = bv - q[e];
                r[e] = rv;
                p[k] = rv * rv;
                pb[k] = bv * bv;
            }
        }
        const T s0 = tile_sum<T>(p[0], p[1], p[2], p[3], lds[0]);
        const T s1 = tile_sum<T>(pb[0], pb[1], pb[2], pb[3], lds[1]);
        if (threadIdx.x == 0) {
            part0[tile] = s0;
            part1[tile] = s1;
        }
    }
}

// rr, bb, thr;  the test on the true residual;  beta, g[0], jj = 0
template <typename T>
__global__ __launch_bounds__(kThreads) void cycle_start(GBlock<T> B, T *part0, T *part1, uint64_t c1, T tol2, uint64_t maxit) {
    __shared__ T lds[kThreads];
    GHead<T> *s = B.s;
    if (s->done != 0) return;
    const T rr = upper_levels<T>(part0, c1, lds);
    const T bb = upper_levels<T>(part1, c1, lds);
    if (threadIdx.x == 0) cycle_start_scalars<T>(B, rr, bb, tol2, maxit);
}

// ww = dot(w, w);  h += c;  hn;  the rotations;  g;  est;  the end of the cycle;  jj, it
template <typename T>
__global__ __launch_bounds__(kThreads) void step_scalars(GBlock<T> B, unsigned j, T *part0, uint64_t c1, uint64_t maxit) {
    __shared__ T lds[kThreads];
    GHead<T> *s = B.s;
    if (!at_step(s, j)) return;
    const T ww = upper_levels<T>(part0, c1, lds);
    step_scalars_body<T>(B, j, ww, maxit);
}

// ---- the end of a cycle ---------------------------------------------------------------------------------------------
// column form: thread l owns g[l];  for k = jj - 1 .. 0:  y[k] = g[k] / H[k, k];  g[l] -= H[l, k] * y[k] for l < k
template <typename T>
__global__ __launch_bounds__(kThreads) void back_substitute(GBlock<T> B) {
    __shared__ T y[kThreads];
    if (!at_cycle_end(B.s)) return;
    back_substitute_body<T>(B, y);
}

// u[i] = (..((y[0] * v_0[i]) + (y[1] * v_1[i])) ..) + (y[jj - 1] * v_{jj-1}[i]);  ADD: out[i] = out[i] + u[i], else out = u
template <typename T, bool ADD>
__global__ __launch_bounds__(kThreads) void combine(GBlock<T> B, Basis<T> V, T *out) {
    if (!at_cycle_end(B.s)) return;
    const unsigned nk = B.s->jj;
    for (uint64_t tile = blockIdx.x; tile < V.tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T u[4] = {T(0), T(0), T(0), T(0)};
        for (unsigned k0 = 0; k0 < nk; k0 += kDotBatch) {
            T v[kDotBatch][4];
#pragma unroll
            for (int b = 0; b < kDotBatch; ++b)
                if (k0 + b < nk) load4<T>(V.v + (uint64_t)(k0 + b) * V.stride, i, V.n, v[b]);
#pragma unroll
            for (int b = 0; b < kDotBatch; ++b) {
                if (k0 + b < nk) {
                    const T yk = B.y[k0 + b];
#pragma unroll
                    for (int k = 0; k < 4; ++k) u[k] = k0 + b == 0 ? yk * v[b][k] : u[k] + (yk * v[b][k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t e = i + (uint64_t)k * kThreads;
            if (e < V.n) out[e] = ADD ? out[e] + u[k] : u[k];
        }
    }
}

// x[i] = x[i] + t[i]  (t = M^-1 u)
template <typename T>
__global__ __launch_bounds__(kThreads) void add_to_x(const GHead<T> *s, const T *t, T *x, uint64_t n) {
    if (!at_cycle_end(s)) return;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) x[i] = x[i] + t[i];
}

// ---- the driver -----------------------------------------------------------------------------------------------------
struct Record {
    uint64_t restart = 0, iterations = 0, cycles = 0, polls = 0, basis_bytes = 0;
    int preconditioned = 0, reason = 0;
    int64_t precond_sweeps = -1, check_every = 0;
    double solve_ms = 0.0;
};
std::string info_json(const Record &r) {
    char buf[512];
    snprintf(buf, sizeof buf,
             "{\"restart\": %llu, \"preconditioned\": %d, \"precond_sweeps\": %lld, \"iterations\": %llu, \"cycles\": %llu, "
             "\"reason\": %d, \"check_every\": %lld, \"polls\": %llu, \"dot_batch\": %d, \"basis_bytes\": %llu, \"solve_ms\": %.4f}",
             (unsigned long long)r.restart, r.preconditioned, (long long)r.precond_sweeps, (unsigned long long)r.iterations,
             (unsigned long long)r.cycles, r.reason, (long long)r.check_every, (unsigned long long)r.polls, kDotBatch,
             (unsigned long long)r.basis_bytes, r.solve_ms);
    return buf;
}

template <typename T, typename H>
struct Run {
    const char *fn;
    H *a, *m;
    hipStream_t st;
    uint64_t n = 0, maxit = 0, c1 = 0, pe = 0, restart = 0;
    unsigned grid = 1;
    T tol2 = T(0);
    int64_t sweeps = -1;
    GBlock<T> B;
    Basis<T> V;
    T *basis = nullptr, *w = nullptr, *q = nullptr, *z = nullptr, *u = nullptr, *w0 = nullptr, *w1 = nullptr, *part = nullptr;
    const T *b = nullptr;
    T *x = nullptr;

    T *v_at(uint64_t k) const { return basis + k * V.stride; }
    int prec(const T *v, T *out) { return prec_dev<T, H>(fn, m, sweeps, v, out, w0, w1, st); }

    // q = A x;  r, rr, bb;  the test;  beta, v_0
    int head() {
        SPAL_TRY(mul_dev(a, x, q, st));
        KRYLOV_LAUNCH((residual<T>), grid, B.s, b, q, v_at(0), part, part + pe, n, V.tiles);
        KRYLOV_LAUNCH((cycle_start<T>), 1, B, part, part + pe, c1, tol2, maxit);
        KRYLOV_LAUNCH((scale<T>), grid, B.s, v_at(0), v_at(0), -1, n);
        return SPAL_OK;
    }
    // step j of a cycle
    int inner(unsigned j) {
        const T *zj = v_at(j);
        if (m) {
            SPAL_TRY(prec(v_at(j), z));
            zj = z;
        }
        SPAL_TRY(mul_dev(a, zj, w, st));
        KRYLOV_LAUNCH((mdot<T>), grid, B.s, V, j, w, part, pe);
        KRYLOV_LAUNCH((mfinish<T>), j + 1, B.s, j, part, pe, c1, B.h);
        KRYLOV_LAUNCH((mupdate<T, false>), grid, B.s, V, j, B.h, w, part);
        KRYLOV_LAUNCH((mdot<T>), grid, B.s, V, j, w, part, pe);
        KRYLOV_LAUNCH((mfinish<T>), j + 1, B.s, j, part, pe, c1, B.c);
        KRYLOV_LAUNCH((mupdate<T, true>), grid, B.s, V, j, B.c, w, part);
        KRYLOV_LAUNCH((step_scalars<T>), 1, B, j, part, c1, maxit);
        KRYLOV_LAUNCH((scale<T>), grid, B.s, w, v_at(j + 1), (int)j, n);
        return SPAL_OK;
    }
    // y;  u = V y;  x += M^-1 u
    int cycle_end() {
        KRYLOV_LAUNCH((back_substitute<T>), 1, B);
        if (!m) {
            KRYLOV_LAUNCH((combine<T, true>), grid, B, V, x);
            return SPAL_OK;
        }
        KRYLOV_LAUNCH((combine<T, false>), grid, B, V, u);
        SPAL_TRY(prec(u, z));
        KRYLOV_LAUNCH((add_to_x<T>), grid, B.s, z, x, n);
        return SPAL_OK;
    }
};

template <typename T, typename H>
int gmres_run(const char *fn, H *a, H *m, const T *b, T *x, uint64_t restart, double tol, uint64_t maxit, hipStream_t st,
              spal_krylov_info *info) {
    const uint64_t n = a->nrows;
    const int64_t check_every = krylov_check_every_of(a, m != nullptr);
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    int64_t sweeps = -1;
    SPAL_TRY(krylov_prepare(fn, a, m, st, &sweeps));

    // the basis and the work vectors in one block, the scratch of `restart` dots, the scalar block
    const uint64_t nvec = (restart + 1) + 2 + (m ? 2 : 0) + (sweeps >= 0 ? 2 : 0);
    const uint64_t stride = (n + 63) & ~(uint64_t)63;   // every vector on a 256-byte boundary at least
    const uint64_t basis_bytes = nvec * stride * sizeof(T);
    DevBuf vecs, parts, scal;
    SolveFrame<GHead<T>> F;
    {
        const hipError_t e = vecs.alloc((size_t)basis_bytes);
        if (e == hipErrorOutOfMemory)
            return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no memory for the basis: %llu vectors of %llu elements (%llu bytes)", fn,
                        (unsigned long long)nvec, (unsigned long long)n, (unsigned long long)basis_bytes);
        SPAL_HIP_TRY(e);
    }
    const uint64_t pe = scratch_elems(n);
    SPAL_HIP_TRY(parts.alloc(std::max<uint64_t>(restart, 2) * pe * sizeof(T)));
    const size_t scal_bytes = sizeof(GHead<T>) + block_elems(restart) * sizeof(T);
    SPAL_HIP_TRY(scal.alloc(scal_bytes));
    SPAL_TRY(F.create(st, 1));

    Run<T, H> R;
    R.fn = fn;
    R.a = a;
    R.m = m;
    R.st = st;
    R.n = n;
    R.maxit = maxit;
    R.c1 = tiles_of(n);
    R.pe = pe;
    R.restart = restart;
    R.grid = first_level_grid(n);
    R.tol2 = (T)(tol * tol);
    R.sweeps = sweeps;
    R.b = b;
    R.x = x;
    R.part = parts.as<T>();
    R.basis = vecs.as<T>();
    R.V.v = R.basis;
    R.V.stride = stride;
    R.V.n = n;
    R.V.tiles = tiles_of(n);
    uint64_t next = restart + 1;
    R.w = R.v_at(next++);
    R.q = R.v_at(next++);
    if (m) {
        R.z = R.v_at(next++);
        R.u = R.v_at(next++);
    }
    if (sweeps >= 0) {
        R.w0 = R.v_at(next++);
        R.w1 = R.v_at(next++);
    }
    R.B = block_parts<T>(scal.as<GHead<T>>(), reinterpret_cast<T *>(reinterpret_cast<char *>(scal.p) + sizeof(GHead<T>)), restart);

    const GHead<T> *h = F.h;
    SPAL_TRY(F.begin(scal.p, scal_bytes));
    SPAL_TRY(R.head());
    uint64_t total = 0;      // inner iterations enqueued; the device's `it` as long as it has not frozen
    bool stopped = false;
    if (maxit == 0) {        // the test after r0 has decided
        SPAL_TRY(F.poll());
        stopped = true;
    }
    while (!stopped) {
        uint64_t j = 0, since = 0;
        bool ended = false;
        while (!ended && !stopped) {
            SPAL_TRY(R.inner((unsigned)j));
            ++j;
            ++total;
            ++since;
            if (since == (uint64_t)check_every || j == restart || total == maxit) {
                SPAL_TRY(F.poll());
                since = 0;
                stopped = h->done != 0;
                ended = h->cyc_end != 0;
                if (j == restart && !ended && !stopped)
                    return fail(SPAL_ERR_HIP, "%s: the device did not end a cycle of %llu iterations", fn, (unsigned long long)restart);
            }
        }
        if (stopped) break;
        total = h->it;       // the cycle may have ended before the host's count
        const bool early = h->jj < restart;
        SPAL_TRY(R.cycle_end());
        SPAL_TRY(R.head());
        if (early || total == maxit) {   // est <= thr or maxit: the test at the head stops the call, or very likely does
            SPAL_TRY(F.poll());
            stopped = h->done != 0;
        }
    }
    float ms = 0.f;
    SPAL_TRY(F.end(&ms));
    if (!h->done) return fail(SPAL_ERR_HIP, "%s: the device did not stop after %llu iterations", fn, (unsigned long long)maxit);
    F.fill(info, 0, ms);
    Record rec;
    rec.restart = restart;
    rec.preconditioned = m ? 1 : 0;
    rec.precond_sweeps = sweeps;
    rec.iterations = info->iterations;
    rec.cycles = h->cycles;
    rec.reason = info->reason;
    rec.check_every = check_every;
    rec.polls = F.polls;
    rec.basis_bytes = basis_bytes;
    rec.solve_ms = info->solve_ms;
    store_info(a, &OpState::gmres_info, info_json(rec));
    return SPAL_OK;
}

// every refusal that needs no device
template <typename T, typename H>
int gmres_check(const char *fn, H *a, H *m, const T *b, T *x, uint64_t restart, double tol, spal_krylov_info *info) {
    if (!a || !b || !x || !info) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (restart == 0 || restart > kMaxRestart)
        return fail(SPAL_ERR_INVALID_ARGUMENT,
                    "%s: restart = %llu must be 1 .. %llu (one Hessenberg column element per thread of the scalar workgroup)", fn,
                    (unsigned long long)restart, (unsigned long long)kMaxRestart);
    return krylov_check_operands<T, H>(fn, a, m, tol);
}

template <typename T, typename H>
int gmres_dev(const char *fn, H *a, H *m, const T *b, T *x, uint64_t restart, double tol, uint64_t maxit, void *stream,
              spal_krylov_info *info) {
    SPAL_TRY((gmres_check<T, H>(fn, a, m, b, x, restart, tol, info)));
    if (x == b) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x_dev == b_dev (b is read in every test of the residual)", fn);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return gmres_run<T, H>(fn, a, m, b, x, restart, tol, maxit, (hipStream_t)stream, info);
}

template <typename T, typename H>
int gmres_host(const char *fn, H *a, H *m, const T *b, uint64_t b_len, T *x, uint64_t x_len, uint64_t restart, double tol,
               uint64_t maxit, spal_krylov_info *info) {
    SPAL_TRY((gmres_check<T, H>(fn, a, m, b, x, restart, tol, info)));
    return with_host_vectors(fn, a, b, b_len, x, x_len, [&](const T *b_dev, T *x_dev, hipStream_t st) {
        return gmres_run<T, H>(fn, a, m, b_dev, x_dev, restart, tol, maxit, st, info);
    });
}

}  // namespace

int gmres_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    return info_describe_append(buf, buf_len, s, solve, "gmres", &OpState::gmres_info);
}

}  // namespace spal

using namespace spal;

extern "C" {

#define SPAL_GMRES_ENTRIES(kind, sfx, T)                                                                               \
    int spal_##kind##_gmres_##sfx(spal_##kind##_t a, spal_##kind##_t m, const T *b, uint64_t b_len, T *x,              \
                                  uint64_t x_len, uint64_t restart, double tol, uint64_t maxit,                        \
                                  spal_krylov_info *info) {                                                            \
        return gmres_host<T, spal_##kind>("spal_" #kind "_gmres", a, m, b, b_len, x, x_len, restart, tol, maxit,       \
                                          info);                                                                       \
    }                                                                                                                  \
    int spal_##kind##_gmres_dev_##sfx(spal_##kind##_t a, spal_##kind##_t m, const T *b_dev, T *x_dev,                  \
                                      uint64_t restart, double tol, uint64_t maxit, void *stream,                      \
                                      spal_krylov_info *info) {                                                        \
        return gmres_dev<T, spal_##kind>("spal_" #kind "_gmres_dev", a, m, b_dev, x_dev, restart, tol, maxit, stream,  \
                                         info);                                                                        \
    }
SPAL_GMRES_ENTRIES(csr, f64, double)
SPAL_GMRES_ENTRIES(csr, f32, float)
SPAL_GMRES_ENTRIES(csc, f64, double)
SPAL_GMRES_ENTRIES(csc, f32, float)
#undef SPAL_GMRES_ENTRIES

}  // extern "C"
