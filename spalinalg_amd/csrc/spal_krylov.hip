// spal_krylov.hip -- the dot product, CG and BiCGStab on the device.  The contracts are written out in
// include/spal.h: dot(a, b, n) = reduce(p), p[i] = a[i] * b[i] rounded; reduce pads with +0.0 to whole tiles of 1024,
// halves every tile (h = 512 .. 1: e[t] = e[t] + e[t + h]) and, when there is more than one tile, reduces the tile sums
// the same way.  The order depends on n alone, so every kernel here returns the bits of the sequential text.
//
// (tile_sum, upper_levels, the scratch sizes, the plan preparation, M^-1 and the shared refusals are in krylov_kernels.hpp,
// which spal_gmres.hip includes too; so are the scalar block Scal, the fused updates VecOp / vec_update and the scalar
// steps FinOp / scalar_step, which spal_krylov_block.hip runs per column of a block of right-hand sides.)
//
// ONE TILE IS ONE TRIP OF A WORKGROUP OF 256.  Thread t holds elements t, t + 256, t + 512, t + 768: strides 512 and 256
// are thread-local ((v0 + v2) + (v1 + v3)), strides 128 and 64 go through LDS, strides 32 .. 1 are __shfl_down inside
// wave 0.  The first level writes one sum per tile to a scratch array; a launch of ONE workgroup (`finish`) walks the
// upper levels, and its thread 0 then does the scalar arithmetic that follows the dot in the loop (alpha, beta, omega,
// the test, the iteration count) in a small block of device memory.  Every vector update is fused with the first level
// of the dot that follows it (`vec`): the same products, the same tile order, one pass less over the vectors.
// ORDER BETWEEN LAUNCHES IS STREAM ORDER ALONE: no spinning, no ticket, nothing another workgroup waits on.
//
// FREEZE AFTER STOP.  The scalar block carries `done`.  It is written by a `finish` launch and read -- never waited
// on -- by every later `vec` / `finish` launch of the call, which then returns before it writes: x, it and rr are the
// values at the stop whatever the poll interval ("krylov_check_every") is.  Products and solves enqueued after the stop
// still run, into work vectors nobody reads again.  BiCGStab's half-step exit needs one vector update AFTER the stop
// was decided (x += alpha * ph): `half` is set with `done`, the next `vec` launch (V_BI_HALF) applies it, and the
// scalar launch after that clears it.
//
// THE DRIVER HOLDS NO HANDLE LOCK ACROSS A PRODUCT OR A SOLVE: it calls the spal_*_spmv_dev_* / spal_*_trsv_dev_* entry
// points, each of which takes what it needs itself (f5b9766: re-entering a handle's lock deadlocks).  A factor whose
// option "trsv_sweeps" is s >= 0 is applied by s Jacobi sweeps per triangle instead (trsv_sweep_enqueue),
// through two more work vectors of the call.  The spal_*_krylov_amg_* entry points run the same two loops with an AMG
// hierarchy `g` in m's place: M^-1 v is one multigrid cycle (amg_apply_enqueue, spal_amg.hip), enqueued into
// the hierarchy's own work vectors under its own lock.  Plans are built before the first iteration; work vectors, the scratch and the scalar block come from the caching allocator per call,
// so concurrent calls on one handle share nothing but the matrix.
#include "krylov_kernels.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

// Nothing is __restrict__: without a preconditioner z is r, ph is p and sh is s.
template <typename T>
struct VecArgs {
    const T *a, *b, *c, *d;
    T *x, *y;
    const Scal<T> *s;   // nullptr: the stand-alone dot
    T *part0, *part1;   // tile sums of d0 / d1
    uint64_t n;
};

template <typename T, int OP>
__device__ __forceinline__ void element(const VecArgs<T> &g, uint64_t i, T alpha, T beta, T omega, T &p0, T &p1) {
    p0 = T(0);
    p1 = T(0);
    if (i >= g.n) return;   // the padding: +0.0, and it is added
    vec_update<T, OP>(g.a + i, g.b + i, g.c + i, g.d + i, g.x + i, g.y + i, alpha, beta, omega, p0, p1);
}

template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void vec(VecArgs<T> g, uint64_t tiles) {
    __shared__ T lds[2][kThreads];
    T alpha = T(0), beta = T(0), omega = T(0);
    if (g.s) {   // uniform: one word for the whole grid, written by an earlier launch
        if (OP == V_BI_HALF ? g.s->half == 0 : g.s->done != 0) return;
        alpha = g.s->alpha;
        beta = g.s->beta;
        omega = g.s->omega;
    }
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T p[4], q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) element<T, OP>(g, i + (uint64_t)k * kThreads, alpha, beta, omega, p[k], q[k]);
        if (Dots<OP>::n >= 1) {
            const T s = tile_sum<T>(p[0], p[1], p[2], p[3], lds[0]);
            if (threadIdx.x == 0) g.part0[tile] = s;
        }
        if (Dots<OP>::n >= 2) {
            const T s = tile_sum<T>(q[0], q[1], q[2], q[3], lds[1]);
            if (threadIdx.x == 0) g.part1[tile] = s;
        }
    }
}

// ---- the upper levels (upper_levels, krylov_kernels.hpp) and the scalars, one workgroup --------------------------------
template <typename T>
struct FinArgs {
    Scal<T> *s;
    T *part0, *part1;
    uint64_t c1;
    T tol2;            // T(tol * tol)
    uint64_t maxit;
    T *out;            // F_STORE
    int unpreconditioned;   // F_TEST_CG: z is r, so rz1 = rr and beta follows here
};

template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void finish(FinArgs<T> g) {
    __shared__ T lds[kThreads];
    Scal<T> *s = g.s;
    if (OP != F_STORE) {
        if (OP == F_OMEGA && threadIdx.x == 0) s->half = 0;   // the half step, if there was one, has been applied
        if (s->done != 0) return;                             // uniform; this launch does not write `done` before here
    }
    const T d0 = upper_levels<T>(g.part0, g.c1, lds);
    T d1 = T(0);
    if (OP == F_INIT || OP == F_OMEGA) d1 = upper_levels<T>(g.part1, g.c1, lds);
    if (threadIdx.x != 0) return;
    if (OP == F_STORE)
        *g.out = d0;
    else
        scalar_step<T, OP>(s, d0, d1, g.tol2, g.maxit, g.unpreconditioned);
}

// ---- host side of the launches --------------------------------------------------------------------------------------
template <typename T, int OP>
hipError_t launch_vec(const VecArgs<T> &g, hipStream_t st) {
    const uint64_t tiles = tiles_of(g.n);
    hipLaunchKernelGGL((vec<T, OP>), dim3(first_level_grid(g.n)), dim3(kThreads), 0, st, g, tiles);
    return hipGetLastError();
}
template <typename T, int OP>
hipError_t launch_finish(const FinArgs<T> &g, hipStream_t st) {
    hipLaunchKernelGGL((finish<T, OP>), dim3(1), dim3(kThreads), 0, st, g);
    return hipGetLastError();
}

// the definition on the host
template <typename T>
T reduce_host(std::vector<T> &v) {
    for (;;) {
        const uint64_t c = tiles_of(v.size());
        v.resize(c * kTile, T(0));
        std::vector<T> sums(c);
        for (uint64_t tile = 0; tile < c; ++tile) {
            T *e = v.data() + tile * kTile;
            for (uint64_t h = kTile / 2; h >= 1; h /= 2)
                for (uint64_t t = 0; t < h; ++t) e[t] = e[t] + e[t + h];
            sums[tile] = e[0];
        }
        if (c == 1) return sums[0];
        v.swap(sums);
    }
}

template <typename T>
int dot_host(const char *fn, const T *a, const T *b, uint64_t n, T *out) {
    if (!out || (n && (!a || !b))) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    std::vector<T> p(n);
    for (uint64_t i = 0; i < n; ++i) p[i] = a[i] * b[i];
    *out = reduce_host<T>(p);
    return SPAL_OK;
}

template <typename T>
int dot_dev(const char *fn, int device, const T *a, const T *b, uint64_t n, T *out, void *stream) {
    if (!out || (n && (!a || !b))) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    DeviceGuard guard(device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    // the stream's own scratch block: returning a block to the caching allocator would wait for the device
    StreamWork work;
    SPAL_TRY(work.take(fn, st, scratch_elems(n) * sizeof(T)));
    VecArgs<T> g = {};
    g.a = a;
    g.b = b;
    g.n = n;
    g.part0 = work.as<T>();
    hipError_t e = launch_vec<T, V_DOT>(g, st);
    FinArgs<T> f = {};
    f.part0 = work.as<T>();
    f.c1 = tiles_of(n);
    f.out = out;
    if (e == hipSuccess) e = launch_finish<T, F_STORE>(f, st);
    if (e != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return SPAL_OK;
}

struct Record {
    int method = 0, preconditioned = 0, reason = 0, amg = 0;
    int64_t precond_sweeps = -1;
    uint64_t iterations = 0, polls = 0;
    int64_t check_every = 0;
    double solve_ms = 0.0;
};
std::string info_json(const Record &r) {
    char buf[384];
    snprintf(buf, sizeof buf,
             "{\"method\": \"%s\", \"preconditioned\": %d, \"iterations\": %llu, \"reason\": %d, \"check_every\": %lld, "
             "\"polls\": %llu, \"solve_ms\": %.4f, \"precond_sweeps\": %lld%s}",
             r.method == SPAL_KRYLOV_CG ? "cg" : "bicgstab", r.preconditioned, (unsigned long long)r.iterations, r.reason,
             (long long)r.check_every, (unsigned long long)r.polls, r.solve_ms, (long long)r.precond_sweeps,
             r.amg ? ", \"precond\": \"amg\"" : "");   // (the objects written without a hierarchy do not change)
    return buf;
}

// What both loops share: the vectors, the scalar block, the scratch of two dots, and the launches by name.
template <typename T, typename H>
struct Run {
    const char *fn;
    H *a, *m;
    spal_amg *g = nullptr;   // the other kind of preconditioner: an AMG hierarchy (spal_amg.hip); m is NULL then
    hipStream_t st;
    uint64_t n = 0, maxit = 0, c1 = 0;
    T tol2 = T(0);
    Scal<T> *s = nullptr;
    T *part0 = nullptr, *part1 = nullptr;
    int64_t sweeps = -1;            // m's option "trsv_sweeps"
    T *w0 = nullptr, *w1 = nullptr; // the sweeps' ping-pong vectors

    int mul(const T *v, T *out) { return mul_dev(a, v, out, st); }
    // out = M^-1 v (out != v); without a preconditioner the caller uses v itself
    int prec(const T *v, T *out) {
        return g ? amg_apply_enqueue(fn, g, v, out, st) : prec_dev<T, H>(fn, m, sweeps, v, out, w0, w1, st);
    }
    template <int OP>
    int v(const T *va, const T *vb, const T *vc, const T *vd, T *x, T *y) {
        VecArgs<T> g = {va, vb, vc, vd, x, y, s, part0, part1, n};
        const hipError_t e = launch_vec<T, OP>(g, st);
        return e == hipSuccess ? SPAL_OK : fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    }
    template <int OP>
    int f(int unpreconditioned = 0) {
        FinArgs<T> g = {s, part0, part1, c1, tol2, maxit, nullptr, unpreconditioned};
        const hipError_t e = launch_finish<T, OP>(g, st);
        return e == hipSuccess ? SPAL_OK : fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    }
};

template <typename T, typename H>
int krylov_run(const char *fn, H *a, int method, H *m, spal_amg *g, const T *b, T *x, double tol, uint64_t maxit,
               hipStream_t st, spal_krylov_info *info) {
    const uint64_t n = a->nrows;
    spal_csr *owner = solve_handle(a);   // whose lock guards a's option and its "krylov" string
    const bool pre = m || g;   // M^-1 is there: z, ph and sh are vectors of their own
    const int64_t check_every = krylov_check_every_of(a, pre);
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    int64_t sweeps = -1;
    SPAL_TRY(krylov_prepare(fn, a, m, st, &sweeps));
    // work vectors, scratch, scalars
    const bool cg = method == SPAL_KRYLOV_CG;
    const int nwork = cg ? (pre ? 4 : 3) : (pre ? 8 : 6);
    const int nvec = nwork + (sweeps >= 0 ? 2 : 0);
    DevBuf vecs, parts, scal;
    PinnedBuf host;
    EventSpans ev;
    const uint64_t stride = (n + 63) & ~(uint64_t)63;   // every vector on a 256-byte boundary at least
    SPAL_HIP_TRY(vecs.alloc((size_t)nvec * stride * sizeof(T)));
    const uint64_t pe = scratch_elems(n);
    SPAL_HIP_TRY(parts.alloc(2 * pe * sizeof(T)));
    SPAL_HIP_TRY(scal.alloc(sizeof(Scal<T>)));
    SPAL_HIP_TRY(hipHostMalloc(&host.p, sizeof(Scal<T>), hipHostMallocDefault));
    SPAL_HIP_TRY(ev.create(1));
    auto vec_at = [&](int k) { return vecs.as<T>() + (uint64_t)k * stride; };

    Run<T, H> R;
    R.fn = fn;
    R.a = a;
    R.m = m;
    R.g = g;
    R.st = st;
    R.n = n;
    R.maxit = maxit;
    R.c1 = tiles_of(n);
    R.tol2 = (T)(tol * tol);
    R.s = scal.as<Scal<T>>();
    R.part0 = parts.as<T>();
    R.part1 = parts.as<T>() + pe;
    R.sweeps = sweeps;
    if (sweeps >= 0) {
        R.w0 = vec_at(nwork);
        R.w1 = vec_at(nwork + 1);
    }

    Scal<T> *h = (Scal<T> *)host.p;
    uint64_t polls = 0;
    auto poll = [&]() -> int {
        SPAL_HIP_TRY(hipMemcpyAsync(h, R.s, sizeof(Scal<T>), hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        ++polls;
        return SPAL_OK;
    };

    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    SPAL_HIP_TRY(hipMemsetAsync(R.s, 0, sizeof(Scal<T>), st));
    T *r = vec_at(0), *q = vec_at(1), *p = vec_at(2);
    // r = b - A x;  rr, bb;  it = 0;  test
    SPAL_TRY(R.mul(x, q));
    SPAL_TRY((R.template v<V_INIT>(b, q, nullptr, nullptr, nullptr, r)));
    SPAL_TRY((R.template f<F_INIT>()));
    uint64_t enqueued = 0;
    bool stopped = false;
    if (cg) {
        T *z = pre ? vec_at(3) : r;
        if (pre) SPAL_TRY(R.prec(r, z));
        SPAL_TRY((R.template v<V_COPY_DOT>(r, z, nullptr, nullptr, nullptr, p)));   // p = z;  rz
        SPAL_TRY((R.template f<F_RZ>()));
        while (enqueued < maxit && !stopped) {
            const uint64_t batch = std::min<uint64_t>((uint64_t)check_every, maxit - enqueued);
            for (uint64_t k = 0; k < batch; ++k) {
                SPAL_TRY(R.mul(p, q));
                SPAL_TRY((R.template v<V_DOT>(p, q, nullptr, nullptr, nullptr, nullptr)));
                SPAL_TRY((R.template f<F_ALPHA_CG>()));
                SPAL_TRY((R.template v<V_CG_XR>(p, q, nullptr, nullptr, x, r)));      // x, r;  rr
                SPAL_TRY((R.template f<F_TEST_CG>(pre ? 0 : 1)));                    // it, test (and beta when z is r)
                if (pre) {
                    SPAL_TRY(R.prec(r, z));
                    SPAL_TRY((R.template v<V_DOT>(r, z, nullptr, nullptr, nullptr, nullptr)));
                    SPAL_TRY((R.template f<F_BETA>()));
                }
                SPAL_TRY((R.template v<V_CG_P>(z, nullptr, nullptr, nullptr, nullptr, p)));
            }
            enqueued += batch;
            SPAL_TRY(poll());
            stopped = h->done != 0;
        }
    } else {
        T *rhat = vec_at(3), *vv = vec_at(4), *t = vec_at(5);
        T *sv = q;   // q is free once r exists
        T *ph = pre ? vec_at(6) : p, *sh = pre ? vec_at(7) : sv;
        SPAL_HIP_TRY(hipMemcpyAsync(rhat, r, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        SPAL_HIP_TRY(hipMemsetAsync(vv, 0, n * sizeof(T), st));
        SPAL_HIP_TRY(hipMemsetAsync(p, 0, n * sizeof(T), st));
        while (enqueued < maxit && !stopped) {
            const uint64_t batch = std::min<uint64_t>((uint64_t)check_every, maxit - enqueued);
            for (uint64_t k = 0; k < batch; ++k) {
                SPAL_TRY((R.template v<V_DOT>(rhat, r, nullptr, nullptr, nullptr, nullptr)));
                SPAL_TRY((R.template f<F_RHO>()));
                SPAL_TRY((R.template v<V_BI_P>(r, vv, nullptr, nullptr, nullptr, p)));
                if (pre) SPAL_TRY(R.prec(p, ph));
                SPAL_TRY(R.mul(ph, vv));
                SPAL_TRY((R.template v<V_DOT>(rhat, vv, nullptr, nullptr, nullptr, nullptr)));
                SPAL_TRY((R.template f<F_ALPHA_BI>()));
                SPAL_TRY((R.template v<V_BI_S>(r, vv, nullptr, nullptr, nullptr, sv)));   // s;  ss
                SPAL_TRY((R.template f<F_HALF>()));                                       // it;  the half-step exit
                SPAL_TRY((R.template v<V_BI_HALF>(ph, sv, nullptr, nullptr, x, r)));      // ... applied, if taken
                if (pre) SPAL_TRY(R.prec(sv, sh));
                SPAL_TRY(R.mul(sh, t));
                SPAL_TRY((R.template v<V_DOT2>(t, sv, nullptr, nullptr, nullptr, nullptr)));   // t . s, t . t
                SPAL_TRY((R.template f<F_OMEGA>()));
                SPAL_TRY((R.template v<V_BI_XR>(ph, sh, sv, t, x, r)));                   // x, r;  rr
                SPAL_TRY((R.template f<F_TEST_BI>()));
            }
            enqueued += batch;
            SPAL_TRY(poll());
            stopped = h->done != 0;
        }
    }
    if (!polls) SPAL_TRY(poll());   // maxit = 0: the test after r0 has decided
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    if (!h->done) return fail(SPAL_ERR_HIP, "%s: the device did not stop after %llu iterations", fn, (unsigned long long)maxit);
    float ms = 0.f;
    SPAL_HIP_TRY(ev.span(0, &ms));
    info->iterations = h->it;
    info->reason = (int)h->reason;
    info->residual_sq = (double)h->rr;
    info->rhs_sq = (double)h->bb;
    info->solve_ms = (double)ms;
    Record rec;
    rec.method = method;
    rec.preconditioned = pre ? 1 : 0;
    rec.amg = g ? 1 : 0;
    rec.precond_sweeps = sweeps;
    rec.reason = info->reason;
    rec.iterations = info->iterations;
    rec.polls = polls;
    rec.check_every = check_every;
    rec.solve_ms = info->solve_ms;
    const std::string json = info_json(rec);
    std::lock_guard<std::mutex> lock(owner->mu);
    a->ops.krylov_info = json;
    return SPAL_OK;
}

// every refusal that needs no device
// (amg: the call takes a hierarchy `g` where m stands, and g is not NULL)
template <typename T, typename H>
int krylov_check(const char *fn, H *a, int method, H *m, const T *b, T *x, double tol, spal_krylov_info *info,
                 bool amg = false, spal_amg *g = nullptr) {
    if (!a || !b || !x || !info || (amg && !g)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (method != SPAL_KRYLOV_CG && method != SPAL_KRYLOV_BICGSTAB)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: method = %d must be 0 (CG) or 1 (BiCGStab)", fn, method);
    SPAL_TRY((krylov_check_operands<T, H>(fn, a, m, tol)));
    return amg ? amg_check_match(fn, g, a->nrows, a->device, a->elem_size) : SPAL_OK;
}

template <typename T, typename H>
int krylov_dev(const char *fn, H *a, int method, H *m, const T *b, T *x, double tol, uint64_t maxit, void *stream,
               spal_krylov_info *info, bool amg = false, spal_amg *g = nullptr) {
    SPAL_TRY((krylov_check<T, H>(fn, a, method, m, b, x, tol, info, amg, g)));
    if (x == b) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x_dev == b_dev (b is read in every test of the residual)", fn);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return krylov_run<T, H>(fn, a, method, m, g, b, x, tol, maxit, (hipStream_t)stream, info);
}

template <typename T, typename H>
int krylov_host(const char *fn, H *a, int method, H *m, const T *b, uint64_t b_len, T *x, uint64_t x_len, double tol,
                uint64_t maxit, spal_krylov_info *info, bool amg = false, spal_amg *g = nullptr) {
    SPAL_TRY((krylov_check<T, H>(fn, a, method, m, b, x, tol, info, amg, g)));
    SPAL_TRY(refuse_lengths(fn, b_len, x_len, a->nrows));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const uint64_t n = a->nrows;
    DevBuf db, dx;
    PooledStream ps;   // a stream of the call's own: the handle's staging stream belongs to whoever holds its lock
    SPAL_HIP_TRY(db.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(dx.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    SPAL_HIP_TRY(hipMemcpyAsync(db.p, b, n * sizeof(T), hipMemcpyHostToDevice, ps.s));
    SPAL_HIP_TRY(hipMemcpyAsync(dx.p, x, n * sizeof(T), hipMemcpyHostToDevice, ps.s));
    SPAL_TRY((krylov_run<T, H>(fn, a, method, m, g, db.as<T>(), dx.as<T>(), tol, maxit, ps.s, info)));
    SPAL_HIP_TRY(hipMemcpyAsync(x, dx.p, n * sizeof(T), hipMemcpyDeviceToHost, ps.s));
    SPAL_HIP_TRY(hipStreamSynchronize(ps.s));
    return SPAL_OK;
}

}  // namespace

int krylov_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status) {
    if (strcmp(key, "krylov_check_every")) return 0;
    if (value < 1) {
        *status = fail(SPAL_ERR_INVALID_ARGUMENT, "krylov_check_every must be >= 1 (iterations enqueued between two polls of the stop flag)");
        return 1;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    s.krylov_check_every = value;
    *status = SPAL_OK;
    return 1;
}

int krylov_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    if (!solve) return SPAL_OK;
    std::string info;
    {
        std::lock_guard<std::mutex> lock(solve->mu);
        info = s.krylov_info;
    }
    return describe_append(buf, buf_len, "krylov", info);
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_dot_f64(const double *a, const double *b, uint64_t n, double *out) { return dot_host<double>("spal_dot", a, b, n, out); }
int spal_dot_f32(const float *a, const float *b, uint64_t n, float *out) { return dot_host<float>("spal_dot", a, b, n, out); }
int spal_dot_dev_f64(int device, const double *a_dev, const double *b_dev, uint64_t n, double *out_dev, void *stream) {
    return dot_dev<double>("spal_dot_dev", device, a_dev, b_dev, n, out_dev, stream);
}
int spal_dot_dev_f32(int device, const float *a_dev, const float *b_dev, uint64_t n, float *out_dev, void *stream) {
    return dot_dev<float>("spal_dot_dev", device, a_dev, b_dev, n, out_dev, stream);
}

int spal_csr_krylov_f64(spal_csr_t a, int method, spal_csr_t m, const double *b, uint64_t b_len, double *x, uint64_t x_len,
                        double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<double, spal_csr>("spal_csr_krylov", a, method, m, b, b_len, x, x_len, tol, maxit, info);
}
int spal_csr_krylov_f32(spal_csr_t a, int method, spal_csr_t m, const float *b, uint64_t b_len, float *x, uint64_t x_len,
                        double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<float, spal_csr>("spal_csr_krylov", a, method, m, b, b_len, x, x_len, tol, maxit, info);
}
int spal_csr_krylov_dev_f64(spal_csr_t a, int method, spal_csr_t m, const double *b_dev, double *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<double, spal_csr>("spal_csr_krylov_dev", a, method, m, b_dev, x_dev, tol, maxit, stream, info);
}
int spal_csr_krylov_dev_f32(spal_csr_t a, int method, spal_csr_t m, const float *b_dev, float *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<float, spal_csr>("spal_csr_krylov_dev", a, method, m, b_dev, x_dev, tol, maxit, stream, info);
}
int spal_csc_krylov_f64(spal_csc_t a, int method, spal_csc_t m, const double *b, uint64_t b_len, double *x, uint64_t x_len,
                        double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<double, spal_csc>("spal_csc_krylov", a, method, m, b, b_len, x, x_len, tol, maxit, info);
}
int spal_csc_krylov_f32(spal_csc_t a, int method, spal_csc_t m, const float *b, uint64_t b_len, float *x, uint64_t x_len,
                        double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<float, spal_csc>("spal_csc_krylov", a, method, m, b, b_len, x, x_len, tol, maxit, info);
}
int spal_csc_krylov_dev_f64(spal_csc_t a, int method, spal_csc_t m, const double *b_dev, double *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<double, spal_csc>("spal_csc_krylov_dev", a, method, m, b_dev, x_dev, tol, maxit, stream, info);
}
int spal_csc_krylov_dev_f32(spal_csc_t a, int method, spal_csc_t m, const float *b_dev, float *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<float, spal_csc>("spal_csc_krylov_dev", a, method, m, b_dev, x_dev, tol, maxit, stream, info);
}

// the same loops with M^-1 v = cycle(0, v) of an AMG hierarchy (spal_amg.hip)
int spal_csr_krylov_amg_f64(spal_csr_t a, int method, spal_amg_t g, const double *b, uint64_t b_len, double *x, uint64_t x_len,
                            double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<double, spal_csr>("spal_csr_krylov_amg", a, method, nullptr, b, b_len, x, x_len, tol, maxit, info, true, g);
}
int spal_csr_krylov_amg_dev_f64(spal_csr_t a, int method, spal_amg_t g, const double *b_dev, double *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<double, spal_csr>("spal_csr_krylov_amg_dev", a, method, nullptr, b_dev, x_dev, tol, maxit, stream, info, true, g);
}
int spal_csr_krylov_amg_f32(spal_csr_t a, int method, spal_amg_t g, const float *b, uint64_t b_len, float *x, uint64_t x_len,
                            double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<float, spal_csr>("spal_csr_krylov_amg", a, method, nullptr, b, b_len, x, x_len, tol, maxit, info, true, g);
}
int spal_csr_krylov_amg_dev_f32(spal_csr_t a, int method, spal_amg_t g, const float *b_dev, float *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<float, spal_csr>("spal_csr_krylov_amg_dev", a, method, nullptr, b_dev, x_dev, tol, maxit, stream, info, true, g);
}
int spal_csc_krylov_amg_f64(spal_csc_t a, int method, spal_amg_t g, const double *b, uint64_t b_len, double *x, uint64_t x_len,
                            double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<double, spal_csc>("spal_csc_krylov_amg", a, method, nullptr, b, b_len, x, x_len, tol, maxit, info, true, g);
}
int spal_csc_krylov_amg_dev_f64(spal_csc_t a, int method, spal_amg_t g, const double *b_dev, double *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<double, spal_csc>("spal_csc_krylov_amg_dev", a, method, nullptr, b_dev, x_dev, tol, maxit, stream, info, true, g);
}
int spal_csc_krylov_amg_f32(spal_csc_t a, int method, spal_amg_t g, const float *b, uint64_t b_len, float *x, uint64_t x_len,
                            double tol, uint64_t maxit, spal_krylov_info *info) {
    return krylov_host<float, spal_csc>("spal_csc_krylov_amg", a, method, nullptr, b, b_len, x, x_len, tol, maxit, info, true, g);
}
int spal_csc_krylov_amg_dev_f32(spal_csc_t a, int method, spal_amg_t g, const float *b_dev, float *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info) {
    return krylov_dev<float, spal_csc>("spal_csc_krylov_amg_dev", a, method, nullptr, b_dev, x_dev, tol, maxit, stream, info, true, g);
}

}  // extern "C"
