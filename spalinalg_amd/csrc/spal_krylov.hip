// spal_krylov.hip -- the dot product, CG, BiCGStab and MINRES on the device.  The contracts are written out in
// include/spal.h: dot(a, b, n) = reduce(p), p[i] = a[i] * b[i] rounded; reduce pads with +0.0 to whole tiles of 1024,
// halves every tile (h = 512 .. 1: e[t] = e[t] + e[t + h]) and, when there is more than one tile, reduces the tile sums
// the same way.  The order depends on n alone, so every kernel here returns the bits of the sequential text.
//
// (tile_sum, upper_levels, the scratch sizes, the plan preparation, M^-1 and the shared refusals are in krylov_kernels.hpp,
// which spal_gmres.hip includes too; so are the scalar block Scal, the fused updates vec_update and the scalar steps
// scalar_step, which spal_krylov_block.hip runs per column of a block of right-hand sides, and the frame of a call:
// KRYLOV_LAUNCH, SolveFrame, store_info, with_host_vectors.  The two loops themselves -- which launch follows which, and
// when the host polls -- are in krylov_loops.hpp with the names VecOp / FinOp, once for this file and the block file:
// `Run` below is the driver type they are instantiated on.)
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
// scalar launch after that clears it.  MINRES (the spal_*_minres_* entry points) reuses the word: its
// test sits in F_MR_ROT, and V_MR_WX behind it still applies that iteration's w and x -- without the next v.
//
// THE DRIVER HOLDS NO HANDLE LOCK ACROSS A PRODUCT OR A SOLVE: it calls the spal_*_spmv_dev_* / spal_*_trsv_dev_* entry
// points, each of which takes what it needs itself (f5b9766: re-entering a handle's lock deadlocks).  A factor whose
// option "trsv_sweeps" is s >= 0 is applied by s Jacobi sweeps per triangle instead (trsv_sweep_enqueue),
// through two more work vectors of the call.  The spal_*_krylov_amg_* entry points run the same two loops with an AMG
// hierarchy `g` in m's place (Precond): M^-1 v is one multigrid cycle (amg_apply_enqueue, spal_amg.hip),
// enqueued into the hierarchy's own work vectors under its own lock.  The spal_*_krylov_fsai_* / spal_*_minres_fsai_*
// entry points put an FSAI factor `f` there (spal_fsai.hip): M^-1 v = Gt (G v), two products through one
// more work vector of the call, so concurrent calls on one f share nothing but its two matrices.  Plans are built before the first iteration; work
// vectors, the scratch and the scalar block come from the caching allocator per call, so concurrent calls on one handle
// share nothing but the matrix.
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
    T *z;               // the third written operand (V_MR_WX)
    T sg;               // MINRES: T(shift)
};

template <typename T, int OP>
__device__ __forceinline__ void element(const VecArgs<T> &g, uint64_t i, const Coef<T> &k, T &p0, T &p1) {
    p0 = T(0);
    p1 = T(0);
    if (i >= g.n) return;   // the padding: +0.0, and it is added
    vec_update<T, OP>(g.a + i, g.b + i, g.c + i, g.d + i, g.x + i, g.y + i, g.z + i, k, p0, p1);
}

template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void vec(VecArgs<T> g, uint64_t tiles) {
    __shared__ T lds[2][kThreads];
    Coef<T> coef = {T(0), T(0), T(0), T(0), T(0), true};
    if (g.s) {   // uniform: one word for the whole grid, written by an earlier launch
        if (!op_live<T, OP>(g.s)) return;
        coef = op_coef<T, OP>(g.s, g.sg);
    }
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T p[4], q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) element<T, OP>(g, i + (uint64_t)k * kThreads, coef, p[k], q[k]);
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
        // the update the stop left behind (BiCGStab's half step, MINRES's w and x), if there was one, has been applied
        if ((OP == F_OMEGA || OP == F_MR_ALFA) && threadIdx.x == 0) s->half = 0;
        if (s->done != 0) return;                             // uniform; this launch does not write `done` before here
    }
    const T d0 = upper_levels<T>(g.part0, g.c1, lds);
    T d1 = T(0);
    if (OP == F_INIT || OP == F_OMEGA || OP == F_MR_INIT) d1 = upper_levels<T>(g.part1, g.c1, lds);
    if (threadIdx.x != 0) return;
    if (OP == F_STORE)
        *g.out = d0;
    else
        scalar_step<T, OP>(s, d0, d1, g.tol2, g.maxit, g.unpreconditioned);
}

// ---- host side of the launches --------------------------------------------------------------------------------------
template <typename T, int OP>
int launch_vec(const char *fn, const VecArgs<T> &g, hipStream_t st) {
    const uint64_t tiles = tiles_of(g.n);
    KRYLOV_LAUNCH((vec<T, OP>), first_level_grid(g.n), g, tiles);
    return SPAL_OK;
}
template <typename T, int OP>
int launch_finish(const char *fn, const FinArgs<T> &g, hipStream_t st) {
    KRYLOV_LAUNCH((finish<T, OP>), 1, g);
    return SPAL_OK;
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
    SPAL_TRY((launch_vec<T, V_DOT>(fn, g, st)));
    FinArgs<T> f = {};
    f.part0 = work.as<T>();
    f.c1 = tiles_of(n);
    f.out = out;
    return launch_finish<T, F_STORE>(fn, f, st);
}

constexpr int kMinres = 2;   // the method of the spal_*_minres_* entry points in here; spal_*_krylov_* refuse it

struct Record {
    int method = 0, preconditioned = 0, reason = 0, amg = 0, fsai = 0;
    int64_t precond_sweeps = -1;
    uint64_t iterations = 0, polls = 0;
    int64_t check_every = 0;
    double solve_ms = 0.0, shift = 0.0;
};
std::string info_json(const Record &r) {
    char buf[448], shift[64] = "";
    if (r.method == kMinres) snprintf(shift, sizeof shift, ", \"shift\": %.17g", r.shift);
    snprintf(buf, sizeof buf,
             "{\"method\": \"%s\", \"preconditioned\": %d, \"iterations\": %llu, \"reason\": %d, \"check_every\": %lld, "
             "\"polls\": %llu, \"solve_ms\": %.4f, \"precond_sweeps\": %lld%s%s}",
             r.method == SPAL_KRYLOV_CG ? "cg" : r.method == kMinres ? "minres" : "bicgstab", r.preconditioned,
             (unsigned long long)r.iterations, r.reason, (long long)r.check_every, (unsigned long long)r.polls, r.solve_ms,
             (long long)r.precond_sweeps, r.amg ? ", \"precond\": \"amg\"" : r.fsai ? ", \"precond\": \"fsai\"" : "",
             shift);   // (the objects written without a hierarchy or an FSAI factor do not change)
    return buf;
}

// The preconditioner of a call: an ILU(0) factor m, an AMG hierarchy g (spal_amg.hip), an FSAI factor f (spal_fsai.hip),
// or none.  Never two.
template <typename H>
struct Precond {
    H *m;
    spal_amg *g;
    spal_fsai *f = nullptr;
    explicit operator bool() const { return m || g || f; }   // M^-1 is there: z, ph and sh are vectors of their own
};

// The driver the loops of krylov_loops.hpp run on: an operand is a device vector; the scalar block, the scratch of two
// dots, and the launches by name.
template <typename T, typename H>
struct Run {
    const char *fn;
    H *a;
    Precond<H> pc;
    hipStream_t st;
    uint64_t n = 0, maxit = 0, c1 = 0, stride = 0;
    T tol2 = T(0), sg = T(0);       // sg: MINRES's T(shift)
    Scal<T> *s = nullptr;
    T *part0 = nullptr, *part1 = nullptr;
    int64_t sweeps = -1;            // m's option "trsv_sweeps"
    T *vecs = nullptr;              // work vector i at vecs + i * stride
    T *w0 = nullptr, *w1 = nullptr; // the sweeps' ping-pong vectors
    T *fu = nullptr;                // FSAI: u = G v, between the two products
    const T *b = nullptr;
    T *x = nullptr;
    SolveFrame<Scal<T>> frame;
    bool stopped = false;

    static T *null() { return nullptr; }
    const T *B() const { return b; }
    T *X() const { return x; }
    T *work(int i) const { return vecs + (uint64_t)i * stride; }
    bool preconditioned() const { return (bool)pc; }
    int mul(const T *v, T *out) { return mul_dev(a, v, out, st); }
    // out = M^-1 v (out != v); without a preconditioner the loops use v itself
    int prec(const T *v, T *out) {
        if (pc.f) return fsai_apply_enqueue(fn, pc.f, v, fu, out, st);
        return pc.g ? amg_apply_enqueue(fn, pc.g, v, out, st) : prec_dev<T, H>(fn, pc.m, sweeps, v, out, w0, w1, st);
    }
    template <int OP>
    int v(const T *va, const T *vb, const T *vc, const T *vd, T *vx, T *vy, T *vz = nullptr) {
        return launch_vec<T, OP>(fn, VecArgs<T>{va, vb, vc, vd, vx, vy, s, part0, part1, n, vz, sg}, st);
    }
    template <int OP>
    int f(int unpreconditioned = 0) {
        return launch_finish<T, OP>(fn, FinArgs<T>{s, part0, part1, c1, tol2, maxit, nullptr, unpreconditioned}, st);
    }
    int copy(T *dst, const T *src) {
        SPAL_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        return SPAL_OK;
    }
    int zero(T *dst) {
        SPAL_HIP_TRY(hipMemsetAsync(dst, 0, n * sizeof(T), st));
        return SPAL_OK;
    }
    int poll() {
        SPAL_TRY(frame.poll());
        stopped = frame.h->done != 0;
        return SPAL_OK;
    }
    bool all_stopped() const { return stopped; }
    uint64_t polls() const { return frame.polls; }
};

template <typename T, typename H>
int krylov_run(const char *fn, H *a, int method, Precond<H> pc, double shift, const T *b, T *x, double tol, uint64_t maxit,
               hipStream_t st, spal_krylov_info *info) {
    const uint64_t n = a->nrows;
    const bool pre = (bool)pc;
    const int64_t check_every = krylov_check_every_of(a, pre);
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    int64_t sweeps = -1;
    SPAL_TRY(krylov_prepare(fn, a, pc.m, st, &sweeps));
    // work vectors, scratch, scalars
    const bool cg = method == SPAL_KRYLOV_CG;
    const bool minres = method == kMinres;   // v, r1 / r2 / t, w1 / w2, and y with a preconditioner
    const int nwork = minres ? (pre ? 7 : 6) : cg ? (pre ? 4 : 3) : (pre ? 8 : 6);
    const int nvec = nwork + (sweeps >= 0 ? 2 : 0) + (pc.f ? 1 : 0);
    DevBuf vecs, parts, scal;
    const uint64_t stride = (n + 63) & ~(uint64_t)63;   // every vector on a 256-byte boundary at least
    SPAL_HIP_TRY(vecs.alloc((size_t)nvec * stride * sizeof(T)));
    const uint64_t pe = scratch_elems(n);
    SPAL_HIP_TRY(parts.alloc(2 * pe * sizeof(T)));
    SPAL_HIP_TRY(scal.alloc(sizeof(Scal<T>)));

    Run<T, H> R;
    SPAL_TRY(R.frame.create(st, 1));
    R.fn = fn;
    R.a = a;
    R.pc = pc;
    R.st = st;
    R.n = n;
    R.maxit = maxit;
    R.c1 = tiles_of(n);
    R.stride = stride;
    R.tol2 = (T)(tol * tol);
    R.sg = (T)shift;
    R.s = scal.as<Scal<T>>();
    R.part0 = parts.as<T>();
    R.part1 = parts.as<T>() + pe;
    R.sweeps = sweeps;
    R.vecs = vecs.as<T>();
    if (sweeps >= 0) {
        R.w0 = R.work(nwork);
        R.w1 = R.work(nwork + 1);
    }
    if (pc.f) R.fu = R.work(nvec - 1);
    R.b = b;
    R.x = x;

    SPAL_TRY(R.frame.begin(R.s, sizeof(Scal<T>)));
    if (minres) {
        SPAL_TRY(minres_start(R));
        SPAL_TRY(minres_loop(R, maxit, (uint64_t)check_every));
    } else {
        SPAL_TRY(krylov_start(R));
        SPAL_TRY(cg ? cg_loop(R, maxit, (uint64_t)check_every) : bicgstab_loop(R, maxit, (uint64_t)check_every));
    }
    float ms = 0.f;
    SPAL_TRY(R.frame.end(&ms));
    if (!R.stopped) return fail(SPAL_ERR_HIP, "%s: the device did not stop after %llu iterations", fn, (unsigned long long)maxit);
    R.frame.fill(info, 0, ms);
    Record rec;
    rec.method = method;
    rec.preconditioned = pre ? 1 : 0;
    rec.amg = pc.g ? 1 : 0;
    rec.fsai = pc.f ? 1 : 0;
    rec.precond_sweeps = sweeps;
    rec.reason = info->reason;
    rec.iterations = info->iterations;
    rec.polls = R.frame.polls;
    rec.check_every = check_every;
    rec.solve_ms = info->solve_ms;
    rec.shift = shift;
    store_info(a, &OpState::krylov_info, info_json(rec));
    return SPAL_OK;
}

// every refusal that needs no device (a hierarchy has to agree with a in rows, device and element type)
// (shift: 0 for CG and BiCGStab, whose entry points have none; `method` is the caller's, or kMinres from the MINRES entries)
template <typename T, typename H>
int krylov_check(const char *fn, H *a, int method, bool minres, Precond<H> pc, double shift, const T *b, T *x, double tol,
                 spal_krylov_info *info) {
    if (!a || !b || !x || !info) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (!minres && method != SPAL_KRYLOV_CG && method != SPAL_KRYLOV_BICGSTAB)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: method = %d must be 0 (CG) or 1 (BiCGStab)", fn, method);
    if (!std::isfinite(shift)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: shift = %g must be finite", fn, shift);
    SPAL_TRY((krylov_check_operands<T, H>(fn, a, pc.m, tol)));
    if (pc.f) return fsai_check_match(fn, pc.f, a->nrows, a->device, a->elem_size);
    return pc.g ? amg_check_match(fn, pc.g, a->nrows, a->device, a->elem_size) : SPAL_OK;
}

template <typename T, typename H>
int krylov_dev(const char *fn, H *a, int method, bool minres, Precond<H> pc, double shift, const T *b, T *x, double tol,
               uint64_t maxit, void *stream, spal_krylov_info *info) {
    SPAL_TRY((krylov_check<T, H>(fn, a, method, minres, pc, shift, b, x, tol, info)));
    if (x == b) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x_dev == b_dev (b is read in every test of the residual)", fn);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return krylov_run<T, H>(fn, a, minres ? kMinres : method, pc, shift, b, x, tol, maxit, (hipStream_t)stream, info);
}

template <typename T, typename H>
int krylov_host(const char *fn, H *a, int method, bool minres, Precond<H> pc, double shift, const T *b, uint64_t b_len, T *x,
                uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info) {
    SPAL_TRY((krylov_check<T, H>(fn, a, method, minres, pc, shift, b, x, tol, info)));
    return with_host_vectors(fn, a, b, b_len, x, x_len, [&](const T *b_dev, T *x_dev, hipStream_t st) {
        return krylov_run<T, H>(fn, a, minres ? kMinres : method, pc, shift, b_dev, x_dev, tol, maxit, st, info);
    });
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
    return info_describe_append(buf, buf_len, s, solve, "krylov", &OpState::krylov_info);
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

// name = krylov: m is an ILU(0) factor or NULL.  name = krylov_amg: the same loops with M^-1 v = cycle(0, v) of an AMG
// hierarchy m (spal_amg.hip), which is not optional.
#define SPAL_KRYLOV_ENTRIES(kind, name, sfx, T, M, NEEDS_M, PRECOND)                                                   \
    int spal_##kind##_##name##_##sfx(spal_##kind##_t a, int method, M m, const T *b, uint64_t b_len, T *x,             \
                                     uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info) {             \
        const char *fn = "spal_" #kind "_" #name;                                                                      \
        if (NEEDS_M && !m) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);                            \
        return krylov_host<T, spal_##kind>(fn, a, method, false, PRECOND, 0.0, b, b_len, x, x_len, tol, maxit, info);             \
    }                                                                                                                  \
    int spal_##kind##_##name##_dev_##sfx(spal_##kind##_t a, int method, M m, const T *b_dev, T *x_dev, double tol,     \
                                         uint64_t maxit, void *stream, spal_krylov_info *info) {                       \
        const char *fn = "spal_" #kind "_" #name "_dev";                                                               \
        if (NEEDS_M && !m) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);                            \
        return krylov_dev<T, spal_##kind>(fn, a, method, false, PRECOND, 0.0, b_dev, x_dev, tol, maxit, stream, info);           \
    }
// MINRES on (A - shift I) x = b: the arguments of spal_*_krylov_* without `method`, with `shift` after m.  name =
// minres: m is a factor or NULL.  name = minres_fsai: m is an FSAI factor, which is not optional.
#define SPAL_MINRES_ENTRIES(kind, name, sfx, T, M, NEEDS_M, PRECOND)                                                   \
    int spal_##kind##_##name##_##sfx(spal_##kind##_t a, M m, double shift, const T *b, uint64_t b_len, T *x,           \
                                     uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info) {             \
        const char *fn = "spal_" #kind "_" #name;                                                                      \
        if (NEEDS_M && !m) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);                            \
        return krylov_host<T, spal_##kind>(fn, a, 0, true, PRECOND, shift, b, b_len, x, x_len, tol, maxit, info);      \
    }                                                                                                                  \
    int spal_##kind##_##name##_dev_##sfx(spal_##kind##_t a, M m, double shift, const T *b_dev, T *x_dev, double tol,   \
                                         uint64_t maxit, void *stream, spal_krylov_info *info) {                       \
        const char *fn = "spal_" #kind "_" #name "_dev";                                                               \
        if (NEEDS_M && !m) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);                            \
        return krylov_dev<T, spal_##kind>(fn, a, 0, true, PRECOND, shift, b_dev, x_dev, tol, maxit, stream, info);     \
    }
#define SPAL_KRYLOV_KINDS(kind, sfx, T)                                                                                \
    SPAL_MINRES_ENTRIES(kind, minres, sfx, T, spal_##kind##_t, false, (Precond<spal_##kind>{m, nullptr}))              \
    SPAL_MINRES_ENTRIES(kind, minres_fsai, sfx, T, spal_fsai_t, true, (Precond<spal_##kind>{nullptr, nullptr, m}))     \
    SPAL_KRYLOV_ENTRIES(kind, krylov, sfx, T, spal_##kind##_t, false, (Precond<spal_##kind>{m, nullptr}))              \
    SPAL_KRYLOV_ENTRIES(kind, krylov_amg, sfx, T, spal_amg_t, true, (Precond<spal_##kind>{nullptr, m}))                \
    SPAL_KRYLOV_ENTRIES(kind, krylov_fsai, sfx, T, spal_fsai_t, true, (Precond<spal_##kind>{nullptr, nullptr, m}))
SPAL_KRYLOV_KINDS(csr, f64, double)
SPAL_KRYLOV_KINDS(csr, f32, float)
SPAL_KRYLOV_KINDS(csc, f64, double)
SPAL_KRYLOV_KINDS(csc, f32, float)
#undef SPAL_KRYLOV_KINDS
#undef SPAL_KRYLOV_ENTRIES
#undef SPAL_MINRES_ENTRIES

}  // extern "C"
