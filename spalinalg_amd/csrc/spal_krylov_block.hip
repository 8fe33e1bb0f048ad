// spal_krylov_block.hip -- CG and BiCGStab for a block of k right-hand sides: k INDEPENDENT iterations run
// in lockstep on shared launches.  B and X are n x k, dense and row-major (element (i, j) at [i * ld + j], ld >= k): the
// layout of SpMM and of the block triangular solves.  Column j follows the loops written out in include/spal.h exactly
// as spal_*_krylov_* does -- its own bb, thr, scalars, it, stop test and reason -- with A v the value spal_*_spmm_*
// defines and M^-1 v column j of the two spal_*_trsm_* (or spal_*_trsm_sweep_*) calls.  One pass over the matrix and one
// walk of the factor's launches serve all k columns; that is the whole point.  It is NOT a block-Krylov method: no
// search space is shared, so every column keeps its sequential text and its bits.
//
// (tile_sum, upper_levels, the scalar block Scal, the ten fused updates and the scalar steps are in krylov_kernels.hpp,
// shared with spal_krylov.hip: the arithmetic of a column is the vector call's, by construction.  Mat, column_tree, the
// column tiles and the routes to SpMM and trsm are there too, shared with spal_gmres_block.hip.)
//
// THE FIRST LEVEL.  A workgroup of 256 covers a tile of 1024 rows x KT columns of the blocks.  Thread t is column
// t % KT of the tile and row group g = t / KT of G = 256 / KT; it owns rows g, g + G, g + 2G, ... of the tile, L = 4 KT
// of them, so the KT lanes of a group read KT consecutive elements of one row and a wave reads 64 / KT consecutive
// rows: with ld == k == KT one load instruction of a wave is 64 consecutive elements.  The header's tree over the tile's
// 1024 rows, h = 512 .. 1: e[t] = e[t] + e[t + h], splits by where row t lives:
//   * h >= G pairs two rows of ONE thread (local indices i and i + h / G): thread-local.  The L values are not all kept
//     in registers: they are taken in C = L / 16 chunks {o, o + C, o + 2C, ...} of 16, each halved to one value (strides
//     8C .. C of the local index), and the C chunk sums are halved in turn (strides C / 2 .. 1) as they arrive.
//   * h < G pairs thread (g, j) with thread (g + h, j), 'h * KT' threads further: strides 128 and 64 go through LDS,
//     strides 32 .. KT are __shfl_down inside wave 0.  Threads 0 .. KT - 1 end with their column's tile sum and store it
//     to part[column][tile].
// Rows past n contribute +0.0, and it is added.  Tiles of rows are grid-strided (blockIdx.x, at most kBlockMaxGrid
// workgroups), tiles of columns too (blockIdx.y): k wider than the tile is covered inside each launch.
// THE FINISH.  gridDim.x = k: workgroup j walks upper_levels for column j and its thread 0 does the column's scalar step
// in Scal<T>[j].
//
// FREEZE, PER COLUMN.  `done` and `half` are read per column, so they are NOT uniform over a first-level workgroup: a
// masked column's lanes skip every load and store (and the store of their tile sum) but run through every barrier and
// shuffle with +0.0.  Once column j has stopped nothing writes its x, r, p, scalars or it again; V_BI_HALF is applied to
// exactly the columns whose `half` is set.  Products and solves keep running on all k columns, into work blocks:
// compacting the active columns is out of scope.  The call ends when the poll counts k stopped columns.
// ORDER BETWEEN LAUNCHES IS STREAM ORDER ALONE: no flags waited on, no spins, no tickets, no float atomics, no grid syncs.
//
// THE DRIVER HOLDS NO HANDLE LOCK ACROSS A PRODUCT OR A SOLVE: it calls spal_*_spmm_dev_*, spal_*_trsm_dev_* and
// spal_*_trsm_sweep_dev_*, each of which takes what it needs itself.  Plans are built and every work block, the dot
// scratch and the scalar blocks are taken before the first iteration; the stream's sweep scratch is grown to n x k there
// too, so no iteration allocates and nothing synchronises but the polls.
#include "krylov_kernels.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace spal {
namespace {

template <typename T>
struct BlockVecArgs {
    Mat<const T> a, b, c, d;
    Mat<T> x, y;
    const Scal<T> *s;   // k records
    T *part0, *part1;   // tile sums of d0 / d1: part[column * pe + tile]
    uint64_t n, pe;
    uint32_t k;
};

template <typename T, int OP, int KT>
__global__ __launch_bounds__(kThreads) void vec_block(BlockVecArgs<T> g, uint64_t tiles) {
    constexpr int G = kThreads / KT;            // row groups of a workgroup
    constexpr int L = (int)kTile / G;           // rows of a thread
    constexpr int CH = L < 16 ? L : 16;         // a chunk of them
    constexpr int C = L / CH;                   // 1, 2, 4 or 8 chunks
    constexpr int LOGC = C == 8 ? 3 : C == 4 ? 2 : C == 2 ? 1 : 0;
    constexpr int U = 4;                       // elements whose loads are in flight together (L >= 4)
    __shared__ T lds[2][kThreads];
    const unsigned j = threadIdx.x % KT, grp = threadIdx.x / KT;
    for (uint64_t ct = blockIdx.y; ct * KT < g.k; ct += gridDim.y) {
        const uint64_t col = ct * KT + j;
        // per column, hence per lane: a masked lane skips its loads and stores and still reaches every barrier
        bool live = col < g.k;
        T alpha = T(0), beta = T(0), omega = T(0);
        if (live) {
            const Scal<T> *s = g.s + col;   // written by an earlier launch
            live = OP == V_BI_HALF ? s->half != 0 : s->done == 0;
            alpha = s->alpha;
            beta = s->beta;
            omega = s->omega;
        }
        for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const uint64_t row0 = tile * kTile + grp;
            // The chunks in bit-reversed order, so that a chunk sum meets its partner of the widest stride first: a sum
            // waits in c0[b] / c1[b] for the one that completes a pair of stride C >> (b + 1), as a binary counter carries.
            T w0 = T(0), w1 = T(0), c0[LOGC + 1] = {}, c1[LOGC + 1] = {};
#pragma unroll 1
            for (int idx = 0; idx < C; ++idx) {
                const int o = LOGC ? (int)(__brev((unsigned)idx) >> (32 - (LOGC ? LOGC : 1))) : 0;   // idx's LOGC bits reversed
                T p[CH], q[CH];
#pragma unroll
                for (int m0 = 0; m0 < CH; m0 += U) {   // U elements: every load, then the arithmetic, then the stores
                    T av[U], bv[U], cv[U], dv[U], xv[U], yv[U];
                    uint64_t i[U];
                    bool in[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        i[u] = row0 + (uint64_t)(o + (m0 + u) * C) * G;
                        in[u] = live && i[u] < g.n;
                        av[u] = bv[u] = cv[u] = dv[u] = xv[u] = yv[u] = T(0);
                        if (in[u]) {
                            av[u] = g.a.p[i[u] * g.a.ld + col];
                            if (Reads<OP>::b) bv[u] = g.b.p[i[u] * g.b.ld + col];
                            if (Reads<OP>::c) cv[u] = g.c.p[i[u] * g.c.ld + col];
                            if (Reads<OP>::d) dv[u] = g.d.p[i[u] * g.d.ld + col];
                            if (Reads<OP>::x) xv[u] = g.x.p[i[u] * g.x.ld + col];
                            if (Reads<OP>::y) yv[u] = g.y.p[i[u] * g.y.ld + col];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        p[m0 + u] = T(0);   // the padding, and a masked column: +0.0, and it is added
                        q[m0 + u] = T(0);
                        if (in[u])
                            vec_value<T, OP>(av[u], bv[u], cv[u], dv[u], xv[u], yv[u], alpha, beta, omega, p[m0 + u], q[m0 + u]);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (in[u]) {
                            if (Writes<OP>::x) g.x.p[i[u] * g.x.ld + col] = xv[u];
                            if (Writes<OP>::y) g.y.p[i[u] * g.y.ld + col] = yv[u];
                        }
                    }
                }
#pragma unroll
                for (int h = CH / 2; h >= 1; h >>= 1) {
#pragma unroll
                    for (int m = 0; m < h; ++m) {
                        if (Dots<OP>::n >= 1) p[m] = p[m] + p[m + h];
                        if (Dots<OP>::n >= 2) q[m] = q[m] + q[m + h];
                    }
                }
                w0 = p[0];
                w1 = q[0];
                bool carry = true;   // uniform: idx is the same in every thread
#pragma unroll
                for (int bit = 0; bit < LOGC; ++bit) {
                    if (carry && (idx >> bit & 1)) {   // the partner waits: it came earlier and holds the lower rows
                        if (Dots<OP>::n >= 1) w0 = c0[bit] + w0;
                        if (Dots<OP>::n >= 2) w1 = c1[bit] + w1;
                    } else if (carry) {
                        c0[bit] = w0;
                        c1[bit] = w1;
                        carry = false;
                    }
                }
            }
            if (Dots<OP>::n >= 1) {
                const T s = column_tree<T, KT>(w0, lds[0]);
                if (grp == 0 && live) g.part0[col * g.pe + tile] = s;
            }
            if (Dots<OP>::n >= 2) {
                const T s = column_tree<T, KT>(w1, lds[1]);
                if (grp == 0 && live) g.part1[col * g.pe + tile] = s;
            }
        }
    }
}

template <typename T>
struct BlockFinArgs {
    Scal<T> *s;
    T *part0, *part1;
    uint64_t c1, pe;
    uint32_t k;
    T tol2;            // T(tol * tol)
    uint64_t maxit;
    int unpreconditioned;
};

template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void finish_block(BlockFinArgs<T> g) {
    __shared__ T lds[kThreads];
    for (uint64_t col = blockIdx.x; col < g.k; col += gridDim.x) {
        Scal<T> *s = g.s + col;
        const bool done = s->done != 0;   // uniform over the workgroup: one column
        __syncthreads();                  // every thread has read it before thread 0 may write it
        if (OP == F_OMEGA && threadIdx.x == 0) s->half = 0;   // the half step, if there was one, has been applied
        if (done) continue;
        const T d0 = upper_levels<T>(g.part0 + col * g.pe, g.c1, lds);
        T d1 = T(0);
        if (OP == F_INIT || OP == F_OMEGA) d1 = upper_levels<T>(g.part1 + col * g.pe, g.c1, lds);
        if (threadIdx.x == 0) scalar_step<T, OP>(s, d0, d1, g.tol2, g.maxit, g.unpreconditioned);
    }
}

// ---- host side of the launches (the tiles, auto_tile, the routes and bytes_of are in krylov_kernels.hpp) ---------------
template <typename T, int OP>
hipError_t launch_vec_block(const BlockVecArgs<T> &g, int tile, hipStream_t st) {
    const uint64_t tiles = tiles_of(g.n);
    const unsigned gx = (unsigned)std::min<uint64_t>(tiles, kBlockMaxGrid);
    const unsigned gy = std::min<unsigned>(grid_of(g.k, (unsigned)tile), kColumnGrid);
#define SPAL_KB_CASE(KT)                                                                                               \
    case KT:                                                                                                           \
        hipLaunchKernelGGL((vec_block<T, OP, KT>), dim3(gx, gy), dim3(kThreads), 0, st, g, tiles);                    \
        break;
    switch (tile) {
        SPAL_KB_CASE(1)
        SPAL_KB_CASE(2)
        SPAL_KB_CASE(4)
        SPAL_KB_CASE(8)
        SPAL_KB_CASE(16)
    default:
        SPAL_KB_CASE(32)
    }
#undef SPAL_KB_CASE
    return hipGetLastError();
}

template <typename T, int OP>
hipError_t launch_finish_block(const BlockFinArgs<T> &g, hipStream_t st) {
    hipLaunchKernelGGL((finish_block<T, OP>), dim3(std::min<unsigned>(g.k, kFinishGrid)), dim3(kThreads), 0, st, g);
    return hipGetLastError();
}

struct Record {
    int method = 0, preconditioned = 0, tile = 0;
    int64_t precond_sweeps = -1, check_every = 0;
    uint64_t k = 0, iterations_min = 0, iterations_max = 0, converged = 0, polls = 0;
    double solve_ms = 0.0;
};
std::string info_json(const Record &r) {
    char buf[512];
    snprintf(buf, sizeof buf,
             "{\"method\": \"%s\", \"k\": %llu, \"preconditioned\": %d, \"precond_sweeps\": %lld, \"tile\": %d, "
             "\"iterations_min\": %llu, \"iterations_max\": %llu, \"converged\": %llu, \"check_every\": %lld, "
             "\"polls\": %llu, \"solve_ms\": %.4f}",
             r.method == SPAL_KRYLOV_CG ? "cg" : "bicgstab", (unsigned long long)r.k, r.preconditioned,
             (long long)r.precond_sweeps, r.tile, (unsigned long long)r.iterations_min, (unsigned long long)r.iterations_max,
             (unsigned long long)r.converged, (long long)r.check_every, (unsigned long long)r.polls, r.solve_ms);
    return buf;
}

// What both loops share: the blocks, the scalar records, the scratch of two dots per column, and the launches by name.
// A work block is packed (leading dimension k).
template <typename T, typename H>
struct Run {
    const char *fn;
    H *a, *m;
    hipStream_t st;
    uint64_t n = 0, maxit = 0, c1 = 0, pe = 0;
    uint32_t k = 0;
    int tile = 1;
    T tol2 = T(0);
    Scal<T> *s = nullptr;
    T *part0 = nullptr, *part1 = nullptr;
    int64_t sweeps = -1;   // m's option "trsv_sweeps"

    int mul(Mat<const T> v, T *out) { return mul_block(a, k, v.p, v.ld, out, k, st); }
    // out = M^-1 v (out != v, both packed); without a preconditioner the caller uses v itself
    int prec(const T *v, T *out) {
        if (sweeps >= 0) {
            SPAL_TRY(sweep_block(m, 0, 1, (uint64_t)sweeps, k, v, k, out, k, st));
            return sweep_block(m, 1, 0, (uint64_t)sweeps, k, out, k, out, k, st);
        }
        SPAL_TRY(solve_block(m, 0, 1, k, v, k, out, k, st));
        return solve_block(m, 1, 0, k, out, k, out, k, st);
    }
    template <int OP>
    int v(Mat<const T> va, Mat<const T> vb, Mat<const T> vc, Mat<const T> vd, Mat<T> x, Mat<T> y) {
        BlockVecArgs<T> g = {va, vb, vc, vd, x, y, s, part0, part1, n, pe, k};
        const hipError_t e = launch_vec_block<T, OP>(g, tile, st);
        return e == hipSuccess ? SPAL_OK : fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    }
    template <int OP>
    int f(int unpreconditioned = 0) {
        BlockFinArgs<T> g = {s, part0, part1, c1, pe, k, tol2, maxit, unpreconditioned};
        const hipError_t e = launch_finish_block<T, OP>(g, st);
        return e == hipSuccess ? SPAL_OK : fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    }
};

template <typename T, typename H>
int block_run(const char *fn, H *a, int method, H *m, uint32_t k, const T *b, uint64_t ldb, T *x, uint64_t ldx,
              double tol, uint64_t maxit, hipStream_t st, spal_krylov_info *info) {
    const uint64_t n = a->nrows;
    spal_csr *owner = solve_handle(a);   // whose lock guards a's options and its "krylov_block" string
    const int64_t check_every = krylov_check_every_of(a, m != nullptr);
    int tile;
    {
        std::lock_guard<std::mutex> lock(owner->mu);
        tile = a->ops.krylov_tile;
    }
    if (!tile) tile = auto_tile(k);
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    int64_t sweeps = -1;
    SPAL_TRY(krylov_prepare(fn, a, m, st, &sweeps));
    // work blocks, scratch, scalars: all at once, before the first iteration
    const bool cg = method == SPAL_KRYLOV_CG;
    const int nwork = cg ? (m ? 4 : 3) : (m ? 8 : 6);
    const uint64_t pe = scratch_elems(n);
    size_t work_bytes = 0, part_bytes = 0, sweep_bytes = 0;
    if (n > (std::numeric_limits<uint64_t>::max() - 63) / k)
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for work blocks of %llu x %u", fn, (unsigned long long)n, k);
    const uint64_t stride = (n * k + 63) & ~(uint64_t)63;   // every block on a 256-byte boundary at least
    if (!bytes_of(stride, (uint64_t)nwork, sizeof(T), 1, &work_bytes) || !bytes_of(pe, k, 2, sizeof(T), &part_bytes) ||
        !bytes_of(stride, 2, sizeof(T), 1, &sweep_bytes))
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for work blocks of %llu x %u", fn, (unsigned long long)n, k);
    DevBuf blocks, parts, scal;
    PinnedBuf host;
    EventSpans ev;
    SPAL_HIP_TRY(blocks.alloc(work_bytes));
    SPAL_HIP_TRY(parts.alloc(part_bytes));
    SPAL_HIP_TRY(scal.alloc((size_t)k * sizeof(Scal<T>)));
    SPAL_HIP_TRY(hipHostMalloc(&host.p, (size_t)k * sizeof(Scal<T>), hipHostMallocDefault));
    SPAL_HIP_TRY(ev.create(1));
    if (m && sweeps >= 1 && n) {   // the stream's sweep scratch holds n x k per ping-pong block from here on
        StreamWork grow;
        SPAL_TRY(grow.take(fn, st, sweep_bytes));
    }
    auto block_at = [&](int i) { return blocks.as<T>() + (uint64_t)i * stride; };
    auto Out = [&](T *p) { return Mat<T>{p, (uint64_t)k}; };
    auto In = [&](const T *p) { return Mat<const T>{p, (uint64_t)k}; };
    const Mat<const T> none = {nullptr, 0};
    const Mat<T> nonew = {nullptr, 0};
    const Mat<const T> B = {b, ldb};
    const Mat<T> X = {x, ldx};

    Run<T, H> R;
    R.fn = fn;
    R.a = a;
    R.m = m;
    R.st = st;
    R.n = n;
    R.maxit = maxit;
    R.c1 = tiles_of(n);
    R.pe = pe;
    R.k = k;
    R.tile = tile;
    R.tol2 = (T)(tol * tol);
    R.s = scal.as<Scal<T>>();
    R.part0 = parts.as<T>();
    R.part1 = parts.as<T>() + pe * k;
    R.sweeps = sweeps;

    Scal<T> *h = (Scal<T> *)host.p;
    uint64_t polls = 0, stopped = 0;
    auto poll = [&]() -> int {   // the k records to pinned memory; how many columns have stopped
        SPAL_HIP_TRY(hipMemcpyAsync(h, R.s, (size_t)k * sizeof(Scal<T>), hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        ++polls;
        stopped = 0;
        for (uint32_t j = 0; j < k; ++j) stopped += h[j].done != 0;
        return SPAL_OK;
    };

    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    SPAL_HIP_TRY(hipMemsetAsync(R.s, 0, (size_t)k * sizeof(Scal<T>), st));
    T *r = block_at(0), *q = block_at(1), *p = block_at(2);
    // r = b - A x;  rr, bb;  it = 0;  test
    SPAL_TRY(R.mul(Mat<const T>{x, ldx}, q));
    SPAL_TRY((R.template v<V_INIT>(B, In(q), none, none, nonew, Out(r))));
    SPAL_TRY((R.template f<F_INIT>()));
    uint64_t enqueued = 0;
    if (cg) {
        T *z = m ? block_at(3) : r;
        if (m) SPAL_TRY(R.prec(r, z));
        SPAL_TRY((R.template v<V_COPY_DOT>(In(r), In(z), none, none, nonew, Out(p))));   // p = z;  rz
        SPAL_TRY((R.template f<F_RZ>()));
        while (enqueued < maxit && stopped < k) {
            const uint64_t batch = std::min<uint64_t>((uint64_t)check_every, maxit - enqueued);
            for (uint64_t i = 0; i < batch; ++i) {
                SPAL_TRY(R.mul(In(p), q));
                SPAL_TRY((R.template v<V_DOT>(In(p), In(q), none, none, nonew, nonew)));
                SPAL_TRY((R.template f<F_ALPHA_CG>()));
                SPAL_TRY((R.template v<V_CG_XR>(In(p), In(q), none, none, X, Out(r))));   // x, r;  rr
                SPAL_TRY((R.template f<F_TEST_CG>(m ? 0 : 1)));                           // it, test (and beta when z is r)
                if (m) {
                    SPAL_TRY(R.prec(r, z));
                    SPAL_TRY((R.template v<V_DOT>(In(r), In(z), none, none, nonew, nonew)));
                    SPAL_TRY((R.template f<F_BETA>()));
                }
                SPAL_TRY((R.template v<V_CG_P>(In(z), none, none, none, nonew, Out(p))));
            }
            enqueued += batch;
            SPAL_TRY(poll());
        }
    } else {
        T *rhat = block_at(3), *vv = block_at(4), *t = block_at(5);
        T *sv = q;   // q is free once r exists
        T *ph = m ? block_at(6) : p, *sh = m ? block_at(7) : sv;
        SPAL_HIP_TRY(hipMemcpyAsync(rhat, r, (size_t)(n * k) * sizeof(T), hipMemcpyDeviceToDevice, st));
        SPAL_HIP_TRY(hipMemsetAsync(vv, 0, (size_t)(n * k) * sizeof(T), st));
        SPAL_HIP_TRY(hipMemsetAsync(p, 0, (size_t)(n * k) * sizeof(T), st));
        while (enqueued < maxit && stopped < k) {
            const uint64_t batch = std::min<uint64_t>((uint64_t)check_every, maxit - enqueued);
            for (uint64_t i = 0; i < batch; ++i) {
                SPAL_TRY((R.template v<V_DOT>(In(rhat), In(r), none, none, nonew, nonew)));
                SPAL_TRY((R.template f<F_RHO>()));
                SPAL_TRY((R.template v<V_BI_P>(In(r), In(vv), none, none, nonew, Out(p))));
                if (m) SPAL_TRY(R.prec(p, ph));
                SPAL_TRY(R.mul(In(ph), vv));
                SPAL_TRY((R.template v<V_DOT>(In(rhat), In(vv), none, none, nonew, nonew)));
                SPAL_TRY((R.template f<F_ALPHA_BI>()));
                SPAL_TRY((R.template v<V_BI_S>(In(r), In(vv), none, none, nonew, Out(sv))));   // s;  ss
                SPAL_TRY((R.template f<F_HALF>()));                                            // it;  the half-step exit
                SPAL_TRY((R.template v<V_BI_HALF>(In(ph), In(sv), none, none, X, Out(r))));    // ... applied, where taken
                if (m) SPAL_TRY(R.prec(sv, sh));
                SPAL_TRY(R.mul(In(sh), t));
                SPAL_TRY((R.template v<V_DOT2>(In(t), In(sv), none, none, nonew, nonew)));     // t . s, t . t
                SPAL_TRY((R.template f<F_OMEGA>()));
                SPAL_TRY((R.template v<V_BI_XR>(In(ph), In(sh), In(sv), In(t), X, Out(r))));   // x, r;  rr
                SPAL_TRY((R.template f<F_TEST_BI>()));
            }
            enqueued += batch;
            SPAL_TRY(poll());
        }
    }
    if (!polls) SPAL_TRY(poll());   // maxit = 0: the test after r0 has decided
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    if (stopped < k)
        return fail(SPAL_ERR_HIP, "%s: %llu of %u columns did not stop after %llu iterations", fn,
                    (unsigned long long)(k - stopped), k, (unsigned long long)maxit);
    float ms = 0.f;
    SPAL_HIP_TRY(ev.span(0, &ms));
    Record rec;
    rec.iterations_min = h[0].it;
    for (uint32_t j = 0; j < k; ++j) {
        info[j].iterations = h[j].it;
        info[j].reason = (int)h[j].reason;
        info[j].residual_sq = (double)h[j].rr;
        info[j].rhs_sq = (double)h[j].bb;
        info[j].solve_ms = (double)ms;
        rec.iterations_min = std::min<uint64_t>(rec.iterations_min, h[j].it);
        rec.iterations_max = std::max<uint64_t>(rec.iterations_max, h[j].it);
        rec.converged += h[j].reason == 0;
    }
    rec.method = method;
    rec.k = k;
    rec.preconditioned = m ? 1 : 0;
    rec.precond_sweeps = sweeps;
    rec.tile = tile;
    rec.polls = polls;
    rec.check_every = check_every;
    rec.solve_ms = (double)ms;
    const std::string json = info_json(rec);
    std::lock_guard<std::mutex> lock(owner->mu);
    a->ops.krylov_block_info = json;
    return SPAL_OK;
}

// Every refusal that needs no device; `who` begins the messages ("spal_csr_krylov_block").  The block's geometry and the
// method come first: they need nothing of the handles.
template <typename T, typename H>
int block_check(const char *who, H *a, int method, H *m, uint64_t k, const T *b, uint64_t ldb, T *x, uint64_t ldx,
                double tol, spal_krylov_info *info) {
    if (!a || !b || !x || !info) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    if (method != SPAL_KRYLOV_CG && method != SPAL_KRYLOV_BICGSTAB)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: method = %d must be 0 (CG) or 1 (BiCGStab)", who, method);
    if (k == 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: k = 0 (B and X need at least one column)", who);
    if (k > 0xffffffffull) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: k = %llu does not fit 32 bits", who, (unsigned long long)k);
    if (ldb < k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ldb = %llu is less than k = %llu", who, (unsigned long long)ldb,
                    (unsigned long long)k);
    if (ldx < k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ldx = %llu is less than k = %llu", who, (unsigned long long)ldx,
                    (unsigned long long)k);
    SPAL_TRY(check_dtype<T>(who, a->elem_size));
    return krylov_check_operands<T, H>(who, a, m, tol);
}

template <typename T, typename H>
int block_dev(const char *who, H *a, int method, H *m, uint64_t k, const T *b, uint64_t ldb, T *x, uint64_t ldx,
              double tol, uint64_t maxit, void *stream, spal_krylov_info *info) {
    SPAL_TRY((block_check<T, H>(who, a, method, m, k, b, ldb, x, ldx, tol, info)));
    if (x == b) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x_dev == b_dev (B is read in every test of the residual)", who);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return block_run<T, H>(who, a, method, m, (uint32_t)k, b, ldb, x, ldx, tol, maxit, (hipStream_t)stream, info);
}

// host blocks: B and X0 go up packed (leading dimension k), the k columns of X come back into the caller's rows
template <typename T, typename H>
int block_host(const char *who, H *a, int method, H *m, uint64_t k, const T *b, uint64_t ldb, uint64_t b_rows, T *x,
               uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit, spal_krylov_info *info) {
    SPAL_TRY((block_check<T, H>(who, a, method, m, k, b, ldb, x, ldx, tol, info)));
    if (b_rows != a->nrows || x_rows != a->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: B has %llu rows and X has %llu rows but the matrix has %llu rows", who,
                    (unsigned long long)b_rows, (unsigned long long)x_rows, (unsigned long long)a->nrows);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const uint64_t n = a->nrows;
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
    SPAL_TRY((block_run<T, H>(who, a, method, m, (uint32_t)k, db.as<T>(), k, dx.as<T>(), k, tol, maxit, ps.s, info)));
    if (n) SPAL_HIP_TRY(hipMemcpy2DAsync(x, (size_t)ldx * sizeof(T), dx.p, row, row, n, hipMemcpyDeviceToHost, ps.s));
    SPAL_HIP_TRY(hipStreamSynchronize(ps.s));
    return SPAL_OK;
}

}  // namespace

int krylov_block_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status) {
    if (strcmp(key, "krylov_tile")) return 0;
    if (value != 0 && !tile_instantiated(value)) {
        *status = fail(SPAL_ERR_INVALID_ARGUMENT, "krylov_tile must be 0 (automatic) or one of 1, 2, 4, 8, 16, 32");
        return 1;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    s.krylov_tile = (int)value;
    *status = SPAL_OK;
    return 1;
}

int krylov_block_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    if (!solve) return SPAL_OK;
    std::string info;
    {
        std::lock_guard<std::mutex> lock(solve->mu);
        info = s.krylov_block_info;
    }
    return describe_append(buf, buf_len, "krylov_block", info);
}

}  // namespace spal

using namespace spal;

extern "C" {

#define SPAL_KRYLOV_BLOCK_ENTRIES(kind, sfx, T)                                                                        \
    int spal_##kind##_krylov_block_##sfx(spal_##kind##_t a, int method, spal_##kind##_t m, uint64_t k, const T *b,     \
                                         uint64_t ldb, uint64_t b_rows, T *x, uint64_t ldx, uint64_t x_rows,           \
                                         double tol, uint64_t maxit, spal_krylov_info *info) {                         \
        return block_host<T, spal_##kind>("spal_" #kind "_krylov_block", a, method, m, k, b, ldb, b_rows, x, ldx,      \
                                          x_rows, tol, maxit, info);                                                   \
    }                                                                                                                  \
    int spal_##kind##_krylov_block_dev_##sfx(spal_##kind##_t a, int method, spal_##kind##_t m, uint64_t k,             \
                                             const T *b_dev, uint64_t ldb, T *x_dev, uint64_t ldx, double tol,         \
                                             uint64_t maxit, void *stream, spal_krylov_info *info) {                   \
        return block_dev<T, spal_##kind>("spal_" #kind "_krylov_block", a, method, m, k, b_dev, ldb, x_dev, ldx, tol,  \
                                         maxit, stream, info);                                                         \
    }
SPAL_KRYLOV_BLOCK_ENTRIES(csr, f64, double)
SPAL_KRYLOV_BLOCK_ENTRIES(csr, f32, float)
SPAL_KRYLOV_BLOCK_ENTRIES(csc, f64, double)
SPAL_KRYLOV_BLOCK_ENTRIES(csc, f32, float)
#undef SPAL_KRYLOV_BLOCK_ENTRIES

}  // extern "C"
