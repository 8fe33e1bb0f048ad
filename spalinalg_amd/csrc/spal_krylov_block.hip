// spal_krylov_block.hip -- CG, BiCGStab and MINRES for a block of k right-hand sides: k INDEPENDENT iterations run
// in lockstep on shared launches.  B and X are n x k, dense and row-major (element (i, j) at [i * ld + j], ld >= k): the
// layout of SpMM and of the block triangular solves.  Column j follows the loops written out in include/spal.h exactly
// as spal_*_krylov_* does -- its own bb, thr, scalars, it, stop test and reason -- with A v the value spal_*_spmm_*
// defines and M^-1 v column j of the two spal_*_trsm_* (or spal_*_trsm_sweep_*) calls.  One pass over the matrix and one
// walk of the factor's launches serve all k columns; that is the whole point.  It is NOT a block-Krylov method: no
// search space is shared, so every column keeps its sequential text and its bits.
//
// (tile_sum, upper_levels, the scalar block Scal, the ten fused updates and the scalar steps are in krylov_kernels.hpp,
// shared with spal_krylov.hip: the arithmetic of a column is the vector call's, by construction.  So is the sequence of
// launches: the two loops are krylov_loops.hpp's, instantiated here on a `Run` whose operands are blocks.  Mat,
// column_tree, the column tiles and their dispatch (KRYLOV_BY_TILE), the routes to SpMM and trsm, M^-1 on a block, the
// refusals of k / ldb / ldx, the sweep scratch and the staging of host blocks are in krylov_kernels.hpp too, shared with
// spal_gmres_block.hip; the frame of a call -- KRYLOV_LAUNCH, SolveFrame, store_info -- with all four drivers.)
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
    Mat<T> z;           // the third written operand (V_MR_WX)
    T sg;               // MINRES: T(shift)
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
        Coef<T> coef = {T(0), T(0), T(0), T(0), T(0), true};
        if (live) {
            const Scal<T> *s = g.s + col;   // written by an earlier launch
            live = op_live<T, OP>(s);
            coef = op_coef<T, OP>(s, g.sg);
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
                    T av[U], bv[U], cv[U], dv[U], xv[U], yv[U], zv[U];
                    uint64_t i[U];
                    bool in[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        i[u] = row0 + (uint64_t)(o + (m0 + u) * C) * G;
                        in[u] = live && i[u] < g.n;
                        av[u] = bv[u] = cv[u] = dv[u] = xv[u] = yv[u] = zv[u] = T(0);
                        if (in[u]) {
                            av[u] = g.a.p[i[u] * g.a.ld + col];
                            if (Reads<OP>::b) bv[u] = g.b.p[i[u] * g.b.ld + col];
                            if (Reads<OP>::c) cv[u] = g.c.p[i[u] * g.c.ld + col];
                            if (Reads<OP>::d) dv[u] = g.d.p[i[u] * g.d.ld + col];
                            if (Reads<OP>::x) xv[u] = g.x.p[i[u] * g.x.ld + col];
                            if (Reads<OP>::y) yv[u] = g.y.p[i[u] * g.y.ld + col];
                            if (Reads<OP>::z) zv[u] = g.z.p[i[u] * g.z.ld + col];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        p[m0 + u] = T(0);   // the padding, and a masked column: +0.0, and it is added
                        q[m0 + u] = T(0);
                        if (in[u])
                            vec_value<T, OP>(av[u], bv[u], cv[u], dv[u], xv[u], yv[u], zv[u], coef, p[m0 + u], q[m0 + u]);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (in[u]) {
                            if (Writes<OP>::x) g.x.p[i[u] * g.x.ld + col] = xv[u];
                            if (Writes<OP>::y) g.y.p[i[u] * g.y.ld + col] = yv[u];
                            if (Writes<OP>::z) g.z.p[i[u] * g.z.ld + col] = zv[u];
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
        // the update the stop left behind (BiCGStab's half step, MINRES's w and x), if there was one, has been applied
        if ((OP == F_OMEGA || OP == F_MR_ALFA) && threadIdx.x == 0) s->half = 0;
        if (done) continue;
        const T d0 = upper_levels<T>(g.part0 + col * g.pe, g.c1, lds);
        T d1 = T(0);
        if (OP == F_INIT || OP == F_OMEGA || OP == F_MR_INIT) d1 = upper_levels<T>(g.part1 + col * g.pe, g.c1, lds);
        if (threadIdx.x == 0) scalar_step<T, OP>(s, d0, d1, g.tol2, g.maxit, g.unpreconditioned);
    }
}

// ---- host side of the launches (the tiles and their dispatch, the routes and bytes_of are in krylov_kernels.hpp) -------
template <typename T, int OP>
int launch_vec_block(const char *fn, const BlockVecArgs<T> &g, int tile, hipStream_t st) {
    const uint64_t tiles = tiles_of(g.n);
    const unsigned gx = (unsigned)std::min<uint64_t>(tiles, kBlockMaxGrid);
    const unsigned gy = std::min<unsigned>(grid_of(g.k, (unsigned)tile), kColumnGrid);
    KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((vec_block<T, OP, KT_>), dim3(gx, gy), g, tiles));
    return SPAL_OK;
}

template <typename T, int OP>
int launch_finish_block(const char *fn, const BlockFinArgs<T> &g, hipStream_t st) {
    KRYLOV_LAUNCH((finish_block<T, OP>), std::min<unsigned>(g.k, kFinishGrid), g);
    return SPAL_OK;
}

constexpr int kMinres = 2;   // the method of the spal_*_minres_block_* entry points in here; spal_*_krylov_block_* refuse it

struct Record {
    int method = 0, preconditioned = 0, tile = 0;
    int64_t precond_sweeps = -1, check_every = 0;
    uint64_t k = 0, iterations_min = 0, iterations_max = 0, converged = 0, polls = 0;
    double solve_ms = 0.0, shift = 0.0;
};
std::string info_json(const Record &r) {
    char buf[576], shift[64] = "";
    if (r.method == kMinres) snprintf(shift, sizeof shift, ", \"shift\": %.17g", r.shift);
    snprintf(buf, sizeof buf,
             "{\"method\": \"%s\", \"k\": %llu, \"preconditioned\": %d, \"precond_sweeps\": %lld, \"tile\": %d, "
             "\"iterations_min\": %llu, \"iterations_max\": %llu, \"converged\": %llu, \"check_every\": %lld, "
             "\"polls\": %llu, \"solve_ms\": %.4f%s}",
             r.method == SPAL_KRYLOV_CG ? "cg" : r.method == kMinres ? "minres" : "bicgstab", (unsigned long long)r.k,
             r.preconditioned, (long long)r.precond_sweeps, r.tile, (unsigned long long)r.iterations_min,
             (unsigned long long)r.iterations_max, (unsigned long long)r.converged, (long long)r.check_every,
             (unsigned long long)r.polls, r.solve_ms, shift);   // (the objects written by CG and BiCGStab do not change)
    return buf;
}

// The driver the loops of krylov_loops.hpp run on: an operand is a block and its leading dimension; the scalar records,
// the scratch of two dots per column, and the launches by name.  A work block is packed (leading dimension k).
template <typename T, typename H>
struct Run {
    const char *fn;
    H *a, *m;
    hipStream_t st;
    uint64_t n = 0, maxit = 0, c1 = 0, pe = 0, stride = 0;
    uint32_t k = 0;
    int tile = 1;
    T tol2 = T(0), sg = T(0);   // sg: MINRES's T(shift)
    Scal<T> *s = nullptr;
    T *part0 = nullptr, *part1 = nullptr;
    int64_t sweeps = -1;   // m's option "trsv_sweeps"
    T *blocks = nullptr;   // work block i at blocks + i * stride
    Mat<const T> b;
    Mat<T> x;
    SolveFrame<Scal<T>> frame;
    uint64_t stopped = 0;   // columns the last poll found stopped

    static Mat<T> null() { return {nullptr, 0}; }
    Mat<const T> B() const { return b; }
    Mat<T> X() const { return x; }
    Mat<T> work(int i) const { return {blocks + (uint64_t)i * stride, (uint64_t)k}; }
    bool preconditioned() const { return m != nullptr; }
    int mul(Mat<T> v, Mat<T> out) { return mul_block(a, k, v.p, v.ld, out.p, out.ld, st); }
    // out = M^-1 v (out != v, both packed); without a preconditioner the loops use v itself
    // (packed: MINRES applies M^-1 to B itself, so a preconditioned MINRES call takes B with ldb == k -- block_run copies)
    template <typename A>   // A: T, or const T where the operand is B
    int prec(Mat<A> v, Mat<T> out) { return prec_block<T, H>(m, sweeps, k, (const T *)v.p, out.p, st); }
    template <int OP, typename A>   // A: T, or const T where the operand is B
    int v(Mat<A> va, Mat<T> vb, Mat<T> vc, Mat<T> vd, Mat<T> vx, Mat<T> vy, Mat<T> vz = {nullptr, 0}) {
        return launch_vec_block<T, OP>(
            fn, BlockVecArgs<T>{{va.p, va.ld}, {vb.p, vb.ld}, {vc.p, vc.ld}, {vd.p, vd.ld}, vx, vy, s, part0, part1, n, pe, k, vz, sg},
            tile, st);
    }
    template <int OP>
    int f(int unpreconditioned = 0) {
        return launch_finish_block<T, OP>(fn, BlockFinArgs<T>{s, part0, part1, c1, pe, k, tol2, maxit, unpreconditioned}, st);
    }
    int copy(Mat<T> dst, Mat<T> src) {
        SPAL_HIP_TRY(hipMemcpyAsync(dst.p, src.p, (size_t)(n * k) * sizeof(T), hipMemcpyDeviceToDevice, st));
        return SPAL_OK;
    }
    int zero(Mat<T> dst) {
        SPAL_HIP_TRY(hipMemsetAsync(dst.p, 0, (size_t)(n * k) * sizeof(T), st));
        return SPAL_OK;
    }
    int poll() {   // the k records to pinned memory; how many columns have stopped
        SPAL_TRY(frame.poll());
        stopped = 0;
        for (uint32_t j = 0; j < k; ++j) stopped += frame.h[j].done != 0;
        return SPAL_OK;
    }
    bool all_stopped() const { return stopped == k; }
    uint64_t polls() const { return frame.polls; }
};

template <typename T, typename H>
int block_run(const char *fn, H *a, int method, H *m, double shift, uint32_t k, const T *b, uint64_t ldb, T *x, uint64_t ldx,
              double tol, uint64_t maxit, hipStream_t st, spal_krylov_info *info) {
    const uint64_t n = a->nrows;
    const int64_t check_every = krylov_check_every_of(a, m != nullptr);
    const int tile = column_tile_of(a, k);
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    int64_t sweeps = -1;
    SPAL_TRY(krylov_prepare(fn, a, m, st, &sweeps));
    // work blocks, scratch, scalars: all at once, before the first iteration
    const bool cg = method == SPAL_KRYLOV_CG;
    const bool minres = method == kMinres;   // v, r1 / r2 / t, w1 / w2, and y with a preconditioner
    const int nwork = minres ? (m ? 7 : 6) : cg ? (m ? 4 : 3) : (m ? 8 : 6);
    const uint64_t pe = scratch_elems(n);
    size_t work_bytes = 0, part_bytes = 0, sweep_bytes = 0;
    if (n > (std::numeric_limits<uint64_t>::max() - 63) / k)
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for work blocks of %llu x %u", fn, (unsigned long long)n, k);
    const uint64_t stride = (n * k + 63) & ~(uint64_t)63;   // every block on a 256-byte boundary at least
    if (!bytes_of(stride, (uint64_t)nwork, sizeof(T), 1, &work_bytes) || !bytes_of(pe, k, 2, sizeof(T), &part_bytes) ||
        !bytes_of(stride, 2, sizeof(T), 1, &sweep_bytes))
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for work blocks of %llu x %u", fn, (unsigned long long)n, k);
    DevBuf blocks, parts, scal;
    SPAL_HIP_TRY(blocks.alloc(work_bytes));
    SPAL_HIP_TRY(parts.alloc(part_bytes));
    SPAL_HIP_TRY(scal.alloc((size_t)k * sizeof(Scal<T>)));

    Run<T, H> R;
    SPAL_TRY(R.frame.create(st, k));
    SPAL_TRY(grow_sweep_scratch(fn, st, m, sweeps, n, sweep_bytes));
    R.fn = fn;
    R.a = a;
    R.m = m;
    R.st = st;
    R.n = n;
    R.maxit = maxit;
    R.c1 = tiles_of(n);
    R.pe = pe;
    R.stride = stride;
    R.k = k;
    R.tile = tile;
    R.tol2 = (T)(tol * tol);
    R.sg = (T)shift;
    R.s = scal.as<Scal<T>>();
    R.part0 = parts.as<T>();
    R.part1 = parts.as<T>() + pe * k;
    R.sweeps = sweeps;
    R.blocks = blocks.as<T>();
    R.b = {b, ldb};
    R.x = {x, ldx};
    // M^-1 takes packed blocks, and MINRES applies it to B itself (bb = dot(b, M^-1 b)): a B with padding is packed once
    DevBuf packed;
    if (minres && m && ldb != k && n) {
        SPAL_HIP_TRY(packed.alloc((size_t)stride * sizeof(T)));
        SPAL_HIP_TRY(hipMemcpy2DAsync(packed.p, (size_t)k * sizeof(T), b, (size_t)ldb * sizeof(T), (size_t)k * sizeof(T), n,
                                      hipMemcpyDeviceToDevice, st));
        R.b = {(const T *)packed.p, (uint64_t)k};
    }

    SPAL_TRY(R.frame.begin(R.s, (size_t)k * sizeof(Scal<T>)));
    if (minres) {
        SPAL_TRY(minres_start(R));
        SPAL_TRY(minres_loop(R, maxit, (uint64_t)check_every));
    } else {
        SPAL_TRY(krylov_start(R));
        SPAL_TRY(cg ? cg_loop(R, maxit, (uint64_t)check_every) : bicgstab_loop(R, maxit, (uint64_t)check_every));
    }
    float ms = 0.f;
    SPAL_TRY(R.frame.end(&ms));
    if (R.stopped < k)
        return fail(SPAL_ERR_HIP, "%s: %llu of %u columns did not stop after %llu iterations", fn,
                    (unsigned long long)(k - R.stopped), k, (unsigned long long)maxit);
    Record rec;
    rec.iterations_min = R.frame.h[0].it;
    for (uint32_t j = 0; j < k; ++j) {
        R.frame.fill(info + j, j, ms);
        rec.iterations_min = std::min<uint64_t>(rec.iterations_min, info[j].iterations);
        rec.iterations_max = std::max<uint64_t>(rec.iterations_max, info[j].iterations);
        rec.converged += info[j].reason == 0;
    }
    rec.method = method;
    rec.k = k;
    rec.preconditioned = m ? 1 : 0;
    rec.precond_sweeps = sweeps;
    rec.tile = tile;
    rec.polls = R.frame.polls;
    rec.check_every = check_every;
    rec.solve_ms = (double)ms;
    rec.shift = shift;
    store_info(a, &OpState::krylov_block_info, info_json(rec));
    return SPAL_OK;
}

// Every refusal that needs no device; `who` begins the messages ("spal_csr_krylov_block").  The method and the block's
// geometry come first: they need nothing of the handles.
template <typename T, typename H>
int block_check(const char *who, H *a, int method, bool minres, H *m, double shift, uint64_t k, const T *b, uint64_t ldb,
                T *x, uint64_t ldx, double tol, spal_krylov_info *info) {
    if (!a || !b || !x || !info) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    if (!minres && method != SPAL_KRYLOV_CG && method != SPAL_KRYLOV_BICGSTAB)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: method = %d must be 0 (CG) or 1 (BiCGStab)", who, method);
    if (!std::isfinite(shift)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: shift = %g must be finite", who, shift);
    SPAL_TRY(check_block_geometry(who, k, ldb, ldx));
    SPAL_TRY(check_dtype<T>(who, a->elem_size));
    return krylov_check_operands<T, H>(who, a, m, tol);
}

template <typename T, typename H>
int block_dev(const char *who, H *a, int method, bool minres, H *m, double shift, uint64_t k, const T *b, uint64_t ldb, T *x,
              uint64_t ldx, double tol, uint64_t maxit, void *stream, spal_krylov_info *info) {
    SPAL_TRY((block_check<T, H>(who, a, method, minres, m, shift, k, b, ldb, x, ldx, tol, info)));
    if (x == b) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x_dev == b_dev (B is read in every test of the residual)", who);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return block_run<T, H>(who, a, minres ? kMinres : method, m, shift, (uint32_t)k, b, ldb, x, ldx, tol, maxit,
                           (hipStream_t)stream, info);
}

template <typename T, typename H>
int block_host(const char *who, H *a, int method, bool minres, H *m, double shift, uint64_t k, const T *b, uint64_t ldb,
               uint64_t b_rows, T *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit, spal_krylov_info *info) {
    SPAL_TRY((block_check<T, H>(who, a, method, minres, m, shift, k, b, ldb, x, ldx, tol, info)));
    return with_host_block(who, a, k, b, ldb, b_rows, x, ldx, x_rows, [&](const T *b_dev, T *x_dev, hipStream_t st) {
        return block_run<T, H>(who, a, minres ? kMinres : method, m, shift, (uint32_t)k, b_dev, k, x_dev, k, tol, maxit, st, info);
    });
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
    return info_describe_append(buf, buf_len, s, solve, "krylov_block", &OpState::krylov_block_info);
}

}  // namespace spal

using namespace spal;

extern "C" {

#define SPAL_KRYLOV_BLOCK_ENTRIES(kind, sfx, T)                                                                        \
    int spal_##kind##_krylov_block_##sfx(spal_##kind##_t a, int method, spal_##kind##_t m, uint64_t k, const T *b,     \
                                         uint64_t ldb, uint64_t b_rows, T *x, uint64_t ldx, uint64_t x_rows,           \
                                         double tol, uint64_t maxit, spal_krylov_info *info) {                         \
        return block_host<T, spal_##kind>("spal_" #kind "_krylov_block", a, method, false, m, 0.0, k, b, ldb, b_rows,  \
                                          x, ldx, x_rows, tol, maxit, info);                                           \
    }                                                                                                                  \
    int spal_##kind##_krylov_block_dev_##sfx(spal_##kind##_t a, int method, spal_##kind##_t m, uint64_t k,             \
                                             const T *b_dev, uint64_t ldb, T *x_dev, uint64_t ldx, double tol,         \
                                             uint64_t maxit, void *stream, spal_krylov_info *info) {                   \
        return block_dev<T, spal_##kind>("spal_" #kind "_krylov_block", a, method, false, m, 0.0, k, b_dev, ldb,       \
                                         x_dev, ldx, tol, maxit, stream, info);                                        \
    }                                                                                                                  \
    /* MINRES on (A - shift I) X = B: the same arguments without `method`, with one `shift` for all columns */         \
    int spal_##kind##_minres_block_##sfx(spal_##kind##_t a, spal_##kind##_t m, double shift, uint64_t k, const T *b,   \
                                         uint64_t ldb, uint64_t b_rows, T *x, uint64_t ldx, uint64_t x_rows,           \
                                         double tol, uint64_t maxit, spal_krylov_info *info) {                         \
        return block_host<T, spal_##kind>("spal_" #kind "_minres_block", a, 0, true, m, shift, k, b, ldb, b_rows, x,   \
                                          ldx, x_rows, tol, maxit, info);                                              \
    }                                                                                                                  \
    int spal_##kind##_minres_block_dev_##sfx(spal_##kind##_t a, spal_##kind##_t m, double shift, uint64_t k,           \
                                             const T *b_dev, uint64_t ldb, T *x_dev, uint64_t ldx, double tol,         \
                                             uint64_t maxit, void *stream, spal_krylov_info *info) {                   \
        return block_dev<T, spal_##kind>("spal_" #kind "_minres_block", a, 0, true, m, shift, k, b_dev, ldb, x_dev,    \
                                         ldx, tol, maxit, stream, info);                                               \
    }
SPAL_KRYLOV_BLOCK_ENTRIES(csr, f64, double)
SPAL_KRYLOV_BLOCK_ENTRIES(csr, f32, float)
SPAL_KRYLOV_BLOCK_ENTRIES(csc, f64, double)
SPAL_KRYLOV_BLOCK_ENTRIES(csc, f32, float)
#undef SPAL_KRYLOV_BLOCK_ENTRIES

}  // extern "C"
