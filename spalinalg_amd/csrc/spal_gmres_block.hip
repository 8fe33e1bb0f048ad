// spal_gmres_block.hip -- restarted GMRES for a block of k right-hand sides: k INDEPENDENT iterations in
// lockstep on shared launches.  B and X are n x k, dense and row-major (element (i, j) at [i * ld + j], ld >= k).
// Column j follows the GMRES text of include/spal.h exactly as spal_*_gmres_* does -- its own bb, thr, it, jj, h, c, cs,
// sn, g, H, y, stop test and reason -- with A v the value spal_*_spmm_* defines and M^-1 v column j of the two
// spal_*_trsm_* (or spal_*_trsm_sweep_*) calls.  It is NOT block GMRES: no Krylov space is shared, so every column keeps
// its sequential text and its bits.
//
// CYCLES ARE COMMON, STEPS ARE PER COLUMN.  All running columns begin a cycle together.  Inside it a column takes inner
// steps until its own text ends its cycle (est <= thr, it == maxit, jj == restart); then it idles -- no kernel writes
// anything of it -- until every running column has ended its cycle; then the back substitution, the update of x and the
// head of the next cycle run for all of them.  A column that has stopped is frozen for the rest of the call.  The idle
// and frozen columns still ride through every product and solve, into work blocks nobody reads: compaction is out of scope.
//
// THE FREEZE PREDICATE IS PER COLUMN, HENCE PER LANE: !done && !cyc_end && jj == j (at_step, gmres_kernels.hpp).  A
// column that runs has jj == j, the host's step, because cycles begin together; a masked lane skips its loads and stores
// and still reaches every barrier and shuffle with +0.0.
//
// GEOMETRY is spal_krylov_block.hip's: a workgroup of 256 covers 1024 rows x KT columns; thread t is column t % KT and
// row group g = t / KT of G = 256 / KT and owns rows g, g + G, ... of the tile, L = 4 KT of them.  The header's tree
// over the tile's 1024 rows splits as there: strides >= G are thread-local, taken in KT chunks {o, o + KT, o + 2 KT,
// o + 3 KT} of 4 local rows whose sums meet in bit-reversed order as a binary counter carries (Carry); strides < G are
// column_tree.  `mdot_block` forms the first level of dot(v_i, w), i = 0 .. j, for every column: the basis blocks are
// taken kBlockDotBatch at a time, and for a batch the w tile is read ONCE; per chunk every load of the batch is issued
// before the first product, and one LDS stage [kBlockDotBatch][256] and the shuffles serve the whole batch.  Every
// single dot keeps reduce()'s operand order.  `mupdate_block` is elementwise: it keeps a chunk of w in registers over
// all the batches, so w is read and written once per pass.
//
// THE SCALARS: k heads (GHead), contiguous so that one copy polls them, then per column block_elems(restart) elements
// holding h, c, cs, sn, g, y, H.  cycle_start_block, step_scalars_block and back_substitute_block run one workgroup per
// column on that column's record; the arithmetic is the vector call's text (gmres_kernels.hpp).
// ORDER BETWEEN LAUNCHES IS STREAM ORDER ALONE: no flags waited on, no spins, no float atomics, no grid syncs.  The
// driver holds no handle lock across a product or a solve; every block, the dot scratch and the scalars are taken and
// the stream's sweep scratch is grown before the first step, so no iteration allocates.
//
// (The host layer of a block call -- KRYLOV_BY_TILE, KRYLOV_LAUNCH, prec_block, check_block_geometry, column_tile_of,
// grow_sweep_scratch, with_host_block -- and the frame -- SolveFrame over the k heads, store_info -- are
// krylov_kernels.hpp's, shared with spal_krylov_block.hip; the cycle loop in gmres_block_run is this file's.)
#include "gmres_kernels.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr int kBlockDotBatch = 4;   // basis blocks per batch of mdot_block / mupdate_block / combine_block ("dot_batch")

// The k scalar records.
template <typename T>
struct GCols {
    GHead<T> *heads;   // k of them, contiguous
    T *elems;          // column j's block_elems(m) elements at elems + j * be
    uint64_t be;
    unsigned m;        // restart
    uint32_t k;
};
template <typename T>
__device__ __forceinline__ GBlock<T> column_of(const GCols<T> &S, uint64_t col) {
    return block_parts<T>(S.heads + col, S.elems + col * S.be, S.m);
}

// The basis: block i at v + i * stride, packed (element (row, col) at [row * k + col]).
template <typename T>
struct BasisB {
    const T *v;
    uint64_t stride, n, tiles;
    uint32_t k;
};

template <int KT>
struct Geo {
    static constexpr int G = kThreads / KT;     // row groups of a workgroup
    static constexpr int L = (int)kTile / G;    // rows of a thread: 4 KT
    static constexpr int C = L / 4;             // chunks {o, o + C, o + 2C, o + 3C} of them: KT
    static constexpr int LOGC = KT == 32 ? 5 : KT == 16 ? 4 : KT == 8 ? 3 : KT == 4 ? 2 : KT == 2 ? 1 : 0;
    // chunk idx in the order the carries want: idx's LOGC bits reversed
    static __device__ __forceinline__ int offset(int idx) { return LOGC ? (int)(__brev((unsigned)idx) >> (32 - (LOGC ? LOGC : 1))) : 0; }
};

// The chunk sums of a thread, halved as they arrive: a sum waits in c[b] for the one that completes a pair of stride
// C >> (b + 1); the partner came earlier and holds the lower rows.  After chunk C - 1 push() returns the thread's sum.
template <typename T, int LOGC>
struct Carry {
    T c[LOGC + 1];
    __device__ __forceinline__ T push(T w, int idx) {
        bool carry = true;   // uniform: idx is the same in every thread
#pragma unroll
        for (int bit = 0; bit < LOGC; ++bit) {
            if (carry && (idx >> bit & 1)) {
                w = c[bit] + w;
            } else if (carry) {
                c[bit] = w;
                carry = false;
            }
        }
        return w;
    }
};

// column_tree for kBlockDotBatch independent sums at once: the same operand order for each, three barriers for all
template <typename T, int KT>
__device__ __forceinline__ void column_tree_batch(T (&a)[kBlockDotBatch], T (*lds)[kThreads]) {
    const unsigned t = threadIdx.x;
#pragma unroll
    for (int b = 0; b < kBlockDotBatch; ++b) lds[b][t] = a[b];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int b = 0; b < kBlockDotBatch; ++b) {
            a[b] = lds[b][t] + lds[b][t + 128];      // h = 128 / KT
            if (t >= 64) lds[b][t] = a[b];
        }
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int b = 0; b < kBlockDotBatch; ++b) {
            a[b] = a[b] + lds[b][t + 64];            // h = 64 / KT
#pragma unroll
            for (int h = 32; h >= KT; h >>= 1) a[b] = a[b] + __shfl_down(a[b], h, 64);
        }
    }
    __syncthreads();
}

// the rows of chunk idx of thread (grp, .) in a tile: row[u] = tile * 1024 + grp + (o + u * C) * G
template <int KT>
__device__ __forceinline__ void chunk_rows(uint64_t tile, unsigned grp, int idx, uint64_t (&row)[4]) {
    const int o = Geo<KT>::offset(idx);
#pragma unroll
    for (int u = 0; u < 4; ++u) row[u] = tile * kTile + grp + (uint64_t)(o + u * Geo<KT>::C) * Geo<KT>::G;
}

// ---- the head of a cycle --------------------------------------------------------------------------------------------
// r = b - q;  first levels of rr = dot(r, r) and bb = dot(b, b) per column:  part0 / part1[column * pe + tile]
template <typename T, int KT, int MODE>
__global__ __launch_bounds__(kThreads) void residual_block(GCols<T> S, Mat<const T> b, const T *q, T *r, T *part0, T *part1,
                                                           uint64_t n, uint64_t tiles, uint64_t pe) {
    __shared__ T lds[2][kThreads];
    const unsigned j = threadIdx.x % KT, grp = threadIdx.x / KT;
    for (uint64_t ct = blockIdx.y; ct * KT < S.k; ct += gridDim.y) {
        const uint64_t col = ct * KT + j;
        const bool live = col < S.k && S.heads[col].done == 0;
        for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            Carry<T, Geo<KT>::LOGC> c0, c1;
            T a0 = T(0), a1 = T(0);
#pragma unroll 1
            for (int idx = 0; idx < Geo<KT>::C; ++idx) {
                uint64_t row[4];
                chunk_rows<KT>(tile, grp, idx, row);
                T bv[4], qv[4], p[4], pb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool in = live && row[u] < n;
                    bv[u] = in ? b.p[row[u] * b.ld + col] : T(0);
                    qv[u] = in ? q[row[u] * S.k + col] : T(0);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    p[u] = pb[u] = T(0);
                    if (live && row[u] < n) {
                        const T rv = bv[u] - qv[u];
                        r[row[u] * S.k + col] = rv;
                        p[u] = rv * rv;
                        pb[u] = bv[u] * bv[u];
                    }
                }
                a0 = c0.push((p[0] + p[2]) + (p[1] + p[3]), idx);
                a1 = c1.push((pb[0] + pb[2]) + (pb[1] + pb[3]), idx);
            }
            const T s0 = column_tree<T, KT>(a0, lds[0]);
            const T s1 = column_tree<T, KT>(a1, lds[1]);
            if (grp == 0 && live) {
                part0[col * pe + tile] = s0;
                part1[col * pe + tile] = s1;
            }
        }
    }
}

// workgroup per column: rr, bb, thr;  the test on the true residual;  beta, g[0], jj = 0
template <typename T>
__global__ __launch_bounds__(kThreads) void cycle_start_block(GCols<T> S, T *part0, T *part1, uint64_t pe, uint64_t c1, T tol2,
                                                              uint64_t maxit) {
    __shared__ T lds[kThreads];
    for (uint64_t col = blockIdx.x; col < S.k; col += gridDim.x) {
        const bool done = S.heads[col].done != 0;   // uniform over the workgroup: one column
        __syncthreads();                            // every thread has read it before thread 0 may write it
        if (done) continue;
        const T rr = upper_levels<T>(part0 + col * pe, c1, lds);
        const T bb = upper_levels<T>(part1 + col * pe, c1, lds);
        if (threadIdx.x == 0) cycle_start_scalars<T>(column_of(S, col), rr, bb, tol2, maxit);
    }
}

// dst = src / beta (step < 0: v_0, in place) or dst = src / hn (v_{step + 1} = w / hn, after step's scalars); packed blocks
template <typename T, int KT, int MODE>
__global__ __launch_bounds__(kThreads) void scale_block(GCols<T> S, const T *src, T *dst, int step, uint64_t n, uint64_t tiles) {
    const unsigned j = threadIdx.x % KT, grp = threadIdx.x / KT;
    for (uint64_t ct = blockIdx.y; ct * KT < S.k; ct += gridDim.y) {
        const uint64_t col = ct * KT + j;
        if (col >= S.k) continue;
        const GHead<T> *s = S.heads + col;
        if (s->done != 0) continue;
        if (step >= 0 && s->jj != (unsigned)step + 1) continue;
        const T d = step < 0 ? s->beta : s->hn;
        for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const uint64_t end = std::min<uint64_t>(n, (tile + 1) * kTile);
            for (uint64_t row = tile * kTile + grp; row < end; row += Geo<KT>::G) dst[row * S.k + col] = src[row * S.k + col] / d;
        }
    }
}

// ---- the orthogonalisation ------------------------------------------------------------------------------------------
// part[(i * k + column) * pe + tile] = the tile's sum of v_i . w of the column, for i = 0 .. j
template <typename T, int KT, int MODE>
__global__ __launch_bounds__(kThreads) void mdot_block(GCols<T> S, BasisB<T> V, unsigned step, const T *w, T *part, uint64_t pe) {
    constexpr int DB = kBlockDotBatch;
    __shared__ T lds[DB][kThreads];
    const unsigned j = threadIdx.x % KT, grp = threadIdx.x / KT;
    const unsigned nk = step + 1;
    for (uint64_t ct = blockIdx.y; ct * KT < V.k; ct += gridDim.y) {
        const uint64_t col = ct * KT + j;
        const bool live = col < V.k && at_step(S.heads + col, step);
        for (uint64_t tile = blockIdx.x; tile < V.tiles; tile += gridDim.x) {
            for (unsigned k0 = 0; k0 < nk; k0 += DB) {
                Carry<T, Geo<KT>::LOGC> cr[DB];
                T a[DB];
#pragma unroll 1
                for (int idx = 0; idx < Geo<KT>::C; ++idx) {
                    uint64_t row[4];
                    chunk_rows<KT>(tile, grp, idx, row);
                    T wv[4], v[DB][4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) wv[u] = live && row[u] < V.n ? w[row[u] * V.k + col] : T(0);
#pragma unroll
                    for (int b = 0; b < DB; ++b) {   // every load of the batch before the first product
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            v[b][u] = live && k0 + b < nk && row[u] < V.n ? V.v[(uint64_t)(k0 + b) * V.stride + row[u] * V.k + col] : T(0);
                    }
#pragma unroll
                    for (int b = 0; b < DB; ++b)
                        a[b] = cr[b].push(((v[b][0] * wv[0]) + (v[b][2] * wv[2])) + ((v[b][1] * wv[1]) + (v[b][3] * wv[3])), idx);
                }
                column_tree_batch<T, KT>(a, lds);
                if (grp == 0 && live) {
#pragma unroll
                    for (int b = 0; b < DB; ++b)
                        if (k0 + b < nk) part[((uint64_t)(k0 + b) * V.k + col) * pe + tile] = a[b];
                }
            }
        }
    }
}

// workgroup (i, column): h[i] (second == 0) or c[i] of the column = the upper levels of its dot i
template <typename T>
__global__ __launch_bounds__(kThreads) void mfinish_block(GCols<T> S, unsigned step, T *part, uint64_t pe, uint64_t c1, int second) {
    __shared__ T lds[kThreads];
    for (uint64_t col = blockIdx.y; col < S.k; col += gridDim.y) {
        if (!at_step(S.heads + col, step)) continue;   // uniform: one column, written by an earlier launch
        const T d = upper_levels<T>(part + ((uint64_t)blockIdx.x * S.k + col) * pe, c1, lds);
        if (threadIdx.x == 0) {
            const GBlock<T> B = column_of(S, col);
            (second ? B.c : B.h)[blockIdx.x] = d;
        }
    }
}

// w[e] = (..((w[e] - (f[0] * v_0[e])) - (f[1] * v_1[e])) ..) - (f[j] * v_j[e]) with f the column's h (second == 0) or c;
// MODE 1: part0[column * pe + tile] = the first level of the column's dot(w, w)
template <typename T, int KT, int MODE>
__global__ __launch_bounds__(kThreads) void mupdate_block(GCols<T> S, BasisB<T> V, unsigned step, int second, T *w, T *part0, uint64_t pe) {
    constexpr int DB = kBlockDotBatch;
    __shared__ T lds[kThreads];
    const unsigned j = threadIdx.x % KT, grp = threadIdx.x / KT;
    const unsigned nk = step + 1;
    for (uint64_t ct = blockIdx.y; ct * KT < V.k; ct += gridDim.y) {
        const uint64_t col = ct * KT + j;
        const bool live = col < V.k && at_step(S.heads + col, step);
        const T *f = nullptr;
        if (live) {
            const GBlock<T> B = column_of(S, col);
            f = second ? B.c : B.h;
        }
        for (uint64_t tile = blockIdx.x; tile < V.tiles; tile += gridDim.x) {
            Carry<T, Geo<KT>::LOGC> cr;
            T a = T(0);
#pragma unroll 1
            for (int idx = 0; idx < Geo<KT>::C; ++idx) {
                uint64_t row[4];
                chunk_rows<KT>(tile, grp, idx, row);
                T wv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) wv[u] = live && row[u] < V.n ? w[row[u] * V.k + col] : T(0);
                for (unsigned k0 = 0; k0 < nk; k0 += DB) {
                    T v[DB][4], fk[DB];
#pragma unroll
                    for (int b = 0; b < DB; ++b) {
                        fk[b] = live && k0 + b < nk ? f[k0 + b] : T(0);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            v[b][u] = live && k0 + b < nk && row[u] < V.n ? V.v[(uint64_t)(k0 + b) * V.stride + row[u] * V.k + col] : T(0);
                    }
#pragma unroll
                    for (int b = 0; b < DB; ++b) {
                        if (k0 + b < nk) {
#pragma unroll
                            for (int u = 0; u < 4; ++u) wv[u] = wv[u] - (fk[b] * v[b][u]);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (live && row[u] < V.n) w[row[u] * V.k + col] = wv[u];
                if (MODE) {
                    T p[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) p[u] = live && row[u] < V.n ? wv[u] * wv[u] : T(0);
                    a = cr.push((p[0] + p[2]) + (p[1] + p[3]), idx);
                }
            }
            if (MODE) {
                const T s = column_tree<T, KT>(a, lds);
                if (grp == 0 && live) part0[col * pe + tile] = s;
            }
        }
    }
}

// workgroup per column: ww = dot(w, w);  h += c;  hn;  the rotations;  g;  est;  the end of the cycle;  jj, it
template <typename T>
__global__ __launch_bounds__(kThreads) void step_scalars_block(GCols<T> S, unsigned step, T *part0, uint64_t pe, uint64_t c1,
                                                               uint64_t maxit) {
    __shared__ T lds[kThreads];
    for (uint64_t col = blockIdx.x; col < S.k; col += gridDim.x) {
        const bool here = at_step(S.heads + col, step);   // uniform over the workgroup: one column
        __syncthreads();                                  // every thread has read it before thread 0 may write it
        if (!here) continue;
        const T ww = upper_levels<T>(part0 + col * pe, c1, lds);
        step_scalars_body<T>(column_of(S, col), step, ww, maxit);
    }
}

// ---- the end of a cycle ---------------------------------------------------------------------------------------------
// workgroup per column: y of the column, with its own jj
template <typename T>
__global__ __launch_bounds__(kThreads) void back_substitute_block(GCols<T> S) {
    __shared__ T y[kThreads];
    for (uint64_t col = blockIdx.x; col < S.k; col += gridDim.x) {
        __syncthreads();   // y is free again
        if (!at_cycle_end(S.heads + col)) continue;
        back_substitute_body<T>(column_of(S, col), y);
    }
}

// u[e] = (..((y[0] * v_0[e]) + (y[1] * v_1[e])) ..) + (y[jj - 1] * v_{jj-1}[e]) per column, with the column's own jj;
// MODE 1: out[e] = out[e] + u[e], else out = u.  No barrier: the loop over the batches may diverge.
template <typename T, int KT, int MODE>
__global__ __launch_bounds__(kThreads) void combine_block(GCols<T> S, BasisB<T> V, Mat<T> out) {
    constexpr int DB = kBlockDotBatch;
    const unsigned j = threadIdx.x % KT, grp = threadIdx.x / KT;
    for (uint64_t ct = blockIdx.y; ct * KT < V.k; ct += gridDim.y) {
        const uint64_t col = ct * KT + j;
        if (col >= V.k || !at_cycle_end(S.heads + col)) continue;
        const unsigned nk = S.heads[col].jj;
        const T *y = column_of(S, col).y;
        for (uint64_t tile = blockIdx.x; tile < V.tiles; tile += gridDim.x) {
#pragma unroll 1
            for (int idx = 0; idx < Geo<KT>::C; ++idx) {
                uint64_t row[4];
                chunk_rows<KT>(tile, grp, idx, row);
                T u[4] = {T(0), T(0), T(0), T(0)};
                for (unsigned k0 = 0; k0 < nk; k0 += DB) {
                    T v[DB][4], yk[DB];
#pragma unroll
                    for (int b = 0; b < DB; ++b) {
                        yk[b] = k0 + b < nk ? y[k0 + b] : T(0);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            v[b][e] = k0 + b < nk && row[e] < V.n ? V.v[(uint64_t)(k0 + b) * V.stride + row[e] * V.k + col] : T(0);
                    }
#pragma unroll
                    for (int b = 0; b < DB; ++b) {
                        if (k0 + b < nk) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) u[e] = k0 + b == 0 ? yk[b] * v[b][e] : u[e] + (yk[b] * v[b][e]);
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (row[e] < V.n) {
                        T *o = out.p + row[e] * out.ld + col;
                        *o = MODE ? *o + u[e] : u[e];
                    }
                }
            }
        }
    }
}

// x[e] = x[e] + t[e]  (t = M^-1 u, packed)
template <typename T, int KT, int MODE>
__global__ __launch_bounds__(kThreads) void add_to_x_block(GCols<T> S, const T *t, Mat<T> x, uint64_t n, uint64_t tiles) {
    const unsigned j = threadIdx.x % KT, grp = threadIdx.x / KT;
    for (uint64_t ct = blockIdx.y; ct * KT < S.k; ct += gridDim.y) {
        const uint64_t col = ct * KT + j;
        if (col >= S.k || !at_cycle_end(S.heads + col)) continue;
        for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const uint64_t end = std::min<uint64_t>(n, (tile + 1) * kTile);
            for (uint64_t row = tile * kTile + grp; row < end; row += Geo<KT>::G)
                x.p[row * x.ld + col] = x.p[row * x.ld + col] + t[row * S.k + col];
        }
    }
}

// ---- the driver -----------------------------------------------------------------------------------------------------
struct Record {
    uint64_t restart = 0, k = 0, iterations_min = 0, iterations_max = 0, cycles = 0, steps = 0, converged = 0, polls = 0,
             basis_bytes = 0;
    int preconditioned = 0, tile = 0;
    int64_t precond_sweeps = -1, check_every = 0;
    double solve_ms = 0.0;
};
std::string info_json(const Record &r) {
    char buf[640];
    snprintf(buf, sizeof buf,
             "{\"restart\": %llu, \"k\": %llu, \"preconditioned\": %d, \"precond_sweeps\": %lld, \"tile\": %d, "
             "\"iterations_min\": %llu, \"iterations_max\": %llu, \"cycles\": %llu, \"steps\": %llu, \"converged\": %llu, "
             "\"check_every\": %lld, \"polls\": %llu, \"dot_batch\": %d, \"basis_bytes\": %llu, \"solve_ms\": %.4f}",
             (unsigned long long)r.restart, (unsigned long long)r.k, r.preconditioned, (long long)r.precond_sweeps, r.tile,
             (unsigned long long)r.iterations_min, (unsigned long long)r.iterations_max, (unsigned long long)r.cycles,
             (unsigned long long)r.steps, (unsigned long long)r.converged, (long long)r.check_every,
             (unsigned long long)r.polls, kBlockDotBatch, (unsigned long long)r.basis_bytes, r.solve_ms);
    return buf;
}

// (KRYLOV_BY_TILE names the column tile KT_; the third template argument is mupdate_block's DOT, combine_block's ADD, 0 in
// the others)
template <typename T, typename H>
struct Run {
    const char *fn;
    H *a, *m;
    hipStream_t st;
    uint64_t n = 0, maxit = 0, c1 = 0, pe = 0, tiles = 0;
    uint32_t k = 0;
    int tile = 1;
    dim3 tgrid, cgrid;   // the tile geometry; one workgroup per column
    T tol2 = T(0);
    int64_t sweeps = -1;
    GCols<T> S;
    BasisB<T> V;
    T *basis = nullptr, *w = nullptr, *q = nullptr, *z = nullptr, *u = nullptr, *part = nullptr;
    Mat<const T> B;
    Mat<T> X;

    T *v_at(uint64_t i) const { return basis + i * V.stride; }
    int mul(const T *v, uint64_t ld, T *out) { return mul_block(a, k, v, ld, out, k, st); }
    // out = M^-1 v (out != v, both packed)
    int prec(const T *v, T *out) { return prec_block<T, H>(m, sweeps, k, v, out, st); }

    // q = A x;  r, rr, bb;  the test;  beta, v_0
    int head() {
        SPAL_TRY(mul(X.p, X.ld, q));
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((residual_block<T, KT_, 0>), tgrid, S, B, q, v_at(0), part, part + pe * k, n, tiles, pe));
        KRYLOV_LAUNCH((cycle_start_block<T>), cgrid, S, part, part + pe * k, pe, c1, tol2, maxit);
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((scale_block<T, KT_, 0>), tgrid, S, v_at(0), v_at(0), -1, n, tiles));
        return SPAL_OK;
    }
    // step j of a cycle, for the columns that are there
    int inner(unsigned j) {
        const T *zj = v_at(j);
        if (m) {
            SPAL_TRY(prec(v_at(j), z));
            zj = z;
        }
        SPAL_TRY(mul(zj, k, w));
        const dim3 fgrid(j + 1, std::min<unsigned>(k, kFinishGrid));
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((mdot_block<T, KT_, 0>), tgrid, S, V, j, w, part, pe));
        KRYLOV_LAUNCH((mfinish_block<T>), fgrid, S, j, part, pe, c1, 0);
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((mupdate_block<T, KT_, 0>), tgrid, S, V, j, 0, w, part, pe));
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((mdot_block<T, KT_, 0>), tgrid, S, V, j, w, part, pe));
        KRYLOV_LAUNCH((mfinish_block<T>), fgrid, S, j, part, pe, c1, 1);
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((mupdate_block<T, KT_, 1>), tgrid, S, V, j, 1, w, part, pe));
        KRYLOV_LAUNCH((step_scalars_block<T>), cgrid, S, j, part, pe, c1, maxit);
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((scale_block<T, KT_, 0>), tgrid, S, w, v_at(j + 1), (int)j, n, tiles));
        return SPAL_OK;
    }
    // y;  u = V y;  x += M^-1 u, for the columns whose cycle has ended
    int cycle_end() {
        KRYLOV_LAUNCH((back_substitute_block<T>), cgrid, S);
        if (!m) {
            KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((combine_block<T, KT_, 1>), tgrid, S, V, X));
            return SPAL_OK;
        }
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((combine_block<T, KT_, 0>), tgrid, S, V, (Mat<T>{u, (uint64_t)k})));
        SPAL_TRY(prec(u, z));
        KRYLOV_BY_TILE(tile, KRYLOV_LAUNCH((add_to_x_block<T, KT_, 0>), tgrid, S, z, X, n, tiles));
        return SPAL_OK;
    }
};

// What a poll found in the k heads.
struct Polled {
    uint64_t stopped = 0, running = 0;   // done;  not done and the cycle not ended
    uint64_t min_it = 0;                 // the fewest iterations of a column that has not stopped
    bool early = false;                  // a column that has not stopped ended its cycle before `restart` steps or is at maxit
};
template <typename T>
Polled poll_heads(const GHead<T> *h, uint32_t k, uint64_t restart, uint64_t maxit) {
    Polled p;
    p.min_it = maxit;
    for (uint32_t j = 0; j < k; ++j) {
        if (h[j].done) {
            ++p.stopped;
            continue;
        }
        if (!h[j].cyc_end) ++p.running;
        p.min_it = std::min<uint64_t>(p.min_it, h[j].it);
        if (h[j].jj < restart || h[j].it == maxit) p.early = true;
    }
    return p;
}

template <typename T, typename H>
int gmres_block_run(const char *fn, H *a, H *m, uint32_t k, const T *b, uint64_t ldb, T *x, uint64_t ldx, uint64_t restart,
                    double tol, uint64_t maxit, hipStream_t st, spal_krylov_info *info) {
    const uint64_t n = a->nrows;
    const int64_t check_every = krylov_check_every_of(a, m != nullptr);
    const int tile = column_tile_of(a, k);
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    int64_t sweeps = -1;
    SPAL_TRY(krylov_prepare(fn, a, m, st, &sweeps));

    // the basis and the work blocks in one allocation, the scratch of `restart` dots per column, the scalar records
    const uint64_t nblk = (restart + 1) + 2 + (m ? 2 : 0);
    const uint64_t pe = scratch_elems(n);
    const uint64_t be = block_elems(restart);
    size_t basis_bytes = 0, part_bytes = 0, sweep_bytes = 0;
    if (n > (std::numeric_limits<uint64_t>::max() - 63) / k)
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for blocks of %llu x %u", fn, (unsigned long long)n, k);
    const uint64_t stride = (n * k + 63) & ~(uint64_t)63;   // every block on a 256-byte boundary at least
    if (!bytes_of(stride, nblk, sizeof(T), 1, &basis_bytes) || !bytes_of(pe, k, std::max<uint64_t>(restart, 2), sizeof(T), &part_bytes) ||
        !bytes_of(stride, 2, sizeof(T), 1, &sweep_bytes))
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for %llu blocks of %llu x %u", fn, (unsigned long long)nblk,
                    (unsigned long long)n, k);
    DevBuf blocks, parts, scal;
    SolveFrame<GHead<T>> F;
    {
        const hipError_t e = blocks.alloc(basis_bytes);
        if (e == hipErrorOutOfMemory)
            return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no memory for the basis: %llu blocks of %llu x %u (%llu bytes)", fn,
                        (unsigned long long)nblk, (unsigned long long)n, k, (unsigned long long)basis_bytes);
        SPAL_HIP_TRY(e);
    }
    SPAL_HIP_TRY(parts.alloc(part_bytes));
    const size_t head_bytes = (size_t)k * sizeof(GHead<T>);
    const size_t scal_bytes = head_bytes + (size_t)k * be * sizeof(T);
    SPAL_HIP_TRY(scal.alloc(scal_bytes));
    SPAL_TRY(F.create(st, k));
    SPAL_TRY(grow_sweep_scratch(fn, st, m, sweeps, n, sweep_bytes));

    Run<T, H> R;
    R.fn = fn;
    R.a = a;
    R.m = m;
    R.st = st;
    R.n = n;
    R.maxit = maxit;
    R.c1 = R.tiles = tiles_of(n);
    R.pe = pe;
    R.k = k;
    R.tile = tile;
    R.tgrid = dim3((unsigned)std::min<uint64_t>(R.tiles, kBlockMaxGrid), std::min<unsigned>(grid_of(k, (unsigned)tile), kColumnGrid));
    R.cgrid = dim3(std::min<unsigned>(k, kFinishGrid));
    R.tol2 = (T)(tol * tol);
    R.sweeps = sweeps;
    R.B = Mat<const T>{b, ldb};
    R.X = Mat<T>{x, ldx};
    R.part = parts.as<T>();
    R.basis = blocks.as<T>();
    R.V.v = R.basis;
    R.V.stride = stride;
    R.V.n = n;
    R.V.tiles = R.tiles;
    R.V.k = k;
    uint64_t next = restart + 1;
    R.w = R.v_at(next++);
    R.q = R.v_at(next++);
    if (m) {
        R.z = R.v_at(next++);
        R.u = R.v_at(next++);
    }
    R.S.heads = scal.as<GHead<T>>();
    R.S.elems = reinterpret_cast<T *>(reinterpret_cast<char *>(scal.p) + head_bytes);
    R.S.be = be;
    R.S.m = (unsigned)restart;
    R.S.k = k;

    const GHead<T> *h = F.h;
    uint64_t steps = 0;
    Polled P;
    auto poll = [&]() -> int {   // the k heads to pinned memory
        SPAL_TRY(F.poll());
        P = poll_heads<T>(h, k, restart, maxit);
        return SPAL_OK;
    };

    SPAL_TRY(F.begin(scal.p, scal_bytes));
    SPAL_TRY(R.head());
    if (maxit == 0) SPAL_TRY(poll());   // the test after r0 has decided every column
    // P.min_it: no column that runs has fewer iterations (0 before the first poll), so after maxit - min_it steps of a
    // cycle, and after `restart` at the latest, every running column has ended its cycle
    while (maxit != 0 && P.stopped < k) {
        const uint64_t limit = std::min<uint64_t>(restart, P.min_it < maxit ? maxit - P.min_it : restart);
        uint64_t j = 0, since = 0;
        bool ended = false;   // every column that has not stopped has ended its cycle
        while (!ended && P.stopped < k) {
            SPAL_TRY(R.inner((unsigned)j));
            ++j;
            ++steps;
            ++since;
            if (since == (uint64_t)check_every || j == limit) {
                SPAL_TRY(poll());
                since = 0;
                ended = P.running == 0;
                if (j == limit && !ended && P.stopped < k)
                    return fail(SPAL_ERR_HIP, "%s: %llu of %u columns did not end a cycle of %llu iterations", fn,
                                (unsigned long long)P.running, k, (unsigned long long)limit);
            }
        }
        if (P.stopped == k) break;
        const bool early = P.early;
        SPAL_TRY(R.cycle_end());
        SPAL_TRY(R.head());
        if (early) SPAL_TRY(poll());   // est <= thr or maxit in some column: the test at the head stops it, or very likely does
    }
    float ms = 0.f;
    SPAL_TRY(F.end(&ms));
    if (P.stopped < k)
        return fail(SPAL_ERR_HIP, "%s: %llu of %u columns did not stop after %llu iterations", fn,
                    (unsigned long long)(k - P.stopped), k, (unsigned long long)maxit);
    Record rec;
    rec.iterations_min = h[0].it;
    for (uint32_t j = 0; j < k; ++j) {
        F.fill(info + j, j, ms);
        rec.iterations_min = std::min<uint64_t>(rec.iterations_min, h[j].it);
        rec.iterations_max = std::max<uint64_t>(rec.iterations_max, h[j].it);
        rec.cycles = std::max<uint64_t>(rec.cycles, h[j].cycles);
        rec.converged += h[j].reason == 0;
    }
    rec.restart = restart;
    rec.k = k;
    rec.preconditioned = m ? 1 : 0;
    rec.precond_sweeps = sweeps;
    rec.tile = tile;
    rec.steps = steps;
    rec.check_every = check_every;
    rec.polls = F.polls;
    rec.basis_bytes = basis_bytes;
    rec.solve_ms = (double)ms;
    store_info(a, &OpState::gmres_block_info, info_json(rec));
    return SPAL_OK;
}

// Every refusal that needs no device; `who` begins the messages ("spal_csr_gmres_block").  The block's geometry and
// restart come first: they need nothing of the handles.
template <typename T, typename H>
int gmres_block_check(const char *who, H *a, H *m, uint64_t k, const T *b, uint64_t ldb, T *x, uint64_t ldx, uint64_t restart,
                      double tol, spal_krylov_info *info) {
    if (!a || !b || !x || !info) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    if (restart == 0 || restart > kMaxRestart)
        return fail(SPAL_ERR_INVALID_ARGUMENT,
                    "%s: restart = %llu must be 1 .. %llu (one Hessenberg column element per thread of the scalar workgroup)", who,
                    (unsigned long long)restart, (unsigned long long)kMaxRestart);
    SPAL_TRY(check_block_geometry(who, k, ldb, ldx));
    SPAL_TRY(check_dtype<T>(who, a->elem_size));
    return krylov_check_operands<T, H>(who, a, m, tol);
}

template <typename T, typename H>
int gmres_block_dev(const char *who, H *a, H *m, uint64_t k, const T *b, uint64_t ldb, T *x, uint64_t ldx, uint64_t restart,
                    double tol, uint64_t maxit, void *stream, spal_krylov_info *info) {
    SPAL_TRY((gmres_block_check<T, H>(who, a, m, k, b, ldb, x, ldx, restart, tol, info)));
    if (x == b) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x_dev == b_dev (B is read in every test of the residual)", who);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return gmres_block_run<T, H>(who, a, m, (uint32_t)k, b, ldb, x, ldx, restart, tol, maxit, (hipStream_t)stream, info);
}

template <typename T, typename H>
int gmres_block_host(const char *who, H *a, H *m, uint64_t k, const T *b, uint64_t ldb, uint64_t b_rows, T *x, uint64_t ldx,
                     uint64_t x_rows, uint64_t restart, double tol, uint64_t maxit, spal_krylov_info *info) {
    SPAL_TRY((gmres_block_check<T, H>(who, a, m, k, b, ldb, x, ldx, restart, tol, info)));
    return with_host_block(who, a, k, b, ldb, b_rows, x, ldx, x_rows, [&](const T *b_dev, T *x_dev, hipStream_t st) {
        return gmres_block_run<T, H>(who, a, m, (uint32_t)k, b_dev, k, x_dev, k, restart, tol, maxit, st, info);
    });
}

}  // namespace

int gmres_block_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    return info_describe_append(buf, buf_len, s, solve, "gmres_block", &OpState::gmres_block_info);
}

}  // namespace spal

using namespace spal;

extern "C" {

#define SPAL_GMRES_BLOCK_ENTRIES(kind, sfx, T)                                                                         \
    int spal_##kind##_gmres_block_##sfx(spal_##kind##_t a, spal_##kind##_t m, uint64_t k, const T *b, uint64_t ldb,    \
                                        uint64_t b_rows, T *x, uint64_t ldx, uint64_t x_rows, uint64_t restart,        \
                                        double tol, uint64_t maxit, spal_krylov_info *info) {                          \
        return gmres_block_host<T, spal_##kind>("spal_" #kind "_gmres_block", a, m, k, b, ldb, b_rows, x, ldx, x_rows, \
                                                restart, tol, maxit, info);                                            \
    }                                                                                                                  \
    int spal_##kind##_gmres_block_dev_##sfx(spal_##kind##_t a, spal_##kind##_t m, uint64_t k, const T *b_dev,          \
                                            uint64_t ldb, T *x_dev, uint64_t ldx, uint64_t restart, double tol,        \
                                            uint64_t maxit, void *stream, spal_krylov_info *info) {                    \
        return gmres_block_dev<T, spal_##kind>("spal_" #kind "_gmres_block", a, m, k, b_dev, ldb, x_dev, ldx, restart, \
                                               tol, maxit, stream, info);                                              \
    }
SPAL_GMRES_BLOCK_ENTRIES(csr, f64, double)
SPAL_GMRES_BLOCK_ENTRIES(csr, f32, float)
SPAL_GMRES_BLOCK_ENTRIES(csc, f64, double)
SPAL_GMRES_BLOCK_ENTRIES(csc, f32, float)
#undef SPAL_GMRES_BLOCK_ENTRIES

}  // extern "C"
