// gmres_kernels.hpp -- what spal_gmres.hip (GMRES on one right-hand side: DESIGN 3.17) and spal_gmres_block.hip (the
// same text on every column of a block: DESIGN 3.23) share on the device: the scalar block of one iteration -- a head
// the host polls, then h, c, cs, sn, g, y and the Hessenberg matrix -- and the three scalar steps on it, each run by one
// workgroup.  The vector call has one such block, the block call one per column; the arithmetic of a column is the
// vector call's because it is this text.  (Not installed.)
#pragma once

#include "krylov_kernels.hpp"

#pragma clang fp contract(off)

namespace spal {

constexpr uint64_t kMaxRestart = 256; // one Hessenberg column element per thread of the scalar workgroup

// What the host polls.
template <typename T>
struct GHead {
    T rr, bb, thr, beta, hn, est;
    unsigned long long it, cycles;
    unsigned done, reason, cyc_end, jj;
};

// The scalar block by its parts (all device pointers into one allocation).
template <typename T>
struct GBlock {
    GHead<T> *s;
    T *h, *c;      // restart + 1 each: the current column, the second pass's corrections
    T *cs, *sn;    // restart each
    T *g;          // restart + 1
    T *y;          // restart
    T *H;          // (restart + 1) x restart, column k at H + k * (restart + 1)
    unsigned m;    // restart
};
inline __host__ __device__ size_t block_elems(uint64_t m) { return (size_t)(3 * (m + 1) + 3 * m + (m + 1) * m); }

// the parts of a block whose head is `s` and whose block_elems(restart) elements begin at `p`
template <typename T>
inline __host__ __device__ GBlock<T> block_parts(GHead<T> *s, T *p, uint64_t restart) {
    GBlock<T> B;
    B.s = s;
    B.m = (unsigned)restart;
    B.h = p;
    p += restart + 1;
    B.c = p;
    p += restart + 1;
    B.cs = p;
    p += restart;
    B.sn = p;
    p += restart;
    B.g = p;
    p += restart + 1;
    B.y = p;
    p += restart;
    B.H = p;
    return B;
}

template <typename T>
__device__ __forceinline__ bool at_step(const GHead<T> *s, unsigned j) {
    return s->done == 0 && s->cyc_end == 0 && s->jj == j;   // written by an earlier launch
}
template <typename T>
__device__ __forceinline__ bool at_cycle_end(const GHead<T> *s) { return s->done == 0 && s->cyc_end != 0; }

// One thread, at the head of a cycle: rr, bb, thr;  the test on the true residual;  beta, g[0], jj = 0
template <typename T>
__device__ __forceinline__ void cycle_start_scalars(GBlock<T> B, T rr, T bb, T tol2, uint64_t maxit) {
    GHead<T> *s = B.s;
    s->bb = bb;
    s->thr = tol2 * bb;
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
    } else {
        const T beta = sqrt(rr);
        s->beta = beta;
        B.g[0] = beta;
        s->jj = 0;
        s->cyc_end = 0;
        s->cycles += 1;
    }
}

// The whole workgroup, after dot(w, w) of step j:  h += c;  hn;  the rotations;  g;  est;  the end of the cycle;  jj, it
template <typename T>
__device__ __forceinline__ void step_scalars_body(GBlock<T> B, unsigned j, T ww, uint64_t maxit) {
    GHead<T> *s = B.s;
    const unsigned t = threadIdx.x;
    T *h = B.h;
    if (t <= j) h[t] = h[t] + B.c[t];
    __syncthreads();
    if (t == 0) {
        const T hn = sqrt(ww);
        s->hn = hn;
        s->it += 1;
        for (unsigned k = 0; k < j; ++k) {
            const T tmp = (B.cs[k] * h[k]) + (B.sn[k] * h[k + 1]);
            h[k + 1] = (B.cs[k] * h[k + 1]) - (B.sn[k] * h[k]);
            h[k] = tmp;
        }
        const T d = sqrt((h[j] * h[j]) + (hn * hn));
        const T cs = h[j] / d, sn = hn / d;
        B.cs[j] = cs;
        B.sn[j] = sn;
        h[j] = d;
        const T gj = B.g[j];
        const T g1 = -(sn * gj);
        B.g[j + 1] = g1;
        B.g[j] = cs * gj;
        const T est = g1 * g1;
        s->est = est;
        s->jj = j + 1;
        if (!isfinite(est)) {
            s->rr = est;
            s->done = 1;
            s->reason = 2;
        } else if (est <= s->thr || s->it == maxit || j + 1 == B.m) {
            s->cyc_end = 1;
        }
    }
    __syncthreads();
    if (t <= j) B.H[(uint64_t)j * (B.m + 1) + t] = h[t];
}

// The whole workgroup, at the end of a cycle; `y` holds kThreads elements of LDS.
// column form: thread l owns g[l];  for k = jj - 1 .. 0:  y[k] = g[k] / H[k, k];  g[l] -= H[l, k] * y[k] for l < k
template <typename T>
__device__ __forceinline__ void back_substitute_body(GBlock<T> B, T *y) {
    const unsigned jj = B.s->jj, t = threadIdx.x, ld = B.m + 1;
    T gl = t < jj ? B.g[t] : T(0);
    for (unsigned k = jj; k-- > 0;) {
        if (t == k) y[k] = gl / B.H[(uint64_t)k * ld + k];
        __syncthreads();
        if (t < k) gl = gl - (B.H[(uint64_t)k * ld + t] * y[k]);
    }
    if (t < jj) B.y[t] = y[t];
}

// ---- the fused Gram-Schmidt step, shared by spal_gmres.hip and spal_eigsh.hip (thick-restart Lanczos) ----
constexpr int kDotBatch = 8;          // basis vectors per batch of mdot / mupdate / combine ("dot_batch")

// The basis and one of its passes.
template <typename T>
struct Basis {
    const T *v;        // v_k at v + k * stride
    uint64_t stride, n, tiles;
};

// thread t's four elements of a tile; the padding is +0.0
template <typename T>
__device__ __forceinline__ void load4(const T *p, uint64_t i, uint64_t n, T (&out)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = i + (uint64_t)k * kThreads < n ? p[i + (uint64_t)k * kThreads] : T(0);
}

// tile_sum for kDotBatch independent sums at once: the same operand order for each, three barriers for all
template <typename T>
__device__ __forceinline__ void tile_sum_batch(T (&a)[kDotBatch], T (*lds)[kThreads]) {
    const unsigned t = threadIdx.x;
#pragma unroll
    for (int b = 0; b < kDotBatch; ++b) lds[b][t] = a[b];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int b = 0; b < kDotBatch; ++b) {
            a[b] = lds[b][t] + lds[b][t + 128];      // h = 128
            if (t >= 64) lds[b][t] = a[b];
        }
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int b = 0; b < kDotBatch; ++b) {
            a[b] = a[b] + lds[b][t + 64];            // h = 64
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) a[b] = a[b] + __shfl_down(a[b], h, 64);
        }
    }
    __syncthreads();
}

// dst = src / beta (step < 0: v_0, in place) or dst = src / hn (v_{step + 1} = w / hn, after step's scalars)
template <typename T>
__global__ __launch_bounds__(kThreads) void scale(const GHead<T> *s, const T *src, T *dst, int step, uint64_t n) {
    if (s->done != 0) return;
    if (step >= 0 && s->jj != (unsigned)step + 1) return;
    const T d = step < 0 ? s->beta : s->hn;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) dst[i] = src[i] / d;
}

// ---- the orthogonalisation ------------------------------------------------------------------------------------------
// part[k * pe + tile] = the tile's sum of v_k . w for k = 0 .. j
template <typename T>
__global__ __launch_bounds__(kThreads) void mdot(const GHead<T> *s, Basis<T> V, unsigned j, const T *w, T *part, uint64_t pe) {
    __shared__ T lds[kDotBatch][kThreads];
    if (!at_step(s, j)) return;
    const unsigned nk = j + 1;
    for (uint64_t tile = blockIdx.x; tile < V.tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T wv[4];
        load4<T>(w, i, V.n, wv);
        for (unsigned k0 = 0; k0 < nk; k0 += kDotBatch) {
            T v[kDotBatch][4];
#pragma unroll
            for (int b = 0; b < kDotBatch; ++b) {   // every load of the batch before the first product
                if (k0 + b < nk) {
                    load4<T>(V.v + (uint64_t)(k0 + b) * V.stride, i, V.n, v[b]);
                } else {
                    v[b][0] = v[b][1] = v[b][2] = v[b][3] = T(0);
                }
            }
            T a[kDotBatch];
#pragma unroll
            for (int b = 0; b < kDotBatch; ++b)
                a[b] = ((v[b][0] * wv[0]) + (v[b][2] * wv[2])) + ((v[b][1] * wv[1]) + (v[b][3] * wv[3]));   // h = 512, 256
            tile_sum_batch<T>(a, lds);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int b = 0; b < kDotBatch; ++b)
                    if (k0 + b < nk) part[(uint64_t)(k0 + b) * pe + tile] = a[b];
            }
        }
    }
}

// workgroup k: dst[k] = the upper levels of dot k
template <typename T>
__global__ __launch_bounds__(kThreads) void mfinish(const GHead<T> *s, unsigned j, T *part, uint64_t pe, uint64_t c1, T *dst) {
    __shared__ T lds[kThreads];
    if (!at_step(s, j)) return;
    const T d = upper_levels<T>(part + (uint64_t)blockIdx.x * pe, c1, lds);
    if (threadIdx.x == 0) dst[blockIdx.x] = d;
}

// w[i] = (..((w[i] - (f[0] * v_0[i])) - (f[1] * v_1[i])) ..) - (f[j] * v_j[i]);  DOT: part0 = the first level of dot(w, w)
template <typename T, bool DOT>
__global__ __launch_bounds__(kThreads) void mupdate(const GHead<T> *s, Basis<T> V, unsigned j, const T *f, T *w, T *part0) {
    __shared__ T lds[kThreads];
    if (!at_step(s, j)) return;
    const unsigned nk = j + 1;
    for (uint64_t tile = blockIdx.x; tile < V.tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T wv[4];
        load4<T>(w, i, V.n, wv);
        for (unsigned k0 = 0; k0 < nk; k0 += kDotBatch) {
            T v[kDotBatch][4];
#pragma unroll
            for (int b = 0; b < kDotBatch; ++b)
                if (k0 + b < nk) load4<T>(V.v + (uint64_t)(k0 + b) * V.stride, i, V.n, v[b]);
#pragma unroll
            for (int b = 0; b < kDotBatch; ++b) {
                if (k0 + b < nk) {
                    const T fk = f[k0 + b];
#pragma unroll
                    for (int k = 0; k < 4; ++k) wv[k] = wv[k] - (fk * v[b][k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + (uint64_t)k * kThreads < V.n) w[i + (uint64_t)k * kThreads] = wv[k];
        if (DOT) {
            T p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = i + (uint64_t)k * kThreads < V.n ? wv[k] * wv[k] : T(0);
            const T sum = tile_sum<T>(p[0], p[1], p[2], p[3], lds);
            if (threadIdx.x == 0) part0[tile] = sum;
        }
    }
}

}  // namespace spal
