// spal_amg.hip -- aggregation AMG on the device: the hierarchy of include/spal.h built level after level
// from the colouring's hashed priority and the COO assembly, and the multigrid cycle that preconditions CG and BiCGStab.
//
// SETUP, PER LEVEL, ORDERED BY THE STREAM ALONE (no flags, no spins, no grid sync):
//   degrees   a merge of A's row and A^T's row (both ascending; transpose_device gives A^T), prio = deg << 32 | mix32;
//   roots     by rounds, as the colouring's: state[v] = (round + 1) << 1 | root, 0 while undecided, one aligned word
//             written once.  In round r a vertex looks at its neighbours of HIGHER priority only and counts one as
//             decided only if its stamp is <= r, so a store of the same launch makes no difference whether seen or
//             not: v is a non-root as soon as one of them is a root, a root once all of them are decided non-roots.
//             The undecided are appended to the other of two lists (one atomic per wave), three counters rotate, the
//             host enqueues a batch of rounds (8 doubling to 512) and reads the poll block;
//   join      a non-root's root = its neighbouring root of highest priority;
//   numbering scan_exclusive over the root flags;  members: a stable counting sort of the rows by aggregate -- what
//             the transpose does to a matrix with one entry per row whose column is the row's aggregate;
//   coarse    the triplets (agg[i], agg[j], v) in storage order into coo_assemble, from device arrays;
//   w         omega / the stored diagonal, found by bisection in the ascending row; a row without one is counted.
//
// THE CYCLE.  Five SpMV-shaped kernels: smooth0, smooth (fused: reads x once, writes x' to the ping-pong vector),
// residual, restrict (a thread per aggregate walks its members in order), prolong (gather and add).  A thread owns a
// row, but a row -- or an aggregate -- of more than kLong entries is summed by its whole wave: 64 products per step are
// formed in parallel, the additions run over them in the text's order (ordered_sum).  So hubs of thousands of entries
// cost a wave, not a workgroup, and every level returns the text's bits whatever the row lengths are.
//
// THE TAIL.  Below a few thousand rows a level costs launch latency, and with gamma = 2 level l is visited 2^l times.
// All levels from the first with n_l <= "amg_tail_rows" down to the coarsest run as ONE launch of ONE workgroup of 1024
// per visit of that level (k_tail): the recursion unrolled into a loop with a visit bit per level, the same device
// functions as the wide kernels (the same bits), __syncthreads() between the steps -- a workgroup reads what it stored
// a step earlier, which the barrier orders at workgroup scope, as in trsv_chain and upper_levels.
#define SPAL_OPS_SCAN
#include "coo_internal.hpp"

#include <cmath>
#include <memory>

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr int kThreads = 256, kTailThreads = 1024;
constexpr uint32_t kFirstBatch = 8, kMaxBatch = 512;
constexpr uint32_t kLong = 32;             // entries of a row beyond which its wave forms the products together
constexpr uint32_t kMaxLevels = 32;
constexpr int64_t kTailRowsDefault = 1024, kTailRowsMax = 4096;   // measured: profiles/amg/tail_sweep_*.json

// ---- the device's view of one level ----------------------------------------------------------------------------------
template <typename T>
struct Lvl {
    const uint32_t *ptr, *ind;
    const T *val, *w;
    const uint32_t *agg, *mptr, *mem;   // of a level that has a coarser one: aggregate of a row; members by aggregate
    T *xa, *xb, *r;                     // the smoother's ping-pong vectors, the residual
    T *b, *e;                           // levels > 0: the restricted right-hand side and the cycle's result
    uint32_t n, nagg;
};
struct Cyc {
    uint32_t nu, coarse_sweeps, gamma, levels;
};

// term(s) + term(s + 1) + ... + term(e - 1) added left to right onto +0.0.  Called by all 64 lanes of a wave together,
// each with its own range (an idle lane: s == e); ranges longer than kLong are taken one after the other by the whole
// wave, 64 terms per step formed in parallel and added in order.
template <typename T, typename F>
__device__ __forceinline__ T ordered_sum(uint32_t s, uint32_t e, F term) {
    const uint32_t lane = threadIdx.x & 63, len = e - s;
    T acc = T(0);
    if (len <= kLong)
        for (uint32_t q = s; q < e; ++q) acc = acc + term(q);
    unsigned long long mask = __ballot(len > kLong);
    while (mask) {
        const int l = __ffsll(mask) - 1;
        mask &= mask - 1;
        const uint32_t s_l = __shfl(s, l, 64), e_l = __shfl(e, l, 64);
        T a = T(0);
        for (uint32_t p = s_l; p < e_l; p += 64) {
            const uint32_t q = p + lane;
            const T t = q < e_l ? term(q) : T(0);
            const uint32_t cnt = min(64u, e_l - p);
            for (uint32_t k = 0; k < cnt; ++k) a = a + __shfl(t, (int)k, 64);
        }
        if ((int)lane == l) acc = a;
    }
    return acc;
}

// rowsum(A_l, x, i) of the text; i >= n: an idle lane
template <typename T>
__device__ __forceinline__ T rowsum(const Lvl<T> &L, const T *x, uint64_t i) {
    uint32_t s = 0, e = 0;
    if (i < L.n) {
        s = L.ptr[i];
        e = L.ptr[i + 1];
    }
    const uint32_t *ind = L.ind;
    const T *val = L.val;
    return ordered_sum<T>(s, e, [=](uint32_t q) { return val[q] * x[ind[q]]; });
}

// The five steps on row / aggregate i.  Nothing is __restrict__: the tail kernel reads what it wrote a step earlier.
template <typename T>
__device__ __forceinline__ void step_smooth0(const Lvl<T> &L, const T *b, T *x, uint64_t i) {
    if (i < L.n) x[i] = L.w[i] * b[i];
}
template <typename T>
__device__ __forceinline__ void step_smooth(const Lvl<T> &L, const T *b, const T *x, T *xo, uint64_t i) {
    const T acc = rowsum<T>(L, x, i);
    if (i < L.n) xo[i] = x[i] + (L.w[i] * (b[i] - acc));
}
template <typename T>
__device__ __forceinline__ void step_residual(const Lvl<T> &L, const T *b, const T *x, T *r, uint64_t i) {
    const T acc = rowsum<T>(L, x, i);
    if (i < L.n) r[i] = b[i] - acc;
}
template <typename T>
__device__ __forceinline__ void step_restrict(const Lvl<T> &L, const T *r, T *bc, uint64_t I) {
    uint32_t s = 0, e = 0;
    if (I < L.nagg) {
        s = L.mptr[I];
        e = L.mptr[I + 1];
    }
    const uint32_t *mem = L.mem;
    const T acc = ordered_sum<T>(s, e, [=](uint32_t q) { return r[mem[q]]; });
    if (I < L.nagg) bc[I] = acc;
}
template <typename T>
__device__ __forceinline__ void step_prolong(const Lvl<T> &L, T *x, const T *e, T alpha, uint64_t i) {
    if (i < L.n) x[i] = x[i] + (alpha * e[L.agg[i]]);
}

// ---- the wide kernels: a thread per row --------------------------------------------------------------------------------
enum Step { S_SMOOTH0, S_SMOOTH, S_RESIDUAL, S_RESTRICT, S_PROLONG };

template <typename T, int STEP>
__global__ __launch_bounds__(kThreads) void k_step(Lvl<T> L, const T *b, const T *x, T *out, T alpha) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (STEP == S_SMOOTH0) step_smooth0<T>(L, b, out, i);
    else if (STEP == S_SMOOTH) step_smooth<T>(L, b, x, out, i);
    else if (STEP == S_RESIDUAL) step_residual<T>(L, b, x, out, i);
    else if (STEP == S_RESTRICT) step_restrict<T>(L, x, out, i);     // x: the residual, out: the coarse right-hand side
    else step_prolong<T>(L, out, x, alpha, i);                       // x: the coarse result, out: this level's x
}

// ---- the tail: cycle(l0, b0) -> out0 by one workgroup -----------------------------------------------------------------
template <typename T, int STEP>
__device__ __forceinline__ void tail_step(const Lvl<T> &L, const T *b, const T *x, T *out, T alpha) {
    const uint32_t rows = STEP == S_RESTRICT ? L.nagg : L.n;
    for (uint32_t base = 0; base < rows; base += kTailThreads) {   // uniform trips: every wave stays whole
        const uint64_t i = base + threadIdx.x;
        if (STEP == S_SMOOTH0) step_smooth0<T>(L, b, out, i);
        else if (STEP == S_SMOOTH) step_smooth<T>(L, b, x, out, i);
        else if (STEP == S_RESIDUAL) step_residual<T>(L, b, x, out, i);
        else if (STEP == S_RESTRICT) step_restrict<T>(L, x, out, i);
        else step_prolong<T>(L, out, x, alpha, i);
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kTailThreads) void k_tail(const Lvl<T> *lv, uint32_t l0, Cyc c, T alpha, const T *b0, T *out0) {
    uint32_t in_xb = 0, visited = 0;   // a bit per level: its x is in xb; its first coarse correction has been added
    uint32_t l = l0;
    bool down = true;
    for (;;) {
        if (down) {
            const Lvl<T> L = lv[l];
            const T *b = l == l0 ? b0 : L.b;
            T *out = l == l0 ? out0 : L.e;
            const bool coarsest = l + 1 == c.levels;
            const uint32_t s = coarsest ? c.coarse_sweeps : c.nu;
            T *x = coarsest && s == 1 ? out : L.xa;
            tail_step<T, S_SMOOTH0>(L, b, nullptr, x, alpha);
            for (uint32_t k = 1; k < s; ++k) {
                T *xo = coarsest && k + 1 == s ? out : (x == L.xa ? L.xb : L.xa);
                tail_step<T, S_SMOOTH>(L, b, x, xo, alpha);
                x = xo;
            }
            if (coarsest) {
                down = false;
                continue;
            }
            in_xb = x == L.xb ? in_xb | 1u << l : in_xb & ~(1u << l);
            visited &= ~(1u << l);
            tail_step<T, S_RESIDUAL>(L, b, x, L.r, alpha);
            tail_step<T, S_RESTRICT>(L, nullptr, L.r, lv[l + 1].b, alpha);
            ++l;
        } else {   // level l has returned: its result is in its e
            if (l == l0) return;
            const T *e = lv[l].e;
            --l;
            const Lvl<T> L = lv[l];
            const T *b = l == l0 ? b0 : L.b;
            T *out = l == l0 ? out0 : L.e;
            T *x = (in_xb >> l & 1u) ? L.xb : L.xa;
            tail_step<T, S_PROLONG>(L, nullptr, e, x, alpha);
            if (c.gamma == 2 && !(visited >> l & 1u)) {
                visited |= 1u << l;
                tail_step<T, S_RESIDUAL>(L, b, x, L.r, alpha);
                tail_step<T, S_RESTRICT>(L, nullptr, L.r, lv[l + 1].b, alpha);
                ++l;
                down = true;
            } else {
                for (uint32_t k = 0; k < c.nu; ++k) {
                    T *xo = k + 1 == c.nu ? out : (x == L.xa ? L.xb : L.xa);
                    tail_step<T, S_SMOOTH>(L, b, x, xo, alpha);
                    x = xo;
                }
            }
        }
    }
}

// ---- setup kernels -----------------------------------------------------------------------------------------------------
struct Graph {
    const uint32_t *ptr, *ind;     // the level's rows ...
    const uint32_t *tptr, *tind;   // ... and its transpose's
};

// prio[i] = min(deg(i), 2^31 - 1) << 32 | mix32(i + seed): both rows ascend, a neighbour in both counts once
__global__ __launch_bounds__(kThreads) void k_prio(Graph g, uint32_t n, uint32_t seed, unsigned long long *prio) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    uint32_t p = g.ptr[i], t = g.tptr[i];
    const uint32_t p1 = g.ptr[i + 1], t1 = g.tptr[i + 1];
    uint64_t deg = 0;
    while (p < p1 || t < t1) {
        const uint32_t a = p < p1 ? g.ind[p] : 0xffffffffu, b = t < t1 ? g.tind[t] : 0xffffffffu;
        const uint32_t j = a < b ? a : b;
        if (p < p1 && a == j) ++p;
        if (t < t1 && b == j) ++t;
        if (j != i) ++deg;
    }
    if (deg > 0x7fffffffull) deg = 0x7fffffffull;
    prio[i] = deg << 32 | colour_mix32(i + seed);
}

struct Poll {
    uint32_t count[3];   // vertices undecided at the start of round r: count[r % 3]
    uint32_t rounds;     // 1 + the last round that decided a vertex
};

__device__ __forceinline__ uint32_t state_load(const uint32_t *state, uint32_t u) {
    return __atomic_load_n(state + u, __ATOMIC_RELAXED);
}

// One pass over the higher-priority neighbours of v in ind[p0, p1): *root when one of them was a root before round r,
// *pending when one of them was not decided before round r.
__device__ __forceinline__ void scan_higher(const uint32_t *__restrict__ ind, uint32_t p0, uint32_t p1, uint32_t v,
                                            unsigned long long pv, const unsigned long long *__restrict__ prio,
                                            const uint32_t *state, uint32_t r, bool *root, bool *pending) {
    for (uint32_t p = p0; p < p1 && !*root; ++p) {
        const uint32_t u = ind[p];
        if (u == v || prio[u] < pv) continue;
        const uint32_t s = state_load(state, u), stamp = s >> 1;
        if (stamp == 0 || stamp > r) *pending = true;   // undecided, or decided by this very launch
        else if (s & 1u) *root = true;
    }
}

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void k_round(Graph g, const unsigned long long *__restrict__ prio, uint32_t n, uint32_t r,
                                                    uint32_t *state, const uint32_t *__restrict__ list_in,
                                                    uint32_t *__restrict__ list_out, Poll *poll) {
    const uint32_t count = FIRST ? n : poll->count[r % 3];
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k == 0) poll->count[(r + 2) % 3] = 0;   // round r + 1 adds to it; round r - 1 read it, nobody touches it now
    bool left = false;
    uint32_t v = 0;
    if (k < count) {
        v = FIRST ? (uint32_t)k : list_in[k];
        const unsigned long long pv = prio[v];
        bool beside_root = false, pending = false;
        scan_higher(g.ind, g.ptr[v], g.ptr[v + 1], v, pv, prio, state, r, &beside_root, &pending);
        scan_higher(g.tind, g.tptr[v], g.tptr[v + 1], v, pv, prio, state, r, &beside_root, &pending);
        if (beside_root || !pending) {   // bit 0: v is a root
            __atomic_store_n(state + v, (r + 1) << 1 | (beside_root ? 0u : 1u), __ATOMIC_RELAXED);
            atomicMax(&poll->rounds, r + 1);
        } else {
            left = true;
        }
    }
    const unsigned long long m = __ballot(left);   // the vertices left over, appended in any order: one atomic per wave
    if (m) {
        const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll(m) - 1;
        uint32_t at = 0;
        if (lane == leader) at = atomicAdd(&poll->count[(r + 1) % 3], (uint32_t)__popcll(m));
        at = __shfl(at, (int)leader, 64);
        if (left) list_out[at + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = v;
    }
}

// rootof[v] and the root flags (flag[n] = 0 closes the scan)
__global__ __launch_bounds__(kThreads) void k_join(Graph g, const unsigned long long *__restrict__ prio, uint32_t n,
                                                   const uint32_t *__restrict__ state, uint32_t *__restrict__ rootof,
                                                   uint32_t *__restrict__ flag) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i64 > n) return;
    if (i64 == n) {
        flag[n] = 0;
        return;
    }
    const uint32_t v = (uint32_t)i64;
    const bool is_root = state[v] & 1u;
    flag[v] = is_root ? 1u : 0u;
    uint32_t best = v;
    if (!is_root) {
        unsigned long long bp = 0;
        bool any = false;
        for (int side = 0; side < 2; ++side) {
            const uint32_t *ptr = side ? g.tptr : g.ptr, *ind = side ? g.tind : g.ind;
            for (uint32_t p = ptr[v]; p < ptr[v + 1]; ++p) {
                const uint32_t u = ind[p];
                if (u == v || !(state[u] & 1u)) continue;
                if (!any || prio[u] > bp) {
                    any = true;
                    bp = prio[u];
                    best = u;
                }
            }
        }
    }
    rootof[v] = best;
}

__global__ __launch_bounds__(kThreads) void k_number(const uint32_t *__restrict__ rootof, const uint32_t *__restrict__ num,
                                                     uint32_t n, uint32_t *__restrict__ agg, uint32_t *__restrict__ iota) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    iota[i] = (uint32_t)i;
    if (i < n) agg[i] = num[rootof[i]];
}

// the relabelled triplets, a thread per entry in storage order
__global__ __launch_bounds__(kThreads) void k_triplets(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ ind,
                                                       const uint32_t *__restrict__ agg, uint32_t n, uint32_t nnz,
                                                       uint32_t *__restrict__ rows, uint32_t *__restrict__ cols) {
    const uint64_t q64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q64 >= nnz) return;
    const uint32_t q = (uint32_t)q64;
    uint32_t lo = 0, hi = n;   // the last row i with ptr[i] <= q
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= q) lo = mid;
        else hi = mid;
    }
    rows[q] = agg[lo];
    cols[q] = agg[ind[q]];
}

// w[i] = omega / the stored (i, i); *missing = the first row without one (n: none)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_weights(const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ ind,
                                                      const T *__restrict__ val, uint32_t n, T omega, T *__restrict__ w,
                                                      uint32_t *missing) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    uint32_t lo = ptr[i], hi = ptr[i + 1];
    const uint32_t end = hi;
    while (lo < hi) {   // the first entry with column >= i
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ind[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    if (lo < end && ind[lo] == i) {
        w[i] = omega / val[lo];
    } else {
        w[i] = T(0);
        atomicMin(missing, i);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct Level {
    uint32_t n = 0, nnz = 0, nagg = 0;
    uint64_t rounds = 0;
    double setup_ms = 0.0;
    DevBuf ptr, ind, val, w, agg, mptr, mem, vecs;
};

}  // namespace
}  // namespace spal

struct spal_amg {
    int device = 0, elem_size = 8;
    spal_amg_params params{};
    std::vector<std::unique_ptr<spal::Level>> levels;
    const char *stopped_by = "";
    spal::DevBuf d_lv;                  // the levels' device views, for the tail kernel
    std::vector<char> h_lv;             // ... and on the host (Lvl<T> x levels)
    int64_t tail_rows = spal::kTailRowsDefault;
    uint32_t tail_from = 0;             // the first level that runs in the tail; levels.size(): none
    std::mutex mu;                      // serialises applies (the work vectors are the handle's) and guards what follows
    hipEvent_t ev = nullptr;            // recorded behind every apply
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
    uint64_t applies = 0;
};

namespace spal {
namespace {

void tail_from_update(spal_amg *g) {
    g->tail_from = (uint32_t)g->levels.size();
    for (uint32_t l = 0; l < g->levels.size(); ++l)
        if ((int64_t)g->levels[l]->n <= g->tail_rows) {
            g->tail_from = l;
            break;
        }
}

void amg_free(spal_amg *g) {
    if (!g) return;
    if (g->ev) (void)hipEventDestroy(g->ev);
    delete g;   // (the levels' blocks return to the allocator with their DevBufs)
}
struct AmgOwner {
    spal_amg *g = nullptr;
    ~AmgOwner() { amg_free(g); }
    spal_amg *release() { spal_amg *p = g; g = nullptr; return p; }
};

int check_params(const char *fn, const spal_amg_params &p) {
    if (p.max_levels < 1 || p.max_levels > kMaxLevels)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: max_levels = %llu must be 1 .. 32", fn, (unsigned long long)p.max_levels);
    if (p.nu < 1 || p.nu > 16) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: nu = %llu must be 1 .. 16", fn, (unsigned long long)p.nu);
    if (p.coarse_sweeps < 1 || p.coarse_sweeps > 1024)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: coarse_sweeps = %llu must be 1 .. 1024", fn, (unsigned long long)p.coarse_sweeps);
    if (p.gamma != 1 && p.gamma != 2)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: gamma = %llu must be 1 (V cycle) or 2 (W cycle)", fn, (unsigned long long)p.gamma);
    if (!std::isfinite(p.omega) || !(p.omega > 0.0)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: omega = %g must be finite and > 0", fn, p.omega);
    if (!std::isfinite(p.alpha) || !(p.alpha > 0.0)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: alpha = %g must be finite and > 0", fn, p.alpha);
    return SPAL_OK;
}

// The aggregates of level `lv` (agg, mptr, mem, nagg, rounds); synchronises `st`.
int aggregate_level(const char *fn, int device, Level &lv, uint64_t seed, hipStream_t st) {
    const uint32_t n = lv.n;
    OpArrays t;   // the level's transpose: its rows are the other half of every row's neighbours
    SPAL_TRY(transpose_device(device, 4, n, n, lv.nnz, lv.ptr.as<uint32_t>(), lv.ind.as<uint32_t>(), lv.ind.p, st, t));
    DevBuf prio, state, lists, poll, rootof, flag, num, iota;
    SPAL_HIP_TRY(prio.alloc((size_t)n * 8));
    SPAL_HIP_TRY(state.alloc((size_t)n * 4));
    SPAL_HIP_TRY(lists.alloc((size_t)n * 8));
    SPAL_HIP_TRY(poll.alloc(sizeof(Poll)));
    SPAL_HIP_TRY(rootof.alloc((size_t)n * 4));
    SPAL_HIP_TRY(flag.alloc(((size_t)n + 1) * 4));
    SPAL_HIP_TRY(num.alloc(((size_t)n + 1) * 4));
    SPAL_HIP_TRY(iota.alloc(((size_t)n + 1) * 4));
    SPAL_HIP_TRY(lv.agg.alloc((size_t)n * 4));
    const Graph g{lv.ptr.as<uint32_t>(), lv.ind.as<uint32_t>(), t.ptr, t.ind};
    const dim3 grid_n(grid_of(n, kThreads)), grid_n1(grid_of((uint64_t)n + 1, kThreads)), block(kThreads);
    hipLaunchKernelGGL(k_prio, grid_n, block, 0, st, g, n, (uint32_t)seed, prio.as<unsigned long long>());
    SPAL_HIP_TRY(hipGetLastError());
    SPAL_HIP_TRY(hipMemsetAsync(state.p, 0, (size_t)n * 4, st));
    SPAL_HIP_TRY(hipMemsetAsync(poll.p, 0, sizeof(Poll), st));
    uint32_t *half[2] = {lists.as<uint32_t>(), lists.as<uint32_t>() + n};
    Poll h{};
    uint32_t r = 0, left = n, batch = kFirstBatch;
    while (left) {
        const dim3 grid(grid_of(left, kThreads));
        for (uint32_t i = 0; i < batch; ++i, ++r) {
            // round r reads the list round r - 1 wrote: half[r & 1]; round 0 reads none
            if (r == 0)
                hipLaunchKernelGGL(k_round<true>, grid, block, 0, st, g, (const unsigned long long *)prio.p, n, r,
                                   state.as<uint32_t>(), (const uint32_t *)nullptr, half[1], poll.as<Poll>());
            else
                hipLaunchKernelGGL(k_round<false>, grid, block, 0, st, g, (const unsigned long long *)prio.p, n, r,
                                   state.as<uint32_t>(), (const uint32_t *)half[r & 1], half[(r + 1) & 1], poll.as<Poll>());
        }
        SPAL_HIP_TRY(hipGetLastError());
        SPAL_HIP_TRY(hipMemcpyAsync(&h, poll.p, sizeof h, hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        const uint32_t now = h.count[r % 3];   // what round r would start with
        if (now >= left && h.rounds + batch <= r)
            return fail(SPAL_ERR_HIP, "%s: %u rounds decided no vertex (%u left): internal error", fn, batch, now);
        left = now;
        batch = std::min(batch * 2, kMaxBatch);
    }
    lv.rounds = h.rounds;
    hipLaunchKernelGGL(k_join, grid_n1, block, 0, st, g, (const unsigned long long *)prio.p, n, (const uint32_t *)state.p,
                       rootof.as<uint32_t>(), flag.as<uint32_t>());
    SPAL_HIP_TRY(hipGetLastError());
    SPAL_HIP_TRY(scan_exclusive<uint32_t>(flag.as<uint32_t>(), num.as<uint32_t>(), (uint64_t)n + 1, st));
    hipLaunchKernelGGL(k_number, grid_n1, block, 0, st, (const uint32_t *)rootof.p, (const uint32_t *)num.p, n,
                       lv.agg.as<uint32_t>(), iota.as<uint32_t>());
    SPAL_HIP_TRY(hipGetLastError());
    uint32_t nagg = 0;
    SPAL_HIP_TRY(hipMemcpyAsync(&nagg, num.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    lv.nagg = nagg;
    // the members of every aggregate, ascending: the rows sorted stably by aggregate (the 8 bytes that travel with a
    // row are its priority: any would do)
    OpArrays by;
    SPAL_TRY(transpose_device(device, 8, n, nagg, n, iota.as<uint32_t>(), lv.agg.as<uint32_t>(), prio.p, st, by));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    lv.mptr.p = by.ptr;
    lv.mem.p = by.ind;
    by.ptr = by.ind = nullptr;
    return SPAL_OK;
}

// w of a level; *missing = its first row without a stored diagonal (n: none).  Synchronises `st`.
template <typename T>
int weights_level(Level &lv, double omega, hipStream_t st, uint32_t *missing) {
    DevBuf miss;
    SPAL_HIP_TRY(miss.alloc(4));
    SPAL_HIP_TRY(lv.w.alloc((size_t)lv.n * sizeof(T)));
    *missing = lv.n;
    SPAL_HIP_TRY(hipMemcpyAsync(miss.p, missing, 4, hipMemcpyHostToDevice, st));
    if (lv.n) {
        hipLaunchKernelGGL(k_weights<T>, dim3(grid_of(lv.n, kThreads)), dim3(kThreads), 0, st, (const uint32_t *)lv.ptr.p,
                           (const uint32_t *)lv.ind.p, (const T *)lv.val.p, lv.n, (T)omega, lv.w.as<T>(), miss.as<uint32_t>());
        SPAL_HIP_TRY(hipGetLastError());
    }
    SPAL_HIP_TRY(hipMemcpyAsync(missing, miss.p, 4, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    return SPAL_OK;
}

// A_{l+1} from level `lv` and its aggregates, through the COO assembly: nothing goes through the host
int coarse_level(int device, int elem_size, const Level &lv, hipStream_t st, Level &out) {
    DevBuf rows, cols;
    SPAL_HIP_TRY(rows.alloc((size_t)lv.nnz * 4));
    SPAL_HIP_TRY(cols.alloc((size_t)lv.nnz * 4));
    if (lv.nnz) {
        hipLaunchKernelGGL(k_triplets, dim3(grid_of(lv.nnz, kThreads)), dim3(kThreads), 0, st, (const uint32_t *)lv.ptr.p,
                           (const uint32_t *)lv.ind.p, (const uint32_t *)lv.agg.p, lv.n, lv.nnz, rows.as<uint32_t>(),
                           cols.as<uint32_t>());
        SPAL_HIP_TRY(hipGetLastError());
    }
    spal_coo c;   // the assembly's view of the triplets: the arrays stay ours, its workspace goes back below
    c.device = device;
    c.elem_size = elem_size;
    c.nrows = c.ncols = lv.nagg;
    c.len = lv.nnz;
    c.d_rows = rows.as<uint32_t>();
    c.d_cols = cols.as<uint32_t>();
    c.d_vals = lv.val.p;   // (read only)
    Assembled res;
    const int status = coo_assemble(&c, false, st, coo_read_knobs(), res);
    (void)dev_free(c.d_work);
    if (c.h_back) (void)hipHostFree(c.h_back);
    (void)dev_free(res.d_gwin);
    res.d_gwin = nullptr;
    SPAL_TRY(status);
    out.n = lv.nagg;
    out.nnz = (uint32_t)res.nnz;
    out.ptr.p = res.ptr;
    out.ind.p = res.ind;
    out.val.p = res.val;
    res.ptr = res.ind = nullptr;
    res.val = nullptr;
    return SPAL_OK;
}

template <typename T>
int finish_views(spal_amg *g, hipStream_t st) {
    const size_t L = g->levels.size();
    g->h_lv.assign(L * sizeof(Lvl<T>), 0);
    Lvl<T> *h = reinterpret_cast<Lvl<T> *>(g->h_lv.data());
    for (size_t l = 0; l < L; ++l) {
        Level &lv = *g->levels[l];
        const uint64_t stride = ((uint64_t)lv.n + 63) & ~(uint64_t)63;   // every vector on a 256-byte boundary at least
        SPAL_HIP_TRY(lv.vecs.alloc((size_t)5 * stride * sizeof(T)));
        T *v = lv.vecs.as<T>();
        const bool last = l + 1 == L;
        h[l] = Lvl<T>{lv.ptr.as<uint32_t>(), lv.ind.as<uint32_t>(), lv.val.as<T>(), lv.w.as<T>(),
                      last ? nullptr : lv.agg.as<uint32_t>(), last ? nullptr : lv.mptr.as<uint32_t>(),
                      last ? nullptr : lv.mem.as<uint32_t>(), v, v + stride, v + 2 * stride, v + 3 * stride, v + 4 * stride,
                      lv.n, last ? 0u : lv.nagg};
    }
    SPAL_HIP_TRY(g->d_lv.alloc(L * sizeof(Lvl<T>)));
    SPAL_HIP_TRY(hipMemcpyAsync(g->d_lv.p, h, L * sizeof(Lvl<T>), hipMemcpyHostToDevice, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    return SPAL_OK;
}

template <typename T>
int setup_run(const char *fn, spal_csr *a, const spal_amg_params &p, hipStream_t st, spal_amg *g) {
    g->device = a->device;
    g->elem_size = a->elem_size;
    g->params = p;
    SPAL_HIP_TRY(hipEventCreateWithFlags(&g->ev, hipEventDisableTiming));
    {   // level 0: the hierarchy's own copy of the CSR arrays
        std::unique_ptr<Level> lv(new Level);
        lv->n = (uint32_t)a->nrows;
        lv->nnz = (uint32_t)a->nnz;
        SPAL_HIP_TRY(lv->ptr.alloc(((size_t)lv->n + 1) * 4));
        SPAL_HIP_TRY(lv->ind.alloc(((size_t)lv->nnz + kStreamPad) * 4));
        SPAL_HIP_TRY(lv->val.alloc(((size_t)lv->nnz + kStreamPad) * sizeof(T)));
        SPAL_HIP_TRY(hipMemcpyAsync(lv->ptr.p, a->d_rowptr, ((size_t)lv->n + 1) * 4, hipMemcpyDeviceToDevice, st));
        if (lv->nnz) {
            SPAL_HIP_TRY(hipMemcpyAsync(lv->ind.p, a->d_colind, (size_t)lv->nnz * 4, hipMemcpyDeviceToDevice, st));
            SPAL_HIP_TRY(hipMemcpyAsync(lv->val.p, a->d_values, (size_t)lv->nnz * sizeof(T), hipMemcpyDeviceToDevice, st));
        }
        uint32_t missing = 0;
        SPAL_TRY(weights_level<T>(*lv, p.omega, st, &missing));
        if (missing < lv->n)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: row %u stores no diagonal entry (the smoother divides by it)", fn, missing);
        g->levels.push_back(std::move(lv));
    }
    for (;;) {
        Level &lv = *g->levels.back();
        const size_t l = g->levels.size() - 1;
        if (!((uint64_t)lv.n > p.coarse_rows)) { g->stopped_by = "coarse_rows"; break; }
        if (!(l + 1 < p.max_levels)) { g->stopped_by = "max_levels"; break; }
        const auto t0 = std::chrono::steady_clock::now();
        SPAL_TRY(aggregate_level(fn, g->device, lv, p.seed, st));
        bool stop = false;
        if (!(lv.nagg < lv.n)) {
            g->stopped_by = "no_coarsening";
            stop = true;
        } else {
            std::unique_ptr<Level> next(new Level);
            SPAL_TRY(coarse_level(g->device, g->elem_size, lv, st, *next));
            uint32_t missing = 0;
            SPAL_TRY(weights_level<T>(*next, p.omega, st, &missing));
            if (missing < next->n) {
                g->stopped_by = "diagonal";
                stop = true;
            } else {
                lv.setup_ms = ms_since(t0);
                g->levels.push_back(std::move(next));
            }
        }
        if (stop) {   // level l stays the coarsest: it has no aggregates
            lv.setup_ms = ms_since(t0);
            lv.nagg = 0;
            lv.rounds = 0;
            for (DevBuf *b : {&lv.agg, &lv.mptr, &lv.mem}) {
                (void)dev_free(b->p);
                b->p = nullptr;
            }
            break;
        }
    }
    SPAL_TRY(finish_views<T>(g, st));
    tail_from_update(g);
    return SPAL_OK;
}

template <typename H>
int setup_entry(const char *fn, H *a, const spal_amg_params *params, void *stream, spal_amg_t *out) {
    if (!a || !params || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    SPAL_TRY(check_params(fn, *params));
    if (row_blocks(a)) return refuse_row_blocks(fn);
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    SPAL_TRY(refuse_capture(fn, st, "the call allocates and synchronises"));
    AmgOwner own;
    own.g = new spal_amg;
    spal_csr *csr = solve_handle(a);   // a CSC handle: its CSR twin
    SPAL_TRY(a->elem_size == 8 ? setup_run<double>(fn, csr, *params, st, own.g) : setup_run<float>(fn, csr, *params, st, own.g));
    *out = own.release();
    return SPAL_OK;
}

// ---- the cycle, enqueued ---------------------------------------------------------------------------------------------
template <typename T>
struct Enqueue {
    spal_amg *g;
    const Lvl<T> *h;
    hipStream_t st;
    Cyc c;
    T alpha;

    template <int STEP>
    void step(const Lvl<T> &L, const T *b, const T *x, T *out) {
        const uint32_t rows = STEP == S_RESTRICT ? L.nagg : L.n;
        if (rows)
            hipLaunchKernelGGL((k_step<T, STEP>), dim3(grid_of(rows, kThreads)), dim3(kThreads), 0, st, L, b, x, out, alpha);
    }
    // cycle(l, b) -> out, the text: out is neither of the level's ping-pong vectors
    void cycle(uint32_t l, const T *b, T *out) {
        const Lvl<T> &L = h[l];
        if (l >= g->tail_from) {
            hipLaunchKernelGGL(k_tail<T>, dim3(1), dim3(kTailThreads), 0, st, (const Lvl<T> *)g->d_lv.p, l, c, alpha, b, out);
            return;
        }
        const bool coarsest = l + 1 == c.levels;
        const uint32_t s = coarsest ? c.coarse_sweeps : c.nu;
        T *x = coarsest && s == 1 ? out : L.xa;
        step<S_SMOOTH0>(L, b, nullptr, x);
        for (uint32_t k = 1; k < s; ++k) {
            T *xo = coarsest && k + 1 == s ? out : (x == L.xa ? L.xb : L.xa);
            step<S_SMOOTH>(L, b, x, xo);
            x = xo;
        }
        if (coarsest) return;
        for (uint32_t k = 0; k < c.gamma; ++k) {
            step<S_RESIDUAL>(L, b, x, L.r);
            step<S_RESTRICT>(L, nullptr, L.r, h[l + 1].b);
            cycle(l + 1, h[l + 1].b, h[l + 1].e);
            step<S_PROLONG>(L, nullptr, h[l + 1].e, x);
        }
        for (uint32_t k = 0; k < c.nu; ++k) {
            T *xo = k + 1 == c.nu ? out : (x == L.xa ? L.xb : L.xa);
            step<S_SMOOTH>(L, b, x, xo);
            x = xo;
        }
    }
};

template <typename T>
int apply_enqueue_t(const char *fn, spal_amg *g, const T *b, T *x, hipStream_t st) {
    SPAL_TRY(refuse_capture(fn, st, "the cycle's launches use the handle's work vectors and its event"));
    std::lock_guard<std::mutex> lock(g->mu);
    if (g->last_valid && g->last_stream != st) SPAL_HIP_TRY(hipStreamWaitEvent(st, g->ev, 0));   // no host wait
    const spal_amg_params &p = g->params;
    Enqueue<T> q{g, reinterpret_cast<const Lvl<T> *>(g->h_lv.data()), st,
                 Cyc{(uint32_t)p.nu, (uint32_t)p.coarse_sweeps, (uint32_t)p.gamma, (uint32_t)g->levels.size()}, (T)p.alpha};
    q.cycle(0, b, x);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    SPAL_HIP_TRY(hipEventRecord(g->ev, st));
    g->last_stream = st;
    g->last_valid = true;
    ++g->applies;
    return SPAL_OK;
}

template <typename T>
int apply_checks(const char *fn, spal_amg *g, const T *b, const T *x) {
    if (!g) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    if (!b || !x) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null vector", fn);
    SPAL_TRY(check_dtype<T>(fn, g->elem_size));
    if (b == x) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x == b (the cycle reads b after it has written x)", fn);
    return SPAL_OK;
}

template <typename T>
int apply_dev(const char *fn, spal_amg *g, const T *b, T *x, void *stream) {
    SPAL_TRY(apply_checks<T>(fn, g, b, x));
    DeviceGuard guard(g->device);
    if (guard.status != SPAL_OK) return guard.status;
    return apply_enqueue_t<T>(fn, g, b, x, (hipStream_t)stream);
}

template <typename T>
int apply_host(const char *fn, spal_amg *g, const T *b, uint64_t b_len, T *x, uint64_t x_len) {
    SPAL_TRY(apply_checks<T>(fn, g, b, x));
    const uint64_t n = g->levels[0]->n;
    if (b_len != n || x_len != n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: b.len() = %llu and x.len() = %llu but the hierarchy has %llu rows", fn,
                    (unsigned long long)b_len, (unsigned long long)x_len, (unsigned long long)n);
    DeviceGuard guard(g->device);
    if (guard.status != SPAL_OK) return guard.status;
    DevBuf db, dx;
    hipStream_t s = nullptr;
    SPAL_HIP_TRY(db.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(dx.alloc(n * sizeof(T)));
    SPAL_HIP_TRY(stream_acquire(&s));
    struct Release {
        hipStream_t s;
        ~Release() { stream_release(s); }
    } release{s};
    SPAL_HIP_TRY(hipMemcpyAsync(db.p, b, n * sizeof(T), hipMemcpyHostToDevice, s));
    SPAL_TRY(apply_enqueue_t<T>(fn, g, db.as<T>(), dx.as<T>(), s));
    SPAL_HIP_TRY(hipMemcpyAsync(x, dx.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
    SPAL_HIP_TRY(hipStreamSynchronize(s));
    return SPAL_OK;
}

std::string list_of(const spal_amg *g, const std::function<std::string(const Level &)> &f) {
    std::string s = "[";
    for (size_t l = 0; l < g->levels.size(); ++l) s += (l ? ", " : "") + f(*g->levels[l]);
    return s + "]";
}

}  // namespace

// ---- what spal_krylov.hip calls (spal_ops.hpp) -------------------------------------------------------------------------
int amg_check_match(const char *fn, const spal_amg *g, uint64_t nrows, int device, int elem_size) {
    if (!g) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument (the hierarchy)", fn);
    if (g->device != device) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: operands on devices %d and %d", fn, device, g->device);
    if (g->elem_size != elem_size)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: operands of element sizes %d and %d", fn, elem_size, g->elem_size);
    if (g->levels[0]->n != nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the hierarchy has %u rows but the matrix %llu", fn, g->levels[0]->n,
                    (unsigned long long)nrows);
    return SPAL_OK;
}
int amg_apply_enqueue(const char *fn, spal_amg *g, const void *b, void *x, hipStream_t st) {
    return g->elem_size == 8 ? apply_enqueue_t<double>(fn, g, (const double *)b, (double *)x, st)
                             : apply_enqueue_t<float>(fn, g, (const float *)b, (float *)x, st);
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_amg_setup(spal_csr_t a, const spal_amg_params *params, void *stream, spal_amg_t *out) {
    return setup_entry("spal_csr_amg_setup", a, params, stream, out);
}
int spal_csc_amg_setup(spal_csc_t a, const spal_amg_params *params, void *stream, spal_amg_t *out) {
    return setup_entry("spal_csc_amg_setup", a, params, stream, out);
}

int spal_amg_destroy(spal_amg_t g) {
    if (!g) return SPAL_OK;
    DeviceGuard guard(g->device);
    amg_free(g);
    return SPAL_OK;
}

int spal_amg_describe(spal_amg_t g, char *buf, size_t buf_len) {
    const char *fn = "spal_amg_describe";
    if (!g || !buf || !buf_len) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    std::lock_guard<std::mutex> lock(g->mu);
    char tmp[512];
    const spal_amg_params &p = g->params;
    std::string s = "{\"dtype\": \"";
    s += g->elem_size == 8 ? "f64" : "f32";
    s += "\", \"levels\": " + std::to_string(g->levels.size());
    s += ", \"rows\": " + list_of(g, [](const Level &l) { return std::to_string(l.n); });
    s += ", \"nnz\": " + list_of(g, [](const Level &l) { return std::to_string(l.nnz); });
    s += ", \"aggregates\": " + list_of(g, [](const Level &l) { return std::to_string(l.nagg); });
    s += ", \"rounds\": " + list_of(g, [](const Level &l) { return std::to_string(l.rounds); });
    s += ", \"setup_ms\": " + list_of(g, [](const Level &l) {
             char b[32];
             snprintf(b, sizeof b, "%.4f", l.setup_ms);
             return std::string(b);
         });
    snprintf(tmp, sizeof tmp,
             ", \"stopped_by\": \"%s\", \"tail_rows\": %lld, \"tail_from_level\": %u, \"applies\": %llu, \"params\": {\"seed\": %llu, "
             "\"max_levels\": %llu, \"coarse_rows\": %llu, \"nu\": %llu, \"coarse_sweeps\": %llu, \"gamma\": %llu, "
             "\"omega\": %.17g, \"alpha\": %.17g}}",
             g->stopped_by, (long long)g->tail_rows, g->tail_from, (unsigned long long)g->applies, (unsigned long long)p.seed,
             (unsigned long long)p.max_levels, (unsigned long long)p.coarse_rows, (unsigned long long)p.nu,
             (unsigned long long)p.coarse_sweeps, (unsigned long long)p.gamma, p.omega, p.alpha);
    s += tmp;
    if (s.size() + 1 > buf_len) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the buffer holds %zu bytes, %zu are needed", fn, buf_len, s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return SPAL_OK;
}

int spal_amg_set_option(spal_amg_t g, const char *key, int64_t value) {
    const char *fn = "spal_amg_set_option";
    if (!g || !key) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (strcmp(key, "amg_tail_rows")) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: unknown option \"%s\"", fn, key);
    if (value < 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "amg_tail_rows must be >= 0 (0: no level runs in the single-workgroup tail)");
    std::lock_guard<std::mutex> lock(g->mu);
    g->tail_rows = std::min(value, kTailRowsMax);
    tail_from_update(g);
    return SPAL_OK;
}

int spal_amg_level_csr(spal_amg_t g, uint64_t level, spal_csr_t *copy) {
    const char *fn = "spal_amg_level_csr";
    if (!g || !copy) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *copy = nullptr;
    if (level >= g->levels.size())
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: level = %llu but the hierarchy has %zu", fn, (unsigned long long)level, g->levels.size());
    DeviceGuard guard(g->device);
    if (guard.status != SPAL_OK) return guard.status;
    const Level &lv = *g->levels[level];
    OpArrays o;
    SPAL_TRY(o.alloc(lv.n, lv.nnz, (size_t)g->elem_size, nullptr));
    SPAL_HIP_TRY(hipMemcpyAsync(o.ptr, lv.ptr.p, ((size_t)lv.n + 1) * 4, hipMemcpyDeviceToDevice, nullptr));
    if (lv.nnz) {
        SPAL_HIP_TRY(hipMemcpyAsync(o.ind, lv.ind.p, (size_t)lv.nnz * 4, hipMemcpyDeviceToDevice, nullptr));
        SPAL_HIP_TRY(hipMemcpyAsync(o.val, lv.val.p, (size_t)lv.nnz * g->elem_size, hipMemcpyDeviceToDevice, nullptr));
    }
    SPAL_HIP_TRY(hipStreamSynchronize(nullptr));
    return o.adopt(g->device, g->elem_size, lv.n, lv.n, copy);
}

int spal_amg_aggregates(spal_amg_t g, uint64_t level, uint64_t *agg_host, uint64_t len) {
    const char *fn = "spal_amg_aggregates";
    if (!g || (!agg_host && len)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (level + 1 >= g->levels.size())
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: level = %llu has no coarser level (the hierarchy has %zu)", fn,
                    (unsigned long long)level, g->levels.size());
    const Level &lv = *g->levels[level];
    if (len != lv.n)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: len = %llu but level %llu has %u rows", fn, (unsigned long long)len,
                    (unsigned long long)level, lv.n);
    DeviceGuard guard(g->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::vector<uint32_t> a32(lv.n);
    SPAL_HIP_TRY(hipMemcpy(a32.data(), lv.agg.p, (size_t)lv.n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < lv.n; ++i) agg_host[i] = a32[i];
    return SPAL_OK;
}

int spal_amg_apply_f64(spal_amg_t g, const double *b, uint64_t b_len, double *x, uint64_t x_len) {
    return apply_host<double>("spal_amg_apply", g, b, b_len, x, x_len);
}
int spal_amg_apply_f32(spal_amg_t g, const float *b, uint64_t b_len, float *x, uint64_t x_len) {
    return apply_host<float>("spal_amg_apply", g, b, b_len, x, x_len);
}
int spal_amg_apply_dev_f64(spal_amg_t g, const double *b_dev, double *x_dev, void *stream) {
    return apply_dev<double>("spal_amg_apply_dev", g, b_dev, x_dev, stream);
}
int spal_amg_apply_dev_f32(spal_amg_t g, const float *b_dev, float *x_dev, void *stream) {
    return apply_dev<float>("spal_amg_apply_dev", g, b_dev, x_dev, stream);
}

}  // extern "C"
