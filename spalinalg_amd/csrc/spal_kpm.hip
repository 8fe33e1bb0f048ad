// spal_kpm.hip -- the KPM moments: mu_i = z^T T_i(A) z for a block of probe columns, spal_*_kpm_moments_*.
// The contract is the sequential text in include/spal.h: the unscaled Chebyshev recurrence of cheb_series per column, the
// doubling identities, rowsum's order in every row and dot's fixed tree in every moment.
//
// THE BLOCK STEP, kpm_step<T, KT, MODE, FUSED>.  A workgroup of 256 threads owns ONE TILE OF 1024 CONSECUTIVE ROWS (dot's
// tile) and KT columns (blockIdx.y = the column tile); thread t owns rows t, t + 256, t + 512, t + 768 of the tile, all KT
// columns of each.  The work blocks hold kp = k rounded up to whole column tiles columns, TILE-MAJOR: column tile c is
// a row-major n x KT block of its own at element c * n * KT, so a row's KT values are one aligned vector and a pass over
// a tile touches only that tile's cache lines (a row-major n x kp block gave every pass lines that were 1/2 .. 1/8 used).
//   * The rows' entries are one contiguous range of `values` / `colind`, walked in chunks as cheb_rowsum walks it: every
//     lane loads its entries' values and columns coalesced and non-temporal, gathers the KT values of row col[q] of
//     t_{i-1} as ONE vector load, and writes the KT rounded products to LDS (entry-major); after a barrier every thread
//     adds the products of its own four rows, in storage order, onto 4 x KT accumulators that it carries from chunk to
//     chunk.  One pass over the matrix advances KT columns; a row of any length is rowsum's chain.
//   * The recurrence epilogue is fused: the thread reads t_{i-1}[r] and t_{i-2}[r] of its rows (vectors again), forms
//     t_i[r] and stores it.
//   * THE FIRST LEVEL OF THE DOTS IS FUSED TOO.  reduce()'s first halving pairs e[t] with e[t + 512] and the second with
//     e[t + 256]: thread t holds exactly those four elements, so (p0 + p2) + (p1 + p3) per column and then tile_sum's
//     tree through LDS (KT columns side by side, the products' LDS reused) is the tile's sum; thread 0 stores one value
//     per (tile, column, dot).  Rows past n contribute +0.0, which is added, as the text pads.
//   * kpm_finish, one workgroup per column, walks upper_levels for the step's dots and writes the moments into the
//     device table; mu_0 and mu_1 stay beside it in T for the later steps.
//   * FIRST (step 1) forms three dots -- (t_0, t_0), (t_1, t_0), (t_1, t_1) --, every later step two.
// Nothing waits on another workgroup and nothing spins: the launches are ordered by the stream alone.
//
// PADDING COLUMNS.  Columns k .. kp - 1 of the work blocks are zero probes; they are advanced like the others (0, or
// NaN under a matrix entry that is not finite) and never returned.  No lane is masked by column.
//
// Options on `a`: "kpm_tile" (0 = automatic = the narrowest of 1, 2, 4, 8 that holds k, at most 8), "kpm_form" (0 =
// automatic = 1 = fused dots; 2 = the same step without them, followed by kpm_dots, which reads t_i and t_{i-1} back and
// runs the same tree: the same bits, kept for the measurement), and "cheb_chunk" (clipped so that chunk * KT * sizeof(T)
// stays within 32 KiB).  None of them changes a bit of the result.
#include "kpm_host.hpp"
#include "krylov_kernels.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

static_assert(kKpmDotTile == kTile, "a workgroup owns dot's tile");
constexpr int kKpmThreads = 256;
constexpr int kKpmRows = 4;   // rows of a thread: kTile / kKpmThreads

enum KpmMode { KPM_FIRST = 0, KPM_STEP = 1 };

// a row's KT values: one load of up to 16 bytes, or several of 16
template <typename T, int KT>
struct alignas(sizeof(T) * KT < 16 ? sizeof(T) * KT : 16) KVec {
    T v[KT];
};

// The KT tile sums of a workgroup's tile, valid in thread 0: tile_sum's tree for KT columns side by side.  a[j] is the
// thread's (p0 + p2) + (p1 + p3) of column j; `lds` holds KT * 256 elements; ends with a barrier.
template <typename T, int KT>
__device__ __forceinline__ void kpm_tile_sums(T (&a)[KT], T *lds) {
    const unsigned t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < KT; ++j) lds[j * kKpmThreads + t] = a[j];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int j = 0; j < KT; ++j) {
            a[j] = lds[j * kKpmThreads + t] + lds[j * kKpmThreads + t + 128];   // h = 128
            if (t >= 64) lds[j * kKpmThreads + t] = a[j];                       // (its own slot)
        }
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int j = 0; j < KT; ++j) {
            a[j] = a[j] + lds[j * kKpmThreads + t + 64];                        // h = 64
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) a[j] = a[j] + __shfl_down(a[j], h, 64);
        }
    }
    __syncthreads();
}

template <typename T>
struct KpmStepArgs {
    const uint32_t *ptr, *ind;
    const T *val;
    uint64_t n, kp, pe;
    const T *y;   // t_{i-1}: gathered
    const T *x;   // t_{i-2} (STEP)
    T *out;       // t_i: a third block
    T *part0;     // (t_i, t_{i-1}) tile sums: part[column * pe + tile]
    T *part1;     // (t_i, t_i)
    T *part2;     // (t_0, t_0), FIRST
    T a, cT;      // a1 (FIRST) or a2
    uint32_t chunk;
};

template <typename T, int KT, int MODE, bool FUSED>
__global__ __launch_bounds__(kKpmThreads) void kpm_step(KpmStepArgs<T> g) {
    using V = KVec<T, KT>;
    constexpr unsigned LOADS = KT >= 4 ? 2 : 4;   // entries a lane has in flight per batch
    extern __shared__ __align__(64) unsigned char kpm_raw[];
    T *prod = reinterpret_cast<T *>(kpm_raw);
    const uint32_t t = threadIdx.x;
    const uint64_t tile = blockIdx.x, row0 = tile * kTile;
    const uint64_t cb = (uint64_t)blockIdx.y * KT;      // cb + KT <= kp
    const uint64_t tb = cb * g.n;                       // the column tile's n x KT block inside a work block
    const uint64_t rend = row0 + kTile < g.n ? row0 + kTile : g.n;
    const uint32_t e0 = g.ptr[row0], e1 = g.ptr[rend];   // row0 < n: the grid has ceil(n / 1024) tiles
    uint32_t s[kKpmRows], e[kKpmRows];
    T acc[kKpmRows][KT];
#pragma unroll
    for (int u = 0; u < kKpmRows; ++u) {
        const uint64_t row = row0 + t + (uint64_t)u * kKpmThreads;
        s[u] = e[u] = 0;
        if (row < g.n) {
            s[u] = g.ptr[row];
            e[u] = g.ptr[row + 1];
        }
#pragma unroll
        for (int j = 0; j < KT; ++j) acc[u][j] = T(0);
    }
    const T *ycol = g.y + tb;
    for (uint32_t c0 = e0; c0 < e1; c0 += g.chunk) {    // uniform in the workgroup; c0 + chunk < 2^32 (kMaxEntries)
        const uint32_t cend = e1 - c0 < g.chunk ? e1 : c0 + g.chunk;
        for (uint32_t q0 = c0 + t; q0 < cend; q0 += LOADS * kKpmThreads) {
            T a[LOADS];
            uint32_t col[LOADS];
            V gy[LOADS];
#pragma unroll
            for (unsigned u = 0; u < LOADS; ++u) {
                const uint32_t q = q0 + u * kKpmThreads;
                if (q < cend) {
                    a[u] = __builtin_nontemporal_load(g.val + q);
                    col[u] = __builtin_nontemporal_load(g.ind + q);
                }
            }
#pragma unroll
            for (unsigned u = 0; u < LOADS; ++u)
                if (q0 + u * kKpmThreads < cend) gy[u] = *reinterpret_cast<const V *>(ycol + (uint64_t)col[u] * KT);
#pragma unroll
            for (unsigned u = 0; u < LOADS; ++u) {
                const uint32_t q = q0 + u * kKpmThreads;
                if (q < cend) {
                    V p;
#pragma unroll
                    for (int j = 0; j < KT; ++j) p.v[j] = a[u] * gy[u].v[j];
                    *reinterpret_cast<V *>(prod + (size_t)(q - c0) * KT) = p;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kKpmRows; ++u) {
            const uint32_t lo = s[u] > c0 ? s[u] : c0, hi = e[u] < cend ? e[u] : cend;
            for (uint32_t q = lo; q < hi; ++q) {
                const V p = *reinterpret_cast<const V *>(prod + (size_t)(q - c0) * KT);
#pragma unroll
                for (int j = 0; j < KT; ++j) acc[u][j] = acc[u][j] + p.v[j];
            }
        }
        __syncthreads();
    }
    // the epilogue: t_i of the thread's rows, and the rounded products of the dots (+0.0 past n)
    T pc[kKpmRows][KT], ps[kKpmRows][KT], pz[kKpmRows][KT];
#pragma unroll
    for (int u = 0; u < kKpmRows; ++u) {
        const uint64_t row = row0 + t + (uint64_t)u * kKpmThreads;
#pragma unroll
        for (int j = 0; j < KT; ++j) pc[u][j] = ps[u][j] = pz[u][j] = T(0);
        if (row < g.n) {
            const V yr = *reinterpret_cast<const V *>(g.y + tb + row * KT);
            V xr, ti;
            if (MODE == KPM_STEP) xr = *reinterpret_cast<const V *>(g.x + tb + row * KT);
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                if (MODE == KPM_FIRST) ti.v[j] = g.a * (acc[u][j] - (g.cT * yr.v[j]));
                else ti.v[j] = (g.a * (acc[u][j] - (g.cT * yr.v[j]))) - xr.v[j];
                if (FUSED) {
                    pc[u][j] = ti.v[j] * yr.v[j];
                    ps[u][j] = ti.v[j] * ti.v[j];
                    if (MODE == KPM_FIRST) pz[u][j] = yr.v[j] * yr.v[j];
                }
            }
            *reinterpret_cast<V *>(g.out + tb + row * KT) = ti;
        }
    }
    if (!FUSED) return;
    T w[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) w[j] = (pc[0][j] + pc[2][j]) + (pc[1][j] + pc[3][j]);   // h = 512, then h = 256
    kpm_tile_sums<T, KT>(w, prod);
    if (t == 0)
#pragma unroll
        for (int j = 0; j < KT; ++j) g.part0[(cb + j) * g.pe + tile] = w[j];
#pragma unroll
    for (int j = 0; j < KT; ++j) w[j] = (ps[0][j] + ps[2][j]) + (ps[1][j] + ps[3][j]);
    kpm_tile_sums<T, KT>(w, prod);
    if (t == 0)
#pragma unroll
        for (int j = 0; j < KT; ++j) g.part1[(cb + j) * g.pe + tile] = w[j];
    if (MODE == KPM_FIRST) {
#pragma unroll
        for (int j = 0; j < KT; ++j) w[j] = (pz[0][j] + pz[2][j]) + (pz[1][j] + pz[3][j]);
        kpm_tile_sums<T, KT>(w, prod);
        if (t == 0)
#pragma unroll
            for (int j = 0; j < KT; ++j) g.part2[(cb + j) * g.pe + tile] = w[j];
    }
}

// Form 2's dots: the same tile sums from t_i (`out`) and t_{i-1} (`y`) read back; the same grid as the step.
template <typename T, int KT, int MODE>
__global__ __launch_bounds__(kKpmThreads) void kpm_dots(KpmStepArgs<T> g) {
    using V = KVec<T, KT>;
    __shared__ __align__(64) T lds[KT * kKpmThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t tile = blockIdx.x, row0 = tile * kTile, cb = (uint64_t)blockIdx.y * KT, tb = cb * g.n;
    T pc[kKpmRows][KT], ps[kKpmRows][KT], pz[kKpmRows][KT];
#pragma unroll
    for (int u = 0; u < kKpmRows; ++u) {
        const uint64_t row = row0 + t + (uint64_t)u * kKpmThreads;
#pragma unroll
        for (int j = 0; j < KT; ++j) pc[u][j] = ps[u][j] = pz[u][j] = T(0);
        if (row < g.n) {
            const V yr = *reinterpret_cast<const V *>(g.y + tb + row * KT);
            const V ti = *reinterpret_cast<const V *>(g.out + tb + row * KT);
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                pc[u][j] = ti.v[j] * yr.v[j];
                ps[u][j] = ti.v[j] * ti.v[j];
                if (MODE == KPM_FIRST) pz[u][j] = yr.v[j] * yr.v[j];
            }
        }
    }
    T w[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) w[j] = (pc[0][j] + pc[2][j]) + (pc[1][j] + pc[3][j]);
    kpm_tile_sums<T, KT>(w, lds);
    if (t == 0)
#pragma unroll
        for (int j = 0; j < KT; ++j) g.part0[(cb + j) * g.pe + tile] = w[j];
#pragma unroll
    for (int j = 0; j < KT; ++j) w[j] = (ps[0][j] + ps[2][j]) + (ps[1][j] + ps[3][j]);
    kpm_tile_sums<T, KT>(w, lds);
    if (t == 0)
#pragma unroll
        for (int j = 0; j < KT; ++j) g.part1[(cb + j) * g.pe + tile] = w[j];
    if (MODE == KPM_FIRST) {
#pragma unroll
        for (int j = 0; j < KT; ++j) w[j] = (pz[0][j] + pz[2][j]) + (pz[1][j] + pz[3][j]);
        kpm_tile_sums<T, KT>(w, lds);
        if (t == 0)
#pragma unroll
            for (int j = 0; j < KT; ++j) g.part2[(cb + j) * g.pe + tile] = w[j];
    }
}

// The upper levels of step i's dots and its moments, one workgroup per column (blockIdx.x, + gridDim.x, ...):
//   FIRST: mu_0 = (t_0, t_0), mu_1 = (t_1, t_0), mu_2 = (2 * (t_1, t_1)) - mu_0 when 2 <= d; base keeps mu_0 and mu_1.
//   STEP i: mu_{2i-1} = (2 * (t_i, t_{i-1})) - mu_1, mu_{2i} = (2 * (t_i, t_i)) - mu_0 when 2i <= d.
template <typename T>
struct KpmFinArgs {
    T *part0, *part1, *part2, *base;   // base[column] = mu_0, base[kp + column] = mu_1
    double *table;                     // table[i * k + column]
    uint64_t c1, pe, kp, i, d;
    uint32_t k;
};

template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void kpm_finish(KpmFinArgs<T> g) {
    __shared__ T lds[kThreads];
    for (uint64_t col = blockIdx.x; col < g.k; col += gridDim.x) {
        const T cross = upper_levels<T>(g.part0 + col * g.pe, g.c1, lds);
        const T self = upper_levels<T>(g.part1 + col * g.pe, g.c1, lds);
        if (MODE == KPM_FIRST) {
            const T mu0 = upper_levels<T>(g.part2 + col * g.pe, g.c1, lds);
            if (threadIdx.x == 0) {
                g.base[col] = mu0;
                g.base[g.kp + col] = cross;
                g.table[col] = (double)mu0;
                g.table[(uint64_t)g.k + col] = (double)cross;
                if (2 <= g.d) g.table[2 * (uint64_t)g.k + col] = (double)((T(2) * self) - mu0);
            }
        } else if (threadIdx.x == 0) {
            g.table[(2 * g.i - 1) * g.k + col] = (double)((T(2) * cross) - g.base[g.kp + col]);
            if (2 * g.i <= g.d) g.table[2 * g.i * g.k + col] = (double)((T(2) * self) - g.base[col]);
        }
    }
}

// t_0: the hashed probes, or the caller's block, into the first work block (tile-major); the padding columns are +0.0
template <typename T, bool HASH>
__global__ __launch_bounds__(kThreads) void kpm_init(uint64_t n, uint32_t k, uint64_t kp, uint32_t tile, uint32_t seed, const T *z,
                                                     uint64_t ldz, T *out) {
    const uint64_t id = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (id >= n * kp) return;
    const uint64_t i = id / kp, j = id % kp;
    T v = T(0);
    if (j < k) {
        if (HASH) v = colour_mix32(colour_mix32((uint32_t)i + seed) + (uint32_t)j) >> 31 ? T(-1) : T(1);
        else v = z[i * ldz + j];
    }
    out[(j / tile) * n * tile + i * tile + j % tile] = v;
}

#define KPM_BY_TILE(tile, launch)                   \
    switch (tile) {                                 \
    case 1: { constexpr int KT_ = 1; launch; } break; \
    case 2: { constexpr int KT_ = 2; launch; } break; \
    case 4: { constexpr int KT_ = 4; launch; } break; \
    default: { constexpr int KT_ = 8; launch; } break; \
    }

#define KPM_CHECK_LAUNCH()                                                                                     \
    do {                                                                                                       \
        const hipError_t le_ = hipGetLastError();                                                              \
        if (le_ != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(le_)); \
    } while (0)

template <typename T, int MODE>
int launch_step(const char *fn, const KpmStepArgs<T> &g, int tile, int form, hipStream_t st) {
    const dim3 grid((unsigned)tiles_of(g.n), (unsigned)(g.kp / (uint64_t)tile));
    const size_t lds = (size_t)g.chunk * (size_t)tile * sizeof(T);
    if (form == 2) {
        KPM_BY_TILE(tile, hipLaunchKernelGGL((kpm_step<T, KT_, MODE, false>), grid, dim3(kKpmThreads), lds, st, g));
        KPM_CHECK_LAUNCH();
        KPM_BY_TILE(tile, hipLaunchKernelGGL((kpm_dots<T, KT_, MODE>), grid, dim3(kKpmThreads), 0, st, g));
    } else {
        KPM_BY_TILE(tile, hipLaunchKernelGGL((kpm_step<T, KT_, MODE, true>), grid, dim3(kKpmThreads), lds, st, g));
    }
    KPM_CHECK_LAUNCH();
    return SPAL_OK;
}

struct KpmOptions {
    int tile, form;
    unsigned chunk;
};
template <typename H>
KpmOptions kpm_options_of(H *a, uint64_t k, size_t elem) {
    std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
    KpmOptions o;
    o.tile = kpm_tile_of(a->ops.kpm_tile, k);
    o.form = a->ops.kpm_form == 2 ? 2 : 1;
    o.chunk = kpm_chunk_of((unsigned)a->ops.cheb_chunk, o.tile, elem);
    return o;
}

// Everything of a call on `st` after its refusals: t_0, the m steps, the moments' copy back; synchronises once, at the end.
// `work` holds L.total bytes.  z == nullptr: hashed probes.
template <typename T>
int kpm_enqueue(const char *fn, spal_csr *a, uint64_t degree, uint32_t k, uint64_t seed, double lo, double hi, const T *z,
                uint64_t ldz, const KpmLayout &L, const KpmOptions &o, unsigned char *work, double *mu, hipStream_t st,
                uint64_t *launches, float *ms) {
    const uint64_t n = a->nrows, m = kpm_steps(degree);
    const KpmScalars<T> sc = kpm_scalars<T>(lo, hi);
    T *blk[3] = {(T *)(work + L.block[0]), (T *)(work + L.block[1]), (T *)(work + L.block[2])};
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(1));
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    const unsigned init_grid = grid_of(n * L.kp, kThreads);
    if (z) hipLaunchKernelGGL((kpm_init<T, false>), dim3(init_grid), dim3(kThreads), 0, st, n, k, L.kp, (uint32_t)o.tile, 0u, z, ldz, blk[0]);
    else hipLaunchKernelGGL((kpm_init<T, true>), dim3(init_grid), dim3(kThreads), 0, st, n, k, L.kp, (uint32_t)o.tile, (uint32_t)seed, z, ldz,
                                blk[0]);
    KPM_CHECK_LAUNCH();
    uint64_t count = 1;
    KpmStepArgs<T> g{};
    g.ptr = (const uint32_t *)a->d_rowptr;
    g.ind = (const uint32_t *)a->d_colind;
    g.val = (const T *)a->d_values;
    g.n = n;
    g.kp = L.kp;
    g.pe = L.pe;
    g.part0 = (T *)(work + L.part[0]);
    g.part1 = (T *)(work + L.part[1]);
    g.part2 = (T *)(work + L.part[2]);
    g.cT = sc.cT;
    g.chunk = o.chunk;
    KpmFinArgs<T> f{g.part0, g.part1, g.part2, (T *)(work + L.base), (double *)(work + L.table), tiles_of(n), L.pe, L.kp, 0, degree, k};
    const unsigned fin_grid = k;
    for (uint64_t i = 1; i <= m; ++i) {   // t_i lives in block i mod 3: t_{i-1} and t_{i-2} are the other two
        g.y = blk[(i - 1) % 3];
        g.x = blk[(i + 1) % 3];
        g.out = blk[i % 3];
        g.a = i == 1 ? sc.a1 : sc.a2;
        f.i = i;
        if (i == 1) {
            SPAL_TRY((launch_step<T, KPM_FIRST>(fn, g, o.tile, o.form, st)));
            hipLaunchKernelGGL((kpm_finish<T, KPM_FIRST>), dim3(fin_grid), dim3(kThreads), 0, st, f);
        } else {
            SPAL_TRY((launch_step<T, KPM_STEP>(fn, g, o.tile, o.form, st)));
            hipLaunchKernelGGL((kpm_finish<T, KPM_STEP>), dim3(fin_grid), dim3(kThreads), 0, st, f);
        }
        KPM_CHECK_LAUNCH();
        count += o.form == 2 ? 3 : 2;
    }
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipMemcpyAsync(mu, work + L.table, (size_t)(degree + 1) * k * sizeof(double), hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    SPAL_HIP_TRY(ev.span(0, ms));
    *launches = count;
    return SPAL_OK;
}

std::string kpm_json(uint64_t degree, uint64_t k, const KpmOptions &o, double lo, double hi, uint64_t launches, double ms) {
    char buf[512];
    snprintf(buf, sizeof buf,
             "{\"degree\": %llu, \"probes\": %llu, \"steps\": %llu, \"tile\": %d, \"form\": %d, \"chunk\": %u, \"lo\": %.17g, "
             "\"hi\": %.17g, \"launches\": %llu, \"solve_ms\": %.6g}",
             (unsigned long long)degree, (unsigned long long)k, (unsigned long long)kpm_steps(degree), o.tile, o.form, o.chunk, lo,
             hi, (unsigned long long)launches, ms);
    return buf;
}

// the refusals that need no device
template <typename T, typename H>
int kpm_check_call(const char *fn, H *a, uint64_t degree, uint64_t k, int automatic, double lo, double hi, bool has_z,
                   uint64_t z_rows, uint64_t ldz, const double *mu, uint64_t mu_len, const spal_kpm_info *info) {
    if (!a || !mu || !info) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    const KpmRefusal r = kpm_check(degree, k, mu_len, has_z, z_rows, ldz, a->nrows, automatic, lo, hi);
    if (r != KPM_OK)
        return fail(SPAL_ERR_INVALID_ARGUMENT,
                    "%s: %s (degree = %llu, k = %llu, mu_len = %llu, ldz = %llu, z_rows = %llu, automatic = %d, lo = %g, hi = %g)", fn,
                    kpm_refusal_text(r), (unsigned long long)degree, (unsigned long long)k, (unsigned long long)mu_len,
                    (unsigned long long)ldz, (unsigned long long)z_rows, automatic, lo, hi);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    if (row_blocks(a)) return refuse_row_blocks(fn);
    return SPAL_OK;
}

// The call on `st` with device probes (or none).  host_form: the work block comes from the caching allocator, else from
// the stream's scratch.  The device is selected and the stream is not capturing.
template <typename T, typename H>
int kpm_run(const char *fn, H *a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo, double hi, const T *z_dev,
            uint64_t ldz, double *mu, spal_kpm_info *info, hipStream_t st, bool host_form) {
    *info = spal_kpm_info{};
    info->degree = degree;
    info->probes = k;
    spal_csr *h = solve_handle(a);
    const uint64_t n = a->nrows;
    const KpmOptions o = kpm_options_of(a, k, sizeof(T));
    double glo = 0.0, ghi = 0.0;
    if (automatic) {
        if (n == 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix has no rows: an automatic interval needs some", fn);
        SPAL_TRY(gershgorin_run(fn, h, st, &glo, &ghi));
        if (!std::isfinite(glo) || !std::isfinite(ghi))
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: Gershgorin's bounds are not finite: no automatic interval", fn);
        cheb_near_auto_interval(glo, ghi, &lo, &hi);
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the automatic interval [%g, %g] is not finite or is empty", fn, lo, hi);
    }
    info->lo = lo;
    info->hi = hi;
    info->glo = glo;
    info->ghi = ghi;
    info->products = kpm_steps(degree);
    uint64_t launches = 0;
    float ms = 0.f;
    if (n == 0) {   // every dot is +0.0, and so is every moment
        std::fill(mu, mu + (degree + 1) * k, 0.0);
    } else {
        KpmLayout L;
        if (!kpm_layout(n, k, o.tile, degree, sizeof(T), &L))
            return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for work blocks of %llu x %llu", fn, (unsigned long long)n,
                        (unsigned long long)k);
        StreamWork sw;
        DevBuf db;
        unsigned char *work = nullptr;
        if (host_form) {
            SPAL_HIP_TRY(db.alloc(L.total));
            work = db.as<unsigned char>();
        } else {
            SPAL_TRY(sw.take(fn, st, L.total));
            work = sw.as<unsigned char>();
        }
        SPAL_TRY(kpm_enqueue<T>(fn, h, degree, (uint32_t)k, seed, lo, hi, z_dev, ldz, L, o, work, mu, st, &launches, &ms));
    }
    info->solve_ms = (double)ms;
    store_info(a, &OpState::kpm_info, kpm_json(degree, k, o, lo, hi, launches, (double)ms));
    return SPAL_OK;
}

template <typename T, typename H>
int kpm_dev(const char *fn, H *a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo, double hi, const T *z_dev,
            uint64_t ldz, double *mu, uint64_t mu_len, void *stream, spal_kpm_info *info) {
    SPAL_TRY((kpm_check_call<T, H>(fn, a, degree, k, automatic, lo, hi, z_dev != nullptr, a ? a->nrows : 0, ldz, mu, mu_len, info)));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    SPAL_TRY(refuse_capture(fn, st, "the call takes its work blocks from the stream's scratch and synchronises"));
    return kpm_run<T, H>(fn, a, degree, k, seed, automatic, lo, hi, z_dev, ldz, mu, info, st, false);
}

template <typename T, typename H>
int kpm_host(const char *fn, H *a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo, double hi, const T *z,
             uint64_t z_rows, uint64_t ldz, double *mu, uint64_t mu_len, spal_kpm_info *info) {
    SPAL_TRY((kpm_check_call<T, H>(fn, a, degree, k, automatic, lo, hi, z != nullptr, z_rows, ldz, mu, mu_len, info)));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const uint64_t n = a->nrows;
    DevBuf dz;
    PooledStream ps;
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    const T *z_dev = nullptr;
    if (z) {
        SPAL_HIP_TRY(dz.alloc((size_t)n * k * sizeof(T)));
        const size_t row = (size_t)k * sizeof(T);
        if (n) SPAL_HIP_TRY(hipMemcpy2DAsync(dz.p, row, z, (size_t)ldz * sizeof(T), row, n, hipMemcpyHostToDevice, ps.s));
        z_dev = (const T *)dz.p;
    }
    return kpm_run<T, H>(fn, a, degree, k, seed, automatic, lo, hi, z_dev, k, mu, info, ps.s, true);
}

}  // namespace

int kpm_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status) {
    if (!strcmp(key, "kpm_form")) {
        if (value < 0 || value > 2) {
            *status = fail(SPAL_ERR_INVALID_ARGUMENT, "kpm_form must be 0 (automatic), 1 (fused dots) or 2 (step and separate dot launches)");
            return 1;
        }
        std::lock_guard<std::mutex> lock(a->mu);
        s.kpm_form = (int)value;
        *status = SPAL_OK;
        return 1;
    }
    if (strcmp(key, "kpm_tile")) return 0;
    if (!kpm_tile_valid(value)) {
        *status = fail(SPAL_ERR_INVALID_ARGUMENT, "kpm_tile must be 0 (automatic), 1, 2, 4 or 8");
        return 1;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    s.kpm_tile = (int)value;
    *status = SPAL_OK;
    return 1;
}

int kpm_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    return info_describe_append(buf, buf_len, s, solve, "kpm", &OpState::kpm_info);
}

}  // namespace spal

using namespace spal;

extern "C" {

#define SPAL_KPM_ENTRIES(kind, sfx, T)                                                                                       \
    int spal_##kind##_kpm_moments_##sfx(spal_##kind##_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic,         \
                                        double lo, double hi, const T *z, uint64_t z_rows, uint64_t ldz, double *mu,          \
                                        uint64_t mu_len, spal_kpm_info *info) {                                               \
        return kpm_host<T, spal_##kind>("spal_" #kind "_kpm_moments", a, degree, k, seed, automatic, lo, hi, z, z_rows, ldz,  \
                                        mu, mu_len, info);                                                                    \
    }                                                                                                                         \
    int spal_##kind##_kpm_moments_dev_##sfx(spal_##kind##_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic,     \
                                            double lo, double hi, const T *z_dev, uint64_t ldz, double *mu, uint64_t mu_len,  \
                                            void *stream, spal_kpm_info *info) {                                              \
        return kpm_dev<T, spal_##kind>("spal_" #kind "_kpm_moments_dev", a, degree, k, seed, automatic, lo, hi, z_dev, ldz,   \
                                       mu, mu_len, stream, info);                                                             \
    }
SPAL_KPM_ENTRIES(csr, f64, double)
SPAL_KPM_ENTRIES(csr, f32, float)
SPAL_KPM_ENTRIES(csc, f64, double)
SPAL_KPM_ENTRIES(csc, f32, float)
#undef SPAL_KPM_ENTRIES

}  // extern "C"
