// spal_spadd.hip -- C = A + B, C = A - B and C = -A for CSR and CSC on the device: `impl Add / Sub / Neg for
// &CsrMatrix<T>` (src/csr/ops/{add,sub,neg}.rs) and the same for `&CscMatrix<T>` (src/csc/ops/...), bit-identical to
// the reference.  CSC runs the same driver on (colptr, rowind): "row" below reads "column" there.
//
// MERGE PATH over the two entry streams.  A's entries in stored order are sorted by the key (row, col), and so are
// B's.  C's entries are the distinct keys of the merge of the two sequences, in merge order, with A before B on equal
// keys: a matched pair is adjacent, A first.  A B element whose key equals its predecessor's is a DUPLICATE; all other
// elements are written.  Row i's part of the merged sequence starts at s_i = A.ptr[i] + B.ptr[i] (rows are found by
// binary search on s: no row ids, no walk over empty rows), and C.ptr[i] = s_i - (duplicates in rows < i).
//
// The merged sequence (64-bit positions: nnz(A) + nnz(B) may pass 2^32) is cut into tiles of `tile` elements, so every
// workgroup gets the same work whatever the row lengths:
//   spadd_partition  every tile boundary d: the row r with s_r <= d < s_{r+1}, then the A/B split of the diagonal
//                    d - s_r inside row r (A first on equal keys) -> the tile's slices of A and B are contiguous
//   spadd_tile<count> the tile's column slices into LDS (coalesced); each thread merges its own `tile / 256` elements
//                    from a diagonal search in LDS: the tile's non-duplicates, the duplicates per row (integer atomics)
//   two exclusive scans (tile counts -> output offsets, duplicates per row -> C.ptr), nnz(C) read back once
//   spadd_tile<fill>  the same walk again: every non-duplicate goes to LDS at its in-tile prefix, then coalesced to C
// PAIRS SPLIT ACROSS TILES: every tile also reads one element past each end of its slices -- A's entry before its first
// (a B element at the head of a row that began in an earlier tile compares with it) and B's entry after its last (an A
// element at the tail compares with it, and a matched one reads that B value from global memory).  Boundaries stay
// where the arithmetic puts them.
// Values follow the reference's loop: A only `a`, B only `b` (Add) or `-b` (Sub, an fneg), both `a + b` / `a - b`.
#define SPAL_OPS_SCAN
#include "spal_ops.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr int kThreads = 256;              // threads of a tile
constexpr uint32_t kTileMax = 2048;        // the default tile: 8 merged elements per thread
constexpr uint32_t kTileMin = 16;

// the largest r in [lo, hi] with s_r = ap[r] + bp[r] <= d (s_lo <= d)
__device__ __forceinline__ uint32_t row_of(const uint32_t *__restrict__ ap, const uint32_t *__restrict__ bp, uint32_t lo,
                                           uint32_t hi, uint64_t d) {
    while (lo < hi) {
        const uint32_t mid = (uint32_t)(((uint64_t)lo + hi + 1) / 2);
        if ((uint64_t)ap[mid] + bp[mid] <= d) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// part[0 .. P): first A entry of every tile, part[P .. 2P): first B entry, part[2P .. 3P): row of the first element;
// P = tiles + 1 (the last boundary is the end of both operands)
__global__ __launch_bounds__(256) void spadd_partition(const uint32_t *__restrict__ ap, const uint32_t *__restrict__ ai,
                                                       const uint32_t *__restrict__ bp, const uint32_t *__restrict__ bi,
                                                       uint32_t m, uint64_t total, uint32_t tile, uint64_t P,
                                                       uint32_t *__restrict__ part) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P) return;
    const uint64_t d = std::min<uint64_t>(t * tile, total);
    const uint32_t r = row_of(ap, bp, 0, m - 1, d);
    const uint32_t sa = ap[r], sb = bp[r];
    const uint64_t la = ap[r + 1] - sa, lb = bp[r + 1] - sb;
    const uint64_t k = d - ((uint64_t)sa + sb);
    uint64_t lo = k > lb ? k - lb : 0, hi = std::min(k, la);
    while (lo < hi) {   // A entries among the row's first k merged elements (A first on equal columns)
        const uint64_t mid = (lo + hi) / 2;
        if (ai[sa + mid] <= bi[sb + (k - 1 - mid)]) lo = mid + 1;
        else hi = mid;
    }
    part[t] = (uint32_t)(sa + lo);
    part[P + t] = (uint32_t)(sb + (k - lo));
    part[2 * P + t] = r;
}

__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, uint32_t *s_wave, uint32_t *total) {
    const int lane = (int)threadIdx.x % 64, w = (int)threadIdx.x / 64;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t before = inc - v, all = 0;
    for (int u = 0; u < kThreads / 64; ++u) {
        if (u < w) before += s_wave[u];
        all += s_wave[u];
    }
    *total = all;
    return before;
}

// what every thread of a tile knows: the operands' pointers, the slices (in LDS) and the elements past their ends
struct TileCtx {
    const uint32_t *ap, *bp, *sa, *sb;
    uint32_t a0, b0, b1, na, nb, r1, a_prev, b_next;
    uint64_t d0;
};

// a thread's place in the tile's merge: next A / B entry (tile-local), the current row and its ends in the slices
struct Cursor {
    uint32_t r, xa, xb, ea, eb;
    int64_t ra;         // the row's first A entry, tile-local (negative: the row began before the slice)
    bool b_beyond;      // the row's B entries go on past the slice
};

// one merged element: flag = an A element is matched / a B element is a duplicate
struct Elem {
    bool from_a, flag;
    uint32_t xa, xb, row;
};

__device__ __forceinline__ void enter_row(const TileCtx &c, Cursor &w, uint32_t q) {
    w.r = q;
    const uint32_t pa = c.ap[q], pa1 = c.ap[q + 1], pb1 = c.bp[q + 1];
    w.ra = (int64_t)pa - c.a0;
    w.ea = std::min(pa1 - c.a0, c.na);
    w.eb = std::min(pb1 - c.b0, c.nb);
    w.b_beyond = pb1 > c.b1;
}

__device__ __forceinline__ Cursor cursor_at(const TileCtx &c, uint32_t r, uint32_t ja, uint32_t jb, bool any) {
    Cursor w{r, ja, jb, 0, 0, 0, false};
    if (any) enter_row(c, w, r);
    return w;
}

// the element at tile-local position p (the cursor's next one)
__device__ __forceinline__ Elem step(const TileCtx &c, Cursor &w, uint32_t p) {
    if (w.xa == w.ea && w.xb == w.eb) {   // the row is done: the next row with elements (binary search over empty ones)
        const uint64_t d = c.d0 + p;
        uint32_t q = w.r + 1;
        if (q < c.r1 && (uint64_t)c.ap[q + 1] + c.bp[q + 1] <= d) q = row_of(c.ap, c.bp, q + 1, c.r1, d);
        enter_row(c, w, q);
    }
    Elem e;
    e.xa = w.xa;
    e.xb = w.xb;
    e.row = w.r;
    if (w.xa < w.ea && (w.xb >= w.eb || c.sa[w.xa] <= c.sb[w.xb])) {
        const uint32_t col = c.sa[w.xa];
        e.from_a = true;
        e.flag = w.xb < w.eb ? c.sb[w.xb] == col : (w.b_beyond && c.b_next == col);
        ++w.xa;
    } else {
        const uint32_t col = c.sb[w.xb];
        const int64_t pa = (int64_t)w.xa - 1;   // the row's A entry before this one, if any
        e.from_a = false;
        e.flag = pa >= w.ra && (pa >= 0 ? c.sa[pa] : c.a_prev) == col;
        ++w.xb;
    }
    return e;
}

// One tile of the merged sequence per workgroup.  FILL = false: the tile's non-duplicates -> tile_cnt[t], duplicates
// per row -> row_dup[r] (atomics).  FILL = true: the tile's entries of C at tile_off[t] ...
template <typename T, bool FILL, bool SUB>
__global__ __launch_bounds__(kThreads) void spadd_tile(const uint32_t *__restrict__ ap, const uint32_t *__restrict__ ai,
                                                       const T *__restrict__ av, const uint32_t *__restrict__ bp,
                                                       const uint32_t *__restrict__ bi, const T *__restrict__ bv,
                                                       uint32_t nnz_b, uint32_t tile, const uint32_t *__restrict__ part,
                                                       uint64_t P, unsigned long long *__restrict__ tile_cnt,
                                                       uint32_t *__restrict__ row_dup,
                                                       const unsigned long long *__restrict__ tile_off,
                                                       uint32_t *__restrict__ cci, T *__restrict__ cv) {
    __shared__ uint32_t s_col[kTileMax];                 // A's columns [0, na), then B's [na, na + nb)
    __shared__ T s_val[FILL ? kTileMax : 1];
    __shared__ uint32_t o_col[FILL ? kTileMax : 1];      // the tile's part of C
    __shared__ T o_val[FILL ? kTileMax : 1];
    __shared__ uint32_t s_wave[kThreads / 64];
    const uint64_t t = blockIdx.x;
    const uint32_t a0 = part[t], a1 = part[t + 1], b0 = part[P + t], b1 = part[P + t + 1];
    const uint32_t r0 = part[2 * P + t], r1 = part[2 * P + t + 1];
    const uint32_t na = a1 - a0, n = na + (b1 - b0), nb = b1 - b0;
    const uint64_t d0 = t * tile;
    {   // the slices into LDS: every thread issues all its loads (one per kThreads elements) before it stores any
        constexpr int L = kTileMax / kThreads;
        uint32_t col[L];
        T val[L];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const uint32_t x = threadIdx.x + k * kThreads;
            if (x < n) {
                const bool from_a = x < na;
                const uint64_t q = from_a ? (uint64_t)a0 + x : (uint64_t)b0 + (x - na);
                col[k] = (from_a ? ai : bi)[q];
                if constexpr (FILL) val[k] = (from_a ? av : bv)[q];
            }
        }
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const uint32_t x = threadIdx.x + k * kThreads;
            if (x < n) {
                s_col[x] = col[k];
                if constexpr (FILL) s_val[x] = val[k];
            }
        }
    }
    // one element past each end: A's entry before the slice, B's entry after it
    const uint32_t a_prev = a0 ? ai[a0 - 1] : 0u;
    const uint32_t b_next = b1 < nnz_b ? bi[b1] : 0u;
    __syncthreads();
    const uint32_t *sa = s_col, *sb = s_col + na;

    // this thread's first element: its row, then the split of the row's diagonal (inside the tile's slices)
    const uint32_t E = (tile + kThreads - 1) / kThreads;
    const uint32_t p0 = std::min<uint32_t>(threadIdx.x * E, n), pend = std::min<uint32_t>(p0 + E, n);
    uint32_t r = r0, ja = 0, jb = 0;
    if (p0 < pend) {
        const uint64_t d = d0 + p0;
        r = row_of(ap, bp, r0, r1, d);
        const int64_t SA = ap[r], SB = bp[r];
        const int64_t K = (int64_t)(d - (uint64_t)SA - (uint64_t)SB);
        const int64_t LA = (int64_t)ap[r + 1] - SA, LB = (int64_t)bp[r + 1] - SB;
        int64_t lo = std::max(std::max<int64_t>(0, K - LB), std::max<int64_t>((int64_t)a0 - SA, K - ((int64_t)b1 - SB)));
        int64_t hi = std::min(std::min(K, LA), std::min<int64_t>((int64_t)a1 - SA, K - ((int64_t)b0 - SB)));
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (sa[SA + mid - a0] <= sb[SB + (K - 1 - mid) - b0]) lo = mid + 1;
            else hi = mid;
        }
        ja = (uint32_t)(SA + lo - a0);
        jb = p0 - ja;
    }

    const TileCtx c{ap, bp, sa, sb, a0, b0, b1, na, nb, r1, a_prev, b_next, d0};
    if constexpr (!FILL) {
        Cursor w = cursor_at(c, r, ja, jb, p0 < pend);
        uint32_t keep = 0, dups = 0, dup_row = r;
        for (uint32_t p = p0; p < pend; ++p) {
            const Elem e = step(c, w, p);
            if (!e.from_a && e.flag) {
                if (e.row != dup_row) {
                    if (dups) atomicAdd(&row_dup[dup_row], dups);
                    dups = 0;
                    dup_row = e.row;
                }
                ++dups;
            } else {
                ++keep;
            }
        }
        if (dups) atomicAdd(&row_dup[dup_row], dups);
        uint32_t total = 0;
        (void)block_exclusive_sum(keep, s_wave, &total);
        if (threadIdx.x == 0) tile_cnt[t] = total;
    } else {
        uint32_t keep = 0;
        Cursor w = cursor_at(c, r, ja, jb, p0 < pend);
        for (uint32_t p = p0; p < pend; ++p) {
            const Elem e = step(c, w, p);
            keep += (e.from_a || !e.flag) ? 1u : 0u;
        }
        uint32_t total = 0;
        uint32_t o = block_exclusive_sum(keep, s_wave, &total);
        w = cursor_at(c, r, ja, jb, p0 < pend);
        for (uint32_t p = p0; p < pend; ++p) {
            const Elem e = step(c, w, p);
            if (e.from_a) {
                const T a = s_val[e.xa];
                T v = a;
                if (e.flag) {
                    const T b = e.xb < nb ? s_val[na + e.xb] : bv[b1];   // (the pair's B entry past the slice)
                    v = SUB ? a - b : a + b;
                }
                o_col[o] = sa[e.xa];
                o_val[o] = v;
                ++o;
            } else if (!e.flag) {
                const T b = s_val[na + e.xb];
                o_col[o] = sb[e.xb];
                o_val[o] = SUB ? -b : b;
                ++o;
            }
        }
        __syncthreads();
        const unsigned long long base = tile_off[t];
        for (uint32_t x = threadIdx.x; x < total; x += kThreads) {
            cci[base + x] = o_col[x];
            cv[base + x] = o_val[x];
        }
    }
}

// C.ptr[i] = s_i - (duplicates in rows < i)
__global__ __launch_bounds__(256) void spadd_rowptr(const uint32_t *__restrict__ ap, const uint32_t *__restrict__ bp,
                                                    const uint32_t *__restrict__ dscan, uint64_t n,
                                                    uint32_t *__restrict__ cp) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) cp[i] = (uint32_t)((uint64_t)ap[i] + bp[i] - dscan[i]);
}

// y = -x, 16 bytes per thread (an fneg: the sign bit flips for +-0, +-inf and NaN alike); the tail element-wise
template <typename T>
__global__ __launch_bounds__(256) void spadd_neg(const T *__restrict__ x, T *__restrict__ y, uint64_t n) {
    constexpr int W = 16 / sizeof(T);
    typedef T V __attribute__((ext_vector_type(W)));
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t nv = n / W;
    if (i < nv) {
        reinterpret_cast<V *>(y)[i] = -reinterpret_cast<const V *>(x)[i];
    } else if (i - nv < n % W) {
        const uint64_t e = nv * W + (i - nv);
        y[e] = -x[e];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
struct Sum {
    OpArrays c;
    uint64_t matched = 0, tiles = 0;
    uint32_t tile = 0;
    float kernel_ms = 0.f;   // device time: the count pass and the scans, then the fill (EventSpans 0 and 1)
};

// the two exclusive scans of the count pass, sharing one temporary block and one synchronisation of `st`
hipError_t scan_two(const unsigned long long *tin, unsigned long long *tout, uint64_t tn, const uint32_t *rin,
                    uint32_t *rout, uint64_t rn, hipStream_t st) {
    size_t b1 = 0, b2 = 0;
    DevBuf tmp;
    hipError_t e = scan_step(nullptr, b1, tin, tout, tn, st);
    if (e == hipSuccess) e = scan_step(nullptr, b2, rin, rout, rn, st);
    if (e == hipSuccess) e = tmp.alloc(std::max(b1, b2));
    if (e == hipSuccess) e = scan_step(tmp.p, b1, tin, tout, tn, st);
    if (e == hipSuccess) e = scan_step(tmp.p, b2, rin, rout, rn, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // (tmp returns to the allocator on exit)
    return e;
}

template <typename T, bool SUB>
int spadd_t(const char *fn, const Operand &A, const Operand &B, uint32_t tile, hipStream_t st, Sum &out) {
    const uint64_t m = A.nmajor, total = A.nnz + B.nnz;
    const uint64_t tiles = (total + tile - 1) / tile, P = tiles + 1;
    out.tile = tile;
    out.tiles = tiles;
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(2));
    DevBuf part, tcnt, toff, rdup, rscan;
    SPAL_HIP_TRY(part.alloc(P * 3 * 4));
    SPAL_HIP_TRY(tcnt.alloc(P * 8));
    SPAL_HIP_TRY(toff.alloc(P * 8));
    SPAL_HIP_TRY(rdup.alloc((m + 1) * 4));
    SPAL_HIP_TRY(rscan.alloc((m + 1) * 4));
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    SPAL_HIP_TRY(hipMemsetAsync(rdup.p, 0, (m + 1) * 4, st));
    SPAL_HIP_TRY(hipMemsetAsync(tcnt.as<unsigned long long>() + tiles, 0, 8, st));
    const uint32_t *part_p = part.as<uint32_t>();
    if (tiles) {
        hipLaunchKernelGGL(spadd_partition, dim3(grid_of(P, 256)), dim3(256), 0, st, A.ptr, A.ind, B.ptr, B.ind,
                           (uint32_t)m, total, tile, P, part.as<uint32_t>());
        hipLaunchKernelGGL((spadd_tile<T, false, SUB>), dim3((unsigned)tiles), dim3(kThreads), 0, st, A.ptr, A.ind,
                           (const T *)A.val, B.ptr, B.ind, (const T *)B.val, (uint32_t)B.nnz, tile, part_p, P,
                           tcnt.as<unsigned long long>(), rdup.as<uint32_t>(), nullptr, nullptr, nullptr);
        SPAL_HIP_TRY(hipGetLastError());
    }
    SPAL_HIP_TRY(scan_two(tcnt.as<unsigned long long>(), toff.as<unsigned long long>(), P, rdup.as<uint32_t>(),
                          rscan.as<uint32_t>(), m + 1, st));
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    unsigned long long nnz = 0;
    uint32_t matched = 0;
    SPAL_HIP_TRY(hipMemcpyAsync(&nnz, toff.as<unsigned long long>() + tiles, 8, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipMemcpyAsync(&matched, rscan.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    if (nnz + matched != total)
        return fail(SPAL_ERR_HIP, "%s: internal error: %llu entries + %u matched pairs != %llu merged", fn, nnz, matched,
                    (unsigned long long)total);
    if (nnz > kMaxEntries)
        return fail(SPAL_ERR_UNSUPPORTED, "%s: the result has %llu entries, more than 32-bit device offsets address", fn, nnz);
    SPAL_TRY(out.c.alloc(m, nnz, sizeof(T), st));
    SPAL_HIP_TRY(hipEventRecord(ev.e[2], st));
    hipLaunchKernelGGL(spadd_rowptr, dim3(grid_of(m + 1, 256)), dim3(256), 0, st, A.ptr, B.ptr, rscan.as<uint32_t>(),
                       m + 1, out.c.ptr);
    if (tiles)
        hipLaunchKernelGGL((spadd_tile<T, true, SUB>), dim3((unsigned)tiles), dim3(kThreads), 0, st, A.ptr, A.ind,
                           (const T *)A.val, B.ptr, B.ind, (const T *)B.val, (uint32_t)B.nnz, tile, part_p, P, nullptr,
                           nullptr, toff.as<unsigned long long>(), out.c.ind, (T *)out.c.val);
    SPAL_HIP_TRY(hipGetLastError());
    SPAL_HIP_TRY(hipEventRecord(ev.e[3], st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    out.kernel_ms = ev.ms(2);
    out.matched = matched;
    return SPAL_OK;
}

int spadd(const char *fn, int elem_size, bool sub, const Operand &A, const Operand &B, uint32_t tile, hipStream_t st,
          Sum &out) {
    tile = tile ? tile : kTileMax;
    if (elem_size == 8)
        return sub ? spadd_t<double, true>(fn, A, B, tile, st, out) : spadd_t<double, false>(fn, A, B, tile, st, out);
    return sub ? spadd_t<float, true>(fn, A, B, tile, st, out) : spadd_t<float, false>(fn, A, B, tile, st, out);
}

// -A: the index arrays copied, the values negated
int spneg(int elem_size, const Operand &A, hipStream_t st, Sum &out) {
    const uint64_t m = A.nmajor, nnz = A.nnz;
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(1));
    SPAL_TRY(out.c.alloc(m, nnz, (size_t)elem_size, st));
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    SPAL_HIP_TRY(hipMemcpyAsync(out.c.ptr, A.ptr, (m + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (nnz) {
        SPAL_HIP_TRY(hipMemcpyAsync(out.c.ind, A.ind, nnz * 4, hipMemcpyDeviceToDevice, st));
        const uint64_t threads = nnz / (16 / elem_size) + 16 / elem_size;
        if (elem_size == 8)
            hipLaunchKernelGGL(spadd_neg<double>, dim3(grid_of(threads, 256)), dim3(256), 0, st, (const double *)A.val,
                               (double *)out.c.val, nnz);
        else
            hipLaunchKernelGGL(spadd_neg<float>, dim3(grid_of(threads, 256)), dim3(256), 0, st, (const float *)A.val,
                               (float *)out.c.val, nnz);
        SPAL_HIP_TRY(hipGetLastError());
    }
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    out.kernel_ms = ev.ms(1);
    return SPAL_OK;
}

std::string info_json(const char *op, const Sum &r, double plan_ms, double ms) {
    char buf[384];
    snprintf(buf, sizeof buf,
             "{\"op\": \"%s\", \"tile\": %u, \"tiles\": %llu, \"matched\": %llu, \"nnz\": %llu, \"kernel_ms\": %.4f, "
             "\"plan_ms\": %.3f, \"call_ms\": %.3f}",
             op, r.tile, (unsigned long long)r.tiles, (unsigned long long)r.matched, (unsigned long long)r.c.nnz,
             (double)r.kernel_ms, plan_ms, ms);
    return buf;
}

// the checks of add.rs:9-10 / sub.rs:9-10 in their order, then what the device needs
template <typename H>
int check_pair(const char *fn, const H *a, const H *b, H **out) {
    if (!a || !b || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    if (a->nrows != b->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: nrows == rhs.nrows (left: %llu, right: %llu)",
                    (unsigned long long)a->nrows, (unsigned long long)b->nrows);
    if (a->ncols != b->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: ncols == rhs.ncols (left: %llu, right: %llu)",
                    (unsigned long long)a->ncols, (unsigned long long)b->ncols);
    return check_same_device_and_dtype(fn, a, b);
}

// what every entry point ends with: a handle of a's type and shape around the result
template <typename H>
int adopt_sum(const char *op, const H *a, Sum &r, std::chrono::steady_clock::time_point t0, H **out) {
    const auto tp = std::chrono::steady_clock::now();
    // CSR: eager plan, as spal_csr_mul's result: a choice, no longer a workaround (a lazily planned handle used to reach
    // csr_blockwin_or_split re-entrantly; the planner's own launches are csr_launch_planned now).  describe()'s
    // plan_ms reports the plan's cost, and the first product of the sum pays nothing.
    SPAL_TRY(r.c.adopt(a->device, a->elem_size, a->nrows, a->ncols, out, true, false));
    (*out)->ops.spadd_info = info_json(op, r, ms_since(tp), ms_since(t0));
    return SPAL_OK;
}

template <typename H>
int binary(const char *fn, bool sub, H *a, H *b, void *stream, H **out) {
    SPAL_TRY(check_pair(fn, a, b, out));
    if (row_blocks(a) || row_blocks(b)) return refuse_row_blocks(fn);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const auto t0 = std::chrono::steady_clock::now();
    Sum r;
    SPAL_TRY(spadd(fn, a->elem_size, sub, operand_of(a), operand_of(b), a->ops.spadd_tile, (hipStream_t)stream, r));
    return adopt_sum(sub ? "sub" : "add", a, r, t0, out);
}

template <typename H>
int negate(const char *fn, H *a, void *stream, H **out) {
    if (!a || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    if (row_blocks(a)) return refuse_row_blocks(fn);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const auto t0 = std::chrono::steady_clock::now();
    Sum r;
    SPAL_TRY(spneg(a->elem_size, operand_of(a), (hipStream_t)stream, r));
    return adopt_sum("neg", a, r, t0, out);
}

}  // namespace

int spadd_option(const char *key, int64_t value, OpState &s, int *status) {
    if (strcmp(key, "spadd_tile")) return 0;
    const bool pow2 = value > 0 && (value & (value - 1)) == 0;
    *status = (value == 0 || (pow2 && value >= (int64_t)kTileMin && value <= (int64_t)kTileMax))
                  ? SPAL_OK
                  : fail(SPAL_ERR_INVALID_ARGUMENT, "spadd_tile must be 0 (default, %u) or a power of two in [%u, %u]",
                         kTileMax, kTileMin, kTileMax);
    if (*status == SPAL_OK) s.spadd_tile = (uint32_t)value;
    return 1;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_add(spal_csr_t a, spal_csr_t b, void *stream, spal_csr_t *out) {
    return binary("spal_csr_add", false, a, b, stream, out);
}
int spal_csr_sub(spal_csr_t a, spal_csr_t b, void *stream, spal_csr_t *out) {
    return binary("spal_csr_sub", true, a, b, stream, out);
}
int spal_csc_add(spal_csc_t a, spal_csc_t b, void *stream, spal_csc_t *out) {
    return binary("spal_csc_add", false, a, b, stream, out);
}
int spal_csc_sub(spal_csc_t a, spal_csc_t b, void *stream, spal_csc_t *out) {
    return binary("spal_csc_sub", true, a, b, stream, out);
}
int spal_csr_neg(spal_csr_t a, void *stream, spal_csr_t *out) { return negate("spal_csr_neg", a, stream, out); }
int spal_csc_neg(spal_csc_t a, void *stream, spal_csc_t *out) { return negate("spal_csc_neg", a, stream, out); }

}  // extern "C"
