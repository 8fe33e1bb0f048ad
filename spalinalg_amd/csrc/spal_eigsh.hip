// spal_eigsh.hip -- extreme eigenpairs of a symmetric matrix on the device: thick-restart Lanczos with full
// orthogonalisation.  The contract is the sequential text in include/spal.h; the device returns its bits in
// f32 and f64.
//
// ONE STEP IS GMRES'S INNER STEP WITHOUT THE ROTATIONS: w = A v_j, two passes of classical Gram-Schmidt against the whole
// basis (mdot / mfinish / mupdate of gmres_kernels.hpp, launched from the same text as spal_gmres.hip), hn = sqrt(dot(w, w)),
// v_{j+1} = w / hn (scale).  The step's scalar kernel (`lanczos_scalars`, one workgroup) adds c to h, stores the column of
// the projected matrix, sets hn and the flags GMRES uses: `jj`, `cyc_end` (the phase is over: ncv vectors, or hn == 0) and
// `done` (hn not finite).  Every kernel of step j returns before it writes unless the device is exactly there; nothing
// waits, nothing spins.  The host polls ONCE PER PHASE: the head and the columns of the phase come down, the projected
// problem is solved on the host in double (eigsh_host.hpp: cyclic Jacobi), and the host decides: stop, or restart.
//
// THE RESTART MOVES THE WHOLE BASIS: v_c <- sum_t Y[t, c] v_t for c < keep, ascending t, every product rounded.  Two forms
// of that rotation, the same bits:
//   rotate_lds    a workgroup stages a tile of R rows x m basis values in LDS (dynamic, up to 128 KiB of gfx950's 160 KiB),
//                 then emits all keep outputs from LDS, eight accumulators per thread and LDS read: V is read ONCE and
//                 the rotation is IN PLACE (a tile's rows are read before any of them is written, and nobody else touches
//                 them); the same launch carries v_m into v_keep.
//   rotate_batch  combine's shape: a thread keeps four rows and eight accumulators each, and walks the basis once per
//                 batch of eight outputs: V is read ceil(keep / 8) times, out of place into a second basis.
// Option "eigsh_rotate" on `a` picks one: 0 = automatic = the LDS form, which measured faster in all six cases of
// tools/bench_eigsh.py at ncv = 30 (f64: 0.102 against 0.139 ms at n = 1M, 1.00 against 1.70 ms at n = 10M; f32: 0.069
// against 0.073 and 0.66 against 0.73 ms) and needs no second basis; 1 = the batched passes.  The tile is kept
// SMALL on purpose (about 16 KiB): with tiles of 64 KiB, two workgroups per CU, the same kernel took 0.173 ms where it now
// takes 0.102 -- staging and the sums alternate inside a workgroup, and only other workgroups on the CU overlap them.  The
// Ritz vectors at the end are the same kernel writing into x (row-major, leading dimension ldx).
//
// FILTERED EIGSH (spal_*_eigsh_filtered_*) is the same Run on p(A): the step's product becomes the Chebyshev
// recurrence of spal_cheb.hip (d launches, stream-ordered), and a phase ends with the rotation FIRST and then the true
// residuals of the leading columns (one rowsum launch, two dots per column) behind a second poll.  The plain call's bits
// are untouched: the filter is a host-side branch in Run::step.
//
// EIGSH NEAR SIGMA (spal_*_eigsh_near_*) is the filtered Run again with the step's product a Chebyshev SERIES,
// the delta filter at sigma (cheb_host.hpp has its coefficients and the interval); no warm-up, the same phase end.
//
// WHAT THE THREE CALLS SHARE, each written once: `Run` (what is enqueued: start, step, the rotations), `Workspace` (every
// allocation of a run of phases and the pointers into them; `phase`: steps keep .. m, the poll, S, the projected problem;
// `restart`), `eigsh_staged` (the host form: lengths, v0 and X through device buffers on a stream of the call's own) and
// `Described` (what a describe object holds beside the public info).  What differs stays apart: `eigsh_run` decides on
// Ritz residuals and rotates only to restart; `filtered_phases` rotates first and decides on true residuals.
#include "eigsh_host.hpp"
#include "gmres_kernels.hpp"

#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr uint64_t kMaxNcv = 256;        // one column element per thread of the scalar workgroup
constexpr int kRotBatch = 8;             // outputs per accumulator batch of both rotation forms
constexpr unsigned kRotMinRows = 64;     // rows of the smallest LDS tile: one wave
constexpr size_t kRotLdsTarget = 16 * 1024;   // a tile doubles its rows while it stays within this (eight or more workgroups per CU); never below kRotMinRows rows
constexpr unsigned kRotMaxGrid = 8192;

// ---- the start vector -----------------------------------------------------------------------------------------------
// v[i] = T((mix32((i + seed) mod 2^32) >> 8) + 1) / T(2^24): exact in f32
template <typename T>
__global__ __launch_bounds__(kThreads) void default_start(T *v, uint64_t n, uint32_t seed) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads)
        v[i] = T((colour_mix32((uint32_t)i + seed) >> 8) + 1u) / T(16777216);
}

// part[tile] = the tile's sum of v[i] * v[i]
template <typename T>
__global__ __launch_bounds__(kThreads) void square_tiles(const T *v, T *part, uint64_t n, uint64_t tiles) {
    __shared__ T lds[kThreads];
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T x[4];
        load4<T>(v, i, n, x);
        const T s = tile_sum<T>(x[0] * x[0], x[1] * x[1], x[2] * x[2], x[3] * x[3], lds);
        if (threadIdx.x == 0) part[tile] = s;
    }
}

// beta = sqrt(dot(v0, v0)); jj = 0
template <typename T>
__global__ __launch_bounds__(kThreads) void start_scalars(GHead<T> *s, T *part, uint64_t c1) {
    __shared__ T lds[kThreads];
    const T vv = upper_levels<T>(part, c1, lds);
    if (threadIdx.x == 0) {
        s->beta = sqrt(vv);
        s->jj = 0;
        s->cyc_end = 0;
    }
}

// a phase begins at step `keep` (after a restart)
template <typename T>
__global__ void phase_start(GHead<T> *s, unsigned keep) {
    if (s->done != 0) return;
    s->jj = keep;
    s->cyc_end = 0;
}

// ---- the step's scalars -----------------------------------------------------------------------------------------------
// ww = dot(w, w);  h += c;  column j of the projected matrix;  hn;  the end of the phase;  jj, it
template <typename T>
__global__ __launch_bounds__(kThreads) void lanczos_scalars(GHead<T> *s, T *h, const T *c, T *H, unsigned m, unsigned j, T *part0,
                                                            uint64_t c1) {
    __shared__ T lds[kThreads];
    if (!at_step(s, j)) return;
    const T ww = upper_levels<T>(part0, c1, lds);
    const unsigned t = threadIdx.x;
    if (t <= j) {
        const T v = h[t] + c[t];
        h[t] = v;
        H[(uint64_t)j * m + t] = v;
    }
    __syncthreads();   // every thread has read the flags before thread 0 moves them
    if (t == 0) {
        const T hn = sqrt(ww);
        s->hn = hn;
        s->it += 1;
        s->jj = j + 1;
        if (!isfinite(hn)) {
            s->done = 1;
            s->reason = 2;
        } else if (hn == T(0) || j + 1 == m) {
            s->cyc_end = 1;
        }
    }
}

// ---- the rotation -----------------------------------------------------------------------------------------------------
// element (r, c) of the result at p[c * cs + r * rs]: basis vectors (cs = stride, rs = 1) or a row-major block (1, ld)
template <typename T>
struct RotOut {
    T *p;
    uint64_t cs, rs;
};

// out(r, c) = (..((Y[0, c] * v_0[r]) + (Y[1, c] * v_1[r])) ..) + (Y[m-1, c] * v_{m-1}[r]) for c < nc.  Y is m x ldy by
// rows, ldy a multiple of kRotBatch (the padding holds zeros and its results are not stored).  A tile of R rows (a power
// of two, >= 64, so a wave shares its batch of outputs) x m values is staged in LDS as lds[t * R + r], then read back
// once per batch of eight outputs.  `out` may be the basis itself: the tile's rows were all read before the barrier.
// carry_dst[r] = carry_src[r] rides along (v_keep = the old v_m; carry_dst may be one of the staged vectors).
template <typename T>
__global__ __launch_bounds__(kThreads) void rotate_lds(Basis<T> V, unsigned m, const T *__restrict__ Y, unsigned ldy, unsigned nc,
                                                       RotOut<T> out, unsigned R, unsigned logR, const T *carry_src, T *carry_dst) {
    extern __shared__ __align__(16) unsigned char rot_raw[];
    T *lds = reinterpret_cast<T *>(rot_raw);
    const uint64_t ntiles = (V.n + R - 1) / R;
    const unsigned groups = (nc + kRotBatch - 1) / kRotBatch;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t row0 = tile * R;
        const unsigned rows = (unsigned)(V.n - row0 < R ? V.n - row0 : R);
        for (unsigned e = threadIdx.x; e < m * R; e += kThreads) {
            const unsigned t = e >> logR, r = e & (R - 1);
            lds[e] = r < rows ? V.v[(uint64_t)t * V.stride + row0 + r] : T(0);
        }
        __syncthreads();
        if (carry_src)
            for (unsigned r = threadIdx.x; r < rows; r += kThreads) carry_dst[row0 + r] = carry_src[row0 + r];
        for (unsigned u = threadIdx.x; u < groups * R; u += kThreads) {
            const unsigned g = __builtin_amdgcn_readfirstlane(u >> logR), r = u & (R - 1);
            const unsigned c0 = g * kRotBatch;
            T acc[kRotBatch];
            const T *y = Y + c0;
            for (unsigned t = 0; t < m; ++t, y += ldy) {
                const T x = lds[t * R + r];
#pragma unroll
                for (int b = 0; b < kRotBatch; ++b) {
                    const T p = y[b] * x;
                    acc[b] = t == 0 ? p : acc[b] + p;
                }
            }
            if (r < rows) {
#pragma unroll
                for (int b = 0; b < kRotBatch; ++b)
                    if (c0 + b < nc) out.p[(uint64_t)(c0 + b) * out.cs + (row0 + r) * out.rs] = acc[b];
            }
        }
        __syncthreads();
    }
}

// The same sums, combine's way: a thread keeps its four rows of a tile of 1024 and eight accumulators for each, and walks
// the basis once per batch of eight outputs.  `out` must not overlap the basis.
template <typename T>
__global__ __launch_bounds__(kThreads) void rotate_batch(Basis<T> V, unsigned m, const T *__restrict__ Y, unsigned ldy, unsigned nc,
                                                         RotOut<T> out) {
    for (uint64_t tile = blockIdx.x; tile < V.tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        for (unsigned c0 = 0; c0 < nc; c0 += kRotBatch) {
            T acc[kRotBatch][4];
            const T *y = Y + c0;
            for (unsigned t = 0; t < m; ++t, y += ldy) {
                T v[4];
                load4<T>(V.v + (uint64_t)t * V.stride, i, V.n, v);
#pragma unroll
                for (int b = 0; b < kRotBatch; ++b) {
                    const T yb = y[b];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const T p = yb * v[k];
                        acc[b][k] = t == 0 ? p : acc[b][k] + p;
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < kRotBatch; ++b) {
                if (c0 + b >= nc) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint64_t e = i + (uint64_t)k * kThreads;
                    if (e < V.n) out.p[(uint64_t)(c0 + b) * out.cs + e * out.rs] = acc[b][k];
                }
            }
        }
    }
}

// rows of an LDS tile for m basis vectors of T: doubles from one wave's 64 while the doubled tile stays within the target
template <typename T>
unsigned rot_tile_rows(uint64_t m) {
    unsigned r = kRotMinRows;
    while (r < kTile && (size_t)2 * r * m * sizeof(T) <= kRotLdsTarget) r *= 2;
    return r;
}

std::atomic<uint64_t> g_lds_f64{0}, g_lds_f32{0};
template <typename T> std::atomic<uint64_t> &lds_done();
template <> std::atomic<uint64_t> &lds_done<double>() { return g_lds_f64; }
template <> std::atomic<uint64_t> &lds_done<float>() { return g_lds_f32; }

// ---- the run: what a call enqueues -------------------------------------------------------------------------------------
struct PinnedBuf {
    void *p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault); }
    template <typename U> U *as() { return reinterpret_cast<U *>(p); }
};

// the true pair of a leading column in the filtered calls: th = x . A x, res = || A x - th x ||
template <typename T>
struct TruePair {
    T th, res;
};

template <typename T>
struct Run {
    const char *fn;
    spal_csr *a;
    hipStream_t st;
    uint64_t n = 0, m = 0, c1 = 0, pe = 0, stride = 0;
    unsigned grid = 1;
    int form = 2, device = 0;
    GHead<T> *s = nullptr;
    T *h = nullptr, *c = nullptr, *H = nullptr;      // the scalar block: h, c (m + 1 each), the m x m columns
    T *basis = nullptr, *alt = nullptr, *w = nullptr, *part = nullptr, *y_dev = nullptr, *y_pin = nullptr;
    Basis<T> V;
    unsigned tile_rows = 0;
    const ChebCoeffs<T> *filter = nullptr;   // filtered eigsh: w = cheb_apply(v_j) through `work`
    T *work = nullptr;
    const ChebSeries<T> *series = nullptr;   // eigsh near sigma: w = cheb_series(v_j) through `work` and `work2`
    T *work2 = nullptr;
    int series_form = 0;
    unsigned chunk = 0;

    T *v_at(uint64_t k) const { return basis + k * stride; }

    // v_0 = v0 / sqrt(dot(v0, v0))
    int start(const T *v0, uint64_t seed) {
        if (!v0) {
            KRYLOV_LAUNCH((default_start<T>), grid, v_at(0), n, (uint32_t)seed);
            v0 = v_at(0);
        }
        KRYLOV_LAUNCH((square_tiles<T>), grid, v0, part, n, V.tiles);
        KRYLOV_LAUNCH((start_scalars<T>), 1, s, part, c1);
        KRYLOV_LAUNCH((scale<T>), grid, s, v0, v_at(0), -1, n);
        return SPAL_OK;
    }
    int step(unsigned j) {
        if (series) SPAL_TRY(cheb_series_enqueue<T>(fn, a, *series, (const T *)v_at(j), w, work, work2, chunk, series_form, st));
        else if (filter) SPAL_TRY(cheb_apply_enqueue<T>(fn, a, *filter, (const T *)v_at(j), w, work, chunk, st));
        else SPAL_TRY(mul_dev(a, (const T *)v_at(j), w, st));
        KRYLOV_LAUNCH((mdot<T>), grid, s, V, j, w, part, pe);
        KRYLOV_LAUNCH((mfinish<T>), j + 1, s, j, part, pe, c1, h);
        KRYLOV_LAUNCH((mupdate<T, false>), grid, s, V, j, h, w, part);
        KRYLOV_LAUNCH((mdot<T>), grid, s, V, j, w, part, pe);
        KRYLOV_LAUNCH((mfinish<T>), j + 1, s, j, part, pe, c1, c);
        KRYLOV_LAUNCH((mupdate<T, true>), grid, s, V, j, c, w, part);
        KRYLOV_LAUNCH((lanczos_scalars<T>), 1, s, h, c, H, (unsigned)m, j, part, c1);
        KRYLOV_LAUNCH((scale<T>), grid, s, w, v_at(j + 1), (int)j, n);
        return SPAL_OK;
    }
    // Y (jj x jj doubles by rows, its first nc columns) goes up rounded to T; out(r, c) = sum_t Y[t, c] v_t[r], t < jj
    int rotate(const RitzPairs &rp, uint64_t jj, uint64_t nc, RotOut<T> out, const T *carry_src, T *carry_dst) {
        const unsigned ldy = (unsigned)((nc + kRotBatch - 1) / kRotBatch * kRotBatch);
        for (uint64_t t = 0; t < jj; ++t)
            for (unsigned cc = 0; cc < ldy; ++cc) y_pin[t * ldy + cc] = cc < nc ? (T)rp.Y[t * jj + cc] : T(0);
        SPAL_HIP_TRY(hipMemcpyAsync(y_dev, y_pin, jj * ldy * sizeof(T), hipMemcpyHostToDevice, st));
        if (form == 1) {
            KRYLOV_LAUNCH((rotate_batch<T>), grid, V, (unsigned)jj, (const T *)y_dev, ldy, (unsigned)nc, out);
            if (carry_src) SPAL_HIP_TRY(hipMemcpyAsync(carry_dst, carry_src, n * sizeof(T), hipMemcpyDeviceToDevice, st));
            return SPAL_OK;
        }
        const unsigned R = rot_tile_rows<T>(jj);
        unsigned logR = 0;
        while ((1u << logR) < R) ++logR;
        const size_t lds_bytes = (size_t)R * jj * sizeof(T);
        if (lds_bytes > 48 * 1024)
            SPAL_HIP_TRY(lds_opt_in(reinterpret_cast<const void *>(&rotate_lds<T>), device, lds_done<T>()));
        const unsigned g = (unsigned)std::min<uint64_t>((n + R - 1) / R, kRotMaxGrid);
        tile_rows = R;
        hipLaunchKernelGGL((rotate_lds<T>), dim3(std::max(g, 1u)), dim3(kThreads), lds_bytes, st, V, (unsigned)jj, (const T *)y_dev, ldy,
                           (unsigned)nc, out, R, logR, carry_src, carry_dst);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) return fail(SPAL_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(le));
        return SPAL_OK;
    }
    // The basis becomes its own first nc rotated columns: v_c <- sum_t Y[t, c] v_t, t < jj; with `carry`, v_nc <- the old
    // v_m.  Form 1 rotates out of place, so the two bases change places; form 2 rotates where the basis is.
    int rotate_basis(const RitzPairs &rp, uint64_t jj, uint64_t nc, bool carry) {
        const T *carry_src = carry ? v_at(m) : nullptr;
        if (form != 1) return rotate(rp, jj, nc, RotOut<T>{basis, stride, 1}, carry_src, v_at(nc));
        SPAL_TRY(rotate(rp, jj, nc, RotOut<T>{alt, stride, 1}, carry_src, alt + nc * stride));
        std::swap(basis, alt);
        V.v = basis;
        return SPAL_OK;
    }
};

template <typename H>
int rotate_form_of(H *a) {
    std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
    return a->ops.eigsh_rotate ? a->ops.eigsh_rotate : 2;   // the faster one where both were measured
}

// ---- the workspace: what a run of phases owns, and the part of a phase that every call shares ---------------------------
enum class PhaseEnd { pairs_ready, device_stopped, ritz_failed };

// The vectors in one block: the basis (m + 1 vectors), w, `extra_vectors` work vectors (none for the plain product, one
// for the recurrence, two for the series) and, for the out-of-place rotation, a second basis.  The scalars in one block:
// the head, h, c, the m x m columns, then `true_pairs` TruePairs.  The host's half of the phases lives here too: S, the
// projected matrix in double, and its Ritz pairs.
template <typename T>
struct Workspace {
    DevBuf vecs, parts, scal, ydev;
    PinnedBuf hpin, ypin, tpin;
    SolveFrame<GHead<T>> F;
    EventSpans rev;   // one span for the driver: the rotation's time, or the true residuals'
    Run<T> R;
    uint64_t m = 0, basis_bytes = 0;
    size_t scal_bytes = 0;
    TruePair<T> *pairs_dev = nullptr;
    std::vector<double> S, Sw;
    RitzPairs rp;
    uint64_t keep = 0, restarts = 0, jj = 0;   // the phase runs steps keep .. m; jj vectors span the space after it

    template <typename H>
    int create(const char *fn, H *a, uint64_t ncv, int form, uint64_t extra_vectors, uint64_t true_pairs, hipStream_t st) {
        const uint64_t n = a->nrows;
        m = ncv;
        const uint64_t nvec = (m + 1) + 1 + extra_vectors + (form == 1 ? m + 1 : 0);
        const uint64_t stride = (n + 63) & ~(uint64_t)63;   // every vector on a 256-byte boundary at least
        basis_bytes = nvec * stride * sizeof(T);
        {
            const hipError_t e = vecs.alloc((size_t)basis_bytes);
            if (e == hipErrorOutOfMemory)
                return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no memory for the basis: %llu vectors of %llu elements (%llu bytes)", fn,
                            (unsigned long long)nvec, (unsigned long long)n, (unsigned long long)basis_bytes);
            SPAL_HIP_TRY(e);
        }
        const uint64_t pe = scratch_elems(n);
        SPAL_HIP_TRY(parts.alloc(std::max<uint64_t>(m, 2) * pe * sizeof(T)));
        const size_t pair_off = sizeof(GHead<T>) + (2 * (m + 1) + m * m) * sizeof(T);
        scal_bytes = pair_off + true_pairs * sizeof(TruePair<T>);
        SPAL_HIP_TRY(scal.alloc(scal_bytes));
        SPAL_HIP_TRY(ydev.alloc(m * kMaxNcv * sizeof(T)));
        SPAL_HIP_TRY(hpin.alloc(m * m * sizeof(T)));
        SPAL_HIP_TRY(ypin.alloc(m * kMaxNcv * sizeof(T)));
        if (true_pairs) SPAL_HIP_TRY(tpin.alloc(true_pairs * sizeof(TruePair<T>)));
        SPAL_TRY(F.create(st, 1));
        SPAL_HIP_TRY(rev.create(1));

        R.fn = fn;
        R.a = solve_handle(a);
        R.st = st;
        R.n = n;
        R.m = m;
        R.c1 = tiles_of(n);
        R.pe = pe;
        R.stride = stride;
        R.grid = first_level_grid(n);
        R.form = form;
        R.device = a->device;
        R.s = scal.as<GHead<T>>();
        R.h = reinterpret_cast<T *>(reinterpret_cast<char *>(scal.p) + sizeof(GHead<T>));
        R.c = R.h + (m + 1);
        R.H = R.c + (m + 1);
        pairs_dev = reinterpret_cast<TruePair<T> *>(reinterpret_cast<char *>(scal.p) + pair_off);
        R.basis = vecs.as<T>();
        R.w = R.basis + (m + 1) * stride;
        R.work = extra_vectors >= 1 ? R.w + stride : nullptr;
        R.work2 = extra_vectors >= 2 ? R.work + stride : nullptr;
        R.alt = form == 1 ? R.w + (1 + extra_vectors) * stride : nullptr;
        R.part = parts.as<T>();
        R.y_dev = ydev.as<T>();
        R.y_pin = ypin.as<T>();
        R.V.v = R.basis;
        R.V.stride = stride;
        R.V.n = n;
        R.V.tiles = tiles_of(n);
        S.assign(m * m, 0.0);
        return SPAL_OK;
    }

    // the span "solve_ms" reports begins; the scalars are zeroed and v_0 is set
    int begin(const T *v0_dev, uint64_t seed) {
        SPAL_TRY(F.begin(scal.p, scal_bytes));
        return R.start(v0_dev, seed);
    }

    // Steps keep .. m, then ONE poll: the head, and the columns with it.  S takes the new columns and the projected
    // problem is solved with `which`: rp holds the pairs, jj their number, F.h->hn the coupling.  The call ends where
    // the device stopped (F.h->reason says why) or the projected problem has no solution (the call's reason 2).
    int phase(int which, PhaseEnd *end) {
        for (uint64_t j = keep; j < m; ++j) SPAL_TRY(R.step((unsigned)j));
        SPAL_HIP_TRY(hipMemcpyAsync(hpin.p, R.H, m * m * sizeof(T), hipMemcpyDeviceToHost, R.st));
        SPAL_TRY(F.poll());
        const GHead<T> *h = F.h;
        if (h->done) {
            *end = PhaseEnd::device_stopped;
            return SPAL_OK;
        }
        if (!h->cyc_end)
            return fail(SPAL_ERR_HIP, "%s: the device did not end a phase of %llu steps", R.fn, (unsigned long long)(m - keep));
        jj = h->jj;
        const T *cols = hpin.as<T>();
        for (uint64_t j = keep; j < jj; ++j)
            for (uint64_t t = 0; t <= j; ++t) S[t * m + j] = S[j * m + t] = (double)cols[j * m + t];   // exact
        Sw.resize(jj * jj);
        for (uint64_t r = 0; r < jj; ++r)
            for (uint64_t q = 0; q < jj; ++q) Sw[r * jj + q] = S[r * m + q];
        *end = eigsh_ritz(jj, Sw.data(), (double)h->hn, which, &rp) ? PhaseEnd::pairs_ready : PhaseEnd::ritz_failed;
        return SPAL_OK;
    }

    // the next phase begins at step `kept`, on a basis that was rotated: S = diag(theta)
    int restart(uint64_t kept) {
        const char *fn = R.fn;
        hipStream_t st = R.st;
        keep = kept;
        KRYLOV_LAUNCH((phase_start<T>), 1, R.s, (unsigned)keep);
        std::fill(S.begin(), S.end(), 0.0);
        for (uint64_t i = 0; i < keep; ++i) S[i * m + i] = rp.theta[i];
        ++restarts;
        return SPAL_OK;
    }
};

// ---- the describe objects ---------------------------------------------------------------------------------------------
// What a describe object reports beside the call's arguments and its public info.  The workspace's values stay zero
// where a call ended before it had one.
struct Described {
    uint64_t keep = 0, polls = 0, basis_bytes = 0, chunk = 0;
    double phase_ms = 0.0;   // the rotations of the plain call ("rotate_ms"), the true residuals of the others ("residual_ms")
    double glo = 0.0, ghi = 0.0;
};
std::string info_json(uint64_t k, int which, uint64_t ncv, int form, unsigned tile_rows, const spal_eigsh_info &i, const Described &d) {
    char buf[640];
    snprintf(buf, sizeof buf,
             "{\"k\": %llu, \"which\": \"%s\", \"ncv\": %llu, \"keep\": %llu, \"restarts\": %llu, \"products\": %llu, "
             "\"converged\": %llu, \"reason\": %d, \"polls\": %llu, \"rotate\": \"%s\", \"rotate_tile_rows\": %u, "
             "\"basis_bytes\": %llu, \"rotate_ms\": %.4f, \"solve_ms\": %.4f}",
             (unsigned long long)k, which == SPAL_EIGSH_LA ? "LA" : "SA", (unsigned long long)ncv, (unsigned long long)d.keep,
             (unsigned long long)i.restarts, (unsigned long long)i.products, (unsigned long long)i.converged, i.reason,
             (unsigned long long)d.polls, form == 1 ? "batch" : "lds", tile_rows, (unsigned long long)d.basis_bytes, d.phase_ms,
             i.solve_ms);
    return buf;
}

// ---- plain eigsh -----------------------------------------------------------------------------------------
// The stop is decided on the Ritz residuals of the projected problem; the basis is rotated only to restart, and once more
// into x.  x_dev: n x ldx by rows, or nullptr; theta, resid: k host values
template <typename T, typename H>
int eigsh_run(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, const T *v0_dev, uint64_t seed, double tol,
              uint64_t maxit, T *theta, T *resid, T *x_dev, uint64_t ldx, hipStream_t st, spal_eigsh_info *info) {
    const uint64_t m = ncv;
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    SPAL_TRY(product_plan(solve_handle(a)));
    const int form = rotate_form_of(a);
    Workspace<T> W;
    SPAL_TRY(W.create(fn, a, m, form, 0, 0, st));
    Run<T> &R = W.R;
    const GHead<T> *h = W.F.h;   // as of the last poll
    SPAL_TRY(W.begin(v0_dev, seed));

    uint64_t conv = 0;
    int reason = 0;
    double rotate_ms = 0.0;
    bool rotating = false;
    for (;;) {
        PhaseEnd end;
        SPAL_TRY(W.phase(which, &end));
        if (rotating) {   // the poll has waited for the restart's rotation
            float ms = 0.f;
            if (W.rev.span(0, &ms) == hipSuccess) rotate_ms += ms;
            rotating = false;
        }
        if (end != PhaseEnd::pairs_ready) {
            reason = end == PhaseEnd::device_stopped ? (int)h->reason : 2;
            break;
        }
        conv = eigsh_converged(W.rp, std::min(k, W.jj), tol);
        if (h->hn == T(0)) {   // the space is exhausted: the pairs are final
            reason = W.jj >= k ? 0 : 3;
            break;
        }
        if (conv == k) {
            reason = 0;
            break;
        }
        if (W.restarts == maxit) {
            reason = 1;
            break;
        }
        const uint64_t keep = eigsh_keep(k, m);
        SPAL_HIP_TRY(hipEventRecord(W.rev.e[0], st));
        SPAL_TRY(R.rotate_basis(W.rp, m, keep, true));
        SPAL_HIP_TRY(hipEventRecord(W.rev.e[1], st));
        rotating = true;
        SPAL_TRY(W.restart(keep));
    }
    const uint64_t nk = reason == 2 ? 0 : std::min(k, W.jj);
    if (nk && x_dev) SPAL_TRY(R.rotate(W.rp, W.jj, nk, RotOut<T>{x_dev, 1, ldx}, nullptr, nullptr));
    float ms = 0.f;
    SPAL_TRY(W.F.end(&ms));
    for (uint64_t i = 0; i < nk; ++i) {
        theta[i] = (T)W.rp.theta[i];
        resid[i] = (T)W.rp.res[i];
    }
    info->restarts = W.restarts;
    info->products = h->it;
    info->converged = reason == 2 ? 0 : conv;
    info->reason = reason;
    info->solve_ms = (double)ms;
    Described d;
    d.keep = eigsh_keep(k, m);
    d.polls = W.F.polls;
    d.basis_bytes = W.basis_bytes;
    d.phase_ms = rotate_ms;
    store_info(a, &OpState::eigsh_info, info_json(k, which, ncv, form, form == 1 ? 0 : rot_tile_rows<T>(m), *info, d));
    return SPAL_OK;
}

// Every refusal that needs no device.  What needs nothing of the handle comes first.
template <typename T, typename H>
int eigsh_check(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, double tol, T *theta, T *resid, const T *x, uint64_t ldx,
                spal_eigsh_info *info) {
    if (!a || !theta || !resid || !info) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (k == 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: k = 0 (at least one eigenpair)", fn);
    if (ncv <= k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ncv = %llu must be greater than k = %llu", fn, (unsigned long long)ncv,
                    (unsigned long long)k);
    if (ncv > kMaxNcv)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ncv = %llu must be at most %llu (one column element per thread of the scalar workgroup)",
                    fn, (unsigned long long)ncv, (unsigned long long)kMaxNcv);
    if (which != SPAL_EIGSH_LA && which != SPAL_EIGSH_SA)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: which = %d must be 0 (LA) or 1 (SA)", fn, which);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: tol = %g must be finite and >= 0", fn, tol);
    if (x && ldx < k)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ldx = %llu is less than k = %llu", fn, (unsigned long long)ldx, (unsigned long long)k);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn, (unsigned long long)a->nrows,
                    (unsigned long long)a->ncols);
    if (ncv > a->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: ncv = %llu exceeds the matrix's %llu rows", fn, (unsigned long long)ncv,
                    (unsigned long long)a->nrows);
    if (row_blocks(a)) return refuse_row_blocks(fn);
    return SPAL_OK;
}

// The host form of all three calls, after the call's own check: the lengths, the device, v0 and X staged on a stream of
// the call's own, `run(v0_dev, x_dev, ldx = k, stream)`, and the columns the call produced copied back -- only those:
// reason 2 leaves X as it was, reason 3 has `converged` = jj < k pairs.
template <typename T, typename H, typename Info, typename Call>
int eigsh_staged(const char *fn, H *a, uint64_t k, const T *v0, uint64_t v0_len, uint64_t theta_len, uint64_t resid_len, T *x,
                 uint64_t ldx, uint64_t x_rows, const Info *info, Call run) {
    const uint64_t n = a->nrows;
    if ((v0 && v0_len != n) || theta_len != k || resid_len != k || (x && x_rows != n))
        return fail(SPAL_ERR_INVALID_ARGUMENT,
                    "%s: v0.len() = %llu and X has %llu rows but the matrix has %llu rows; theta.len() = %llu and resid.len() = %llu but "
                    "k = %llu", fn, (unsigned long long)v0_len, (unsigned long long)x_rows, (unsigned long long)n,
                    (unsigned long long)theta_len, (unsigned long long)resid_len, (unsigned long long)k);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    size_t bytes = 0;
    if (!bytes_of(n, k, sizeof(T), 1, &bytes))
        return fail(SPAL_ERR_OUT_OF_MEMORY, "%s: no room for a block of %llu x %llu", fn, (unsigned long long)n, (unsigned long long)k);
    const size_t row = (size_t)k * sizeof(T);
    DevBuf dv, dx;
    PooledStream ps;   // a stream of the call's own
    if (v0) SPAL_HIP_TRY(dv.alloc(n * sizeof(T)));
    if (x) SPAL_HIP_TRY(dx.alloc(bytes));
    SPAL_HIP_TRY(stream_acquire(&ps.s));
    if (v0) SPAL_HIP_TRY(hipMemcpyAsync(dv.p, v0, n * sizeof(T), hipMemcpyHostToDevice, ps.s));
    SPAL_TRY(run(v0 ? (const T *)dv.p : nullptr, x ? dx.as<T>() : nullptr, k, ps.s));
    const uint64_t got = info->reason == 2 ? 0 : info->reason == 3 ? info->converged : k;
    if (x && got) {
        SPAL_HIP_TRY(hipMemcpy2DAsync(x, (size_t)ldx * sizeof(T), dx.p, row, (size_t)got * sizeof(T), n, hipMemcpyDeviceToHost, ps.s));
        SPAL_HIP_TRY(hipStreamSynchronize(ps.s));
    }
    return SPAL_OK;
}

template <typename T, typename H>
int eigsh_dev(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, const T *v0_dev, uint64_t seed, double tol, uint64_t maxit,
              T *theta, T *resid, T *x_dev, uint64_t ldx, void *stream, spal_eigsh_info *info) {
    SPAL_TRY((eigsh_check<T, H>(fn, a, k, which, ncv, tol, theta, resid, x_dev, ldx, info)));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return eigsh_run<T, H>(fn, a, k, which, ncv, v0_dev, seed, tol, maxit, theta, resid, x_dev, ldx, (hipStream_t)stream, info);
}

template <typename T, typename H>
int eigsh_host(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, const T *v0, uint64_t v0_len, uint64_t seed, double tol,
               uint64_t maxit, T *theta, uint64_t theta_len, T *resid, uint64_t resid_len, T *x, uint64_t ldx, uint64_t x_rows,
               spal_eigsh_info *info) {
    SPAL_TRY((eigsh_check<T, H>(fn, a, k, which, ncv, tol, theta, resid, x, ldx, info)));
    return eigsh_staged<T>(fn, a, k, v0, v0_len, theta_len, resid_len, x, ldx, x_rows, info,
                           [&](const T *v0_dev, T *x_dev, uint64_t ld, hipStream_t st) {
                               return eigsh_run<T, H>(fn, a, k, which, ncv, v0_dev, seed, tol, maxit, theta, resid, x_dev, ld, st, info);
                           });
}


// ---- filtered eigsh ---------------------------------------------------------------------------------------
// Lanczos on p(A), a Chebyshev polynomial of A (spal_cheb.hip): the step above with w = cheb_apply(v_j).  The projected
// problem then holds values of p, so convergence is decided on TRUE residuals with A: at a phase end the host rotates
// first (the columns are the restart's), then per leading column one product, two dots and two scalar launches, and a
// second poll brings the nk pairs (th, res) down.

// part[tile] = the tile's sum of a[i] * b[i]
template <typename T>
__global__ __launch_bounds__(kThreads) void dot_tiles(const T *a, const T *b, T *part, uint64_t n, uint64_t tiles) {
    __shared__ T lds[kThreads];
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T x[4], y[4];
        load4<T>(a, i, n, x);
        load4<T>(b, i, n, y);
        const T s = tile_sum<T>(x[0] * y[0], x[1] * y[1], x[2] * y[2], x[3] * y[3], lds);
        if (threadIdx.x == 0) part[tile] = s;
    }
}

// part[tile] = the tile's sum of r[i] * r[i], r[i] = q[i] - (th * x[i]); the padding is +0.0 whatever th is
template <typename T>
__global__ __launch_bounds__(kThreads) void resid_tiles(const T *q, const T *x, const T *th_p, T *part, uint64_t n, uint64_t tiles) {
    __shared__ T lds[kThreads];
    const T th = *th_p;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTile + threadIdx.x;
        T p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t e = i + (uint64_t)k * kThreads;
            T r = T(0);
            if (e < n) r = q[e] - (th * x[e]);
            p[k] = r * r;
        }
        const T s = tile_sum<T>(p[0], p[1], p[2], p[3], lds);
        if (threadIdx.x == 0) part[tile] = s;
    }
}

// *dst = the dot whose first level is in part (ROOT: its square root)
template <typename T, bool ROOT>
__global__ __launch_bounds__(kThreads) void finish_dot(T *part, uint64_t c1, T *dst) {
    __shared__ T lds[kThreads];
    const T d = upper_levels<T>(part, c1, lds);
    if (threadIdx.x == 0) *dst = ROOT ? sqrt(d) : d;
}

// x[i * ldx + c] = v_c[i] for c < nc
template <typename T>
__global__ __launch_bounds__(kThreads) void columns_out(Basis<T> V, unsigned nc, T *x, uint64_t ldx) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < V.n; i += (uint64_t)gridDim.x * kThreads)
        for (unsigned c = 0; c < nc; ++c) x[i * ldx + c] = V.v[(uint64_t)c * V.stride + i];
}

// a double as JSON: a value that is not finite (Gershgorin's bounds of a matrix that holds one) is null
std::string json_number(double v) {
    if (!std::isfinite(v)) return "null";
    char buf[40];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}
std::string filter_json(uint64_t k, int which, uint64_t ncv, int automatic, const spal_eigsh_filter_info &i, const Described &d) {
    char buf[1280];
    snprintf(buf, sizeof buf,
             "{\"k\": %llu, \"which\": \"%s\", \"ncv\": %llu, \"keep\": %llu, \"degree\": %llu, \"interval\": \"%s\", \"lo\": %s, "
             "\"hi\": %s, \"a0\": %s, \"glo\": %s, \"ghi\": %s, \"warm_restarts\": %llu, \"warm_products\": %llu, "
             "\"restarts\": %llu, \"products\": %llu, \"converged\": %llu, \"reason\": %d, \"polls\": %llu, \"chunk\": %llu, "
             "\"basis_bytes\": %llu, \"residual_ms\": %.4f, \"solve_ms\": %.4f}",
             (unsigned long long)k, which == SPAL_EIGSH_LA ? "LA" : "SA", (unsigned long long)ncv, (unsigned long long)d.keep,
             (unsigned long long)i.degree, automatic ? "auto" : "given", json_number(i.lo).c_str(), json_number(i.hi).c_str(),
             json_number(i.a0).c_str(), json_number(d.glo).c_str(), json_number(d.ghi).c_str(),
             (unsigned long long)i.warm_restarts, (unsigned long long)i.warm_products, (unsigned long long)i.restarts,
             (unsigned long long)i.products, (unsigned long long)i.converged, i.reason, (unsigned long long)d.polls,
             (unsigned long long)d.chunk, (unsigned long long)d.basis_bytes, d.phase_ms, i.solve_ms);
    return buf;
}

template <typename H>
unsigned cheb_chunk_of(H *a) {
    std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
    return (unsigned)a->ops.cheb_chunk;
}

// The filtered phases; `info` (the filtered call's or the near call's) may hold a warm-up's solve_ms already.  The step's
// product is the recurrence with `coef`, or, where `series` is given (eigsh near sigma), the series with its coefficients
// in the form `series_form`.  The projected problem holds values of the polynomial, which is largest at the wanted end:
// its pairs are taken descending, and the stop is decided on the true pairs, behind the phase's second poll.
template <typename T, typename H, typename Info>
int filtered_phases(const char *fn, H *a, uint64_t k, uint64_t ncv, const T *v0_dev, uint64_t seed, double tol_scale, uint64_t maxit,
                    const ChebCoeffs<T> *coef, const ChebSeries<T> *series, int series_form, T *theta, T *resid, T *x_dev,
                    uint64_t ldx, hipStream_t st, Info *info, Described *d) {
    const uint64_t n = a->nrows, m = ncv, degree = series ? series->k.size() - 1 : coef->alpha.size();
    Workspace<T> W;
    SPAL_TRY(W.create(fn, a, m, rotate_form_of(a), series ? 2 : 1, k, st));
    Run<T> &R = W.R;
    R.filter = coef;
    R.series = series;
    R.series_form = series_form;
    R.chunk = cheb_chunk_of(a);
    const GHead<T> *h = W.F.h;   // as of the last poll
    TruePair<T> *pairs_dev = W.pairs_dev;
    const TruePair<T> *pairs = W.tpin.template as<TruePair<T>>();
    SPAL_TRY(W.begin(v0_dev, seed));

    uint64_t conv = 0, nk = 0, true_products = 0;
    int reason = 0;
    double residual_ms = 0.0;
    for (;;) {
        PhaseEnd end;
        SPAL_TRY(W.phase(SPAL_EIGSH_LA, &end));
        if (end != PhaseEnd::pairs_ready) {
            reason = end == PhaseEnd::device_stopped ? (int)h->reason : 2;
            break;
        }
        const bool exhausted = h->hn == T(0);
        nk = std::min(k, W.jj);
        const uint64_t kc = std::min(eigsh_keep(k, m), W.jj);
        // rotate first: x_c = the new v_c, and a restart goes on from these columns
        SPAL_TRY(R.rotate_basis(W.rp, W.jj, kc, !exhausted));
        SPAL_HIP_TRY(hipEventRecord(W.rev.e[0], st));
        for (uint64_t c = 0; c < nk; ++c) {
            SPAL_TRY(cheb_rowsum_enqueue<T>(fn, R.a, (const T *)R.v_at(c), R.w, R.chunk, st));
            KRYLOV_LAUNCH((dot_tiles<T>), R.grid, (const T *)R.v_at(c), (const T *)R.w, R.part, n, R.V.tiles);
            KRYLOV_LAUNCH((finish_dot<T, false>), 1, R.part, R.c1, &pairs_dev[c].th);
            KRYLOV_LAUNCH((resid_tiles<T>), R.grid, (const T *)R.w, (const T *)R.v_at(c), (const T *)&pairs_dev[c].th, R.part, n, R.V.tiles);
            KRYLOV_LAUNCH((finish_dot<T, true>), 1, R.part, R.c1, &pairs_dev[c].res);
        }
        true_products += nk;
        SPAL_HIP_TRY(hipEventRecord(W.rev.e[1], st));
        SPAL_HIP_TRY(hipMemcpyAsync(W.tpin.p, pairs_dev, nk * sizeof(TruePair<T>), hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));   // the second poll: the true pairs
        ++W.F.polls;
        {
            float ms = 0.f;
            if (W.rev.span(0, &ms) == hipSuccess) residual_ms += ms;
        }
        bool finite = true;
        for (uint64_t c = 0; c < nk; ++c) finite = finite && std::isfinite((double)pairs[c].th) && std::isfinite((double)pairs[c].res);
        if (!finite) {
            reason = 2;
            break;
        }
        conv = 0;
        while (conv < nk && (double)pairs[conv].res <= tol_scale) ++conv;
        if (exhausted) {   // the space is exhausted: the pairs are final
            reason = W.jj >= k ? 0 : 3;
            if (reason == 3) conv = nk;
            break;
        }
        if (conv == k) {
            reason = 0;
            break;
        }
        if (W.restarts == maxit) {
            reason = 1;
            break;
        }
        SPAL_TRY(W.restart(kc));
    }
    if (reason == 2) nk = 0;
    if (nk && x_dev) KRYLOV_LAUNCH((columns_out<T>), R.grid, R.V, (unsigned)nk, x_dev, ldx);
    float ms = 0.f;
    SPAL_TRY(W.F.end(&ms));
    for (uint64_t i = 0; i < nk; ++i) {
        theta[i] = pairs[i].th;
        resid[i] = pairs[i].res;
    }
    info->restarts = W.restarts;
    info->products = h->it * degree + true_products;
    info->converged = reason == 2 ? 0 : conv;
    info->reason = reason;
    info->solve_ms += (double)ms;
    d->keep = eigsh_keep(k, m);
    d->polls = W.F.polls;
    d->basis_bytes = W.basis_bytes;
    d->chunk = R.chunk;
    d->phase_ms = residual_ms;
    return SPAL_OK;
}

// x_dev: n x ldx by rows, or nullptr; theta, resid: k host values
template <typename T, typename H>
int eigsh_filtered_run(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, const T *v0_dev, uint64_t seed, double tol,
                       uint64_t maxit, uint64_t degree, int automatic, double lo, double hi, uint64_t warmup, T *theta, T *resid,
                       T *x_dev, uint64_t ldx, hipStream_t st, spal_eigsh_filter_info *fi) {
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    SPAL_TRY(product_plan(solve_handle(a)));
    *fi = spal_eigsh_filter_info{};
    fi->degree = degree;
    tol = cheb_tol<T>(tol);
    Described d;
    SPAL_TRY(gershgorin_run(fn, solve_handle(a), st, &d.glo, &d.ghi));
    auto finish = [&]() {
        store_info(a, &OpState::eigsh_filter_info, filter_json(k, which, ncv, automatic, *fi, d));
        return SPAL_OK;
    };
    if (!std::isfinite(d.glo) || !std::isfinite(d.ghi)) {   // a value of the matrix is not finite
        fi->a0 = (double)NAN;
        fi->reason = 2;
        return finish();
    }
    const double a0 = cheb_a0(which, d.glo, d.ghi);
    fi->a0 = a0;
    if (automatic) {
        spal_eigsh_info warm;
        SPAL_TRY((eigsh_run<T, H>(fn, a, k, which, ncv, v0_dev, seed, tol, std::min(warmup, maxit), theta, resid, x_dev, ldx, st, &warm)));
        fi->warm_restarts = fi->restarts = warm.restarts;
        fi->warm_products = fi->products = warm.products;
        fi->converged = warm.converged;
        fi->reason = warm.reason;
        fi->solve_ms = warm.solve_ms;
        if (warm.reason != 1) return finish();
        if (!cheb_auto_interval(which, d.glo, d.ghi, (double)theta[k - 1], &lo, &hi)) return finish();
    } else if (cheb_check(degree, lo, hi, a0) != CHEB_OK || !cheb_wanted_side(which, lo, hi, a0)) {
        return fail(SPAL_ERR_INVALID_ARGUMENT,
                    "%s: a0 = %.17g (Gershgorin's %s bound) must lie strictly %s the interval [%.17g, %.17g]", fn, a0,
                    which == SPAL_EIGSH_LA ? "upper" : "lower", which == SPAL_EIGSH_LA ? "above" : "below", lo, hi);
    }
    fi->lo = lo;
    fi->hi = hi;
    const ChebCoeffs<T> coef = cheb_coefficients<T>(degree, lo, hi, a0);
    SPAL_TRY((filtered_phases<T, H>(fn, a, k, ncv, v0_dev, seed, tol * cheb_scale(d.glo, d.ghi), maxit, &coef,
                                    (const ChebSeries<T> *)nullptr, 0, theta, resid, x_dev, ldx, st, fi, &d)));
    return finish();
}

template <typename T, typename H>
int eigsh_filtered_check(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, double tol, uint64_t degree, int automatic,
                         double lo, double hi, T *theta, T *resid, const T *x, uint64_t ldx, spal_eigsh_filter_info *fi) {
    if (!fi) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (degree < 1 || degree > kChebMaxDegree)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: degree = %llu must be 1 .. %llu", fn, (unsigned long long)degree,
                    (unsigned long long)kChebMaxDegree);
    if (automatic != 0 && automatic != 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: auto = %d must be 0 or 1", fn, automatic);
    if (!automatic && (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the interval [%g, %g] must be finite with lo < hi", fn, lo, hi);
    spal_eigsh_info plain;
    return eigsh_check<T, H>(fn, a, k, which, ncv, tol, theta, resid, x, ldx, &plain);
}

template <typename T, typename H>
int eigsh_filtered_dev(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, const T *v0_dev, uint64_t seed, double tol,
                       uint64_t maxit, uint64_t degree, int automatic, double lo, double hi, uint64_t warmup, T *theta, T *resid,
                       T *x_dev, uint64_t ldx, void *stream, spal_eigsh_filter_info *fi) {
    SPAL_TRY((eigsh_filtered_check<T, H>(fn, a, k, which, ncv, tol, degree, automatic, lo, hi, theta, resid, x_dev, ldx, fi)));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return eigsh_filtered_run<T, H>(fn, a, k, which, ncv, v0_dev, seed, tol, maxit, degree, automatic, lo, hi, warmup, theta, resid,
                                    x_dev, ldx, (hipStream_t)stream, fi);
}

template <typename T, typename H>
int eigsh_filtered_host(const char *fn, H *a, uint64_t k, int which, uint64_t ncv, const T *v0, uint64_t v0_len, uint64_t seed,
                        double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi, uint64_t warmup, T *theta,
                        uint64_t theta_len, T *resid, uint64_t resid_len, T *x, uint64_t ldx, uint64_t x_rows,
                        spal_eigsh_filter_info *fi) {
    SPAL_TRY((eigsh_filtered_check<T, H>(fn, a, k, which, ncv, tol, degree, automatic, lo, hi, theta, resid, x, ldx, fi)));
    return eigsh_staged<T>(fn, a, k, v0, v0_len, theta_len, resid_len, x, ldx, x_rows, fi,
                           [&](const T *v0_dev, T *x_dev, uint64_t ld, hipStream_t st) {
                               return eigsh_filtered_run<T, H>(fn, a, k, which, ncv, v0_dev, seed, tol, maxit, degree, automatic, lo, hi,
                                                               warmup, theta, resid, x_dev, ld, st, fi);
                           });
}

// ---- eigsh near sigma -------------------------------------------------------------------------------------
// The filtered phases on rho(A), the Fejer-damped delta function at sigma as a Chebyshev series (spal_cheb.hip): no
// warm-up, the interval is Gershgorin's with a margin or the caller's, everything else is the filtered call's.
std::string near_json(uint64_t k, uint64_t ncv, int automatic, int series_form, const spal_eigsh_near_info &i, const Described &d) {
    char buf[1280];
    snprintf(buf, sizeof buf,
             "{\"k\": %llu, \"sigma\": %s, \"gamma\": %s, \"ncv\": %llu, \"keep\": %llu, \"degree\": %llu, \"interval\": \"%s\", "
             "\"lo\": %s, \"hi\": %s, \"glo\": %s, \"ghi\": %s, \"restarts\": %llu, \"products\": %llu, \"converged\": %llu, "
             "\"reason\": %d, \"polls\": %llu, \"chunk\": %llu, \"form\": \"%s\", \"basis_bytes\": %llu, \"residual_ms\": %.4f, "
             "\"solve_ms\": %.4f}",
             (unsigned long long)k, json_number(i.sigma).c_str(), json_number(i.gamma).c_str(), (unsigned long long)ncv,
             (unsigned long long)d.keep, (unsigned long long)i.degree, automatic ? "auto" : "given", json_number(i.lo).c_str(),
             json_number(i.hi).c_str(), json_number(d.glo).c_str(), json_number(d.ghi).c_str(), (unsigned long long)i.restarts,
             (unsigned long long)i.products, (unsigned long long)i.converged, i.reason, (unsigned long long)d.polls,
             (unsigned long long)d.chunk, series_form == 2 ? "unfused" : "fused", (unsigned long long)d.basis_bytes, d.phase_ms,
             i.solve_ms);
    return buf;
}

// x_dev: n x ldx by rows, or nullptr; theta, resid: k host values
template <typename T, typename H>
int eigsh_near_run(const char *fn, H *a, uint64_t k, double sigma, uint64_t ncv, const T *v0_dev, uint64_t seed, double tol,
                   uint64_t maxit, uint64_t degree, int automatic, double lo, double hi, T *theta, T *resid, T *x_dev, uint64_t ldx,
                   hipStream_t st, spal_eigsh_near_info *ni) {
    SPAL_TRY(refuse_capture(fn, st, "the call polls and synchronises"));
    *ni = spal_eigsh_near_info{};
    ni->degree = degree;
    ni->sigma = sigma;
    tol = cheb_tol<T>(tol);
    Described d;
    SPAL_TRY(gershgorin_run(fn, solve_handle(a), st, &d.glo, &d.ghi));
    int series_form = 0;
    {
        std::lock_guard<std::mutex> lock(solve_handle(a)->mu);
        series_form = a->ops.cheb_series_form;
    }
    auto finish = [&]() {
        store_info(a, &OpState::eigsh_near_info, near_json(k, ncv, automatic, series_form, *ni, d));
        return SPAL_OK;
    };
    if (!std::isfinite(d.glo) || !std::isfinite(d.ghi)) {   // a value of the matrix is not finite
        ni->reason = 2;
        return finish();
    }
    if (automatic) cheb_near_auto_interval(d.glo, d.ghi, &lo, &hi);
    std::vector<double> coef(degree + 1);
    double gamma = 0.0;
    const ChebSeriesRefusal r = cheb_near_filter(degree, sigma, lo, hi, &gamma, coef.data());
    if (r != CHEB_SERIES_OK)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: %s (sigma = %.17g, the interval [%.17g, %.17g]%s)", fn, cheb_series_refusal_text(r),
                    sigma, lo, hi, automatic ? ", Gershgorin's with its margin" : "");
    ni->lo = lo;
    ni->hi = hi;
    ni->gamma = gamma;
    const ChebSeries<T> series = cheb_series_scalars<T>(lo, hi, coef.data(), coef.size());
    SPAL_TRY((filtered_phases<T, H>(fn, a, k, ncv, v0_dev, seed, tol * cheb_scale(d.glo, d.ghi), maxit, (const ChebCoeffs<T> *)nullptr,
                                    &series, series_form, theta, resid, x_dev, ldx, st, ni, &d)));
    return finish();
}

template <typename T, typename H>
int eigsh_near_check(const char *fn, H *a, uint64_t k, double sigma, uint64_t ncv, double tol, uint64_t degree, int automatic,
                     double lo, double hi, T *theta, T *resid, const T *x, uint64_t ldx, spal_eigsh_near_info *ni) {
    if (!ni) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (automatic != 0 && automatic != 1) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: auto = %d must be 0 or 1", fn, automatic);
    const ChebSeriesRefusal r = cheb_near_check(degree, sigma, automatic, lo, hi);
    if (r != CHEB_SERIES_OK)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: %s (degree = %llu, sigma = %g, the interval [%g, %g])", fn,
                    cheb_series_refusal_text(r), (unsigned long long)degree, sigma, lo, hi);
    spal_eigsh_info plain;
    return eigsh_check<T, H>(fn, a, k, SPAL_EIGSH_LA, ncv, tol, theta, resid, x, ldx, &plain);
}

template <typename T, typename H>
int eigsh_near_dev(const char *fn, H *a, uint64_t k, double sigma, uint64_t ncv, const T *v0_dev, uint64_t seed, double tol,
                   uint64_t maxit, uint64_t degree, int automatic, double lo, double hi, T *theta, T *resid, T *x_dev, uint64_t ldx,
                   void *stream, spal_eigsh_near_info *ni) {
    SPAL_TRY((eigsh_near_check<T, H>(fn, a, k, sigma, ncv, tol, degree, automatic, lo, hi, theta, resid, x_dev, ldx, ni)));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    return eigsh_near_run<T, H>(fn, a, k, sigma, ncv, v0_dev, seed, tol, maxit, degree, automatic, lo, hi, theta, resid, x_dev, ldx,
                                (hipStream_t)stream, ni);
}

template <typename T, typename H>
int eigsh_near_host(const char *fn, H *a, uint64_t k, double sigma, uint64_t ncv, const T *v0, uint64_t v0_len, uint64_t seed,
                    double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi, T *theta, uint64_t theta_len,
                    T *resid, uint64_t resid_len, T *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_near_info *ni) {
    SPAL_TRY((eigsh_near_check<T, H>(fn, a, k, sigma, ncv, tol, degree, automatic, lo, hi, theta, resid, x, ldx, ni)));
    return eigsh_staged<T>(fn, a, k, v0, v0_len, theta_len, resid_len, x, ldx, x_rows, ni,
                           [&](const T *v0_dev, T *x_dev, uint64_t ld, hipStream_t st) {
                               return eigsh_near_run<T, H>(fn, a, k, sigma, ncv, v0_dev, seed, tol, maxit, degree, automatic, lo, hi,
                                                           theta, resid, x_dev, ld, st, ni);
                           });
}


}  // namespace

int eigsh_option(spal_csr *a, const char *key, int64_t value, OpState &s, int *status) {
    if (strcmp(key, "eigsh_rotate")) return 0;
    if (value < 0 || value > 2) {
        *status = fail(SPAL_ERR_INVALID_ARGUMENT, "eigsh_rotate must be 0 (automatic), 1 (batched passes) or 2 (LDS row tiles)");
        return 1;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    s.eigsh_rotate = (int)value;
    *status = SPAL_OK;
    return 1;
}

int eigsh_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    return info_describe_append(buf, buf_len, s, solve, "eigsh", &OpState::eigsh_info);
}

int eigsh_filter_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    return info_describe_append(buf, buf_len, s, solve, "eigsh_filter", &OpState::eigsh_filter_info);
}

int eigsh_near_describe_append(char *buf, size_t buf_len, const OpState &s, spal_csr *solve) {
    return info_describe_append(buf, buf_len, s, solve, "eigsh_near", &OpState::eigsh_near_info);
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_eigsh_jacobi(uint64_t m, const double *s, double *theta, double *y, uint64_t *sweeps) {
    if (!s || !theta || !y) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_eigsh_jacobi: null argument");
    if (m == 0 || m > kMaxNcv)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_eigsh_jacobi: m = %llu must be 1 .. %llu", (unsigned long long)m,
                    (unsigned long long)kMaxNcv);
    std::vector<double> w(s, s + m * m);
    for (uint64_t i = 0; i < m; ++i)
        for (uint64_t j = 0; j < m; ++j)
            if (!std::isfinite(w[i * m + j]) || w[i * m + j] != w[j * m + i])
                return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_eigsh_jacobi: S[%llu, %llu] is not finite or S is not symmetric",
                            (unsigned long long)i, (unsigned long long)j);
    const unsigned n = eigsh_jacobi(m, w.data(), y);
    for (uint64_t i = 0; i < m; ++i) theta[i] = w[i * m + i];
    if (sweeps) *sweeps = n;
    return SPAL_OK;
}

#define SPAL_EIGSH_ENTRIES(kind, sfx, T)                                                                               \
    int spal_##kind##_eigsh_##sfx(spal_##kind##_t a, uint64_t k, int which, uint64_t ncv, const T *v0, uint64_t v0_len, \
                                  uint64_t seed, double tol, uint64_t maxit, T *theta, uint64_t theta_len, T *resid,   \
                                  uint64_t resid_len, T *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_info *info) {    \
        return eigsh_host<T, spal_##kind>("spal_" #kind "_eigsh", a, k, which, ncv, v0, v0_len, seed, tol, maxit,      \
                                          theta, theta_len, resid, resid_len, x, ldx, x_rows, info);                   \
    }                                                                                                                  \
    int spal_##kind##_eigsh_dev_##sfx(spal_##kind##_t a, uint64_t k, int which, uint64_t ncv, const T *v0_dev,         \
                                      uint64_t seed, double tol, uint64_t maxit, T *theta, T *resid, T *x_dev,         \
                                      uint64_t ldx, void *stream, spal_eigsh_info *info) {                             \
        return eigsh_dev<T, spal_##kind>("spal_" #kind "_eigsh_dev", a, k, which, ncv, v0_dev, seed, tol, maxit,       \
                                         theta, resid, x_dev, ldx, stream, info);                                      \
    }
SPAL_EIGSH_ENTRIES(csr, f64, double)
SPAL_EIGSH_ENTRIES(csr, f32, float)
SPAL_EIGSH_ENTRIES(csc, f64, double)
SPAL_EIGSH_ENTRIES(csc, f32, float)
#undef SPAL_EIGSH_ENTRIES

#define SPAL_EIGSH_FILTERED_ENTRIES(kind, sfx, T)                                                                          \
    int spal_##kind##_eigsh_filtered_##sfx(spal_##kind##_t a, uint64_t k, int which, uint64_t ncv, const T *v0,             \
                                           uint64_t v0_len, uint64_t seed, double tol, uint64_t maxit, uint64_t degree,     \
                                           int automatic, double lo, double hi, uint64_t warmup, T *theta,                  \
                                           uint64_t theta_len, T *resid, uint64_t resid_len, T *x, uint64_t ldx,            \
                                           uint64_t x_rows, spal_eigsh_filter_info *info) {                                 \
        return eigsh_filtered_host<T, spal_##kind>("spal_" #kind "_eigsh_filtered", a, k, which, ncv, v0, v0_len, seed,     \
                                                   tol, maxit, degree, automatic, lo, hi, warmup, theta, theta_len, resid,  \
                                                   resid_len, x, ldx, x_rows, info);                                        \
    }                                                                                                                       \
    int spal_##kind##_eigsh_filtered_dev_##sfx(spal_##kind##_t a, uint64_t k, int which, uint64_t ncv, const T *v0_dev,     \
                                               uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic,   \
                                               double lo, double hi, uint64_t warmup, T *theta, T *resid, T *x_dev,         \
                                               uint64_t ldx, void *stream, spal_eigsh_filter_info *info) {                  \
        return eigsh_filtered_dev<T, spal_##kind>("spal_" #kind "_eigsh_filtered_dev", a, k, which, ncv, v0_dev, seed,      \
                                                  tol, maxit, degree, automatic, lo, hi, warmup, theta, resid, x_dev, ldx,  \
                                                  stream, info);                                                            \
    }
SPAL_EIGSH_FILTERED_ENTRIES(csr, f64, double)
SPAL_EIGSH_FILTERED_ENTRIES(csr, f32, float)
SPAL_EIGSH_FILTERED_ENTRIES(csc, f64, double)
SPAL_EIGSH_FILTERED_ENTRIES(csc, f32, float)
#undef SPAL_EIGSH_FILTERED_ENTRIES

#define SPAL_EIGSH_NEAR_ENTRIES(kind, sfx, T)                                                                              \
    int spal_##kind##_eigsh_near_##sfx(spal_##kind##_t a, uint64_t k, double sigma, uint64_t ncv, const T *v0,              \
                                       uint64_t v0_len, uint64_t seed, double tol, uint64_t maxit, uint64_t degree,         \
                                       int automatic, double lo, double hi, T *theta, uint64_t theta_len, T *resid,         \
                                       uint64_t resid_len, T *x, uint64_t ldx, uint64_t x_rows,                             \
                                       spal_eigsh_near_info *info) {                                                        \
        return eigsh_near_host<T, spal_##kind>("spal_" #kind "_eigsh_near", a, k, sigma, ncv, v0, v0_len, seed, tol, maxit, \
                                               degree, automatic, lo, hi, theta, theta_len, resid, resid_len, x, ldx,       \
                                               x_rows, info);                                                               \
    }                                                                                                                       \
    int spal_##kind##_eigsh_near_dev_##sfx(spal_##kind##_t a, uint64_t k, double sigma, uint64_t ncv, const T *v0_dev,      \
                                           uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic,       \
                                           double lo, double hi, T *theta, T *resid, T *x_dev, uint64_t ldx, void *stream,  \
                                           spal_eigsh_near_info *info) {                                                    \
        return eigsh_near_dev<T, spal_##kind>("spal_" #kind "_eigsh_near_dev", a, k, sigma, ncv, v0_dev, seed, tol, maxit,  \
                                              degree, automatic, lo, hi, theta, resid, x_dev, ldx, stream, info);           \
    }
SPAL_EIGSH_NEAR_ENTRIES(csr, f64, double)
SPAL_EIGSH_NEAR_ENTRIES(csr, f32, float)
SPAL_EIGSH_NEAR_ENTRIES(csc, f64, double)
SPAL_EIGSH_NEAR_ENTRIES(csc, f32, float)
#undef SPAL_EIGSH_NEAR_ENTRIES

}  // extern "C"
