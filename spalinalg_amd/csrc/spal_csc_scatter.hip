// spal_csc_scatter.hip -- CSC y = A*x by atomic scatter over COLUMN tiles: the kernel and its launcher.
//
// Contract (reference src/csc/ops/mul.rs:26-46): for
// every stored entry (i, k): y[i] += values[p] * x[k]; rows never touched
// give 0.0.  On the GPU the adds into one y[i] arrive in no fixed order
// (hardware f64/f32 atomics), so parity with the sequential CPU order is to
// rounding (<= 1e-10 relative, tested), not bitwise.
//
// Two scatter paths in one launch, chosen per SUPER-TILE of 512 columns:
//   LDS-privatised : the rows a super-tile touches form a window
//                    [rmin, rmax]; when it fits LDS the adds go to an LDS copy
//                    of that window (ds_add_f64: conflicts cost cycles, not
//                    memory round trips) and the window is flushed once with
//                    contiguous global atomics (full-rate shape: 256 B per
//                    wave instruction).  Entries are streamed coalesced with a
//                    packed 32-bit (row - rmin | (col - k0) << 16) per entry.
//   global scatter : one global atomic per entry (windows that do not fit).
// The plan (windows, modes, hand-off eligibility) is spal_csc_plan.hip's; the handle and the route choice spal_csc.hip's.
#include "csr_kernels.hpp"
#include "spal_internal.hpp"

namespace spal {

#ifndef SPAL_CSC_U
#define SPAL_CSC_U 2
#endif
#ifndef SPAL_CSC_BLOCK
#define SPAL_CSC_BLOCK 1024
#endif
#ifndef SPAL_CSC_FENCES
#define SPAL_CSC_FENCES 0   // 1: release / acquire fences around the hand-off's flag (see csc_spmv_scatter)
#endif

constexpr int kCscBlock = SPAL_CSC_BLOCK;      // threads of the scatter kernel
// Columns per super-tile: the widest of 4096 / 2048 / 1024 whose row windows fit LDS (csc_plan_build).  Wider
// super-tiles flush fewer window rows per column -- the contiguous global atomics of the flush are what bounds
// config 4: 1024 columns 39.7 MB of atomics 53.5 us, 2048 23.8 MB 44.6 us, 4096 15.9 MB 42.7 us
// (profiles/r02/csc_scatter_column_tiles.txt) -- and 245 workgroups are one round of the device.
constexpr int kCscColsMax = 4096;   // (the x tile of the widest form: 32 KiB of f64)
static_assert(kCscColsMax % kCscBlock == 0, "whole x elements per thread");
// LDS y window budget (+ 8 KiB x tile): two 1024-thread workgroups per CU either way; a band's
// clamped edge needs more rows than its interior (config 4: 6717 against 5120), and ONE super-tile
// left to the global-atomic path kept the whole launch busy (47 us -> 78 us)
// (x tile + window <= 80 KiB: 70 KiB of window beside 1024 columns of f64 x, 64 KiB beside 2048)
// LDS of a workgroup: x tile + y window.  1024 / 2048 columns: 80 KiB in all, two workgroups per CU; 4096 columns:
// 32 KiB of x + 94 KiB of window, one.
constexpr uint32_t csc_window_bytes(int cols) { return (cols >= 4096 ? 94u : cols >= 2048 ? 64u : 70u) * 1024u; }
// ... in elements of the handle's dtype, and no more than the 16 bits a packed entry has for its row
uint32_t csc_window_budget(const spal_csc *a, int cols) {
    return std::min<uint32_t>(csc_window_bytes(cols) / (uint32_t)a->elem_size, 65536u);
}

// ---- the scatter kernel ------------------------------------------------------------
// desc[b] = {window base row, window length, mode, 0}
template <typename T, int kCscCols>
__global__ __launch_bounds__(kCscBlock, kCscBlock >= 1024 ? 1 : 2) void csc_spmv_scatter(
    const uint32_t *__restrict__ colptr, const uint32_t *__restrict__ rowind,
    const uint32_t *__restrict__ meta, const T *__restrict__ vals, const T *__restrict__ x,
    T *__restrict__ y, const uint4 *__restrict__ desc, uint32_t ncols, uint32_t nblocks,
    uint32_t per_xcd, uint32_t last_pair, T *__restrict__ windows, const uint32_t *__restrict__ prev_hi,
    uint32_t *__restrict__ flags, uint32_t epoch, uint32_t nrows, uint32_t ticket_base, uint32_t use_ticket,
    uint32_t spin_bound, uint32_t *__restrict__ gave_up, uint32_t ulen) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spal_smem[];
    using pair_t = typename Pair<T>::type;
    using u2_t = __attribute__((ext_vector_type(2))) uint32_t;
    T *xt = reinterpret_cast<T *>(spal_smem);  // x of the super-tile's columns
    T *yw = xt + kCscCols;                     // y window accumulators

    // Neighbour hand-off: super-tile b waits for b - 1, which must therefore have STARTED before it.  The super-tile a
    // workgroup takes is its ticket -- one atomicAdd on flags[nblocks + 1] per workgroup, ticket_base = the counter's
    // value when this launch began (launches of one handle are chained) -- i.e. the order in which workgroups actually
    // start, not their blockIdx: the holder of b started after the holders of 0 ... b - 1, which are resident or
    // done, so the wait below always ends, whatever order the dispatcher takes the workgroups in.  (use_ticket = 0:
    // blockIdx order, option "ticket"; enough when all workgroups of the launch are resident together.)
    // Without the hand-off each XCD takes a contiguous run of super-tiles.
    uint32_t b;
    if (prev_hi) {
        b = blockIdx.x;
        if (use_ticket) {
            // (through the first word of the dynamic LDS: the kernel may use all 160 KiB of it, a static variable would not fit)
            uint32_t *s_ticket = reinterpret_cast<uint32_t *>(spal_smem);
            if (threadIdx.x == 0) *s_ticket = atomicAdd(&flags[nblocks + 1], 1u) - ticket_base;
            __syncthreads();
            b = *s_ticket;
            __syncthreads();   // before the x tile is written there
        }
    } else {
        b = xcd_contiguous_block(blockIdx.x, per_xcd);
    }
    if (b >= nblocks) return;
    const uint32_t k0 = b * kCscCols, k1 = min(k0 + (uint32_t)kCscCols, ncols);
    // desc and the two column pointers are independent loads: one round trip for the three
    const uint4 d = desc[b];  // block-uniform
    // (every column of the matrix holds ulen - 1 entries: the column pointers are arithmetic, and the first batch of
    //  entries can be requested without waiting for them -- one memory round trip less at the start of a workgroup
    //  that lives for a dozen)
    const uint32_t p0 = ulen ? k0 * (ulen - 1u) : colptr[k0], p1 = ulen ? k1 * (ulen - 1u) : colptr[k1];  // uniform

    if (d.z == kCscModeLds) {
        // entries in pairs from an even start; a batch = U pairs per thread.  The FIRST batch and this
        // thread's element of the x tile are requested before the window is zeroed and before the
        // barrier: zeroing and staging hide behind those loads.
        constexpr uint32_t U = SPAL_CSC_U;
        constexpr uint32_t kBatch = 2 * U * kCscBlock;
        static_assert(kCscCols % kCscBlock == 0 || kCscCols < kCscBlock, "whole x elements per thread");
        constexpr uint32_t XPT = kCscCols > kCscBlock ? kCscCols / kCscBlock : 1;   // x elements per thread
        uint32_t batch0 = p0 & ~1u;   // uniform: first entry of the current batch
        const uint32_t tile_last_pair = min(last_pair, p1 ? (p1 - 1u) & ~1u : 0u);   // pair holding the super-tile's last entry
        pair_t v[U];
        u2_t m[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            // unconditional loads; a batch may reach past the super-tile's last entry: stay inside
            // the allocation (last_pair = last even index of the padded arrays)
            const uint32_t e = min(batch0 + threadIdx.x * 2 + u * (kCscBlock * 2), last_pair);
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const pair_t *>(vals + e));
            m[u] = __builtin_nontemporal_load(reinterpret_cast<const u2_t *>(meta + e));
        }
        T xk[XPT];
#pragma unroll
        for (uint32_t q = 0; q < XPT; ++q) xk[q] = x[min(k0 + threadIdx.x + q * kCscBlock, k1 - 1u)];
        for (uint32_t i = threadIdx.x; i < d.y; i += kCscBlock) yw[i] = T(0);
#pragma unroll
        for (uint32_t q = 0; q < XPT; ++q)
            if (threadIdx.x + q * kCscBlock < k1 - k0) xt[threadIdx.x + q * kCscBlock] = xk[q];
        __syncthreads();
        // Two batches in flight: the next batch's loads are issued before this one's LDS adds (loads return in
        // order, so the adds wait for the older batch only) -- with one batch the wave sat out a full memory
        // round trip per batch, six times per super-tile of config 4.
        while (true) {
            const uint32_t next0 = batch0 + kBatch;
            const bool more = next0 < p1;   // uniform
            pair_t vn[U];
            u2_t mn[U];
            // (unconditional: loads under a uniform branch make the compiler wait for ALL loads before the adds;
            //  lanes past the super-tile's last pair re-read that pair: one line, no traffic)
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t e = min(next0 + threadIdx.x * 2 + u * (kCscBlock * 2), tile_last_pair);
                vn[u] = __builtin_nontemporal_load(reinterpret_cast<const pair_t *>(vals + e));
                mn[u] = __builtin_nontemporal_load(reinterpret_cast<const u2_t *>(meta + e));
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t e = batch0 + threadIdx.x * 2 + u * (kCscBlock * 2);
                if (e >= p0 && e < p1) lds_add(&yw[m[u].x & 0xffffu], v[u].x * xt[m[u].x >> 16]);
                if (e + 1 >= p0 && e + 1 < p1) lds_add(&yw[m[u].y & 0xffffu], v[u].y * xt[m[u].y >> 16]);
            }
            if (!more) break;
            batch0 = next0;
            for (uint32_t u = 0; u < U; ++u) { v[u] = vn[u]; m[u] = mn[u]; }
        }
        __syncthreads();
        if (windows) {
            // two-phase flush: the window goes to this super-tile's slot (plain coalesced
            // stores); csc_window_reduce adds the overlapping windows row by row
            T *slot = windows + d.w;
            for (uint32_t i = threadIdx.x; i < d.y; i += kCscBlock) slot[i] = yw[i];
            return;
        }
        if (prev_hi) {
            // Neighbour hand-off (plan: windows ascend, only adjacent super-tiles overlap).  Rows from the end of
            // the previous window on are this super-tile's own: STORED (written through, `sc1`), with zeros for
            // rows no window covers; then a flag.  The rows shared with the previous super-tile are updated after
            // ITS flag: y[r] = (previous tile's sum) + (this tile's) -- columns ascending, no atomics, no memset.
            const uint32_t lo = d.x, hi = d.x + d.y, ph = prev_hi[b];       // ph <= hi; ph = 0 for b = 0
            const uint32_t own0 = max(lo, ph);
            for (uint32_t r = min(ph, lo) + threadIdx.x; r < lo; r += kCscBlock) y[r] = T(0);   // gap before the window
            for (uint32_t r = own0 + threadIdx.x; r < hi; r += kCscBlock)
                __hip_atomic_store(&y[r], yw[r - lo], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b + 1 == nblocks)
                for (uint32_t r = hi + threadIdx.x; r < nrows; r += kCscBlock) y[r] = T(0);     // rows after the last window
            // Publication.  Every access that takes part is an agent-scope atomic (sc1): the stores of y above are
            // written through to the device's point of coherence and acknowledged from there, and `s_waitcnt vmcnt(0)`
            // holds every storing wave until its acknowledgements are in -- the rows are PERFORMED at agent scope before
            // the barrier, the flag is stored after it.  The consumer reads the flag, then (control dependency + the
            // barrier) the rows, again with sc1 loads, which are served from the point of coherence, never from a line
            // its XCD's L2 happens to hold.  That is the ISA-level contract (gfx942 / gfx950 memory model: agent-scope
            // atomics bypass the non-coherent levels); what release / acquire would ADD is a write-back of the L2's
            // dirty non-atomic lines (`buffer_wbl2 sc1`) and an invalidate (`buffer_inv sc1`) -- there are no
            // non-atomic lines in this exchange.  Measured (-DSPAL_CSC_FENCES=1: flag stored with release, acquire fence
            // after the spin): 44.9 instead of 39.0 us per product at config 4, +15 % (profiles/r03/csc_handoff.txt),
            // hence off by default; tests/test_gpu_csc_coo.py runs 600 checked products back to back either way.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
#if SPAL_CSC_FENCES
            if (threadIdx.x == 0) __hip_atomic_store(&flags[b], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#else
            if (threadIdx.x == 0) __hip_atomic_store(&flags[b], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
            if (ph > lo) {   // uniform: rows [lo, ph) also belong to super-tile b - 1, which stores them
                if (threadIdx.x == 0) {
                    uint32_t spins = 0;
                    while (__hip_atomic_load(&flags[b - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
                        if (++spins > spin_bound) {   // a backstop, so that the wave ends whatever happens: the host is told
                            __hip_atomic_store(gave_up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (host memory)
                            break;
                        }
                        __builtin_amdgcn_s_sleep(8);
                    }
#if SPAL_CSC_FENCES
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
                }
                __syncthreads();
                for (uint32_t r = lo + threadIdx.x; r < min(ph, hi); r += kCscBlock) {
                    const T before = __hip_atomic_load(&y[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    y[r] = before + yw[r - lo];
                }
            }
            return;
        }
        // flush: contiguous, one atomic per touched row (adding 0.0 changes nothing)
        for (uint32_t i = threadIdx.x; i < d.y; i += kCscBlock) {
            const T s = yw[i];
            if (s != T(0) || s != s) atomicAdd(&y[d.x + i], s);
        }
        return;
    }

    // Super-tiles whose row window does not fit LDS (at a band's clamped edges, or scattered rows):
    // one global atomic per entry, entry-parallel.  The tile's column pointers and x go to LDS;
    // thread t takes entries p0 + t, p0 + t + 1024, ...: coalesced loads of (row, value), all of a
    // batch in flight together, the entry's column by binary search in the LDS column pointers.
    // (A lanes-per-column walk costs three dependent memory round trips per 64 columns; on config 4
    // the two edge super-tiles alone kept the kernel busy for 75 us while all others took 47.)
    {
        uint32_t *cp = reinterpret_cast<uint32_t *>(yw);   // k1 - k0 + 1 column pointers
        const uint32_t nk = k1 - k0;
        for (uint32_t i = threadIdx.x; i <= nk; i += kCscBlock) cp[i] = colptr[k0 + i];
        for (uint32_t i = threadIdx.x; i < nk; i += kCscBlock) xt[i] = x[k0 + i];
        __syncthreads();
        constexpr uint32_t U = 4;   // (p0 = cp[0], p1 = cp[nk])
        for (uint32_t base = p0 + threadIdx.x; base < p1; base += kCscBlock * U) {
            uint32_t row[U];
            T val[U];
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t e = min(base + u * kCscBlock, p1 - 1u);   // in bounds; the extra lanes re-read
                row[u] = load_stream(rowind + e);
                val[u] = load_stream(vals + e);
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t e = base + u * kCscBlock;
                if (e < p1) {
                    uint32_t lo = 0, hi = nk;   // largest c with cp[c] <= e (empty columns share a pointer with their successor)
                    while (hi - lo > 1) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (cp[mid] <= e) lo = mid; else hi = mid;
                    }
                    atomicAdd(&y[row[u]], val[u] * xt[lo]);  // -munsafe-fp-atomics: global_atomic_add_f64 / _f32
                }
            }
        }
    }
}

// Second phase of the two-phase flush: one workgroup per chunk of kCscChunk rows adds
// the windows of the super-tiles that overlap the chunk, in ascending super-tile
// (= column) order, and writes y (ASSIGN: no super-tile went the global-atomic way,
// y was not zeroed) or adds to it (the kernel before has finished: plain update).
template <typename T, bool ASSIGN>
__global__ __launch_bounds__(256) void csc_window_reduce(const T *__restrict__ windows,
                                                         const uint4 *__restrict__ desc,
                                                         const uint32_t *__restrict__ chunk_ptr,
                                                         const uint32_t *__restrict__ chunk_blk,
                                                         T *__restrict__ y, uint32_t nrows) {
    const uint32_t c0 = chunk_ptr[blockIdx.x], c1 = chunk_ptr[blockIdx.x + 1];  // uniform
    if (!ASSIGN && c0 == c1) return;
    const uint32_t r0 = blockIdx.x * kCscChunk;
    T acc[kCscChunk / 256];
#pragma unroll
    for (uint32_t k = 0; k < kCscChunk / 256; ++k) acc[k] = T(0);
    for (uint32_t c = c0; c < c1; ++c) {
        const uint4 d = desc[chunk_blk[c]];  // uniform: {window base, length, mode, slot offset}
#pragma unroll
        for (uint32_t k = 0; k < kCscChunk / 256; ++k) {
            const uint32_t i = r0 + threadIdx.x + 256u * k;
            if (i >= d.x && i - d.x < d.y) acc[k] = acc[k] + windows[d.w + (i - d.x)];
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kCscChunk / 256; ++k) {
        const uint32_t i = r0 + threadIdx.x + 256u * k;
        if (i < nrows) {
            if (ASSIGN) y[i] = acc[k];
            else y[i] = y[i] + acc[k];
        }
    }
}

// LDS of a workgroup: x tile + the y window; global-mode super-tiles keep their column pointers where the window would be
size_t csc_scatter_lds_bytes(const spal_csc *a) {
    const size_t cols = (size_t)a->cols_per_block, es = (size_t)a->elem_size;
    return std::max((cols + a->lds_entries) * es, cols * es + (cols + 2) * sizeof(uint32_t));
}

// the opt-in of one instance of the kernel for more than 48 KiB of dynamic LDS
template <typename T, int COLS>
static hipError_t scatter_opt_in(const spal_csc *a, size_t lds) {
    static std::atomic<uint64_t> done{0};
    return lds > 48 * 1024 ? lds_opt_in((const void *)csc_spmv_scatter<T, COLS>, a->device, done) : hipSuccess;
}

// f(kernel) for the instance of csc_spmv_scatter<T, .> that a's column tile selects, opted in for `lds` bytes
template <typename T, typename F>
static hipError_t with_scatter_kernel(const spal_csc *a, size_t lds, F &&f) {
    auto go = [&](auto cols) {
        constexpr int COLS = decltype(cols)::value;
        const hipError_t e = scatter_opt_in<T, COLS>(a, lds);
        return e == hipSuccess ? f(csc_spmv_scatter<T, COLS>) : e;
    };
    switch (a->cols_per_block) {
        case 1024: return go(std::integral_constant<int, 1024>{});
        case 2048: return go(std::integral_constant<int, 2048>{});
        case 4096: return go(std::integral_constant<int, 4096>{});
        default: return hipErrorInvalidValue;
    }
}

// workgroups of the scatter kernel one CU holds at once -- asked of the runtime (registers, LDS and wave slots of the
// compiled kernel), not derived from LDS alone; 0 when it cannot say
template <typename T>
static int scatter_per_cu_t(const spal_csc *a) {
    const size_t lds = csc_scatter_lds_bytes(a);
    int n = 0;
    const hipError_t e = with_scatter_kernel<T>(a, lds, [&](auto kern) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)kern, (int)kCscBlock, lds);
    });
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess ? n : 0;
}
int csc_scatter_per_cu(const spal_csc *a) {
    return a->elem_size == 8 ? scatter_per_cu_t<double>(a) : scatter_per_cu_t<float>(a);
}

// ---- the give-up word: a super-tile hit the hand-off's spin bound (the backstop; the kernel reports it through host
// memory, so looking costs nothing) and that product's y is invalid ----
// Under a->mu_launch: true when a product gave up since the last look -- the handle flushes with global atomics from now on.
bool csc_gave_up_consume(spal_csc *a) {
    if (!a->h_gave_up || !__atomic_load_n(a->h_gave_up, __ATOMIC_RELAXED)) return false;
    __atomic_store_n(a->h_gave_up, 0u, __ATOMIC_RELAXED);
    a->ordered = 0;
    a->handoff_timeouts++;
    return true;
}
// invalid products so far: the consumed ones and one not looked at yet
int csc_invalid_products(const spal_csc *a) {
    return a->handoff_timeouts + ((a->h_gave_up && __atomic_load_n(a->h_gave_up, __ATOMIC_RELAXED)) ? 1 : 0);
}

// Neighbour hand-off: the super-tiles of one launch talk through the handle's flags, so launches of one handle are
// chained (each waits for the event of the one before, whatever its stream).  Under a->mu_launch: puts this launch on
// `st` behind the handle's last one and gives it its epoch and its first ticket.
static hipError_t csc_handoff_chain(spal_csc *a, hipStream_t st, uint32_t *epoch, uint32_t *ticket_base) {
    // A super-tile of an EARLIER launch gave up: the caller is told here, once.  (The host-vector path sees it after
    // its own synchronisation and repeats the product itself, csc_spmv_host.)
    if (csc_gave_up_consume(a)) return hipErrorLaunchTimeOut;
    hipError_t e = hipSuccess;
    // launches of one handle share its flags: each must run after the one before.  On ONE stream that is the
    // stream's order and costs nothing; only a launch on another stream than the last waits for an event, recorded
    // now on that last stream (it covers everything submitted there so far).  (An event wait + record around
    // every launch cost ~3 us of a 38 us product in a loop.)
    if (a->last_stream_valid && a->last_stream != st) {
        if (!a->ev_last) {
            e = hipEventCreateWithFlags(&a->ev_last, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        e = hipEventRecord(a->ev_last, a->last_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, a->ev_last, 0);
        if (e != hipSuccess) {   // (the caller may have destroyed that stream meanwhile: everything it held has then run or is flushed here)
            (void)hipGetLastError();
            e = hipDeviceSynchronize();
        }
        if (e != hipSuccess) return e;
    }
    a->last_stream = st;
    a->last_stream_valid = 1;
    if (++a->epoch == 0) {   // (wrapped after 2^32 launches: the flags and the ticket counter start over)
        e = hipMemsetAsync(a->d_flags, 0, ((size_t)a->nblocks + 2) * 4, st);
        if (e != hipSuccess) return e;
        a->epoch = 1;
        a->ticket_next = 0;
    }
    *epoch = a->epoch;
    *ticket_base = a->ticket_next;               // every workgroup of the grid takes one ticket
    a->ticket_next += ((a->nblocks + 7) / 8) * 8;
    return hipSuccess;
}

template <typename T>
static hipError_t launch_scatter_t(spal_csc *a, const void *x, void *y, hipStream_t st) {
    const bool two_phase = a->flush == 1 && a->d_windows;
    const bool assign = two_phase && a->all_lds;   // the reduce writes every row of y: no memset
    hipError_t e = hipSuccess;
    // The hand-off, where the plan allows it -- but not while the stream is being captured into a graph (an event
    // from outside the capture cannot be waited for): global atomics then.
    bool ordered = a->flush == 0 && a->ordered && a->nnz != 0;
    if (ordered) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) ordered = false;
    }
    std::unique_lock<std::mutex> chain(a->mu_launch, std::defer_lock);
    uint32_t epoch = 0, ticket_base = 0;
    if (ordered) {
        chain.lock();
        e = csc_handoff_chain(a, st, &epoch, &ticket_base);
        if (e != hipSuccess) return e;
    }
    if (!ordered && (!assign || a->nnz == 0)) {
        // (a kernel, not hipMemsetAsync: as a node of a captured graph the memset zeroed every other element from
        //  the second replay on -- ROCm 7.2, tools/lab.py csc_capture)
        hipLaunchKernelGGL(fill_zero<T>, dim3((uint32_t)((a->nrows + 255) / 256)), dim3(256), 0, st, (T *)y, a->nrows);
        e = hipGetLastError();
    }
    if (e != hipSuccess || a->nnz == 0) return e;
    const uint32_t per_xcd = (a->nblocks + 7) / 8;
    const size_t lds = csc_scatter_lds_bytes(a);
    e = with_scatter_kernel<T>(a, lds, [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(kCscBlock), lds, st, a->d_colptr, a->d_rowind,
                           a->d_meta, (const T *)a->d_values, (const T *)x, (T *)y, a->d_desc,
                           (uint32_t)a->ncols, a->nblocks, per_xcd,
                           (uint32_t)(((a->nnz + kStreamPad) & ~(uint64_t)1) - 2),
                           two_phase ? (T *)a->d_windows : (T *)nullptr,
                           epoch ? a->d_prev_hi : (const uint32_t *)nullptr, a->d_flags, epoch, (uint32_t)a->nrows,
                           ticket_base, (uint32_t)(a->use_ticket < 0 ? a->ticket_auto : a->use_ticket), a->spin_bound, a->d_gave_up,
                           a->uniform_cols);
        return hipGetLastError();
    });
    if (ordered || e != hipSuccess || !two_phase) return e;
    auto reduce = assign ? csc_window_reduce<T, true> : csc_window_reduce<T, false>;
    hipLaunchKernelGGL(reduce, dim3(a->nchunks), dim3(256), 0, st, (const T *)a->d_windows, a->d_desc, a->d_chunk_ptr,
                       a->d_chunk_blk, (T *)y, (uint32_t)a->nrows);
    return hipGetLastError();
}

hipError_t launch_csc_scatter(spal_csc *a, const void *x, void *y, hipStream_t st) {
    return a->elem_size == 8 ? launch_scatter_t<double>(a, x, y, st) : launch_scatter_t<float>(a, x, y, st);
}

}  // namespace spal
