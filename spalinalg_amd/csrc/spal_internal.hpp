// spal_internal.hpp -- shared declarations of libspal_hip.so (not installed).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/spal.h"

namespace spal {

// ---- thread-local error message -------------------------------------------
std::string &last_error_ref();
int fail(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define SPAL_HIP_TRY(expr)                                                          \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) {                                                     \
            int st_ = (e_ == hipErrorOutOfMemory) ? SPAL_ERR_OUT_OF_MEMORY          \
                      : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice)     \
                          ? SPAL_ERR_NO_DEVICE                                      \
                          : SPAL_ERR_HIP;                                           \
            return ::spal::fail(st_, "%s failed: %s (%s:%d)", #expr,                \
                                hipGetErrorString(e_), __FILE__, __LINE__);         \
        }                                                                           \
    } while (0)

#define SPAL_TRY(expr)                    \
    do {                                  \
        int st_ = (expr);                 \
        if (st_ != SPAL_OK) return st_;   \
    } while (0)

// A call that allocates, copies back to the host or synchronises cannot become nodes of a graph, and trying it
// invalidates the caller's capture: such a call asks here first, before any device work.  `why` says what the call does,
// `instead` what to call before the capture (or nullptr).  A stream whose status cannot be read counts as capturing.
inline int refuse_capture(const char *fn, hipStream_t st, const char *why, const char *instead = nullptr) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: %s: it cannot be captured into a graph%s%s", fn, why,
                    instead ? ": " : "", instead ? instead : "");
    return SPAL_OK;
}

// Selects `device` for the calling thread, restores the previous one on exit.
struct DeviceGuard {
    int prev = -1;
    int status = SPAL_OK;
    explicit DeviceGuard(int device);
    ~DeviceGuard();
};

// ---- device memory ---------------------------------------------------------------
// hipMalloc / hipFree of hundreds of MB cost milliseconds (and on some hosts
// tens of ms) each; a handle that is assembled, used and destroyed in a loop
// would pay that every time.  dev_alloc / dev_free keep a small per-device
// cache of freed blocks (exact-fit-ish reuse, bounded by SPAL_CACHE_BYTES, default a quarter
// of the device's memory, at least 8 GiB).  dev_free synchronises the device first,
// like hipFree does, so a cached block is never handed out while work that used
// it is still in flight.  Small blocks are rounded up to a power of two.  (spal_device.hip, like the placement blocks and
// the stream pool below.)

// Stored entries a handle accepts: entry offsets are 32-bit on the device and the kernels compute
// `offset + a batch` (at most a few thousand entries past the end, clamped afterwards) in 32 bits.
constexpr uint64_t kMaxEntries = 0xffffffffull - 65536ull;
// THE padding contract: the entry arrays of every handle (indices, values, packed copies) are allocated with this many
// spare entries behind the last one -- the streaming kernels read whole steps and clamp afterwards.  Whoever builds
// arrays for csr_adopt_device / csc_adopt_device allocates nnz + kStreamPad and passes that capacity on.
constexpr int kStreamPad = 256;

// Kernels that use more than 48 KiB of dynamic LDS opt in once per device: `done` is the caller's word for ONE kernel
// (a bit per device); `device` is the current one.
inline hipError_t lds_opt_in(const void *kernel, int device, std::atomic<uint64_t> &done) {
    const uint64_t bit = 1ull << (device & 63);
    if (done.load(std::memory_order_relaxed) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
    return e;
}

// ---- placement blocks: blocks of 1 GiB found by ONE walk per process and device, kept, and shared by every
// handle's vectors and 16-bit columns as pieces (first fit, 4 KB granules).  Two are kept when the walk met two classes of
// region: the place where the first handle ran fastest and the one where it ran slowest -- a later handle, whose values lie
// wherever they lie, times itself in each (no hipMalloc) and takes the better.
struct PlaceBlock { void *base; size_t size; };
int place_block_count(int device);
PlaceBlock place_block(int device, int index);
void *place_alloc(int device, int index, size_t bytes);        // a piece of block `index`, or nullptr
void place_free(int device, void *ptr);                        // a piece (nullptr is fine)
void place_adopt(int device, void *base, size_t size);         // a hipMalloc'ed block becomes a placement block
size_t place_free_bytes(int device);                           // what the retained blocks still have to give
void place_trim();                                             // blocks without pieces back to the driver
bool place_walked(int device);
void place_set_walked(int device);
hipError_t dev_alloc(void **ptr, size_t bytes);   // on the current device
hipError_t dev_free(void *ptr);                   // on the current device; NULL is fine
// a device block that returns to the allocator when it goes out of scope (early returns included)
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)dev_free(p); }
    hipError_t alloc(size_t bytes) { return dev_alloc((void **)&p, bytes ? bytes : 1); }
    template <typename U> U *as() { return reinterpret_cast<U *>(p); }
    void *release() { void *q = p; p = nullptr; return q; }
};
void dev_cache_trim();                            // releases every cached block
// Scratch of the _dev calls that need some (the sweeps' ping-pong vectors, a dot's partial sums): ONE block per
// (device, stream handle), taken from the runtime's stream-ordered allocator on that stream when the stream's first such
// call comes, grown the same way when a call needs more, and KEPT: every later call on the stream makes no allocator
// call and does not wait for the stream.  (Taking and returning a block per call was the first form.  The runtime's
// hipFreeAsync waits ON THE HOST when the block it returns had been handed out again while its previous return was still
// pending on a busy stream, so every second call on a busy stream waited for the stream to drain: DESIGN 3.21.)
//   * A StreamWork holds its stream's block from take() until it goes out of scope, so the launches of two host threads
//     on one stream do not interleave between a call's passes; leaving, it records an event behind the call, and the next
//     holder makes its stream wait for that event first.  On one stream that orders nothing new; it is what keeps the
//     block safe when a handle's value names ANOTHER stream than last time (given out again after hipStreamDestroy).
//   * hipStreamPerThread is one value and a different stream in every thread: such a call takes and returns a block of
//     its own, as every call once did.  hipStreamLegacy is the null stream.
//   * A capturing stream is refused, always: a graph would hold a pointer the library may free (growth, trim).
//   * spal_cache_trim synchronises every device that holds blocks, once, and releases them; the next call takes a new one.
struct StreamWork {
    void *p = nullptr;
    StreamWork() = default;
    StreamWork(const StreamWork &) = delete;
    StreamWork &operator=(const StreamWork &) = delete;
    ~StreamWork();
    int take(const char *fn, hipStream_t st, size_t bytes);   // p: at least `bytes` (256-byte aligned); current device
    template <typename U> U *as() { return reinterpret_cast<U *>(p); }

  private:
    void *slot_ = nullptr;
    hipStream_t st_ = nullptr, own_ = nullptr;   // own_: the block is this call's alone and goes back on that stream
};
int stream_work_trim();
hipError_t stream_acquire(hipStream_t *out);      // a non-blocking stream of the current device (pooled)
void stream_release(hipStream_t s);               // synchronises it and returns it to the pool

// ---- setup-time timer ----------------------------------------------------------
// The planner, the autotune and the placement walk choose between forms of a product by time.  A SetupTimer owns two
// events for its lifetime (created by the first run, destroyed on every path out of its scope) and does one thing: `warm`
// untimed and `n` timed calls of `fn` -- which returns a status, e.g. a csr_launch -- on `st`; *ms = what the n took
// together.  The first failing call of fn ends the run with its status, a failing HIP call with SPAL_ERR_HIP and
// "<who>: <HIP's text>".
struct SetupTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    SetupTimer() = default;
    SetupTimer(const SetupTimer &) = delete;
    SetupTimer &operator=(const SetupTimer &) = delete;
    ~SetupTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    template <typename F>
    int run(hipStream_t st, int warm, int n, F &&fn, float *ms, const char *who) {
        *ms = 0.f;
        hipError_t e = e0 ? hipSuccess : hipEventCreate(&e0);
        if (e == hipSuccess && !e1) e = hipEventCreate(&e1);
        for (int i = 0; i < warm && e == hipSuccess; ++i) SPAL_TRY(fn());
        if (e == hipSuccess) e = hipEventRecord(e0, st);
        for (int i = 0; i < n && e == hipSuccess; ++i) SPAL_TRY(fn());
        if (e == hipSuccess) e = hipEventRecord(e1, st);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
        return e == hipSuccess ? SPAL_OK : fail(SPAL_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
};

// ---- host helpers ------------------------------------------------------------
unsigned host_threads();
// fn(begin, end, tid) over [0, n) split into contiguous chunks, one per thread.
void parallel_for(uint64_t n, const std::function<void(uint64_t, uint64_t, unsigned)> &fn,
                  uint64_t min_chunk = 1u << 16);

// Compressed-format invariants (src/csr.rs:144-156); reason ordinal or 0.
int compressed_validate(uint64_t nrows, uint64_t ncols, bool major_is_rows,
                        const uint64_t *ptr, uint64_t ptr_len, const uint64_t *ind,
                        uint64_t ind_len, uint64_t val_len);
const char *invariant_text(int reason, bool csr);

// ---- device matrices ---------------------------------------------------------
struct CsrPlan {
    // kernel family: 1 = "vector" (L lanes per row, shuffle reduction, optional
    // LDS-staged x window); 2 = "stream" (lane per row, products through LDS,
    // 16-bit columns = position in the paged LDS x window; vector fallback per super-tile)
    int kernel = 0;          // 0 = not planned yet
    int user_kernel = 0;     // 0 = auto
    bool user_persistent = false;  // `persistent` was set by the caller or by the autotune
    int lanes_per_row = 0;   // L in {2,4,8,16,32,64}
    int unroll = 1;          // row groups in flight per wave iteration
    int vec_col16 = 0;       // vector kernel (long rows, LDS windows): reads 16-bit window-relative columns
    int vec_col16_allowed = 1;
    int long_rows = 0;       // vector kernel: batched rest-of-row loop (mean row length above 64)
    int threads = 512;       // workgroup size: 512 or 1024
    int tiles_per_wave = 4;  // stream kernel: tiles per wave (4 or 8)
    int rows_per_tile = 64;  // stream kernel: rows of a wave-tile (64, 32 or 16)
    int persistent = 0;      // stream kernel: fixed grid walking chunks of super-tiles
    int nt_store = 0;        // stream kernel: non-temporal stores of y
    int skew = 0;            // stream kernel: skewed product strips (rows a multiple of 128 bytes long: LDS bank conflicts)
    bool user_skew = false;
    int stream_row_max = 128; // stream kernel: tiles with a longer row go to the overflow kernel (a lane sums a row)
    int window_pages = 0;    // stream kernel: page budget of a super-tile's LDS x window (0 = automatic)
    int stream_global = 1;   // stream kernel: super-tiles whose pages exceed the LDS budget gather x from global
    int uniform_rows = 1;    // stream kernel: super-tiles whose rows all have one length do not read rowptr
    int prefetch = 1;        // stream kernel: tiles of loads a wave keeps in flight ahead of the one it works on (1 or 2)
    // the sliding-window kernel (csr_slide.hpp): band-like stream plans
    int slide_user = -1;     // -1 auto, 0 never
    int slide_on = 1;        // launch it (0: the one-super-tile-per-workgroup kernels on the same ring plan)
    int slide = 0;           // the plan is eligible and built for it
    int ring_pages = 0;      // the LDS x window is a ring of this many pages (col16 = (page % ring) * 256 + column in page)
    uint32_t slide_steps = 0;  // steps of 4 * rows_per_tile rows
    int panel_pages = 192;   // wide bands: super-tiles with a column span of at most this many pages go to csr_spmv_panel (0: never)
    int panel_on = 1;        // launch it (0: those super-tiles gather x from global memory in the stream kernels)
    int panel_window_pages = 0;  // pages of one panel (LDS)
    int panel_window_user = 0;   // option "panel_window" (0 = 80 KB)
    int slide_run = 0;       // steps per run (0 = one run per workgroup: fully persistent)
    int xcd_chunk = 32;      // one-super-tile stream kernel: chunks of super-tiles per XCD (0 = one run per XCD)
    // the column-blocked kernel (csr_cblock.hpp): matrices whose columns are not local
    int cblock_user = -1;    // option "cblock": -1 = when the plan finds most rows gathering x from beyond L2, 0 never, 1 always (tests)
    int cblock = 0;          // the tiled copy is built
    int cblock_pending = 0;  // the matrix qualifies; the copy is built by the first product (handles assembled on the device:
                             // the assembly call does not pay for a second copy nobody may use)
    int cblock_on = 1;       // launch it (autotune: 0 when the stream kernels measured faster)
    int cblock_rows = 0;     // rows of a row block (one workgroup each)
    int cblock_strip = 0;    // entries of the product strip (the fullest tile fits)
    int cblock_rows_user = 0, cblock_shift_user = 0;   // options "cblock_rows", "cblock_shift"
    int cblock_form_user = -1;   // option "cblock_form": -1 = by the entries per run, 0 = entry-parallel, 1 = rows form
    int cblock_form = 0;         // 0: csr_spmv_cblock (entry-parallel, rows16), 1: csr_spmv_cblock_rows (threads own rows, cnt8)
    float cblock_run = 0.f;      // entries per (row, column block) that holds any
    int cblock_shift = 0;    // a column block holds 2^shift columns
    int cblock_nbc = 0;      // column blocks
    uint32_t cblock_nrb = 0; // row blocks = workgroups
    double nonlocal_row_fraction = 0.0;   // rows of super-tiles that gather x from global memory over a span no panel holds
    int slide_S = 0;         // 128-entry steps of the largest streamed tile: every tile issues that many loads
    int slide_uniform = 0;   // 1 + the length of every row when all streamed rows have one length (rowptr is not read), else 0
    int all_rows_uniform = 0; // ... and EVERY row of the matrix has it (rowptr[r] = r * length): tile bounds are arithmetic
    int arith_bounds = 1;    // option "arith_bounds": use that (0: load the tiles' bounds from rowptr as before)
    int slide_fill_ok = 1;   // the sliding kernel's tiles are full enough for its fixed count of loads per tile (csr_slide plan)
    int slide_fill_user = -1; // -1 = by the tiles' average fill, 1 = "slide_on" was asked for by name
    int slide_even = 1;      // option "slide_even": one run per workgroup -> the XCD's steps split evenly over all its workgroups
    // row records (csr_rowrec.hpp): the sliding kernel streams one Elias-Fano record per row instead of the row's col16
    int rowrec_user = -1;    // option "rowrec": -1 auto (where the plan qualifies), 0 never, 1 as -1
    int rowrec_on = 1;       // option "rowrec_on": launch the record form (0: the same plan streams col16 -- A/B, autotune)
    int rowrec = 0;          // the records are built and verified against col16; = the rows' length (12, 14 or 16)
    int rowrec_failed = 0;   // a built record did not decode to its row's col16 (cannot be): the records were dropped
    // packed values (csr_valpack.hpp): the record form streams fixed-point row blocks instead of the f64 values
    int valpack_user = -1;   // option "valpack": -1 auto (where the plan has records and the values share a quantum), 0 never, 1 as -1
    int valpack_on = 1;      // option "valpack_on": launch the packed form (0: the same plan streams the values -- A/B, autotune)
    int valpack = 0;         // the row blocks are built and verified against the values; = the rows' length (12, 14 or 16)
    int valpack_failed = 0;  // a built block did not decode to its row's values (cannot be): the array was dropped
    int valpack_bits = 0;    // bits of the widest k, sign included
    int valpack_exp = 0;     // e of the quantum 2^e
    int blockwin = -1;       // option "blockwin": -1 = timed against the row split where that is built, 0 never, 1 whenever the windows fit (tests)
    int row_split = -1;      // option "row_split": -1 = when long rows keep a tenth of the 64-row tiles from streaming, 0 never, 1 always (tests)
    int split_threshold = 128;   // option "row_split_threshold": rows above it are "long"
    int place_tries = 8;     // autotune: blocks of 1 GiB the 16-bit columns are tried in, at most (see csr_autotune)
    int split_tiles_on = 1;  // sliding kernel: tiles above 1024 entries whose halves fit go through the strip twice
    int diag = 0;            // ablation builds (-DSPAL_DIAG) only: parts of the stream kernel switched off
    int persistent_blocks = 0;    // its grid; 0 = what the device holds at once (LDS per workgroup decides: f64 band 512)
    int rows_per_block = 0;  // R
    int lds_x = 0;           // stage the block's x window in LDS
    uint32_t lds_entries = 0;  // LDS window capacity (elements) when lds_x
    uint32_t nblocks = 0;
    double lds_row_fraction = 0.0;  // rows whose block window fits
    double stream_row_fraction = 0.0;  // rows handled by the stream path (kernel 2)
    double uniform_row_fraction = 0.0; // rows in super-tiles that do not read rowptr (all rows one length)
    bool user_rows_per_block = false, user_lanes = false, user_lds = false,
         user_unroll = false, user_threads = false, user_rows_per_tile = false;
};

// implemented in spal_host.cpp: appends `, "<key>": <body>` before the closing brace of the line in buf (no-op for an
// empty body); refused, with buf unchanged, when the result and its NUL do not fit buf_len or buf does not end in '}'
int describe_append(char *buf, size_t buf_len, const char *key, const std::string &body);
// implemented in spal_host.cpp: the level analysis of spal_trsv_levels on the device's 32-bit arrays; *first_missing_diag
// = n when every row stores its diagonal (no error either way), dpos[i] = the first entry of row i with column >= i
int trsv_levels_u32(uint64_t n, const uint32_t *rowptr, const uint32_t *colind, int uplo, uint32_t *level_of,
                    uint64_t *nlevels, uint64_t *first_missing_diag, uint32_t *dpos);
int trsv_missing_diag(const char *fn, uint64_t row);   // the error of a non-unit solve on such a matrix
// implemented in spal_csc.hip: handle around device arrays it takes ownership of (on failure they stay with the caller);
// cap_entries = allocated entries of d_rowind / d_values, refused when below nnz + kStreamPad
int csc_adopt_device(int device, int elem_size, uint64_t nrows, uint64_t ncols, uint64_t nnz, uint64_t cap_entries,
                     uint32_t *d_colptr, uint32_t *d_rowind, void *d_values, spal_csc **out);

// Triangular solve (spal_trsv.hip): the plan of one triangle of a handle.
struct TrsvLaunch { uint32_t level0, level1; int chain; };   // levels [level0, level1); chain: one workgroup walks them
struct TrsvPlan {
    uint64_t levels = 0, max_level_rows = 0;
    uint64_t first_missing_diag = 0;       // nrows when every row stores its diagonal
    uint2 *d_rows = nullptr;               // nrows x {row, first entry with column >= row}, ordered by (level, row)
    uint32_t *d_level_ptr = nullptr;       // levels + 1 offsets into d_rows
    std::vector<uint32_t> level_ptr;       // ... and on the host, for the launch list
    std::vector<TrsvLaunch> launches;
    uint64_t chain_launches = 0;
    double analysis_ms = 0.0;              // copy back + levels + ordering + upload, host clock
};
constexpr int64_t kTrsvChainRowsDefault = 256;
// ... the plan of `uplo`, built now (under a->mu, which the caller holds; counted in trsv_analyses) if the handle has
// none; refuses row-block handles, matrices that are not square and, unless unit_diag, a row without a diagonal
int trsv_plan_get(const char *fn, spal_csr *a, int uplo, int unit_diag, hipStream_t st, TrsvPlan **out);
constexpr int64_t kIluWideWorkDefault = 4096;   // ILU(0) (spal_ilu.hip): the option "ilu_wide_work"

// What the sparse operations keep on a handle of either type (spal_ops.hpp sets and describes it): the options of this
// handle as the LEFT operand, and what built it if it is a result.  An info string is the object of that name in
// describe(), empty when the handle is no such result.
struct OpState {
    int spgemm_route = 0;          // option "spgemm_route": 0 auto, 1 LDS tiers wherever they fit, 2 every row through the large tier
    int64_t spgemm_lds_cap = 0;    // option "spgemm_lds_cap": 0 default, else the largest product count of a row sent to LDS
    uint32_t spadd_tile = 0;       // option "spadd_tile": merged elements per workgroup, 0 = default
    int spmm_tile = 0;             // option "spmm_tile": column tile, 0 = automatic (SpMM always runs on the CSR handle or twin)
    std::string spgemm_info;       // "spgemm": a product of spal_*_mul
    std::string spadd_info;        // "spadd": a result of spal_*_add / _sub / _neg
    std::string ilu_info;          // "ilu0": a factor of spal_*_ilu0
    std::string ilu_sweep_info;    // "ilu0_sweep": a factor of spal_*_ilu0_sweep (spal_ilu_sweep.hip)
    int64_t krylov_check_every = 0; // option "krylov_check_every": iterations between two polls, 0 = default (spal_krylov.hip)
    std::string krylov_info;       // "krylov": the last spal_*_krylov_* call with this handle as A (guarded by the solve handle's mu)
    std::string gmres_info;        // "gmres": the last spal_*_gmres_* call with this handle as A (the same lock; spal_gmres.hip)
    int krylov_tile = 0;           // option "krylov_tile": column tile of the block Krylov vector kernels, 0 = automatic (spal_krylov_block.hip, spal_gmres_block.hip)
    std::string krylov_block_info; // "krylov_block": the last spal_*_krylov_block_* call with this handle as A (the same lock)
    std::string gmres_block_info;  // "gmres_block": the last spal_*_gmres_block_* call with this handle as A (the same lock)
    int eigsh_rotate = 0;          // option "eigsh_rotate": the restart's rotation kernel, 0 = automatic, 1 = batched passes, 2 = LDS row tiles (spal_eigsh.hip)
    std::string eigsh_info;        // "eigsh": the last spal_*_eigsh_* call with this handle as A (the same lock)
    int cheb_chunk = 0;            // option "cheb_chunk": entries per chunk of the Chebyshev step kernel, 0 = 16 KiB of products (spal_cheb.hip)
    std::string eigsh_filter_info; // "eigsh_filter": the last spal_*_eigsh_filtered_* call with this handle as A (the same lock)
    int cheb_series_form = 0;      // option "cheb_series_form": 0 = automatic, 1 = the fused series step, 2 = step and accumulation apart (spal_cheb.hip)
    std::string eigsh_near_info;   // "eigsh_near": the last spal_*_eigsh_near_* call with this handle as A (the same lock)
    int kpm_tile = 0;              // option "kpm_tile": column tile of the KPM block step, 0 = automatic (spal_kpm.hip)
    int kpm_form = 0;              // option "kpm_form": 0 = automatic, 1 = dots fused into the step, 2 = step and dot launches apart
    std::string kpm_info;          // "kpm": the last spal_*_kpm_moments_* call with this handle as A (the same lock)
    int64_t fsai_max_row = 32;     // option "fsai_max_row": the largest local system of a row of G, 1 .. 64 (spal_fsai.hip)
    // a result of spal_*_permute / _multicolour (spal_colour.hip): written once, before the handle is
    // returned, and only read afterwards
    uint32_t *d_perm = nullptr;    // nrows: new -> old; freed by ordering_free (csr_free, csc_free)
    uint64_t ordering_colours = 0; // 0: the permutation was the caller's
    std::string ordering_info;     // "ordering"
};
void ordering_free(OpState &s);    // spal_colour.hip

// The priority of a row in the multicolour ordering (include/spal.h): a bijection of the 32-bit words.
__host__ __device__ inline uint32_t colour_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
}  // namespace spal

// The opaque handle types of spal.h.
struct spal_csr {
    int device = 0;
    int elem_size = 8;  // 8 = f64, 4 = f32
    uint64_t nrows = 0, ncols = 0, nnz = 0;
    uint32_t *d_rowptr = nullptr;  // nrows + 1
    uint32_t *d_colind = nullptr;  // nnz
    void *d_values = nullptr;      // nnz * elem_size
    uint16_t *d_col16 = nullptr;   // nnz (+pad): page slot * 256 + column inside the page, streamable super-tiles
    uint32_t *d_ovtiles = nullptr; // [count][first rows of the n_ovtiles tiles the stream kernels skip (csr_spmv_overflow)]
    uint32_t n_ovtiles = 0;
    uint32_t *d_pages = nullptr;   // blocks * page budget: ascending page ids of super-tiles whose pages are not one run
    uint32_t *d_ptiles = nullptr;  // panel kernel: the super-tiles it takes
    uint2 *d_pwin = nullptr;       // ... and {first page, pages} of their column spans
    uint32_t n_ptiles = 0;
    uint2 *d_sdesc = nullptr;      // sliding kernel: per step {first page, pages | skip << 8 | flags << 16 | split << 20}
    uint32_t *d_ovtiles_slide = nullptr;   // first rows of the tiles left to csr_spmv_overflow when the sliding kernel runs
    uint32_t n_ovtiles_slide = 0, n_split_tiles = 0;   // ... and the number it takes itself, in two halves
    uint4 *d_desc = nullptr;       // per row block: Stream {first page / offset into d_pages, pages, mode, contiguous};
                                   // VectorLds {window base column, window length, mode, 0}
    uint64_t cap_entries = 0;      // allocated entries of d_colind / d_values (>= nnz + pad)
    // column-blocked copy (csr_cblock.hpp): entries ordered (row block, column block, row, column)
    void *d_cb_val = nullptr;
    uint32_t *d_cb_col = nullptr, *d_cb_tile = nullptr;   // columns; first entry of every tile (+ the end)
    uint8_t *d_cb_cnt = nullptr;   // entries per (tile, row): the builder's scratch
    uint16_t *d_cb_row = nullptr;  // row of every entry inside its row block
    float cblock_us[2] = {0.f, 0.f};   // autotune: per launch {stream kernels, column-blocked kernel}
    // ROW SPLIT (skewed row lengths: a few long rows poison the 64-row tiles of the stream kernel): the matrix is multiplied as
    // A = A_short + A_long -- `split_short` is a complete handle of its own over a compacted copy of the rows of at most
    // `split_threshold` entries (the long rows are empty rows in it: it writes every row of y), `d_split_rows` lists the
    // long rows, which csr_spmv_row_list then overwrites out of THIS handle's arrays.  No temporaries: concurrent products stay safe.
    spal_csr *split_short = nullptr;
    uint32_t *d_split_rows = nullptr;
    uint32_t split_nlong = 0, split_nheavy = 0;   // listed rows (longest first); the first split_nheavy hold more than 1024 entries
    uint64_t split_long_entries = 0;
    int split_child = 0;           // this handle IS the short part of a split (never splits again)
    // BLOCK WINDOW kernel (spal_csr_blockwin.hip): blocks of bw_rows rows, a window of at most bw_cols columns each; bw_on: the products run it
    uint32_t *d_bworder = nullptr; // 32-byte records {block, first entry, one past the last, window's first column, columns, -, -, -} in the order the blocks are dealt
    uint32_t bw_blocks = 0, bw_rows = 0, bw_cols = 0, bw_grid = 0;   // (bw_grid: resident workgroups, 8 x the walks per XCD)
    uint32_t bw_list_rows = 0;     // rows of 8 records in d_bworder (a walk's blocks are J rows apart)
    int bw_on = 0;
    float bw_us[2] = {0.f, 0.f};   // setup: per product {what it was timed against, the block-window kernel}
    int plan_pending = 0;          // a device-assembled handle: the product kernels' plan is built by whoever needs it first (csr_ensure_plan)
    int cblock_lazy = 0;           // build the tiled copy with the first product, not with the plan (csr_adopt_device)
    int cblock_failed = 0;         // building it failed (out of memory, ...): the stream kernels run instead
    // spal_csr_alloc_vectors: the block of 1 GiB (or more) that holds the caller's x and y, found by the placement walk
    void *d_vec_block = nullptr;       // x and y: a piece of one of the process's placement blocks (place_*), or a block of its own
    int vec_block_owned = 0;           // 1: hipMalloc'ed for this handle alone (small matrices: nothing to place)
    size_t vec_x_off = 0, vec_y_off = 0;
    float walk_us[2] = {0.f, 0.f};     // fastest / slowest candidate of the walk (per product)
    int walk_blocks = 0;               // NEW blocks of 1 GiB this handle's call took from the device (0 once the process has its blocks)
    int walk_probes = 0;               // places timed (new blocks + the process's retained ones)
    int walk_max = 8;                  // option "walk_blocks": blocks of 1 GiB a walk may hold at once = how far it reaches
    int col16_placed = 0;              // d_col16 is a piece of a placement block (place_free, not dev_free)
    uint32_t *d_rowrec = nullptr;      // row records (csr_rowrec.hpp): [4 * slide_steps tiles][NR][64] dwords; col16 stays beside them
    size_t rowrec_bytes = 0;
    int rowrec_placed = 0;             // d_rowrec is a piece of a placement block
    float rowrec_us[2] = {0.f, 0.f};   // autotune: per launch {col16, row records} on the kept form
    void *d_valpack = nullptr;         // packed values (csr_valpack.hpp): [4 * slide_steps tiles][NQ][64] chunks of 16 B; the values stay beside them
    size_t valpack_bytes = 0;
    float valpack_us[2] = {0.f, 0.f};  // autotune: per launch {values, packed values} on the kept form
    float valpack_build_ms = 0.f;      // the scan, the builder and the verify pass of the last plan
    std::mutex mu_cb;
    // autotune: microseconds per launch of {plain, persistent} x {plain, non-temporal y stores}
    float tuned_us[4] = {0.f, 0.f, 0.f, 0.f};
    float place_us[2] = {0.f, 0.f};   // autotune: per launch before / after re-placing the values array
    int place_tried = 0;
    spal::CsrPlan plan;
    std::vector<uint2> win_base;   // host copy of the per-256-row column windows (planner cache)
    // a device-assembled handle: {first column, one past the last} of every group of 2^win_group_bits rows as the assembly's
    // group kernel saw them, still on the device -- fetched and folded into win_base when the plan is built (csr_plan_build)
    uint2 *d_win_groups = nullptr;
    uint32_t win_groups = 0, win_group_bits = 0;
    // host-convenience staging (spal_csr_spmv_*): guarded by mu
    std::mutex mu;
    void *d_x = nullptr, *d_y = nullptr;
    hipStream_t stream = nullptr;
    // More stored entries than 32-bit device offsets address (the reference's are usize, src/csr.rs:66-72): the
    // handle is then a list of ROW BLOCKS, each a complete handle of its own (own plan, offsets relative to the
    // block's first entry) over the same columns; this parent owns no matrix arrays.  A product launches the blocks
    // one after the other on the caller's stream, block b writing y[part_row0[b] ...).
    std::vector<spal_csr *> parts;
    std::vector<uint64_t> part_row0, part_entry0;   // first row / first entry of every block, then nrows / nnz
    spal::OpState ops;             // sparse x sparse, A +- B, Y = A * X, ILU(0): options and what built this handle
    uint64_t spmm_last = 0;        // {tile << 32 | k} of the last SpMM on this handle (0: none yet), for describe
    // L x = b, U x = b (spal_trsv.hip); guarded by mu
    int64_t trsv_chain_rows = spal::kTrsvChainRowsDefault;   // option "trsv_chain_rows": the widest level the chain kernel takes
    spal::TrsvPlan *trsv[2] = {nullptr, nullptr};            // [uplo], built by the first solve or by spal_csr_trsv_analyse
    int trsv_analyses = 0;         // plans built so far (describe)
    // ILU(0) (spal_ilu.hip); the option guarded by mu
    int64_t ilu_wide_work = spal::kIluWideWorkDefault;   // option "ilu_wide_work": rows with at least this much work take the wide form
    // Jacobi sweeps on a triangle (spal_trsv_sweep.hip); guarded by mu
    int64_t trsv_sweeps = -1;      // option "trsv_sweeps": how spal_*_krylov_* applies this handle as M (-1: exact solves)
    uint2 *d_sweep_rows = nullptr; // nrows x {first entry with column >= row, that + 1 if it is the diagonal}, built by the first sweep
    int sweep_prepared = 0;
    uint64_t sweep_first_missing = 0;   // the first row without a stored diagonal, nrows when there is none
    double sweep_prepare_ms = 0.0;      // launch + read back, host clock
    uint64_t sweep_calls = 0;           // sweep calls enqueued so far (describe)
    // Solves for a block of right-hand sides (spal_trsm.hip); guarded by mu
    int trsm_tile = 0;                  // option "trsm_tile": column tile, 0 = automatic
    uint32_t trsm_last_tile = 0, trsm_last_k = 0;   // of the last block call (describe)
    uint64_t trsm_last_launches = 0;    // launches the last block call enqueued
    uint64_t trsm_calls = 0, trsm_sweep_calls = 0;   // block calls enqueued so far, exact and sweeps
};

struct spal_csc {
    int device = 0;
    int elem_size = 8;
    uint64_t nrows = 0, ncols = 0, nnz = 0;
    uint32_t *d_colptr = nullptr;  // ncols + 1
    uint32_t *d_rowind = nullptr;  // nnz (+pad)
    void *d_values = nullptr;      // nnz (+pad)
    uint32_t *d_meta = nullptr;    // nnz (+pad): (row - window base) | (col - tile base) << 16
    uint4 *d_desc = nullptr;       // per super-tile of columns {window base row, length, mode, offset of its window in d_windows}
    // two-phase flush (flush == 1): LDS-mode super-tiles store their y windows here; csc_window_reduce
    // adds, for every chunk of 1024 rows, the windows that overlap it (ascending super-tile = column order)
    void *d_windows = nullptr;     // sum of the LDS-mode window lengths, elements
    uint32_t *d_chunk_ptr = nullptr, *d_chunk_blk = nullptr;  // CSR-like cover lists: chunk -> super-tiles
    uint32_t nchunks = 0;
    uint64_t windows_entries = 0;
    int flush = 0;                 // 0 = neighbour hand-off when the plan allows it (else global atomics), 1 = windows + ordered reduce, 2 = global atomics
    // neighbour hand-off (`ordered`): row windows ascend and only adjacent super-tiles overlap, so every row of y is
    // STORED by the first super-tile that covers it and updated by the next one after a flag: no memset, no atomics
    int ordered = 0;
    uint32_t *d_prev_hi = nullptr; // per super-tile: end of the previous super-tile's window (where its own rows begin)
    uint32_t *d_flags = nullptr;   // per super-tile: the launch number whose owned rows are in y; [nblocks + 1] = the ticket counter
    uint32_t *h_gave_up = nullptr, *d_gave_up = nullptr;   // one word of mapped host memory: a super-tile hit its spin bound
    uint32_t ticket_next = 0;      // value of the ticket counter when the next launch begins (guarded by mu_launch)
    uint32_t spin_bound = 1u << 22;
    int use_ticket = -1;           // option "ticket": -1 = ticket_auto
    uint32_t uniform_cols = 0;     // 1 + the length of every column when all columns have one length (the kernel computes colptr), else 0
    int ticket_auto = 0;           // plan: the launch has more workgroups than the device holds at once
    int handoff_timeouts = 0;      // products of this handle that hit the spin bound (their y was invalid)
    uint32_t epoch = 0;            // launch number (guarded by mu, with ev_last)
    hipEvent_t ev_last = nullptr;  // launches of one handle run one after the other (they share d_flags): stream order, or this event across streams
    hipStream_t last_stream = nullptr;
    int last_stream_valid = 0;
    std::mutex mu_launch;          // ... chained under this lock
    // row tiles (spal_csc_rowtiles.hip): the entries a second time, ordered (row tile, column, row) -- a workgroup owns rows
    // of y outright, no hand-off; built where every tile's window of x fits LDS, and then the scatter path's default
    int rowtiles = 0;              // the copy is built
    int rowtiles_failed = 0;       // building it failed (out of memory, ...): the column tiles run instead
    int rowtiles_user = -1;        // option "row_tiles": -1 / 1 = where it qualifies, 0 = never (the column tiles run)
    uint32_t rt_rows = 0, rt_ntiles = 0, rt_xcap = 0;   // rows of a tile, tiles, widest x window (elements)
    uint32_t rt_rows_user = 0;     // option "row_tile_rows": 0 = the tallest of 4096 / 2048 / 1024 that fits
    void *d_rt_val = nullptr;      // nnz (+pad)
    uint32_t *d_rt_meta = nullptr; // nnz (+pad): (row - tile's first row) | (col - window's first column) << 16
    uint32_t *d_rt_ptr = nullptr;  // ntiles + 1
    uint4 *d_rt_desc = nullptr;    // {first row, rows, first column of the x window, columns}
    int all_lds = 0;               // every super-tile with entries is in LDS mode: y needs no memset
    int cols_per_block = 1024;     // columns of a super-tile: 4096 / 2048 / 1024 (the widest whose row windows fit LDS)
    int user_cols = 0;             // option "cols_per_block" (0 = automatic)
    uint32_t nblocks = 0;
    uint32_t lds_entries = 0;      // largest LDS y window (elements); 0 = global scatter only
    double lds_col_fraction = 0.0;
    int use_lds = 1;
    int kernel = 2;                // 1 = atomic scatter (LDS-privatised / global), 2 = transposed (CSR kernels; default)
    spal_csr *as_csr = nullptr;    // the CSR twin: the same matrix as CSR.  INVARIANT: every live spal_csc owns one, built on the
                                   // device by its constructor (csc_finish) and kept until csc_free -- kernel 2, SpMM and the
                                   // triangular solve read it without asking
    int lanes_per_col = 0;
    std::mutex mu;
    void *d_x = nullptr, *d_y = nullptr;
    hipStream_t stream = nullptr;
    spal::OpState ops;             // as spal_csr's; SpMM, the solve and the factorisation run on as_csr
};

struct spal_coo {
    int device = 0;
    int elem_size = 8;
    uint64_t nrows = 0, ncols = 0, len = 0;
    uint32_t *d_rows = nullptr, *d_cols = nullptr;
    void *d_vals = nullptr;
    void *d_work = nullptr;   // sort buffers + scratch of the assembly, allocated at upload
    // a HINT only: the fullest group of rows [0] / columns [1] the last assembly met (it picks the group kernel's LDS
    // capacity without a host round trip; the kernel verifies it, see coo_local_sort).  Nothing else about the triplets
    // is kept between assemblies.
    uint32_t cap_hint[2] = {0, 0};
    int loop_hint[2] = {0, 0};   // the last assembly by rows [0] / columns [1] met a row beyond the network form's reach
    int last_row_sort = 0;
    size_t work_bytes = 0;
    void *h_back = nullptr;   // pinned host memory the assembly's few results come back into
    size_t h_back_bytes = 0;
    std::mutex mu;            // serialises assemblies on one handle (shared workspace)
    int last_group_rows = 0, last_group_cap = 0;  // geometry of the last assembly's local sort (0 = general route)
    int last_relaunches = 0;        // group kernel launched again because the capacity hint was too small
    int last_lookback_gave_up = 0;  // assemblies of this handle whose look-back hit its spin bound (backstop taken)
    int last_ticket = 0, last_packed = 0, last_offsets = 0;   // how ids were handed out (0 blockIdx, 1 one counter, 8 class counters); packed payload; offsets from the passes' counts
};

namespace spal {
// implemented in spal_csr_plan.hip: chooses the kernel family of the products and builds its tables
int csr_plan_build(spal_csr *a);
constexpr uint32_t kWinBase = 256;     // rows per entry of spal_csr::win_base, the planner's cache of column windows
// implemented in spal_csr_split.hip (for csr_plan_build): the row split, *did = it was built; and, once it is, the
// block-window kernel timed against it (the faster form stays)
int csr_try_row_split(spal_csr *a, bool *did);
int csr_blockwin_or_split(spal_csr *a);
// implemented in spal_csr.hip
int csr_launch(spal_csr *a, const void *x_dev, void *y_dev, hipStream_t stream);          // ensures the plan, then:
int csr_launch_planned(spal_csr *a, const void *x_dev, void *y_dev, hipStream_t stream);  // (the plan exists or the caller is building it)
int csr_ensure_plan(spal_csr *a, hipStream_t launch_stream, bool from_launch);
void csr_free(spal_csr *a);            // the handle and everything it owns (NULL is fine)
// implemented in spal_spmm.hip: Y = A * X enqueued on `stream` (tile 0 = automatic); reads a's plain arrays only, no plan
int spmm_launch(spal_csr *a, int tile, uint64_t k, const void *x_dev, uint64_t ldx, void *y_dev, uint64_t ldy,
                hipStream_t stream);
// implemented in spal_trsv.hip: frees a handle's solve plans (csr_free)
void trsv_free(spal_csr *a);
// implemented in spal_trsv_sweep.hip: frees a handle's sweep preparation (csr_free)
void trsv_sweep_free(spal_csr *a);
// implemented in spal_csr_slide.hip: the sliding-window kernel for a plan with plan.slide set
hipError_t launch_slide(const spal_csr *a, const void *x, void *y, hipStream_t st);
// ... its plan (for csr_plan_build): decides whether it can run the chosen stream plan and builds its step descriptors
int slide_plan(spal_csr *a, uint32_t rpt, const std::vector<uint4> &desc, const std::vector<uint32_t> &skip, uint32_t super_pages);
// ... the row records of a plan that qualifies (after col16 is encoded: they are verified against it), and their release
int rowrec_plan(spal_csr *a);
void rowrec_free(spal_csr *a);
inline bool rowrec_runs(const spal_csr *a) { return a->plan.rowrec && a->plan.rowrec_on && a->d_rowrec; }
// ... and the packed values of a plan with records (after rowrec_plan), their release
int valpack_plan(spal_csr *a);
void valpack_free(spal_csr *a);
inline bool valpack_runs(const spal_csr *a) { return rowrec_runs(a) && a->plan.valpack && a->plan.valpack_on && a->d_valpack; }
// ... and the column-panel kernel over a->d_ptiles
hipError_t launch_panel(const spal_csr *a, const void *x, void *y, hipStream_t st);
// The CSC scatter route over column tiles.  Implemented in spal_csc_plan.hip: windows, modes, hand-off eligibility, then
// csc_rowtiles_plan
int csc_plan_build(spal_csc *a);
constexpr uint32_t kCscModeGlobal = 0, kCscModeLds = 1;   // desc[b].z of a super-tile: one global atomic per entry / LDS window
constexpr uint32_t kCscChunk = 1024;                      // rows per chunk of the two-phase flush's cover lists
// ... and in spal_csc_scatter.hip: the kernel's launcher (hipErrorLaunchTimeOut: an earlier product gave up in the
// hand-off, nothing was launched), and what the plan asks about the kernel
hipError_t launch_csc_scatter(spal_csc *a, const void *x, void *y, hipStream_t st);
uint32_t csc_window_budget(const spal_csc *a, int cols);   // elements of the largest LDS y window beside `cols` columns of x
size_t csc_scatter_lds_bytes(const spal_csc *a);           // dynamic LDS of a launch under the current plan
int csc_scatter_per_cu(const spal_csc *a);                 // workgroups a CU holds at that size (0: the runtime cannot say)
// the hand-off's give-up word: consumed under a->mu_launch (true: a product gave up since the last look; the handle
// leaves the hand-off and counts it), and the invalid products so far, consumed or not
bool csc_gave_up_consume(spal_csc *a);
int csc_invalid_products(const spal_csc *a);
// implemented in spal_csc_rowtiles.hip: CSC scatter over row tiles
int csc_rowtiles_plan(spal_csc *a);
void csc_rowtiles_free(spal_csc *a);
hipError_t launch_csc_rowtiles(const spal_csc *a, const void *x, void *y, hipStream_t st);
// implemented in spal_csr_cblock.hip: the column-blocked kernel (tiled copy of the matrix, x slices kept in L2)
int cblock_plan(spal_csr *a, bool force);
void cblock_free(spal_csr *a);
hipError_t launch_cblock(const spal_csr *a, const void *x, void *y, hipStream_t st);
// spal_csr_blockwin.hip: skewed row lengths with columns near the rows -- entries streamed, one LDS window of x per row block
int blockwin_plan(spal_csr *a);        // measures the windows; a->bw_rows != 0 when the matrix fits the kernel
void blockwin_free(spal_csr *a);
hipError_t blockwin_launch(const spal_csr *a, const void *x, void *y, hipStream_t st);
// builds a handle around device arrays it takes ownership of (used by the COO
// assembly, which produces CSR directly on the device)
// (cap_entries = allocated entries of d_colind / d_values; re-allocated with
// padding when smaller than nnz + the kernels' over-read margin)
// (d_win_groups: optional {first column, one past the last} of every group of 2^win_group_bits <= 256 rows, on the
//  device, if the caller has it; ownership passes to the handle)
int csr_adopt_device(int device, int elem_size, uint64_t nrows, uint64_t ncols,
                     uint64_t nnz, uint64_t cap_entries, uint32_t *d_rowptr,
                     uint32_t *d_colind, void *d_values, spal_csr **out,
                     bool eager_copies = false, bool lazy_plan = false,
                     uint2 *d_win_groups = nullptr, uint32_t win_groups = 0, uint32_t win_group_bits = 0);
}  // namespace spal
