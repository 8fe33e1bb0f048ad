// spal_colour.hip -- multicolour reordering on the device: the greedy colouring of include/spal.h by
// Jones-Plassmann rounds, B = P A P^T for any permutation, and the vector gather / scatter that go with it.
//
// THE COLOURING.  The text visits the rows by descending key(i) = mix32(i + seed); a row takes the smallest colour none
// of its already-visited neighbours has.  "Already visited" is "has a higher key", so row v's colour is a function of
// the colours of its higher-key neighbours alone, and any schedule that colours v after them returns the text's
// colours.  A round is one launch over the rows still uncoloured; row v is READY in round r when every higher-key
// neighbour (of A's row v or of A^T's row v) was coloured in a round BEFORE r.  Lower-key neighbours are never looked
// at: they may or may not be coloured already, and must not matter.
//
// ONE ARRAY, WRITTEN IN PLACE.  state[v] = (round + 1) << 32 | colour, 0 while uncoloured: one aligned 64-bit word, read
// and written whole.  A row coloured in round r carries stamp r + 1; a reader in round r counts a neighbour as coloured
// only if its stamp is <= r, so it makes no difference whether a store of the same launch is seen or not: the round in
// which a row is coloured is 1 + the latest round among its higher-key neighbours, whatever the hardware's order.
// rounds = the longest path of descending keys, in vertices.  A word is written once and never changes.
//
// ORDER BETWEEN ROUNDS IS STREAM ORDER ALONE: no flags, no spins, no grid sync (the rule of DESIGN 3.11).  The rows left
// over by a round are appended to the other of two lists (one atomic per wave); three counters rotate so that a round
// reads its input count, adds to its output count and zeroes the next round's output count without a launch in
// between.  The host enqueues a BATCH of rounds with a grid for the count it last read, then reads the poll block
// (counts, largest colour, last round); a batch doubles from 8 to 512 rounds, so that a chain of thousands of rounds is
// a few dozen polls.  Rounds enqueued past the end find a count of 0 and return.
//
// THE SMALLEST FREE COLOUR is found in windows of 64 colours, a 64-bit mask per window; the first window is filled by
// the pass that tests readiness.  A colour never exceeds the number of higher-key neighbours, so the windows end.  A
// thread owns a row, whatever its length (rows of thousands of neighbours are correct and slow: they are read once per
// round until the first uncoloured higher-key neighbour, and once per window when ready).
#define SPAL_OPS_SCAN
#include "spal_ops.hpp"

namespace spal {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kFirstBatch = 8, kMaxBatch = 512;

// what the host reads between two batches: 20 bytes
struct Poll {
    uint32_t count[3];     // rows uncoloured at the start of round r: count[r % 3]
    uint32_t ncolours;     // 1 + the largest colour so far
    uint32_t rounds;       // 1 + the last round that coloured a row
};

struct Graph {
    const uint32_t *__restrict__ ptr, *__restrict__ ind;     // the operand's rows ...
    const uint32_t *__restrict__ tptr, *__restrict__ tind;   // ... and its transpose's
    uint32_t seed;
};

__device__ __forceinline__ uint64_t state_load(const uint64_t *state, uint32_t u) {
    return __atomic_load_n(state + u, __ATOMIC_RELAXED);
}

// One pass over the higher-key neighbours of v listed in ind[p0, p1): false as soon as one of them was not coloured
// before round r; else their colours inside [base, base + 64) are added to mask.
__device__ __forceinline__ bool scan_neighbours(const uint32_t *__restrict__ ind, uint32_t p0, uint32_t p1, uint32_t v,
                                                uint32_t kv, uint32_t seed, const uint64_t *state, uint32_t r,
                                                uint32_t base, uint64_t &mask) {
    for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t u = ind[p];
        if (u == v || colour_mix32(u + seed) < kv) continue;
        const uint64_t s = state_load(state, u);
        const uint32_t stamp = (uint32_t)(s >> 32);
        if (stamp == 0 || stamp > r) return false;   // uncoloured, or coloured by this very launch
        const uint32_t c = (uint32_t)s - base;       // (wraps below base: >= 64)
        if (c < 64) mask |= 1ull << c;
    }
    return true;
}

// Round r.  FIRST: round 0, whose list is every row.  list_in / list_out: the two halves of one block.
template <bool FIRST>
__global__ __launch_bounds__(kThreads) void colour_round(Graph g, uint32_t n, uint32_t r, uint64_t *state,
                                                         const uint32_t *__restrict__ list_in,
                                                         uint32_t *__restrict__ list_out, Poll *poll) {
    const uint32_t count = FIRST ? n : poll->count[r % 3];
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k == 0) poll->count[(r + 2) % 3] = 0;   // round r + 1 adds to it; round r - 1 read it, nobody touches it now
    bool left = false;
    uint32_t v = 0;
    if (k < count) {
        v = FIRST ? k : list_in[k];
        const uint32_t kv = colour_mix32(v + g.seed);
        const uint32_t a0 = g.ptr[v], a1 = g.ptr[v + 1], t0 = g.tptr[v], t1 = g.tptr[v + 1];
        uint64_t mask = 0;
        bool ready = scan_neighbours(g.ind, a0, a1, v, kv, g.seed, state, r, 0, mask) &&
                     scan_neighbours(g.tind, t0, t1, v, kv, g.seed, state, r, 0, mask);
        if (ready) {
            uint32_t base = 0;
            while (mask == ~0ull) {   // the window is full: the next 64 colours
                base += 64;
                mask = 0;
                (void)scan_neighbours(g.ind, a0, a1, v, kv, g.seed, state, r, base, mask);
                (void)scan_neighbours(g.tind, t0, t1, v, kv, g.seed, state, r, base, mask);
            }
            const uint32_t c = base + (uint32_t)__ffsll((unsigned long long)~mask) - 1;
            __atomic_store_n(state + v, (uint64_t)(r + 1) << 32 | c, __ATOMIC_RELAXED);
            atomicMax(&poll->ncolours, c + 1);
            atomicMax(&poll->rounds, r + 1);
        }
        left = !ready;
    }
    // the rows left over, appended in any order: one atomic per wave
    const uint64_t m = __ballot(left);
    if (m) {
        const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((unsigned long long)m) - 1;
        uint32_t at = 0;
        if (lane == leader) at = atomicAdd(&poll->count[(r + 1) % 3], (uint32_t)__popcll(m));
        at = __shfl(at, leader, 64);
        if (left) list_out[at + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = v;
    }
}

// colour[v] as the 32-bit minor index of a one-entry row (for the ordering) and / or as the caller's uint64
__global__ __launch_bounds__(kThreads) void colour_unpack(const uint64_t *__restrict__ state, uint32_t n,
                                                          uint32_t *__restrict__ c32, unsigned long long *__restrict__ c64) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    const uint32_t c = (uint32_t)state[v];
    if (c32) c32[v] = c;
    if (c64) c64[v] = c;
}

__global__ __launch_bounds__(kThreads) void iota(uint32_t *__restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = i;
}

// inv[perm[i']] = i', and the length of new row i' (len[n] = 0 closes the scan)
__global__ __launch_bounds__(kThreads) void permute_rows(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ ptr,
                                                         uint32_t n, uint32_t *__restrict__ inv, uint32_t *__restrict__ len) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        len[n] = 0;
        return;
    }
    const uint32_t old = perm[i];
    inv[old] = i;
    len[i] = ptr[old + 1] - ptr[old];
}

// Relabel and gather, a thread per entry of the result: entry q of new row i' is entry (q - newptr[i']) of old row
// perm[i'], its column relabelled; the columns of a row come out in A's order, not ascending (the transposes sort them).
template <typename T>
__global__ __launch_bounds__(kThreads) void permute_gather(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ inv,
                                                           const uint32_t *__restrict__ newptr, uint32_t n, uint32_t nnz,
                                                           const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ ind,
                                                           const T *__restrict__ val, uint32_t *__restrict__ oind,
                                                           T *__restrict__ oval) {
    const uint64_t q64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q64 >= nnz) return;
    const uint32_t q = (uint32_t)q64;
    uint32_t lo = 0, hi = n;   // the last row i' with newptr[i'] <= q (rows without entries are skipped by "last")
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (newptr[mid] <= q) lo = mid;
        else hi = mid;
    }
    const uint32_t p = ptr[perm[lo]] + (q - newptr[lo]);
    oind[q] = inv[ind[p]];
    oval[q] = val[p];
}

// direction 0: y[i'] = x[perm[i']];  1: y[perm[i']] = x[i']
template <typename T>
__global__ __launch_bounds__(kThreads) void permute_vec(const uint32_t *__restrict__ perm, uint32_t n, int direction,
                                                        const T *__restrict__ x, T *__restrict__ y) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (direction == 0) y[i] = x[perm[i]];
    else y[perm[i]] = x[i];
}

// ---- host side -----------------------------------------------------------------------------------------------------

struct Colouring {
    DevBuf state;          // n x uint64
    uint64_t ncolours = 0, rounds = 0, polls = 0;
    float ms = 0.f;
};

// square, not held as row blocks: what every entry point here asks of its operand
template <typename H>
int check_operand(const char *fn, const H *a) {
    if (row_blocks(a)) return refuse_row_blocks(fn);
    if (a->nrows != a->ncols)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (%llu x %llu)", fn,
                    (unsigned long long)a->nrows, (unsigned long long)a->ncols);
    return SPAL_OK;
}

// The colours of op's graph into out.state; synchronises `st`.  (The graph of A^T is A's: a CSC handle's arrays serve.)
int colour_run(const char *fn, int device, int elem_size, const Operand &op, uint64_t seed, hipStream_t st, Colouring &out) {
    const uint32_t n = (uint32_t)op.nmajor;
    OpArrays t;   // the operand's transpose: its rows are the other half of every row's neighbours
    SPAL_TRY(transpose_device(device, elem_size, op.nmajor, op.nminor, op.nnz, op.ptr, op.ind, op.val, st, t));
    DevBuf lists, poll;
    SPAL_HIP_TRY(out.state.alloc((size_t)n * 8));
    SPAL_HIP_TRY(lists.alloc((size_t)n * 8));
    SPAL_HIP_TRY(poll.alloc(sizeof(Poll)));
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(1));
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    SPAL_HIP_TRY(hipMemsetAsync(out.state.p, 0, (size_t)n * 8, st));
    SPAL_HIP_TRY(hipMemsetAsync(poll.p, 0, sizeof(Poll), st));
    const Graph g{op.ptr, op.ind, t.ptr, t.ind, (uint32_t)seed};
    uint32_t *half[2] = {lists.as<uint32_t>(), lists.as<uint32_t>() + n};
    Poll h{};
    uint32_t r = 0, left = n, batch = kFirstBatch;
    while (left) {
        const unsigned grid = grid_of(left, kThreads);
        for (uint32_t i = 0; i < batch; ++i, ++r) {
            // round r reads the list round r - 1 wrote: half[r & 1]; round 0 reads none
            if (r == 0)
                hipLaunchKernelGGL(colour_round<true>, dim3(grid), dim3(kThreads), 0, st, g, n, r, out.state.as<uint64_t>(),
                                   (const uint32_t *)nullptr, half[1], poll.as<Poll>());
            else
                hipLaunchKernelGGL(colour_round<false>, dim3(grid), dim3(kThreads), 0, st, g, n, r, out.state.as<uint64_t>(),
                                   (const uint32_t *)half[r & 1], half[(r + 1) & 1], poll.as<Poll>());
        }
        SPAL_HIP_TRY(hipGetLastError());
        SPAL_HIP_TRY(hipMemcpyAsync(&h, poll.p, sizeof h, hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        ++out.polls;
        const uint32_t now = h.count[r % 3];   // what round r would start with
        if (now >= left && h.rounds + batch <= r)
            return fail(SPAL_ERR_HIP, "%s: %u rounds coloured no row (%u left): internal error", fn, batch, now);
        left = now;
        batch = std::min(batch * 2, kMaxBatch);
    }
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    out.ncolours = h.ncolours;
    out.rounds = h.rounds;
    out.ms = ev.ms(1);
    return SPAL_OK;
}

// perm (new -> old, n x uint32, the caller's) from the colours: a stable sort of the rows by colour, which is what the
// transpose does to the entries of a matrix with one entry per row whose column is the row's colour
int order_by_colour(int device, const Colouring &c, uint32_t n, hipStream_t st, DevBuf &perm) {
    DevBuf ptr, col;
    SPAL_HIP_TRY(ptr.alloc(((size_t)n + 1) * 4));
    SPAL_HIP_TRY(col.alloc((size_t)n * 4));
    hipLaunchKernelGGL(iota, dim3(grid_of((uint64_t)n + 1, kThreads)), dim3(kThreads), 0, st, ptr.as<uint32_t>(), n + 1);
    hipLaunchKernelGGL(colour_unpack, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, st,
                       (const uint64_t *)c.state.p, n, col.as<uint32_t>(), (unsigned long long *)nullptr);
    SPAL_HIP_TRY(hipGetLastError());
    OpArrays bycolour;   // (the "values" that travel with the rows are the state words: any 8 bytes per row would do)
    SPAL_TRY(transpose_device(device, 8, n, c.ncolours, n, ptr.as<uint32_t>(), col.as<uint32_t>(), c.state.p, st, bycolour));
    SPAL_HIP_TRY(perm.alloc((size_t)n * 4));
    SPAL_HIP_TRY(hipMemcpyAsync(perm.p, bycolour.ind, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    return SPAL_OK;
}

// P op P^T for the device permutation d_perm into `out` (columns ascending); synchronises `st`
int permute_run(int device, int elem_size, const Operand &op, const uint32_t *d_perm, hipStream_t st, OpArrays &out,
                float *ms) {
    const uint32_t n = (uint32_t)op.nmajor, nnz = (uint32_t)op.nnz;
    EventSpans ev;
    SPAL_HIP_TRY(ev.create(1));
    SPAL_HIP_TRY(hipEventRecord(ev.e[0], st));
    DevBuf inv, len;
    OpArrays g;   // rows permuted, columns relabelled, not yet in order
    SPAL_HIP_TRY(inv.alloc((size_t)n * 4));
    SPAL_HIP_TRY(len.alloc(((size_t)n + 1) * 4));
    SPAL_TRY(g.alloc(n, nnz, (size_t)elem_size, st));
    hipLaunchKernelGGL(permute_rows, dim3(grid_of((uint64_t)n + 1, kThreads)), dim3(kThreads), 0, st, d_perm, op.ptr, n,
                       inv.as<uint32_t>(), len.as<uint32_t>());
    SPAL_HIP_TRY(hipGetLastError());
    SPAL_HIP_TRY(scan_exclusive<uint32_t>(len.as<uint32_t>(), g.ptr, (uint64_t)n + 1, st));
    if (nnz) {
        const dim3 grid(grid_of(nnz, kThreads));
        if (elem_size == 8)
            hipLaunchKernelGGL(permute_gather<double>, grid, dim3(kThreads), 0, st, d_perm, (const uint32_t *)inv.p,
                               (const uint32_t *)g.ptr, n, nnz, op.ptr, op.ind, (const double *)op.val, g.ind, (double *)g.val);
        else
            hipLaunchKernelGGL(permute_gather<float>, grid, dim3(kThreads), 0, st, d_perm, (const uint32_t *)inv.p,
                               (const uint32_t *)g.ptr, n, nnz, op.ptr, op.ind, (const float *)op.val, g.ind, (float *)g.val);
        SPAL_HIP_TRY(hipGetLastError());
    }
    // two stable sorts by the minor index: the first orders every column's rows, the second every row's columns
    OpArrays t;
    SPAL_TRY(transpose_device(device, elem_size, n, n, nnz, g.ptr, g.ind, g.val, st, t));
    SPAL_TRY(transpose_device(device, elem_size, n, n, nnz, t.ptr, t.ind, t.val, st, out));
    SPAL_HIP_TRY(hipEventRecord(ev.e[1], st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    *ms = ev.ms(1);
    return SPAL_OK;
}

// the result's handle around `arrays`, with the permutation and its description
template <typename H>
int adopt_ordered(const H *a, OpArrays &arrays, DevBuf &perm, const Colouring &c, uint64_t seed, float permute_ms, H **out) {
    SPAL_TRY(arrays.adopt(a->device, a->elem_size, a->nrows, a->ncols, out));
    OpState &s = (*out)->ops;
    s.d_perm = (uint32_t *)perm.release();
    s.ordering_colours = c.ncolours;
    char buf[256];
    snprintf(buf, sizeof buf, "{\"colours\": %llu, \"rounds\": %llu, \"seed\": %llu, \"colour_ms\": %.4f, \"permute_ms\": %.4f}",
             (unsigned long long)c.ncolours, (unsigned long long)c.rounds, (unsigned long long)seed, (double)c.ms,
             (double)permute_ms);
    s.ordering_info = buf;
    return SPAL_OK;
}

template <typename H>
int colour_entry(const char *fn, H *a, uint64_t seed, void *stream, uint64_t *colour_host, uint64_t *ncolours,
                 uint64_t *rounds) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    if (!ncolours || !rounds) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    SPAL_TRY(check_operand(fn, a));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    Colouring c;
    SPAL_TRY(colour_run(fn, a->device, a->elem_size, operand_of(a), seed, st, c));
    if (colour_host) {
        const uint32_t n = (uint32_t)a->nrows;
        DevBuf wide;
        SPAL_HIP_TRY(wide.alloc((size_t)n * 8));
        hipLaunchKernelGGL(colour_unpack, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, st, (const uint64_t *)c.state.p, n,
                           (uint32_t *)nullptr, wide.as<unsigned long long>());
        SPAL_HIP_TRY(hipGetLastError());
        SPAL_HIP_TRY(hipMemcpyAsync(colour_host, wide.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
    }
    *ncolours = c.ncolours;
    *rounds = c.rounds;
    return SPAL_OK;
}

template <typename H>
int permute_entry(const char *fn, H *a, const uint64_t *perm_host, uint64_t n, void *stream, H **out) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    if (!out || !perm_host) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    SPAL_TRY(check_operand(fn, a));
    if (n != a->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: perm has %llu entries but the matrix %llu rows", fn, (unsigned long long)n,
                    (unsigned long long)a->nrows);
    std::vector<uint32_t> p32(n);
    std::vector<bool> seen(n, false);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t v = perm_host[i];
        if (v >= n)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: perm[%llu] = %llu is out of range (n = %llu): not a permutation", fn,
                        (unsigned long long)i, (unsigned long long)v, (unsigned long long)n);
        if (seen[v])
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: perm[%llu] = %llu repeats an earlier entry: not a permutation", fn,
                        (unsigned long long)i, (unsigned long long)v);
        seen[v] = true;
        p32[i] = (uint32_t)v;
    }
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    DevBuf perm;
    SPAL_HIP_TRY(perm.alloc(n * 4));
    SPAL_HIP_TRY(hipMemcpyAsync(perm.p, p32.data(), n * 4, hipMemcpyHostToDevice, st));
    OpArrays b;
    float ms = 0.f;
    SPAL_TRY(permute_run(a->device, a->elem_size, operand_of(a), perm.as<uint32_t>(), st, b, &ms));
    return adopt_ordered(a, b, perm, Colouring{}, 0, ms, out);
}

template <typename H>
int multicolour_entry(const char *fn, H *a, uint64_t seed, void *stream, H **out, uint64_t *ncolours) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    if (!out || !ncolours) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    SPAL_TRY(check_operand(fn, a));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const hipStream_t st = (hipStream_t)stream;
    const Operand op = operand_of(a);
    Colouring c;
    SPAL_TRY(colour_run(fn, a->device, a->elem_size, op, seed, st, c));
    DevBuf perm;
    SPAL_TRY(order_by_colour(a->device, c, (uint32_t)a->nrows, st, perm));
    OpArrays b;
    float ms = 0.f;
    SPAL_TRY(permute_run(a->device, a->elem_size, op, perm.as<uint32_t>(), st, b, &ms));
    SPAL_TRY(adopt_ordered(a, b, perm, c, seed, ms, out));
    *ncolours = c.ncolours;
    return SPAL_OK;
}

template <typename H>
int ordering_entry(const char *fn, H *a, uint64_t *perm_host, uint64_t *ncolours) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    if (!perm_host || !ncolours) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (!a->ops.d_perm)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the handle has no ordering (it is no result of permute or multicolour)", fn);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    std::vector<uint32_t> p32(a->nrows);
    SPAL_HIP_TRY(hipMemcpy(p32.data(), a->ops.d_perm, a->nrows * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < a->nrows; ++i) perm_host[i] = p32[i];
    *ncolours = a->ops.ordering_colours;
    return SPAL_OK;
}

template <typename T, typename H>
int vec_checks(const char *fn, H *a, const T *x, const T *y, int direction) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: handle is NULL", fn);
    SPAL_TRY(check_dtype<T>(fn, a->elem_size));
    if (direction != 0 && direction != 1)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: direction = %d must be 0 (into the handle's order) or 1 (back)", fn, direction);
    if (!x || !y) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null vector", fn);
    if (x == y) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x == y (a permutation is not applied in place)", fn);
    if (!a->ops.d_perm)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the handle has no ordering (it is no result of permute or multicolour)", fn);
    return SPAL_OK;
}

template <typename T, typename H>
int vec_dev(const char *fn, H *a, const T *x, T *y, int direction, void *stream) {
    SPAL_TRY(vec_checks<T>(fn, a, x, y, direction));
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const uint32_t n = (uint32_t)a->nrows;
    hipLaunchKernelGGL(permute_vec<T>, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       (const uint32_t *)a->ops.d_perm, n, direction, x, y);
    SPAL_HIP_TRY(hipGetLastError());
    return SPAL_OK;
}

template <typename T, typename H>
int vec_host(const char *fn, H *a, const T *x, uint64_t x_len, T *y, uint64_t y_len, int direction) {
    SPAL_TRY(vec_checks<T>(fn, a, x, y, direction));
    if (x_len != a->nrows || y_len != a->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: x.len() = %llu and y.len() = %llu but the matrix has %llu rows", fn,
                    (unsigned long long)x_len, (unsigned long long)y_len, (unsigned long long)a->nrows);
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const size_t bytes = a->nrows * sizeof(T);
    DevBuf dx, dy;
    SPAL_HIP_TRY(dx.alloc(bytes));
    SPAL_HIP_TRY(dy.alloc(bytes));
    std::lock_guard<std::mutex> lock(a->mu);   // a->stream is the handle's staging stream
    SPAL_HIP_TRY(hipMemcpyAsync(dx.p, x, bytes, hipMemcpyHostToDevice, a->stream));
    SPAL_TRY((vec_dev<T, H>(fn, a, dx.as<T>(), dy.as<T>(), direction, a->stream)));
    SPAL_HIP_TRY(hipMemcpyAsync(y, dy.p, bytes, hipMemcpyDeviceToHost, a->stream));
    SPAL_HIP_TRY(hipStreamSynchronize(a->stream));
    return SPAL_OK;
}

}  // namespace

void ordering_free(OpState &s) {
    (void)dev_free(s.d_perm);
    s.d_perm = nullptr;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_colour(spal_csr_t a, uint64_t seed, void *stream, uint64_t *colour_host, uint64_t *ncolours, uint64_t *rounds) {
    return colour_entry("spal_csr_colour", a, seed, stream, colour_host, ncolours, rounds);
}
int spal_csc_colour(spal_csc_t a, uint64_t seed, void *stream, uint64_t *colour_host, uint64_t *ncolours, uint64_t *rounds) {
    return colour_entry("spal_csc_colour", a, seed, stream, colour_host, ncolours, rounds);
}
int spal_csr_permute(spal_csr_t a, const uint64_t *perm_host, uint64_t n, void *stream, spal_csr_t *out) {
    return permute_entry("spal_csr_permute", a, perm_host, n, stream, out);
}
int spal_csc_permute(spal_csc_t a, const uint64_t *perm_host, uint64_t n, void *stream, spal_csc_t *out) {
    return permute_entry("spal_csc_permute", a, perm_host, n, stream, out);
}
int spal_csr_multicolour(spal_csr_t a, uint64_t seed, void *stream, spal_csr_t *out, uint64_t *ncolours) {
    return multicolour_entry("spal_csr_multicolour", a, seed, stream, out, ncolours);
}
int spal_csc_multicolour(spal_csc_t a, uint64_t seed, void *stream, spal_csc_t *out, uint64_t *ncolours) {
    return multicolour_entry("spal_csc_multicolour", a, seed, stream, out, ncolours);
}
int spal_csr_ordering(spal_csr_t a, uint64_t *perm_host, uint64_t *ncolours) {
    return ordering_entry("spal_csr_ordering", a, perm_host, ncolours);
}
int spal_csc_ordering(spal_csc_t a, uint64_t *perm_host, uint64_t *ncolours) {
    return ordering_entry("spal_csc_ordering", a, perm_host, ncolours);
}
int spal_csr_permute_vec_f64(spal_csr_t a, const double *x, uint64_t x_len, double *y, uint64_t y_len, int direction) {
    return vec_host<double>("spal_csr_permute_vec", a, x, x_len, y, y_len, direction);
}
int spal_csr_permute_vec_f32(spal_csr_t a, const float *x, uint64_t x_len, float *y, uint64_t y_len, int direction) {
    return vec_host<float>("spal_csr_permute_vec", a, x, x_len, y, y_len, direction);
}
int spal_csr_permute_vec_dev_f64(spal_csr_t a, const double *x_dev, double *y_dev, int direction, void *stream) {
    return vec_dev<double>("spal_csr_permute_vec_dev", a, x_dev, y_dev, direction, stream);
}
int spal_csr_permute_vec_dev_f32(spal_csr_t a, const float *x_dev, float *y_dev, int direction, void *stream) {
    return vec_dev<float>("spal_csr_permute_vec_dev", a, x_dev, y_dev, direction, stream);
}
int spal_csc_permute_vec_f64(spal_csc_t a, const double *x, uint64_t x_len, double *y, uint64_t y_len, int direction) {
    return vec_host<double>("spal_csc_permute_vec", a, x, x_len, y, y_len, direction);
}
int spal_csc_permute_vec_f32(spal_csc_t a, const float *x, uint64_t x_len, float *y, uint64_t y_len, int direction) {
    return vec_host<float>("spal_csc_permute_vec", a, x, x_len, y, y_len, direction);
}
int spal_csc_permute_vec_dev_f64(spal_csc_t a, const double *x_dev, double *y_dev, int direction, void *stream) {
    return vec_dev<double>("spal_csc_permute_vec_dev", a, x_dev, y_dev, direction, stream);
}
int spal_csc_permute_vec_dev_f32(spal_csc_t a, const float *x_dev, float *y_dev, int direction, void *stream) {
    return vec_dev<float>("spal_csc_permute_vec_dev", a, x_dev, y_dev, direction, stream);
}

}  // extern "C"
