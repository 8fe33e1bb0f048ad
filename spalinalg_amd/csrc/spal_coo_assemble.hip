// spal_coo_assemble.hip -- device-side COO -> CSR / CSC assembly on the stable radix sort of spal_coo_sort.hip.
//
// Contract (reference src/csr/conv/coo.rs:4-115):
//   order entries by (row, col), STABLY w.r.t. insertion order;
//   sum every run of equal (row, col) left to right (separately rounded adds);
//   drop sums that compare equal to zero (-0.0 dropped, NaN kept);
//   emit CSR (columns strictly increasing inside a row).
// rowptr / colind / values are bit-identical to the reference's result: every
// reordering step is stable and each run is summed by ONE thread in insertion
// order.
//
// Pipeline (device only; one read-back at the end: the output size and {flags, fullest group}).  Everything that
// depends on the triplets is computed inside the assembly call; the handle keeps hints only (coo_local_sort):
//   1. stable LSD radix sort by the ROW BITS ABOVE gbits only (8 bits per pass: 2 passes at config 5), carrying
//      (col, value) as payload -- the entries of a group end up contiguous, still in insertion order.  Each pass:
//      per-tile digit histogram -> scan -> scatter that first reorders the tile in LDS so every digit leaves as
//      one contiguous, coalesced run.  Then the offsets of the groups of 2^gbits consecutive rows (about a thousand
//      entries each) in the row-sorted order, and the fullest group, which decides the LDS capacity of step 2
//      (512 ... 2048 entries; the first launch takes a guess).
//   2. one workgroup per group, everything in LDS and entry-parallel: counting sort by the low row bits, stable
//      rank by column inside each row, run heads sum their runs in insertion order, zeros dropped; the group's
//      place in the result comes from a decoupled look-back over the groups before it, and the survivors and
//      the rowptr of the group's rows are written once, at their final offsets.
// If some group holds more than 2048 entries the assembly runs the general
// route -- LSD passes over the column bits first, then all row bits -- and a
// lane-sequential run summation, which is correct for any input, only slower.
#include "coo_internal.hpp"

namespace spal {

// ---- general route (any row length): entries fully sorted by (row, col) ------
template <typename T>
__global__ __launch_bounds__(256) void coo_run_sums(const uint32_t *__restrict__ row,
                                                    const uint32_t *__restrict__ col,
                                                    const T *__restrict__ vals, uint64_t len,
                                                    T *__restrict__ runsum,
                                                    uint32_t *__restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const uint32_t r = row[i], c = col[i];
    uint32_t flag = 0;
    if (i == 0 || row[i - 1] != r || col[i - 1] != c) {
        // coo.rs:42-46: colval[prev] += val, one entry after the other
        T acc = vals[i];
        for (uint64_t j = i + 1; j < len && row[j] == r && col[j] == c; ++j) acc = acc + vals[j];
        runsum[i] = acc;
        flag = (acc != T(0)) ? 1u : 0u;  // coo.rs:64  `colval[ptr] != T::zero()`
    }
    keep[i] = flag;
}

template <typename T>
__global__ __launch_bounds__(256) void coo_compact(const uint32_t *__restrict__ row,
                                                   const uint32_t *__restrict__ col,
                                                   const T *__restrict__ runsum,
                                                   const uint32_t *__restrict__ keep,
                                                   const uint32_t *__restrict__ pos, uint64_t len,
                                                   uint32_t *__restrict__ out_row,
                                                   uint32_t *__restrict__ out_col,
                                                   T *__restrict__ out_val) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len || !keep[i]) return;
    const uint32_t q = pos[i];
    out_row[q] = row[i];
    out_col[q] = col[i];
    out_val[q] = runsum[i];
}

#ifndef SPAL_COO_GROUP_TARGET
#define SPAL_COO_GROUP_TARGET 1400
#endif
// rows of a group the local sort finishes in LDS: about a thousand entries on average
static uint32_t coo_group_bits(uint64_t len, uint64_t n_major) {
    const double mean = (double)len / (double)n_major;
    const uint32_t rbits = bits_for(n_major);
    uint32_t gbits = 8;
    while (gbits > 0 && mean * (double)(1u << gbits) > (double)SPAL_COO_GROUP_TARGET) --gbits;
    if (gbits >= rbits) gbits = rbits - 1;  // at least one pass: it also brings the triplets into the workspace
    return gbits;
}
static uint32_t coo_group_count(uint64_t len, uint64_t n_major) {
    const uint32_t gbits = coo_group_bits(len, n_major);
    return (uint32_t)((n_major + (1ull << gbits) - 1) >> gbits);
}

CooWorkspace coo_workspace_layout(uint64_t len, uint64_t nrows, size_t elem) {
    CooWorkspace w;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += (n + 255) & ~(size_t)255; return r; };
    const uint64_t scan_n = std::max<uint64_t>(len, 1);   // (the general route scans one flag per entry)
    const uint64_t ngroups = len ? coo_group_count(len, nrows) : 1;
    for (int i = 0; i < 2; ++i) {
        w.off_key[i] = take(len * 4);
        w.off_aux[i] = take(len * 4);
        w.off_val[i] = take(len * elem);
    }
    for (int i = 0; i < 2; ++i) {   // PassCounts of the two passes
        w.off_raw[i] = take(256ull * std::max<uint32_t>(sort_stride(len), kHistGroup) * 4);
        w.off_gt[i] = take(256ull * std::max<uint32_t>(sort_groups(len), 1) * 4);
        w.off_dt[i] = take(256 * 4);
    }
    w.off_sums = take(((scan_n + kScanTile - 1) / kScanTile) * 4);
    w.off_state = take(ngroups * 8 + kTailWords * 4);   // the look-back words of coo_group_sort, then {error flags, fullest group, -, -, tickets[8]}
    w.off_total = take(4);
    w.off_gstart = take((ngroups + 1) * 4); // first sorted entry of every group
    (void)take(4096);                       // (the group kernel's last lanes read up to 255 entries past the sorted arrays' end)
    w.bytes = o;
    return w;
}

template <typename T>
SortBuffers<T> coo_workspace_sort_buffers(char *wb, const CooWorkspace &ws) {
    SortBuffers<T> sb;
    for (int i = 0; i < 2; ++i) {
        sb.key[i] = (uint32_t *)(wb + ws.off_key[i]);
        sb.aux[i] = (uint32_t *)(wb + ws.off_aux[i]);
        sb.val[i] = (T *)(wb + ws.off_val[i]);
    }
    sb.counts = PassCounts{(uint32_t *)(wb + ws.off_raw[0]), (uint32_t *)(wb + ws.off_gt[0]), (uint32_t *)(wb + ws.off_dt[0])};
    sb.counts2 = PassCounts{(uint32_t *)(wb + ws.off_raw[1]), (uint32_t *)(wb + ws.off_gt[1]), (uint32_t *)(wb + ws.off_dt[1])};
    sb.sums = (uint32_t *)(wb + ws.off_sums);
    return sb;
}
template SortBuffers<double> coo_workspace_sort_buffers<double>(char *, const CooWorkspace &);
template SortBuffers<float> coo_workspace_sort_buffers<float>(char *, const CooWorkspace &);

CooKnobs coo_read_knobs() {
    CooKnobs k;
    if (const char *e = getenv("SPAL_COO_LOOKBACK_SPINS")) k.lookback_spins = (uint32_t)strtoul(e, nullptr, 10);
    if (const char *e = getenv("SPAL_COO_TICKET")) k.ticket_mode = e[0] == '0' ? 0 : (e[0] == '1' && !e[1]) ? 1 : 8;
    k.no_offsets = getenv("SPAL_COO_NO_OFFSETS") != nullptr;
    k.no_pack = getenv("SPAL_COO_NO_PACK") != nullptr;
    k.loop_ranks = getenv("SPAL_COO_LOOP_RANKS") != nullptr;
    k.debug = getenv("SPAL_COO_DEBUG") != nullptr;
    if (const char *e = getenv("SPAL_COO_EAGER_PLAN")) k.eager_plan = e[0] == '1';
    return k;
}

// What one assembly call works on: the handle, which of its dimensions is the major one, and its bound workspace.
template <typename T>
struct CooJob {
    spal_coo *c;
    int o;                                 // 0 = by rows, 1 = by columns: the index of the handle's hints
    uint64_t len;
    uint32_t nrows, rbits, cbits;          // "rows" = the major index; bits of a major / minor index
    const uint32_t *d_major, *d_minor;     // the uploaded triplets (left untouched)
    hipStream_t st;
    const CooKnobs &knobs;
    CooWorkspace ws;
    char *wb;                              // the workspace block ...
    SortBuffers<T> sb;                     // ... and the sort buffers inside it
};

// the finished arrays leave their DevBufs for the caller (cap >= nnz + 256: see Assembled)
static void hand_over(Assembled &res, DevBuf &ptr, DevBuf &ind, DevBuf &val, uint64_t nnz, uint64_t cap) {
    res.ptr = (uint32_t *)ptr.release(); res.ind = (uint32_t *)ind.release();
    res.val = val.release(); res.nnz = nnz; res.cap = cap;
}

// LDS of the group kernel is 13 B per entry of capacity: the smallest capacity that holds the fullest group
// (more workgroups per CU); none -> general route
static int cap_for(uint32_t fullest) {
    return fullest <= 512 ? 512 : fullest <= 1024 ? 1024 : fullest <= 1536 ? 1536 : fullest <= (uint32_t)kGroupCap ? kGroupCap : 0;
}
struct GroupForm {
    int cap;        // LDS capacity of the group kernel in entries, 0 = none: the general route
    bool row_sort;  // step 2 by the per-row network (false: every entry counts its place for itself)
};
// The retry decision: what the group kernel's flags (bit 0: a look-back gave up waiting, bit 1: a group did not fit the
// capacity, bit 2: a row beyond the network form's reach) and the fullest group say about the next launch.
// The guess was too small: once more at the capacity the fullest group needs (the sorted triplets and
// the groups' offsets stand), or the general route when no capacity holds it; a row beyond the network
// form's reach: once more with the other form.
static GroupForm group_retry(uint32_t flags, uint32_t fullest, GroupForm now) {
    GroupForm next = now;
    next.cap = (flags & 1u) ? 0 : (flags & 2u) ? cap_for(fullest) : now.cap;
    if (flags & 4u) next.row_sort = false;
    return next;
}

// many duplicates summed: do not keep len-sized arrays (trimmed when a quarter or more is unused)
template <typename T>
static int coo_trim(DevBuf &ocol, DevBuf &oval, uint32_t nnz, uint64_t &cap, hipStream_t st) {
    if (((uint64_t)nnz + 256) * 4 > cap * 3) return SPAL_OK;
    DevBuf tcol, tval;
    const uint64_t tcap = (uint64_t)nnz + 256;
    SPAL_HIP_TRY(tcol.alloc(tcap * 4));
    SPAL_HIP_TRY(tval.alloc(tcap * sizeof(T)));
    SPAL_HIP_TRY(hipMemcpyAsync(tcol.p, ocol.p, tcap * 4, hipMemcpyDeviceToDevice, st));
    SPAL_HIP_TRY(hipMemcpyAsync(tval.p, oval.p, tcap * sizeof(T), hipMemcpyDeviceToDevice, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    std::swap(tcol.p, ocol.p);
    std::swap(tval.p, oval.p);
    cap = tcap;
    return SPAL_OK;
}

// ---- local-sort route: sort by the high row bits, the groups' offsets, the group kernel (launched again when its
// capacity or form did not hold), the trim.  *done = the result is in `res`; otherwise (a group beyond every capacity,
// or the look-back gave up waiting -- its backstop: see group_lookback) the caller takes the general route.
// The groups of 2^gbits rows (about a thousand entries on average) that are finished in LDS.  EVERYTHING that
// depends on the triplets is computed here, in the assembly (the reference's `from` counts and scans inside the
// call too, src/csr/conv/coo.rs:9-22; a `push` would invalidate anything kept from an earlier one): both passes'
// digit counts, the groups' offsets (from the sorted keys) and the fullest group.  Only a HINT survives on the
// handle: the fullest group of the last assembly, which picks the LDS capacity of the group kernel without a host
// round trip in the middle; the kernel checks it (a group that does not fit raises a flag) and the device computes
// the true maximum beside, so a wrong hint costs a second launch of that kernel, never a wrong result.
template <typename T>
static int coo_local_sort(CooJob<T> &j, DevBuf &rowptr, Assembled &res, bool *done) {
    spal_coo *c = j.c;
    const CooKnobs &knobs = j.knobs;
    const uint64_t len = j.len;
    hipStream_t st = j.st;
    SortBuffers<T> &sb = j.sb;
    *done = false;
    const uint32_t gbits = coo_group_bits(len, j.nrows);
    const uint32_t ngroups = coo_group_count(len, j.nrows);
    uint32_t guess = c->cap_hint[j.o];
    if (!guess) {   // first assembly: indices spread evenly would give Poisson counts per group -- mean + 6 sigma
        const double gmean = (double)len / (double)ngroups;
        guess = (uint32_t)std::min<double>(gmean + 6.0 * std::sqrt(gmean) + 16.0, (double)kGroupCap);
    }
    // step 2 of the group kernel by the per-row network (columns << 5 | place-in-row must fit a word; a row beyond 256
    // entries sends the assembly to the kernel's other form: remembered on the handle like the capacity)
    GroupForm form{cap_for(guess), j.cbits <= 27 && !c->loop_hint[j.o] && !knobs.loop_ranks};
    if (!form.cap) return SPAL_OK;
    uint32_t *d_gstart = reinterpret_cast<uint32_t *>(j.wb + j.ws.off_gstart);
    // (the groups' column spans stay on the device, in a block of their own that goes with the result: the CSR planner
    //  fetches them when -- if -- a plan is built; round 3 copied 312 KB back inside every assembly)
    DevBuf gwin_buf;
    SPAL_HIP_TRY(gwin_buf.alloc((size_t)ngroups * sizeof(uint2)));
    unsigned long long *d_state = reinterpret_cast<unsigned long long *>(j.wb + j.ws.off_state);
    uint32_t *d_err = reinterpret_cast<uint32_t *>(d_state + ngroups);   // {flags, fullest, -, -, tickets[8]}
    SPAL_HIP_TRY(hipMemsetAsync(d_state, 0, (size_t)ngroups * 8 + kTailWords * 4, st));
    // ---- 1. stable sort by the row bits above gbits, (col, value) carried along; the first pass reads the
    // uploaded triplets directly (they stay untouched).  Exactly two passes (config 5: 16 bits): the groups' offsets
    // come out of the passes' scanned counts (group_offsets), and when a column and the row inside its group fit one
    // word the second pass writes that word instead of key + column (radix_scatter<T, true>).
    const uint32_t sort_bits = j.rbits - gbits;
    const bool two_pass = sort_bits > 8 && sort_bits <= 16 && !knobs.no_offsets;
    const bool packed = two_pass && j.cbits + gbits <= 32 && !knobs.no_pack;
    int cur = 0;
    SPAL_HIP_TRY(radix_sort_bits<T>(sb, len, gbits, sort_bits, cur, st, j.d_major, j.d_minor, (const T *)c->d_vals,
                                    two_pass, packed ? (int)gbits : -1));
    // ---- 2. the groups' offsets in the sorted triplets, and the fullest group (the kernel's capacity is a guess: see above)
    launch_group_starts<T>(sb, cur, two_pass, len, gbits, ngroups, d_gstart, d_err + 1, st);
    // ---- 3. per group: rows, columns, run sums, zero drop in LDS; its place in the result by look-back over
    // the groups before it; survivors and rowptr written at their final offsets.  The result arrays are sized
    // for no entry dropped (the count is only known afterwards) and trimmed when a quarter or more is unused.
    uint64_t cap = len + 256;  // + the stream kernel's over-read margin
    DevBuf ocol, oval;
    SPAL_HIP_TRY(ocol.alloc(cap * 4));
    SPAL_HIP_TRY(oval.alloc(cap * sizeof(T)));
    // what comes back: the last group's state word (survivors of all groups) and {flags, fullest} -- into PINNED host
    // memory kept on the handle (copies into pageable memory cost 0.12 ms of the call)
    const size_t back_bytes = 16;
    if (!c->h_back || c->h_back_bytes < back_bytes) {
        if (c->h_back) { (void)hipHostFree(c->h_back); c->h_back = nullptr; c->h_back_bytes = 0; }
        SPAL_HIP_TRY(hipHostMalloc(&c->h_back, back_bytes, hipHostMallocDefault));
        c->h_back_bytes = back_bytes;
    }
    unsigned long long *tail = reinterpret_cast<unsigned long long *>(c->h_back);
    tail[0] = tail[1] = 0;
    // ids: 8 class counters (default), the single counter of round 3 (SPAL_COO_TICKET=1) or blockIdx (=0)
    const int ticket_mode = knobs.ticket_mode;
    uint32_t *d_tickets = ticket_mode == 0 ? nullptr : ticket_mode == 1 ? d_err + 2 : d_err + 4;
    const GroupSortArgs<T> args{d_gstart, sb.key[cur], sb.aux[cur], sb.val[cur], j.nrows, gbits, ngroups, d_state, d_err,
                                d_tickets, ticket_mode == 1 ? 1u : kTicketClasses, knobs.lookback_spins,
                                rowptr.as<uint32_t>(), ocol.as<uint32_t>(), oval.as<T>(), gwin_buf.as<uint2>()};
    for (int attempt = 0; attempt < 3 && form.cap; ++attempt) {
        SPAL_TRY(launch_group_sort<T>(form.cap, packed, form.row_sort, args, st));
        SPAL_HIP_TRY(hipMemcpyAsync(tail, d_state + (ngroups - 1), 16, hipMemcpyDeviceToHost, st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        const uint32_t flags = (uint32_t)tail[1], fullest = (uint32_t)(tail[1] >> 32);
        c->cap_hint[j.o] = std::max<uint32_t>(fullest, 1u);
        c->last_ticket = ticket_mode;
        c->last_packed = packed ? 1 : 0;
        c->last_offsets = two_pass ? 1 : 0;
        if (knobs.debug)
            fprintf(stderr, "[spal coo] %.2f entries/row -> groups of %u rows, guessed %u, fullest %u, capacity %d, flags %u, ticket mode %d, %s, %s\n",
                    (double)len / (double)j.nrows, 1u << gbits, guess, fullest, form.cap, flags, ticket_mode, packed ? "packed" : "key + column",
                    two_pass ? "offsets from the counts" : "offsets from the sorted keys");
        c->last_row_sort = form.row_sort ? 1 : 0;
        if (!(flags & 6u)) break;              // every group fitted, no row too long for the kernel's form
        form = group_retry(flags, fullest, form);
        if (flags & 4u) c->loop_hint[j.o] = 1;
        c->last_relaunches++;
        if (form.cap) {   // states, flags, tickets (the fullest group stands: it is a property of the sorted triplets)
            SPAL_HIP_TRY(hipMemsetAsync(d_state, 0, (size_t)ngroups * 8 + 4, st));
            SPAL_HIP_TRY(hipMemsetAsync(d_err + 2, 0, (kTailWords - 2) * 4, st));
        }
    }
    if (!(form.cap && (uint32_t)tail[1] == 0 && (tail[0] >> 32) == 2)) {   // a flag stands, or the last group does not know its inclusive count
        if (knobs.debug) fprintf(stderr, "[spal coo] flags %u: general route\n", (uint32_t)tail[1]);
        c->last_lookback_gave_up += ((uint32_t)tail[1] & 1u) ? 1 : 0;
        return SPAL_OK;   // (the result arrays return to the allocator here: the general route sizes its own)
    }
    const uint32_t nnz = (uint32_t)tail[0];
    c->last_group_rows = (int)(1u << gbits);
    c->last_group_cap = form.cap;
    res.d_gwin = (uint2 *)gwin_buf.release(); res.gwin_n = ngroups; res.gwin_bits = gbits;
    SPAL_TRY(coo_trim<T>(ocol, oval, nnz, cap, st));
    hand_over(res, rowptr, ocol, oval, nnz, cap);
    *done = true;
    return SPAL_OK;
}

// ---- general route: sort by column bits, then by row bits (LSD), with the
// column as key first (key <-> aux swapped for the column passes)
template <typename T>
static int coo_general(CooJob<T> &j, DevBuf &rowptr, Assembled &res) {
    const uint64_t len = j.len;
    hipStream_t st = j.st;
    SortBuffers<T> &sb = j.sb;
    uint32_t *total = reinterpret_cast<uint32_t *>(j.wb + j.ws.off_total);
    int cur = 0;
    SPAL_HIP_TRY(radix_sort_bits<T>(sb, len, 0, j.cbits, cur, st, j.d_minor, j.d_major,
                                    (const T *)j.c->d_vals));
    std::swap(sb.key[0], sb.aux[0]);  // now key = row, aux = col
    std::swap(sb.key[1], sb.aux[1]);
    SPAL_HIP_TRY(radix_sort_bits<T>(sb, len, 0, j.rbits, cur, st));
    uint32_t *s_row = sb.key[cur], *s_col = sb.aux[cur];
    T *s_val = sb.val[cur];
    uint32_t *d_keep = sb.key[cur ^ 1], *d_pos = sb.aux[cur ^ 1];  // scratch
    T *runsum = sb.val[cur ^ 1];
    const uint32_t g256 = (uint32_t)((len + 255) / 256);
    hipLaunchKernelGGL(coo_run_sums<T>, dim3(g256), dim3(256), 0, st, s_row, s_col, s_val, len, runsum,
                       d_keep);
    SPAL_HIP_TRY(exclusive_scan_u32(d_keep, d_pos, len, sb.sums, total, st));
    uint32_t nnz = 0;
    SPAL_HIP_TRY(hipMemcpyAsync(&nnz, total, 4, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    DevBuf orow, ocol, oval;
    const uint64_t cap = (uint64_t)nnz + 256;
    SPAL_HIP_TRY(orow.alloc((size_t)nnz * 4));
    SPAL_HIP_TRY(ocol.alloc(cap * 4));
    SPAL_HIP_TRY(oval.alloc(cap * sizeof(T)));
    SPAL_HIP_TRY(hipMemsetAsync((char *)ocol.p + (size_t)nnz * 4, 0, 256 * 4, st));
    SPAL_HIP_TRY(hipMemsetAsync((char *)oval.p + (size_t)nnz * sizeof(T), 0, 256 * sizeof(T), st));
    hipLaunchKernelGGL(coo_compact<T>, dim3(g256), dim3(256), 0, st, s_row, s_col, runsum, d_keep,
                       d_pos, len, orow.as<uint32_t>(), ocol.as<uint32_t>(), oval.as<T>());
    launch_row_starts(orow.as<uint32_t>(), nnz, j.nrows, rowptr.as<uint32_t>(), st);
    SPAL_HIP_TRY(hipGetLastError());
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    hand_over(res, rowptr, ocol, oval, nnz, cap);
    return SPAL_OK;
}

template <typename T>
static int coo_assemble_t(spal_coo *c, bool by_cols, hipStream_t st, const CooKnobs &knobs, Assembled &res) {
    const uint64_t len = c->len;
    const uint64_t n_major = by_cols ? c->ncols : c->nrows, n_minor = by_cols ? c->nrows : c->ncols;
    const uint32_t nrows = (uint32_t)n_major;  // "rows" below = the major index
    DevBuf rowptr;
    SPAL_HIP_TRY(rowptr.alloc(((size_t)nrows + 1) * 4));
    if (len == 0) {  // no entries at all: an empty matrix -- rowptr of zeros and nothing but the over-read margin
        DevBuf ocol, oval;
        SPAL_HIP_TRY(ocol.alloc(256 * 4));
        SPAL_HIP_TRY(oval.alloc(256 * sizeof(T)));
        SPAL_HIP_TRY(hipMemsetAsync(rowptr.p, 0, ((size_t)nrows + 1) * 4, st));
        SPAL_HIP_TRY(hipMemsetAsync(ocol.p, 0, 256 * 4, st));
        SPAL_HIP_TRY(hipMemsetAsync(oval.p, 0, 256 * sizeof(T), st));
        SPAL_HIP_TRY(hipStreamSynchronize(st));
        hand_over(res, rowptr, ocol, oval, 0, 256);
        return SPAL_OK;
    }

    std::lock_guard<std::mutex> lock(c->mu);  // one assembly at a time per handle (shared workspace)
    const CooWorkspace ws = coo_workspace_layout(len, nrows, sizeof(T));
    if (!c->d_work || c->work_bytes < ws.bytes) {
        if (c->d_work) { (void)dev_free(c->d_work); c->d_work = nullptr; }
        SPAL_HIP_TRY(dev_alloc((void **)&c->d_work, ws.bytes));
        c->work_bytes = ws.bytes;
    }
    char *wb = (char *)c->d_work;
    CooJob<T> job{c, by_cols ? 1 : 0, len, nrows, bits_for(n_major), bits_for(n_minor),
                  by_cols ? c->d_cols : c->d_rows, by_cols ? c->d_rows : c->d_cols, st, knobs,
                  ws, wb, coo_workspace_sort_buffers<T>(wb, ws)};
    c->last_group_rows = 0;
    c->last_group_cap = 0;
    c->last_relaunches = 0;
    bool done = false;
    SPAL_TRY(coo_local_sort<T>(job, rowptr, res, &done));
    if (!done) SPAL_TRY(coo_general<T>(job, rowptr, res));
    return SPAL_OK;
}

int coo_assemble(spal_coo *c, bool by_cols, hipStream_t st, const CooKnobs &knobs, Assembled &res) {
    return c->elem_size == 8 ? coo_assemble_t<double>(c, by_cols, st, knobs, res)
                             : coo_assemble_t<float>(c, by_cols, st, knobs, res);
}

}  // namespace spal
