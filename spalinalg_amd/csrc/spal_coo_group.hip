// spal_coo_group.hip -- the group kernel of the COO assembly (coo_group_sort: one workgroup finishes a group of rows
// in LDS) with its look-back, the selection among its 16 instantiations per type, and the lab statistics of
// -DSPAL_COO_STAMPS builds.
#include "coo_internal.hpp"

#include <numeric>

namespace spal {

// The local sort.  The radix passes order the entries by the row bits ABOVE gbits
// only, so a group of 2^gbits consecutive rows is one contiguous segment
// [gstart[grp], gstart[grp + 1]) that still holds its entries in insertion order.
// One workgroup (4 waves) per group finishes the job in LDS -- in effect the last
// radix pass, the per-row column sort, the duplicate sums and the zero drop in
// one kernel, with one read and one write of the data.  All phases are
// entry-parallel:
//   0. one batch of global loads: (row, col, val) of every entry -> registers.
//      Wave w owns the entries [w * chunk, (w + 1) * chunk) and walks them 64 at
//      a time, so insertion order = (wave, round, lane).
//   1. stable counting sort by the low row bits: the rank of an entry among the
//      group's entries of the same row = entries of earlier waves + earlier
//      rounds of this wave + earlier lanes of this round (ballots and per-wave
//      counters, no atomics); a scan of the row totals gives the row starts rs[].
//      The column goes to c1[rs[row] + rank]: rows contiguous, insertion order
//      inside each row.
//   2. the stable rank of an entry by column inside its row = number of entries
//      j of the row with col_j < col_i, or col_j == col_i and j before i.  The
//      entry is scattered to position rs[row] + rank of c2 / v2 / r2: the group
//      is now sorted by (row, col), equal (row, col) in insertion order.
//      (Quadratic in the row length, which the group capacity bounds.)
//   3. a sorted position starts a run when its (row, col) differs from its
//      predecessor's; the head sums its run left to right = insertion order
//      (coo.rs:42-46); sums that compare equal to zero are dropped (coo.rs:64).
//   4. survivors are numbered in sorted order (ballots + a scan of the 4 x K
//      wave counts); the group learns how many survivors the groups before it
//      hold (group_lookback) and writes its own at their FINAL offsets of
//      colind / values, and rowptr of its rows (LDS counters + a scan).
// state[g] of the look-back below: (status << 32) | count, status 0 = nothing yet, 1 = the group's own number of
// survivors, 2 = survivors of groups 0 ... g inclusive.
constexpr unsigned long long kGroupOwn = 1ull << 32, kGroupUpTo = 2ull << 32;
#ifndef SPAL_COO_LBW
#define SPAL_COO_LBW 1
#endif

// Survivors in all groups before `grp`, for the group that holds `total` of its own: decoupled look-back over the
// groups' 8-byte state words (wave 0 of the workgroup, all 64 lanes: 64 predecessors per round).  The count travels
// IN the word that flags it (relaxed agent-scope stores / loads: written through, read past L1), so no release /
// acquire fence is paid -- with fences (an L2 write-back per group) this form lost to a separate pack kernel.
// Progress: a group waits only for groups with a SMALLER id, and ids are handed out by a device ticket (one atomicAdd
// per workgroup, coo_group_sort) in the order in which workgroups actually start: whoever holds id g started after the
// holders of 0 ... g - 1, which are therefore resident or finished -- the lowest unfinished group waits for nobody,
// whatever order the dispatcher takes the workgroups in.  The spin bound stays as a backstop (a wave that gives up
// raises *err bit 0, publishes nothing further and the host repeats the assembly on the general route; forced by
// SPAL_COO_LOOKBACK_SPINS=0 in tests/test_gpu_csc_coo.py).  (A resident grid whose workgroups walk the
// groups b, b + grid, ... with the next group's loads in flight during the look-back needs no ticket either; it
// was measured and is slower: 1.93 vs 1.68 ms per assembly, the static order keeps a fast workgroup from running ahead.)
// Memory order: the only data a successor reads from a predecessor is the count, and it travels in the SAME 8-byte
// word as the status (single-copy atomic 8-byte store / load at agent scope: sc1, written through to / read from the
// memory side of the per-XCD L2s) -- there is no second location whose visibility would have to be ordered against
// the flag, hence relaxed suffices and no release / acquire fence (an L2 write-back per group) is paid.
// Measured (config 5, profiles/r02/coo_lookback.txt): the wait costs 174 us of coo_group_sort's 750 (groups finish in
// order, so a workgroup also waits out every slower predecessor still in flight) against 193 + 32 us for the pack
// kernel and row scan it replaces, and 1.2 GB less traffic.  Polling 128 or 512 predecessors per round trip is slower
// (1.86 / 1.98 vs 1.75 ms per assembly), the sleep between polls does not matter (1 ... 64: 1.75 - 1.79 ms).
__device__ __forceinline__ uint32_t group_lookback(unsigned long long *state, uint32_t grp, uint32_t total,
                                                   uint32_t lane, uint32_t *err, uint32_t spin_bound,
                                                   uint32_t *dbg = nullptr) {
    constexpr int W = SPAL_COO_LBW;
    if (lane == 0)
        __hip_atomic_store(&state[grp], (grp ? kGroupOwn : kGroupUpTo) | total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (grp == 0) return 0;
#ifdef SPAL_COO_FAKE_LOOKBACK   // lab builds: what the kernel costs WITHOUT the wait (wrong offsets, results discarded)
    if (lane == 0) __hip_atomic_store(&state[grp], kGroupUpTo | (unsigned long long)(grp * 1264u + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return grp * 1264u;
#endif
    uint32_t mine = 0, spins = 0;                         // lane-local part of the sum
    int64_t base = (int64_t)grp - 1;                      // lane 0 looks at the nearest predecessor
    for (;;) {
        // one round trip covers W windows of 64 predecessors (nearest first): W loads per lane issued back to back
        unsigned long long sv[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int64_t idx = base - (int64_t)lane - 64 * j;
            sv[j] = idx >= 0 ? __hip_atomic_load(&state[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                             : kGroupUpTo;                // before group 0: nothing
        }
        uint32_t part = 0;
        bool wait = false, done = false;
#pragma unroll
        for (int j = 0; j < W; ++j) {                     // (all tests wave-uniform)
            if (wait || done) continue;
            const uint32_t status = (uint32_t)(sv[j] >> 32);
            const uint64_t missing = __ballot(status == 0), upto = __ballot(status == 2);
            // the nearest predecessor that knows its inclusive count ends the walk; everyone nearer must have reported
            const uint64_t need = upto ? ((2ull << __builtin_ctzll(upto)) - 1ull) : ~0ull;
            if (missing & need) { wait = true; continue; }
            if ((need >> lane) & 1ull) part += (uint32_t)sv[j];
            if (upto) done = true;
        }
        if (wait) {
            if (++spins > spin_bound) {
                if (lane == 0) atomicOr(err, 1u);
                break;
            }
            __builtin_amdgcn_s_sleep(4);
            continue;
        }
        mine += part;
        if (done) break;
        base -= 64 * W;
    }
    if (dbg) { dbg[0] = spins; dbg[1] = (uint32_t)(((int64_t)grp - 1 - base) / (64 * W)) + 1u; }   // (lab builds: polls that waited, windows walked)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o, 64);
    if (lane == 0)
        __hip_atomic_store(&state[grp], kGroupUpTo | (unsigned long long)(uint32_t)(mine + total), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    return mine;
}

// Bitonic sorting network on N registers (N a power of two, fully unrolled: every compare-exchange is one v_min_u32 and
// one v_max_u32 with compile-time directions) -- a row's columns, one row per thread (coo_group_sort, step 2).
template <int N>
__device__ __forceinline__ void bitonic_sort_regs(uint32_t (&k)[N]) {
#pragma unroll
    for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool up = (i & size) == 0;
                    const uint32_t lo = min(k[i], k[j]), hi = max(k[i], k[j]);
                    k[i] = up ? lo : hi;
                    k[j] = up ? hi : lo;
                }
            }
        }
    }
}
// One thread sorts ONE row's columns: reads the row's L <= N columns out of c1[a ...) (row order = insertion order), sorts
// the keys column << 5 | place-in-row (unique, so ties between equal columns fall in insertion order: stable), and writes
// to every entry's slot its place in (row, col) order instead of its column (the entries keep their columns in registers).
template <int N>
__device__ __forceinline__ void sort_row_in_regs(uint32_t *c1, uint32_t a, uint32_t L) {
    uint32_t key[N];
#pragma unroll
    for (int u = 0; u < N; ++u) key[u] = (uint32_t)u < L ? (c1[a + u] << 5 | (uint32_t)u) : 0xffffffffu;
    bitonic_sort_regs<N>(key);
#pragma unroll
    for (int u = 0; u < N; ++u)
        if ((uint32_t)u < L) c1[a + (key[u] & 31u)] = a + (uint32_t)u;
}

// ---- the group kernel (round 4) ------------------------------------------------------------------------------------
// One workgroup per group, as in round 3; what changed:
//  * ids come from kTicketClasses = 8 counters: workgroup b draws from counter b & 7 and takes id = 8 * ticket + (b & 7)
//    (class c has exactly as many workgroups as ids).  One device atomic on ONE address per workgroup is served at 87 M/s
//    (tools/micro/ticket.hip): 39 063 tickets cost 447 us whatever else happens, +0.13 ms per assembly in round 3; eight
//    addresses are served side by side (72 us per 39 063, spread over the launch).
//  * the per-wave counters of the counting sort are read and written as LDS (lds_peek / lds_poke), not as volatile flat
//    accesses with a full wait each.
//  * PACKED: the last radix pass left column | row-in-group << (32 - gbits) in ONE word (12 instead of 16 bytes per entry).
// Progress.  A group waits only for groups with SMALLER ids.  Class c hands its ids out in the order in which its
// workgroups actually start, so inside a class the holder of an id started after the holders of all smaller ids of that
// class.  Let g* be the lowest unfinished id, of class c.  If a workgroup holds it, it waits for nobody.  If nobody holds
// it yet, every class-c workgroup that has started holds a smaller id and is therefore finished and gone; g* goes to the
// next class-c workgroup the dispatcher starts.  That this workgroup does start is where the single counter of round 3
// assumed nothing and this form assumes something: workgroups b & 7 == c run on XCD c (round-robin dispatch), whose slots
// are only ever taken by class-c workgroups -- all finished, so free; what is assumed is that the dispatcher hands XCD c
// its next workgroup while other XCDs are full of waiting workgroups (no head-of-line blocking across XCDs beyond what
// blockIdx order already implies: under strictly ordered dispatch ids equal blockIdx and no workgroup ever waits for one
// dispatched after it).  The spin bound is the backstop it always was: a look-back that gives up raises the error flag and
// the host repeats the assembly on the general route (tested: SPAL_COO_LOOKBACK_SPINS=0); SPAL_COO_TICKET=1 takes the
// single counter again, 0 takes blockIdx.
// Measured and not kept (profiles/r04/coo_assembly.txt): a RESIDENT grid of occupancy x CUs workgroups walking through
// dynamically drawn groups with the next group's entries in flight in a second register set, its bounds and the ticket
// after that in flight too -- 1.39-1.59 ms for this kernel instead of 0.74, whatever the occupancy (3, 4, 5 workgroups per
// CU): every workgroup holds the ids of its next groups while it works on (or waits in the look-back of) the current one,
// every other workgroup's look-back needs those ids' counts, and whoever falls behind by one iteration stalls everyone by
// one iteration.  One group per workgroup lets the dispatcher start the next group the moment a slot is free; a waiting
// workgroup holds nothing anybody needs.
#ifndef SPAL_COO_PRIO
#define SPAL_COO_PRIO 3   // wave priority of the group kernel's phases before its count is published (0: none); -15 us per assembly
#endif
#ifndef SPAL_COO_LB_1536
#define SPAL_COO_LB_1536 7
#endif
// -DSPAL_COO_STAMPS (lab builds): thread 0 of every workgroup of coo_group_sort records wall_clock64() (100 MHz) at its
// phase boundaries into g_coo_stamps[group][8]; the host writes the phases' mean durations to stderr after the assembly
#ifdef SPAL_COO_STAMPS
__device__ unsigned long long *g_coo_stamps = nullptr;
#define SPAL_STAMP(i) do { if (threadIdx.x == 0 && g_coo_stamps) g_coo_stamps[(size_t)stamp_slot * 16 + (i)] = wall_clock64(); } while (0)
#else
#define SPAL_STAMP(i) do { } while (0)
#endif
// state[] tail behind the groups' look-back words: {error flags, fullest group, single ticket, -, tickets[kTicketClasses]}
// The class counters lie kTicketStride words apart: atomics on ONE line are served one after the other whatever their address in
// the line (87 M/s; eight counters in consecutive words were one hot line -- the 1 792 workgroups of the launch's first round waited
// 18 us for their ids, and the steady 62 M tickets/s kept that line 70 % busy), counters 256 bytes apart are served side by side.
#ifndef SPAL_COO_TICKET_STRIDE
#define SPAL_COO_TICKET_STRIDE 64
#endif
constexpr uint32_t kTicketStride = SPAL_COO_TICKET_STRIDE;
const uint32_t kTailWords = 4 + kTicketClasses * kTicketStride;

// ROWSORT: step 2 by the per-row network and the wave-per-long-row pass (columns below 2^27, rows of at most 256 entries: a
// group with a longer row raises *err bit 2 and the host runs the kernel again with ROWSORT = false, where every entry
// counts its place for itself as in rounds 1-3 -- two kernels rather than two paths in one: the unused path's registers
// were spilled by the used one).
template <typename T, int CAP, bool PACKED, bool ROWSORT>
// (workgroups per CU the LDS footprint allows; eight at CAP = 1536 measured behind seven)
__global__ __launch_bounds__(256, CAP == 1536 ? SPAL_COO_LB_1536 : CAP == 2048 ? 5 : 8) void coo_group_sort(const uint32_t *__restrict__ gstart,
                                                      const uint32_t *__restrict__ sorted_row,
                                                      const uint32_t *__restrict__ cols, const T *__restrict__ vals,
                                                      uint32_t nrows, uint32_t gbits, uint32_t ngroups,
                                                      unsigned long long *__restrict__ state, uint32_t *__restrict__ err,
                                                      uint32_t *__restrict__ tickets, uint32_t ticket_classes, uint32_t spin_bound,
                                                      uint32_t *__restrict__ rowptr, uint32_t *__restrict__ out_col,
                                                      T *__restrict__ out_val, uint2 *__restrict__ gwin) {
    constexpr int K = CAP / 256;  // rounds per wave = sorted positions per thread
    // LDS: the sorted values (written only after every rank is known) share their space with the per-wave row counters
    // and the row starts of the counting sort, which are dead by then -- 21 instead of 26 KB at CAP = 1536 (f64): seven
    // workgroups per CU instead of six.  The survivors' row counters of step 4 live there as well.
    constexpr size_t kCntBytes = 4 * 256 * sizeof(uint32_t), kRsBytes = 260 * sizeof(uint32_t);
    constexpr size_t kRegion = CAP * sizeof(T) > kCntBytes + kRsBytes ? CAP * sizeof(T) : kCntBytes + kRsBytes;
    __shared__ __attribute__((aligned(16))) unsigned char s_region[kRegion];
    T *s_v2 = reinterpret_cast<T *>(s_region);
    // lanes of a wave hand counts to each other through this array between two rounds (lds_peek / lds_poke)
    uint32_t (*s_cnt)[256] = reinterpret_cast<uint32_t (*)[256]>(s_region);
    uint32_t *s_rs = reinterpret_cast<uint32_t *>(s_region + kCntBytes);   // 257 row starts
    __shared__ uint32_t s_c1[CAP];
    uint32_t *s_c2 = s_c1;   // (row, col) order replaces the row order in place (a barrier in between)
    uint32_t *s_rk = reinterpret_cast<uint32_t *>(s_region);   // survivors per row: counted when the sorted values are dead too
    __shared__ uint32_t s_wsum[4], s_wlong[4];
    __shared__ uint32_t s_wc[K * 4];
    __shared__ uint32_t s_cmin, s_cmax;   // columns of the survivors (the CSR planner's window input)
    __shared__ uint32_t s_base, s_total;  // survivors of the groups before this one / of this one
    __shared__ uint8_t s_r2[CAP];
    __shared__ uint32_t s_nlong;          // rows of more than 16 entries, listed for the wave-per-row pass of step 2
    __shared__ uint8_t s_long[256];

    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t lt = (1ull << lane) - 1ull;
#if SPAL_COO_PRIO
    // everything up to the group's published count is what OTHER workgroups wait for in their look-back: those phases run at a
    // raised wave priority, the stores behind the look-back at the normal one
    __builtin_amdgcn_s_setprio(SPAL_COO_PRIO);
#endif
    uint32_t row_len = 0, row_a = 0;      // thread t's row of the group: entries, first place in row order
#ifdef SPAL_COO_STAMPS
    const uint32_t stamp_slot = blockIdx.x;
#endif
    SPAL_STAMP(0);
    // The group this workgroup takes: its ticket (start order inside its class), not its blockIdx (see above).
    if (t == 0) {
        uint32_t id = blockIdx.x;
        if (tickets) {
            if (ticket_classes > 1) {
                const uint32_t cls = blockIdx.x & (kTicketClasses - 1);
                id = atomicInc(&tickets[cls * kTicketStride], 0xffffffffu) * kTicketClasses + cls;
            } else {
                id = atomicInc(tickets, 0xffffffffu);
            }
        }
        s_base = id;
    }
    __syncthreads();
    const uint32_t grp = s_base;                          // < ngroups (ngroups workgroups; every class has as many workgroups as ids)
    SPAL_STAMP(1);
    const uint32_t e0 = gstart[grp], e1 = gstart[grp + 1];
    __syncthreads();                                      // (s_base is written again below)
    SPAL_STAMP(2);
    const uint32_t r0 = grp << gbits;                     // < nrows (there are ceil(nrows / 2^gbits) groups)
    const uint32_t nr = min(1u << gbits, nrows - r0);     // rows of this group, <= 256
    uint32_t n = e1 - e0;
    const bool last = grp + 1 == ngroups;
    // The capacity is the host's guess (the last assembly's fullest group, or mean + 6 sigma): a group that does not
    // fit raises *err bit 1, takes part in the look-back as an empty group (nobody waits for it) and the host runs
    // the kernel again at the capacity the fullest group needs -- the device computes that beside (group_offsets / groups_check).
    if (n > (uint32_t)CAP) {
        if (t == 0) atomicOr(err, 2u);
        n = 0;
    }
    if (n == 0) {  // block-uniform: no entries, but the group's rows start where the groups before it end
        if (w == 0) {
            const uint32_t before = group_lookback(state, grp, 0u, lane, err, spin_bound);
            if (lane == 0) s_base = before;
        }
        __syncthreads();
        const uint32_t before = s_base;
        if (t < nr) rowptr[r0 + t] = before;
        if (last) {
            if (t == 0) rowptr[nrows] = before;
            out_col[before + t] = 0u;                     // the stream kernel's over-read margin (256 entries)
            out_val[before + t] = T(0);
        }
        if (t == 0) gwin[grp] = make_uint2(0xffffffffu, 0u);
        return;
    }
    // 0. one batch of loads (clamped lanes re-read the last entry: every load is issued unconditionally, back to
    // back); wave w owns the entries [w * chunk, (w + 1) * chunk)
    const uint32_t chunk = ((n + 255) / 256) * 64;        // entries per wave, a multiple of 64, <= 64 K
    // (the VALUES are requested later, behind step 2: nothing before the scatter into (row, col) order looks at them, and
    //  their registers -- 12 of 72 for f64 -- are what the row-sorting network of step 2 needs; the kernel is bound by its
    //  VALU instructions, so the other workgroups of the CU cover the wait)
    uint32_t rc[K], pr[K];   // column; (row inside the group) << 16 | position (step 1: among the row's entries, then in the group)
    // (lanes beyond the group's last entry read the next group's entries, or up to 255 entries past the end of the sorted
    //  arrays, which lie inside the workspace -- never looked at: one base address and immediate offsets instead of a clamp
    //  and an address per load.  Price: 3 KB per group that its neighbour fetches again, 0.12 of the 4.85 GB per assembly at
    //  config 5; clamped, the network form spills 37 - 66 registers at seven workgroups per CU.)
    const size_t my0 = (size_t)e0 + w * chunk + lane;
    {
        const uint32_t cmask = gbits ? (0xffffffffu >> gbits) : 0xffffffffu, rshift = 32u - gbits;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (PACKED) {
                const uint32_t q = cols[my0 + 64u * k];
                rc[k] = q & cmask;
                pr[k] = (gbits ? (q >> rshift) : 0u) << 16;
            } else {
                rc[k] = cols[my0 + 64u * k];
                pr[k] = (sorted_row[my0 + 64u * k] - r0) << 16;
            }
        }
    }
    {
        for (uint32_t i = t; i < 4 * 256; i += 256) s_cnt[i >> 8][i & 255] = 0;
        if (t == 0) { s_cmin = 0xffffffffu; s_cmax = 0u; s_nlong = 0u; }
        __syncthreads();
        // 1. stable counting sort by row inside the group
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (64u * k >= chunk) break;  // block-uniform
            const bool ok = w * chunk + 64u * k + lane < n;
            const uint32_t d = pr[k] >> 16;
            uint64_t peers = __ballot(ok);   // lanes of this round with the same row
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint64_t m = __ballot((d >> b) & 1u);
                peers &= ((d >> b) & 1u) ? m : ~m;
            }
            const uint32_t before = ok ? lds_peek(&s_cnt[w][d]) : 0u;
            pr[k] |= before + (uint32_t)__popcll(peers & lt);
            // the lowest peer lane publishes the new count (one writer per row)
            if (ok && (peers & lt) == 0) lds_poke(&s_cnt[w][d], before + (uint32_t)__popcll(peers));
        }
        __syncthreads();
        SPAL_STAMP(3);
        {   // thread d: exclusive prefix of row d's counts over the waves, then the row starts
            uint32_t run = 0;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) {
                const uint32_t c = s_cnt[ww][t];
                s_cnt[ww][t] = run;
                run += c;
            }
            const uint32_t inc = wave_inclusive_scan(run);
            uint32_t longest = run;                             // the longest row of this wave's 64 rows
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, o, 64));
            if (lane == 63) { s_wsum[w] = inc; s_wlong[w] = longest; }
            __syncthreads();
            uint32_t base = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (i < w) base += s_wsum[i];
            s_rs[t] = base + inc - run;
            if (t == 255) s_rs[256] = base + inc;  // = n
            row_len = run;
            row_a = base + inc - run;
        }
        __syncthreads();
        SPAL_STAMP(12);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (64u * k >= chunk) break;
            if (w * chunk + 64u * k + lane < n) {
                pr[k] += s_rs[pr[k] >> 16] + s_cnt[w][pr[k] >> 16];   // place in row order, insertion order inside the row
                s_c1[pr[k] & 0xffffu] = rc[k];
            }
        }
        __syncthreads();
        SPAL_STAMP(13);
        // 2. rank by column inside the row -> (row, col) order.  The kernel is bound by its VALU instructions (8 400 wave
        // instructions per group of 1 280 entries, a wave instruction holds a SIMD for four cycles: profiles/r04/
        // coo_assembly.txt), and the entry-parallel count -- every entry walks its row -- was a third of them.  Now:
        //  * a row of at most kRowNet = 16 entries is sorted by ONE thread in registers (thread t: row t; 80 compare-exchanges
        //    of two instructions) which leaves every entry's place in the entry's slot of c1;
        //  * longer rows (up to 256 entries) are listed and taken by a whole wave each, a lane per entry (four at most), the row
        //    read as broadcasts -- a wave that met one such entry used to walk the loop for all its lanes;
        //  * the entries pick their places up.
        // Rows beyond 256 entries, or columns that leave no 5 bits free: the kernel's other form (ROWSORT = false).
        constexpr uint32_t kRowNet = 16;
        if (ROWSORT) {
            const uint32_t group_longest = max(max(s_wlong[0], s_wlong[1]), max(s_wlong[2], s_wlong[3]));
            if (group_longest > 256u && t == 0) atomicOr(err, 4u);   // (the result is discarded: the host takes the other kernel)
            if (row_len > kRowNet) s_long[atomicAdd(&s_nlong, 1u)] = (uint8_t)t;     // (order of the list does not matter)
            else if (s_wlong[w] > 1u) sort_row_in_regs<16>(s_c1, row_a, row_len);    // (wave-uniform: some row of this wave holds two or more)
            else if (row_len) s_c1[row_a] = row_a;
            __syncthreads();
            for (uint32_t li = w; li < s_nlong; li += 4) {   // wave-uniform
                const uint32_t d = s_long[li], a = s_rs[d], L = min(s_rs[d + 1] - a, 256u);
                uint32_t ci[4], rank[4] = {0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < 4; ++c) ci[c] = s_c1[a + min(lane + 64u * c, L - 1)];
                for (uint32_t j = 0; j < L; ++j) {
                    const uint32_t q = s_c1[a + j];               // one address for the wave: a broadcast
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (64u * c < L) rank[c] += (uint32_t)((q < ci[c]) | ((q == ci[c]) & (j < lane + 64u * c)));   // (wave-uniform test)
                }
#pragma unroll
                for (int c = 0; c < 4; ++c)                       // (after the wave's last read of the row: LDS keeps a wave's order)
                    if (lane + 64u * c < L) s_c1[a + lane + 64u * c] = a + rank[c];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (64u * k >= chunk) break;
                if (w * chunk + 64u * k + lane < n) pr[k] = (pr[k] & 0xffff0000u) | s_c1[pr[k] & 0xffffu];
            }
        } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (64u * k >= chunk) break;
            if (w * chunk + 64u * k + lane < n) {
                const uint32_t d = pr[k] >> 16, a = s_rs[d], b = s_rs[d + 1], ci = rc[k], i = pr[k] & 0xffffu;
                uint32_t rank = 0, j = a;
                for (; j + 4 <= b; j += 4) {
                    const uint32_t q0 = s_c1[j], q1 = s_c1[j + 1], q2 = s_c1[j + 2], q3 = s_c1[j + 3];
                    rank += (uint32_t)((q0 < ci) | ((q0 == ci) & (j < i)));
                    rank += (uint32_t)((q1 < ci) | ((q1 == ci) & (j + 1 < i)));
                    rank += (uint32_t)((q2 < ci) | ((q2 == ci) & (j + 2 < i)));
                    rank += (uint32_t)((q3 < ci) | ((q3 == ci) & (j + 3 < i)));
                }
                for (; j < b; ++j) {
                    const uint32_t q = s_c1[j];
                    rank += (uint32_t)((q < ci) | ((q == ci) & (j < i)));
                }
                pr[k] = (pr[k] & 0xffff0000u) | (a + rank);
            }
        }
        }
        T rv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) rv[k] = vals[my0 + 64u * k];
        __syncthreads();   // every rank is known (and picked up): the row-ordered columns may be overwritten
        SPAL_STAMP(14);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (64u * k >= chunk) break;
            if (w * chunk + 64u * k + lane < n) {
                s_c2[pr[k] & 0xffffu] = rc[k];
                s_v2[pr[k] & 0xffffu] = rv[k];
                s_r2[pr[k] & 0xffffu] = (uint8_t)(pr[k] >> 16);
            }
        }
        __syncthreads();
        SPAL_STAMP(15);
        const uint32_t cur_n = n;
        // 3. heads and run sums; thread t takes the sorted positions t, t + 256, ...
        T acc[K];
        uint32_t kinfo[K];   // bit 31: survivor; low bits: survivors of the same wave round before it
#pragma unroll
        for (int k = 0; k < K; ++k) {
            kinfo[k] = 0;
            acc[k] = T(0);
            if (256u * k >= cur_n) continue;  // block-uniform
            const uint32_t p = 256u * k + t;
            const bool live = p < cur_n;
            const uint32_t pc = live ? p : cur_n - 1, pp = pc ? pc - 1 : 0, pn = min(pc + 1, cur_n - 1);
            const uint32_t cp = s_c2[pc], cprev = s_c2[pp], cnext = s_c2[pn];
            const uint32_t rp = s_r2[pc], rprev = s_r2[pp], rnext = s_r2[pn];
            T a = s_v2[pc];
            const bool head = live && (pc == 0 || cprev != cp || rprev != rp);
            const bool dup = head && pn != pc && cnext == cp && rnext == rp;
            if (__any(dup)) {  // duplicates are rare: most waves skip this
                if (dup) {
                    for (uint32_t q = pc + 1; q < cur_n && s_c2[q] == cp && s_r2[q] == rp; ++q) a = a + s_v2[q];
                }
            }
            const bool keep = head && a != T(0);
            acc[k] = a;
            const uint64_t km = __ballot(keep);
            if (keep) kinfo[k] = 0x80000000u | (uint32_t)__popcll(km & lt);
            if (lane == 0) s_wc[k * 4 + w] = (uint32_t)__popcll(km);
        }
        __syncthreads();
        SPAL_STAMP(4);
        // 4. numbering in sorted order = (round, wave, lane); the group's place in the result (look-back over the
        // groups before it); survivors written at their FINAL offsets; rowptr of the group's rows
        s_rk[t] = 0;   // (in the sorted values' space: the run sums above were their last readers)
        if (t < 64) {  // K * 4 <= 64 wave counts: one wave scans them
            const uint32_t kk = min(t, (uint32_t)(K * 4 - 1));
            const uint32_t c = (t < (uint32_t)(K * 4) && 256u * (kk >> 2) < cur_n) ? s_wc[kk] : 0u;
            const uint32_t inc = wave_inclusive_scan(c);
            if (t < (uint32_t)(K * 4)) s_wc[t] = inc - c;
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
#ifdef SPAL_COO_STAMPS
            uint32_t dbg[2] = {0, 0};
            const uint32_t before = group_lookback(state, grp, total, lane, err, spin_bound, dbg);
            if (t == 0 && g_coo_stamps) {
                g_coo_stamps[(size_t)stamp_slot * 16 + 8] = grp;
                g_coo_stamps[(size_t)stamp_slot * 16 + 9] = dbg[0];
                g_coo_stamps[(size_t)stamp_slot * 16 + 10] = dbg[1];
            }
#else
            const uint32_t before = group_lookback(state, grp, total, lane, err, spin_bound);
#endif
            if (t == 0) { s_base = before; s_total = total; }
        }
#if SPAL_COO_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        __syncthreads();
        SPAL_STAMP(5);
        const uint32_t before = s_base;
        uint32_t cmin = 0xffffffffu, cmax = 0u;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (256u * k >= cur_n) continue;
            if (kinfo[k] >> 31) {
                const uint32_t p = 256u * k + t;
                const uint32_t o = before + s_wc[k * 4 + w] + (kinfo[k] & 0x7fffffffu);
                const uint32_t cp = s_c2[p];
                out_col[o] = cp;
                out_val[o] = acc[k];
                atomicAdd(&s_rk[s_r2[p]], 1u);
                cmin = min(cmin, cp);
                cmax = max(cmax, cp + 1u);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, o, 64));
            cmax = max(cmax, (uint32_t)__shfl_xor((int)cmax, o, 64));
        }
        if (lane == 0) { atomicMin(&s_cmin, cmin); atomicMax(&s_cmax, cmax); }
        __syncthreads();
        if (t == 0) gwin[grp] = make_uint2(s_cmin, s_cmax);
        {   // rowptr[r0 + i] = survivors before the group + those of its rows before row i
            const uint32_t c = s_rk[t];                       // (0 beyond the group's rows)
            const uint32_t inc = wave_inclusive_scan(c);
            if (lane == 63) s_wsum[w] = inc;
            __syncthreads();
            uint32_t pre = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (i < w) pre += s_wsum[i];
            if (t < nr) rowptr[r0 + t] = before + pre + inc - c;
        }
        if (last) {
            const uint32_t nnz = before + s_total;
            if (t == 0) rowptr[nrows] = nnz;
            out_col[nnz + t] = 0u;                            // the stream kernel's over-read margin (256 entries)
            out_val[nnz + t] = T(0);
        }
        SPAL_STAMP(6);
#ifdef SPAL_COO_STAMPS
        __builtin_amdgcn_s_waitcnt(0);   // (the stores have drained)
        SPAL_STAMP(7);
#endif
    }
}

#ifdef SPAL_COO_STAMPS
static unsigned long long *d_stamps = nullptr;   // (lab builds: one buffer per process, never freed)
// before a launch: the stamps' buffer holds ngroups workgroups and is zero
static int stamps_begin(uint32_t ngroups, hipStream_t st) {
    static uint32_t stamps_for = 0;
    if (stamps_for < ngroups) {
        if (d_stamps) (void)hipFree(d_stamps);
        SPAL_HIP_TRY(hipMalloc((void **)&d_stamps, (size_t)ngroups * 16 * 8));
        stamps_for = ngroups;
        SPAL_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_coo_stamps), &d_stamps, sizeof(d_stamps)));
    }
    SPAL_HIP_TRY(hipMemsetAsync(d_stamps, 0, (size_t)ngroups * 16 * 8, st));
    return SPAL_OK;
}
// after a launch: waits for the kernel and writes the phases' durations to stderr
static int stamps_report(uint32_t ngroups, hipStream_t st) {
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    std::vector<unsigned long long> hs((size_t)ngroups * 16);
    SPAL_HIP_TRY(hipMemcpy(hs.data(), d_stamps, hs.size() * 8, hipMemcpyDeviceToHost));
    // order of the stamps in time
    static const int order[12] = {0, 1, 2, 3, 12, 13, 14, 15, 4, 5, 6, 7};
    static const char *name[12] = {"", "ticket", "bounds", "loads+rowsort", "row starts", "placed in row order", "ranks", "sorted arrays",
                                   "heads+sums", "look-back", "stores issued", "stores drained"};
    double sum[12] = {0};
    unsigned long long first = ~0ull, lastt = 0, cnt = 0;
    for (uint32_t g = 0; g < ngroups; ++g) {
        const unsigned long long *q = &hs[(size_t)g * 16];
        if (!q[7]) continue;
        for (int i = 1; i < 12; ++i) sum[i] += (double)(q[order[i]] - q[order[i - 1]]);
        first = std::min(first, q[0]); lastt = std::max(lastt, q[7]); ++cnt;
    }
    if (cnt) {
        fprintf(stderr, "[spal coo stamps] %llu workgroups, kernel %.1f us; mean us per phase:", cnt, (double)(lastt - first) / 100.0);
        double tot = 0;
        for (int i = 1; i < 12; ++i) { fprintf(stderr, " %s %.2f,", name[i], sum[i] / cnt / 100.0); tot += sum[i] / cnt / 100.0; }
        fprintf(stderr, " residence %.2f (= %.0f workgroups in flight on average)\n", tot, tot * (double)cnt / ((double)(lastt - first) / 100.0));
        // who waits for whom: time from start to the published count and the wait behind it, by percentile; the wait
        // a group cannot avoid is the time until the LAST of its predecessors (by id) has published its count
        std::vector<double> pub, wait, spins, wins;
        std::vector<unsigned long long> pub_at(ngroups, 0), ready_at(ngroups, 0);
        for (uint32_t g = 0; g < ngroups; ++g) {
            const unsigned long long *q = &hs[(size_t)g * 16];
            if (!q[7] || q[8] >= ngroups) continue;
            pub.push_back((double)(q[4] - q[0]) / 100.0);
            wait.push_back((double)(q[5] - q[4]) / 100.0);
            spins.push_back((double)q[9]);
            wins.push_back((double)q[10]);
            pub_at[q[8]] = q[4];
            ready_at[q[8]] = q[5];
        }
        double natural = 0, measured = 0;
        unsigned long long latest = 0;
        for (uint32_t id = 0; id < ngroups; ++id) {
            if (!pub_at[id]) continue;
            if (latest > pub_at[id]) natural += (double)(latest - pub_at[id]) / 100.0;
            measured += (double)(ready_at[id] - pub_at[id]) / 100.0;
            latest = std::max(latest, pub_at[id]);
        }
        {   // which phase the slow groups are slow in: per phase p50 / p99, and the phases' means over the slowest 1 % to publish
            std::vector<std::vector<double>> ph(12);
            std::vector<std::pair<double, uint32_t>> by_pub;
            for (uint32_t g = 0; g < ngroups; ++g) {
                const unsigned long long *q = &hs[(size_t)g * 16];
                if (!q[7]) continue;
                for (int i = 1; i < 12; ++i) ph[i].push_back((double)(q[order[i]] - q[order[i - 1]]) / 100.0);
                by_pub.push_back({(double)(q[4] - q[0]) / 100.0, g});
            }
            fprintf(stderr, "[spal coo stamps] p50 / p99 per phase:");
            for (int i = 1; i < 12; ++i) {
                std::sort(ph[i].begin(), ph[i].end());
                fprintf(stderr, " %s %.1f / %.1f,", name[i], ph[i][ph[i].size() / 2], ph[i][(size_t)(0.99 * (ph[i].size() - 1))]);
            }
            std::sort(by_pub.begin(), by_pub.end());
            const size_t n1 = std::max<size_t>(by_pub.size() / 100, 1);
            double slow[12] = {0};
            unsigned long long t_lo = ~0ull, t_hi = 0;
            for (size_t k = by_pub.size() - n1; k < by_pub.size(); ++k) {
                const unsigned long long *q = &hs[(size_t)by_pub[k].second * 16];
                for (int i = 1; i < 12; ++i) slow[i] += (double)(q[order[i]] - q[order[i - 1]]) / 100.0 / (double)n1;
                t_lo = std::min(t_lo, q[0]); t_hi = std::max(t_hi, q[0]);
            }
            fprintf(stderr, "\n[spal coo stamps] the slowest 1 %% to publish (started between %.1f and %.1f us of the kernel), mean us per phase:",
                    (double)(t_lo - first) / 100.0, (double)(t_hi - first) / 100.0);
            for (int i = 1; i < 12; ++i) fprintf(stderr, " %s %.1f,", name[i], slow[i]);
            // start times of the slowest 1 % by decile of the kernel
            int dec[10] = {0};
            for (size_t k = by_pub.size() - n1; k < by_pub.size(); ++k) {
                const unsigned long long *q = &hs[(size_t)by_pub[k].second * 16];
                dec[std::min<int>(9, (int)(10.0 * (double)(q[0] - first) / (double)(lastt - first)))]++;
            }
            fprintf(stderr, "\n[spal coo stamps] their starts by tenth of the kernel:");
            for (int i = 0; i < 10; ++i) fprintf(stderr, " %d", dec[i]);
            fprintf(stderr, "\n");
        }
        auto pct = [](std::vector<double> &v, double p) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[(size_t)(p * (v.size() - 1))]; };
        fprintf(stderr, "[spal coo stamps] start -> count published us: p50 %.1f p90 %.1f p99 %.1f max %.1f; look-back us: p50 %.1f p90 %.1f p99 %.1f max %.1f; "
                "polls that waited: mean %.1f p99 %.0f; windows walked: mean %.2f p99 %.0f max %.0f; mean wait %.2f us of which until the last predecessor had published %.2f us\n",
                pct(pub, 0.5), pct(pub, 0.9), pct(pub, 0.99), pct(pub, 1.0), pct(wait, 0.5), pct(wait, 0.9), pct(wait, 0.99), pct(wait, 1.0),
                std::accumulate(spins.begin(), spins.end(), 0.0) / std::max<size_t>(spins.size(), 1), pct(spins, 0.99),
                std::accumulate(wins.begin(), wins.end(), 0.0) / std::max<size_t>(wins.size(), 1), pct(wins, 0.99), pct(wins, 1.0),
                measured / cnt, natural / cnt);
    }
    return SPAL_OK;
}
#endif

template <typename T>
int launch_group_sort(int cap, bool packed, bool row_sort, const GroupSortArgs<T> &a, hipStream_t st) {
    decltype(&coo_group_sort<T, kGroupCap, true, true>) k_sort;
#define SPAL_GROUP_KERNEL(P, R) (cap == 512 ? coo_group_sort<T, 512, P, R> : cap == 1024 ? coo_group_sort<T, 1024, P, R> \
                                 : cap == 1536 ? coo_group_sort<T, 1536, P, R> : coo_group_sort<T, kGroupCap, P, R>)
    if (packed) k_sort = row_sort ? SPAL_GROUP_KERNEL(true, true) : SPAL_GROUP_KERNEL(true, false);
    else k_sort = row_sort ? SPAL_GROUP_KERNEL(false, true) : SPAL_GROUP_KERNEL(false, false);
#undef SPAL_GROUP_KERNEL
#ifdef SPAL_COO_STAMPS
    SPAL_TRY(stamps_begin(a.ngroups, st));
#endif
    hipLaunchKernelGGL(k_sort, dim3(a.ngroups), dim3(256), 0, st, a.gstart, a.sorted_row, a.cols, a.vals, a.nrows, a.gbits,
                       a.ngroups, a.state, a.err, a.tickets, a.ticket_classes, a.spin_bound, a.rowptr, a.out_col, a.out_val,
                       a.gwin);
    SPAL_HIP_TRY(hipGetLastError());
#ifdef SPAL_COO_STAMPS
    SPAL_TRY(stamps_report(a.ngroups, st));
#endif
    return SPAL_OK;
}
template int launch_group_sort<double>(int, bool, bool, const GroupSortArgs<double> &, hipStream_t);
template int launch_group_sort<float>(int, bool, bool, const GroupSortArgs<float> &, hipStream_t);

}  // namespace spal
