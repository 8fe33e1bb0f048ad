// spal_spgemm.hip -- C = A * B, sparse x sparse: `impl Mul for &CsrMatrix<T>` (src/csr/ops/mul.rs:5-59) and
// `impl Mul for &CscMatrix<T>` (src/csc/ops/mul.rs:5-60) on the device, bit-identical to the reference.
//
// Row-wise Gustavson, count then fill, rows binned by their product count ub[i] = sum over A's row i of nnz(B row k):
//   tier 0       ub == 0: an empty row of C
//   tiers 1..5   ub <= cap: one LDS hash table per row, a group of 16 / 32 / 64 lanes or a whole workgroup per row;
//                a symbolic pass counts the row's distinct columns, a numeric pass accumulates, sorts the occupied
//                slots by column (bitonic in LDS) and writes the row into C
//   tier 6       ub > cap: expand, sort, compress -- the products of these rows in expansion order, two stable
//                transposes (transpose_device) to sort every row by column, one thread folds each run
// THE ORDER INVARIANT (every (i, j) sums its products in ascending k, the first one assigned): the LDS group walks A's row
// in stored (= ascending k) order; at one step its lanes hold distinct entries of ONE row of B, i.e. distinct columns, so
// no two lanes touch one slot within a step; a step is complete and visible before the next (group_sync); the lane whose
// CAS claims an empty slot assigns the product, every later touch adds.  The large tier keeps it by the stability of the
// two transposes (equal columns stay in expansion order = k order) and a left-to-right fold.
#define SPAL_OPS_SCAN
#include "spal_ops.hpp"

// Products are rounded before they are added: no contraction into FMA (the reference's `vec[j] += a * b` is two
// roundings).  tests/test_spgemm_host.py checks the kernels' ISA for fused forms.
#pragma clang fp contract(off)

namespace spal {
namespace {

constexpr uint32_t kEmpty = 0xffffffffu;   // a free hash slot (columns are < 2^32 - 1)
constexpr int kTiers = 7;                  // 0 empty, 1 g16, 2 g32, 3 wave, 4 block (4096 slots), 5 block (8192 slots), 6 large
constexpr uint32_t kDefaultCap = 2048;     // route 0: rows above it go to the large tier
constexpr uint32_t kMaxCap = 4096;         // the largest table the LDS holds (f64: 144 KB)
const char *const kTierNames[kTiers] = {"empty", "g16", "g32", "wave", "block4k", "block8k", "large"};

struct Counters {
    uint32_t tier[8];
    uint32_t cursor[8];
    unsigned long long products, large_products;
};

__device__ __forceinline__ int tier_of(uint32_t ub, uint32_t cap, int route) {
    if (ub == 0) return 0;
    if (route == 2 || ub > cap) return 6;
    return ub <= 64 ? 1 : ub <= 256 ? 2 : ub <= 1024 ? 3 : ub <= 2048 ? 4 : 5;
}

// ---- phase 1: products per row, tiers, row lists ----------------------------------------------------------------
__global__ __launch_bounds__(256) void spgemm_count(const uint32_t *__restrict__ arp, const uint32_t *__restrict__ aci,
                                                    const uint32_t *__restrict__ brp, uint32_t m, uint32_t cap, int route,
                                                    uint32_t *__restrict__ ub_out, uint8_t *__restrict__ tier_out,
                                                    Counters *__restrict__ c) {
    __shared__ uint32_t s_cnt[kTiers];
    __shared__ unsigned long long s_prod[2];
    if (threadIdx.x < kTiers) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_prod[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        uint64_t s = 0;
        for (uint32_t p = arp[i]; p < arp[i + 1]; ++p) {
            const uint32_t k = aci[p];
            s += brp[k + 1] - brp[k];
        }
        const uint32_t ub = s > 0xffffffffull ? 0xffffffffu : (uint32_t)s;
        const int t = tier_of(ub, cap, route);
        ub_out[i] = ub;
        tier_out[i] = (uint8_t)t;
        atomicAdd(&s_cnt[t], 1u);
        if (s) atomicAdd(&s_prod[0], (unsigned long long)s);
        if (t == 6) atomicAdd(&s_prod[1], (unsigned long long)s);
    }
    __syncthreads();
    if (threadIdx.x < kTiers && s_cnt[threadIdx.x]) atomicAdd(&c->tier[threadIdx.x], s_cnt[threadIdx.x]);
    if (threadIdx.x == 0 && s_prod[0]) atomicAdd(&c->products, s_prod[0]);
    if (threadIdx.x == 1 && s_prod[1]) atomicAdd(&c->large_products, s_prod[1]);
}

// rows of tiers 1..6 listed tier after tier (order inside a tier is arbitrary: each row writes only its own part of C)
__global__ __launch_bounds__(256) void spgemm_bin(const uint8_t *__restrict__ tier, uint32_t m, Counters *__restrict__ c,
                                                  uint32_t *__restrict__ list) {
    __shared__ uint32_t s_cnt[kTiers], s_base[kTiers];
    if (threadIdx.x < kTiers) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    int t = 0;
    uint32_t local = 0;
    if (i < m) {
        t = tier[i];
        if (t > 0) local = atomicAdd(&s_cnt[t], 1u);
    }
    __syncthreads();
    if (threadIdx.x > 0 && threadIdx.x < kTiers && s_cnt[threadIdx.x]) {
        uint32_t start = 0;
        for (uint32_t u = 1; u < threadIdx.x; ++u) start += c->tier[u];
        s_base[threadIdx.x] = start + atomicAdd(&c->cursor[threadIdx.x], s_cnt[threadIdx.x]);
    }
    __syncthreads();
    if (t > 0) list[s_base[t] + local] = (uint32_t)i;
}

// ---- LDS tiers -----------------------------------------------------------------------------------------------------
// A step of a group is complete and visible to all its lanes before the next one begins.
template <int G>
__device__ __forceinline__ void group_sync() {
    if constexpr (G > 64) {
        __syncthreads();
    } else {   // the group is part of one wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

__device__ __forceinline__ uint32_t slot_of(uint32_t j, int bits) { return (j * 0x9E3779B1u) >> (32 - bits); }

// One row of the tier per group of G lanes, GPB groups per workgroup, a table of TS slots per group (TS >= 2 ub).
// NUMERIC = false: counts the row's distinct columns into cnt[row].  NUMERIC = true: writes the row at C[off[row] ...).
template <typename T, int G, int TS, int GPB, bool NUMERIC>
__global__ __launch_bounds__(G * GPB) void spgemm_lds(const uint32_t *__restrict__ rows, uint32_t nrows_tier,
                                                      const uint32_t *__restrict__ arp, const uint32_t *__restrict__ aci,
                                                      const T *__restrict__ av, const uint32_t *__restrict__ brp,
                                                      const uint32_t *__restrict__ bci, const T *__restrict__ bv,
                                                      unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ off,
                                                      uint32_t *__restrict__ cci, T *__restrict__ cv) {
    static_assert(G * GPB <= 1024 && (G <= 64 || GPB == 1) && (TS & (TS - 1)) == 0, "group geometry");
    constexpr int BITS = __builtin_ctz(TS);
    constexpr int CS = TS / 2;                 // >= ub >= the row's distinct columns
    constexpr int V = NUMERIC ? GPB : 1;
    constexpr int VS = NUMERIC ? TS : 1;
    constexpr int VC = NUMERIC ? CS : 1;
    __shared__ uint32_t s_key[GPB][TS];
    __shared__ T s_val[V][VS];
    __shared__ uint32_t s_ck[V][VC];
    __shared__ T s_cv[V][VC];
    __shared__ uint32_t s_n[GPB];
    const int g = (int)threadIdx.x / G, lane = (int)threadIdx.x % G;
    const uint32_t slot = blockIdx.x * GPB + g;
    if (slot >= nrows_tier) return;            // (G > 64: GPB == 1, the whole workgroup leaves)
    const uint32_t i = rows[slot];
    uint32_t *key = s_key[g];
    for (int s = lane; s < TS; s += G) key[s] = kEmpty;
    if (lane == 0) s_n[g] = 0;
    group_sync<G>();
    uint32_t claimed = 0;
    for (uint32_t p = arp[i]; p < arp[i + 1]; ++p) {          // k ascending: A's stored order
        const uint32_t k = aci[p];
        const T a = av[p];
        const uint32_t q1 = brp[k + 1];
        for (uint32_t qb = brp[k]; qb < q1; qb += G) {        // a step: distinct entries of B's row k
            const uint32_t q = qb + (uint32_t)lane;
            if (q < q1) {
                const uint32_t j = bci[q];
                uint32_t h = slot_of(j, BITS);
                while (true) {
                    const uint32_t cur = key[h];
                    if (cur == j) {                               // claimed at an earlier step: add
                        if constexpr (NUMERIC) s_val[g][h] = s_val[g][h] + a * bv[q];
                        break;
                    }
                    if (cur == kEmpty) {
                        const uint32_t old = atomicCAS(&key[h], kEmpty, j);
                        if (old == kEmpty) {                      // this lane claims the slot: the first product is assigned
                            if constexpr (NUMERIC) s_val[g][h] = a * bv[q];
                            else ++claimed;
                            break;
                        }
                        if (old == j) {                           // (symbolic pass only: no steps there)
                            if constexpr (NUMERIC) s_val[g][h] = s_val[g][h] + a * bv[q];
                            break;
                        }
                    }
                    h = (h + 1) & (TS - 1);
                }
            }
            if constexpr (NUMERIC) group_sync<G>();
        }
    }
    if constexpr (!NUMERIC) {
        if (claimed) atomicAdd(&s_n[g], claimed);
        group_sync<G>();
        if (lane == 0) cnt[i] = s_n[g];
        return;
    } else {
        // occupied slots -> the compact area (any order), then sorted by COLUMN (never by slot)
        uint32_t *ck = s_ck[g];
        T *cvv = s_cv[g];
        for (int s = lane; s < TS; s += G) {
            const uint32_t kk = key[s];
            if (kk != kEmpty) {
                const uint32_t pos = atomicAdd(&s_n[g], 1u);
                ck[pos] = kk;
                cvv[pos] = s_val[g][s];
            }
        }
        group_sync<G>();
        const uint32_t n = s_n[g];
        uint32_t P = 1;
        while (P < n) P <<= 1;
        for (uint32_t t = n + (uint32_t)lane; t < P; t += G) ck[t] = kEmpty;
        group_sync<G>();
        for (uint32_t kk = 2; kk <= P; kk <<= 1) {
            for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
                for (uint32_t t = (uint32_t)lane; t < P; t += G) {
                    const uint32_t u = t ^ jj;
                    if (u > t) {
                        const bool up = (t & kk) == 0;
                        const uint32_t kt = ck[t], ku = ck[u];
                        if ((kt > ku) == up) {
                            ck[t] = ku; ck[u] = kt;
                            const T vt = cvv[t];
                            cvv[t] = cvv[u]; cvv[u] = vt;
                        }
                    }
                }
                group_sync<G>();
            }
        }
        const unsigned long long o = off[i];
        for (uint32_t t = (uint32_t)lane; t < n; t += G) {
            cci[o + t] = ck[t];
            cv[o + t] = cvv[t];
        }
    }
}

// ---- large tier: expand, sort (two stable transposes), compress ---------------------------------------------------
__global__ __launch_bounds__(256) void spgemm_gather_ub(const uint32_t *__restrict__ list, uint32_t n,
                                                        const uint32_t *__restrict__ ub, uint32_t *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) out[t] = ub[list[t]];
    if (t == n) out[t] = 0;
}

// the products of large row list[t] at sptr[t] ...: k ascending, then B's stored order; the value is the rounded product
template <typename T>
__global__ __launch_bounds__(256) void spgemm_expand(const uint32_t *__restrict__ list, const uint32_t *__restrict__ sptr,
                                                     const uint32_t *__restrict__ arp, const uint32_t *__restrict__ aci,
                                                     const T *__restrict__ av, const uint32_t *__restrict__ brp,
                                                     const uint32_t *__restrict__ bci, const T *__restrict__ bv,
                                                     uint32_t *__restrict__ sci, T *__restrict__ sv) {
    const uint32_t i = list[blockIdx.x];
    uint32_t cur = sptr[blockIdx.x];
    for (uint32_t p = arp[i]; p < arp[i + 1]; ++p) {
        const uint32_t k = aci[p];
        const T a = av[p];
        const uint32_t q0 = brp[k], len = brp[k + 1] - q0;
        for (uint32_t x = threadIdx.x; x < len; x += 256) {
            sci[cur + x] = bci[q0 + x];
            sv[cur + x] = a * bv[q0 + x];
        }
        cur += len;
    }
}

// runs of equal columns in the sorted scratch row blockIdx.x -> cnt[list[blockIdx.x]]
__global__ __launch_bounds__(256) void spgemm_run_count(const uint32_t *__restrict__ list, const uint32_t *__restrict__ rp,
                                                        const uint32_t *__restrict__ ci, unsigned long long *__restrict__ cnt) {
    __shared__ uint32_t s_total;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    const uint32_t b = rp[blockIdx.x], e = rp[blockIdx.x + 1];
    uint32_t heads = 0;
    for (uint32_t x = b + threadIdx.x; x < e; x += 256) heads += (x == b || ci[x] != ci[x - 1]) ? 1u : 0u;
    if (heads) atomicAdd(&s_total, heads);
    __syncthreads();
    if (threadIdx.x == 0) cnt[list[blockIdx.x]] = s_total;
}

// one thread per run: the first product assigned, the rest added left to right; zeros are kept
template <typename T>
__global__ __launch_bounds__(256) void spgemm_run_fill(const uint32_t *__restrict__ list, const uint32_t *__restrict__ rp,
                                                       const uint32_t *__restrict__ ci, const T *__restrict__ val,
                                                       const unsigned long long *__restrict__ off,
                                                       uint32_t *__restrict__ cci, T *__restrict__ cv) {
    __shared__ uint32_t s_wave[4];
    const uint32_t b = rp[blockIdx.x], e = rp[blockIdx.x + 1];
    unsigned long long o = off[list[blockIdx.x]];
    const int w = (int)threadIdx.x / 64, l = (int)threadIdx.x % 64;
    for (uint32_t x0 = b; x0 < e; x0 += 256) {
        const uint32_t x = x0 + threadIdx.x;
        const bool head = x < e && (x == b || ci[x] != ci[x - 1]);
        const unsigned long long mask = __ballot(head);
        if (l == 0) s_wave[w] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = (uint32_t)__popcll(mask & ((1ull << l) - 1ull)), total = 0;
        for (int u = 0; u < 4; ++u) {
            if (u < w) before += s_wave[u];
            total += s_wave[u];
        }
        if (head) {
            const uint32_t j = ci[x];
            T s = val[x];
            for (uint32_t y = x + 1; y < e && ci[y] == j; ++y) s = s + val[y];
            cci[o + before] = j;
            cv[o + before] = s;
        }
        o += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void spgemm_rowptr32(const unsigned long long *__restrict__ off, uint64_t n,
                                                       uint32_t *__restrict__ rp) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) rp[t] = (uint32_t)off[t];
}

// ---- host ----------------------------------------------------------------------------------------------------------
struct Product {
    OpArrays c;
    uint32_t tier[kTiers] = {};
    uint64_t products = 0, large_products = 0;
};

template <typename T, int G, int TS, int GPB>
void launch_tier(bool numeric, const uint32_t *rows, uint32_t n, const Operand &A, const Operand &B,
                 unsigned long long *cnt, const unsigned long long *off, uint32_t *cci, T *cv, hipStream_t st) {
    if (!n) return;
    const dim3 grid(grid_of(n, GPB)), block(G * GPB);
    if (numeric)
        hipLaunchKernelGGL((spgemm_lds<T, G, TS, GPB, true>), grid, block, 0, st, rows, n, A.ptr, A.ind, (const T *)A.val,
                           B.ptr, B.ind, (const T *)B.val, cnt, off, cci, cv);
    else
        hipLaunchKernelGGL((spgemm_lds<T, G, TS, GPB, false>), grid, block, 0, st, rows, n, A.ptr, A.ind, (const T *)A.val,
                           B.ptr, B.ind, (const T *)B.val, cnt, off, cci, cv);
}

template <typename T>
void launch_lds_tiers(bool numeric, const uint32_t *list, const uint32_t *tier_start, const uint32_t *tier_n,
                      const Operand &A, const Operand &B, unsigned long long *cnt, const unsigned long long *off,
                      uint32_t *cci, T *cv, hipStream_t st) {
    launch_tier<T, 16, 128, 16>(numeric, list + tier_start[1], tier_n[1], A, B, cnt, off, cci, cv, st);
    launch_tier<T, 32, 512, 4>(numeric, list + tier_start[2], tier_n[2], A, B, cnt, off, cci, cv, st);
    launch_tier<T, 64, 2048, 1>(numeric, list + tier_start[3], tier_n[3], A, B, cnt, off, cci, cv, st);
    launch_tier<T, 256, 4096, 1>(numeric, list + tier_start[4], tier_n[4], A, B, cnt, off, cci, cv, st);
    launch_tier<T, 256, 8192, 1>(numeric, list + tier_start[5], tier_n[5], A, B, cnt, off, cci, cv, st);
}

// C (A.nmajor x B.nminor) = A * B on `st`; C's arrays are returned in `out.c`.
template <typename T>
int spgemm_t(int device, const Operand &A, const Operand &B, int route, uint32_t cap, hipStream_t st, Product &out) {
    const uint64_t m = A.nmajor;
    DevBuf ub, tier, cnt, off, list, ctr;
    SPAL_HIP_TRY(ub.alloc(m * 4));
    SPAL_HIP_TRY(tier.alloc(m));
    SPAL_HIP_TRY(cnt.alloc((m + 1) * 8));
    SPAL_HIP_TRY(off.alloc((m + 1) * 8));
    SPAL_HIP_TRY(list.alloc(m * 4));
    SPAL_HIP_TRY(ctr.alloc(sizeof(Counters)));
    SPAL_HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(Counters), st));
    SPAL_HIP_TRY(hipMemsetAsync(cnt.p, 0, (m + 1) * 8, st));
    hipLaunchKernelGGL(spgemm_count, dim3(grid_of(m, 256)), dim3(256), 0, st, A.ptr, A.ind, B.ptr, (uint32_t)m, cap, route,
                       ub.as<uint32_t>(), tier.as<uint8_t>(), ctr.as<Counters>());
    hipLaunchKernelGGL(spgemm_bin, dim3(grid_of(m, 256)), dim3(256), 0, st, tier.as<uint8_t>(), (uint32_t)m,
                       ctr.as<Counters>(), list.as<uint32_t>());
    SPAL_HIP_TRY(hipGetLastError());
    Counters h{};
    SPAL_HIP_TRY(hipMemcpyAsync(&h, ctr.p, sizeof(Counters), hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    uint32_t start[kTiers] = {};
    for (int t = 0; t < kTiers; ++t) out.tier[t] = h.tier[t];
    for (int t = 2; t < kTiers; ++t) start[t] = start[t - 1] + h.tier[t - 1];
    start[1] = 0;
    out.products = h.products;
    out.large_products = h.large_products;
    if (h.large_products > kMaxEntries)
        return fail(SPAL_ERR_UNSUPPORTED, "spal_csr_mul: the large-row tier's %llu products do not fit 32-bit device offsets",
                    (unsigned long long)h.large_products);

    const uint32_t *lst = list.as<uint32_t>();
    unsigned long long *d_cnt = cnt.as<unsigned long long>(), *d_off = off.as<unsigned long long>();
    // symbolic: distinct columns of every LDS-tier row
    launch_lds_tiers<T>(false, lst, start, h.tier, A, B, d_cnt, d_off, nullptr, nullptr, st);
    SPAL_HIP_TRY(hipGetLastError());
    // large tier: expand, two stable transposes (each row sorted by column, equal columns in k order), runs counted
    const uint32_t nL = h.tier[6];
    const uint32_t *lrows = lst + start[6];
    DevBuf sptr;
    OpArrays sorted;   // the expansion, every row sorted by column
    if (nL) {
        const uint64_t L = h.large_products;
        {
            DevBuf sci, sv;
            SPAL_HIP_TRY(sptr.alloc(((uint64_t)nL + 1) * 4));
            SPAL_HIP_TRY(sci.alloc(L * 4));
            SPAL_HIP_TRY(sv.alloc(L * sizeof(T)));
            DevBuf raw;
            SPAL_HIP_TRY(raw.alloc(((uint64_t)nL + 1) * 4));
            hipLaunchKernelGGL(spgemm_gather_ub, dim3(grid_of((uint64_t)nL + 1, 256)), dim3(256), 0, st, lrows, nL,
                               ub.as<uint32_t>(), raw.as<uint32_t>());
            SPAL_HIP_TRY(hipGetLastError());
            SPAL_HIP_TRY(scan_exclusive<uint32_t>(raw.as<uint32_t>(), sptr.as<uint32_t>(), (uint64_t)nL + 1, st));
            hipLaunchKernelGGL((spgemm_expand<T>), dim3(nL), dim3(256), 0, st, lrows, sptr.as<uint32_t>(), A.ptr, A.ind,
                               (const T *)A.val, B.ptr, B.ind, (const T *)B.val, sci.as<uint32_t>(), sv.as<T>());
            SPAL_HIP_TRY(hipGetLastError());
            OpArrays bycol;
            SPAL_TRY(transpose_device(device, (int)sizeof(T), nL, B.nminor, L, sptr.as<uint32_t>(), sci.as<uint32_t>(),
                                      sv.p, st, bycol));
            SPAL_TRY(transpose_device(device, (int)sizeof(T), B.nminor, nL, L, bycol.ptr, bycol.ind, bycol.val, st, sorted));
        }
        hipLaunchKernelGGL(spgemm_run_count, dim3(nL), dim3(256), 0, st, lrows, sorted.ptr, sorted.ind, d_cnt);
        SPAL_HIP_TRY(hipGetLastError());
    }
    // offsets of C's rows; nnz(C) back to the host (the size of C's arrays)
    SPAL_HIP_TRY(scan_exclusive<unsigned long long>(d_cnt, d_off, m + 1, st));
    unsigned long long nnz = 0;
    SPAL_HIP_TRY(hipMemcpyAsync(&nnz, d_off + m, 8, hipMemcpyDeviceToHost, st));
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    if (nnz > kMaxEntries)
        return fail(SPAL_ERR_UNSUPPORTED, "spal_csr_mul: the product has %llu entries, more than 32-bit device offsets address",
                    nnz);
    OpArrays &c = out.c;
    SPAL_TRY(c.alloc(m, nnz, sizeof(T), st));
    hipLaunchKernelGGL(spgemm_rowptr32, dim3(grid_of(m + 1, 256)), dim3(256), 0, st, d_off, m + 1, c.ptr);
    launch_lds_tiers<T>(true, lst, start, h.tier, A, B, d_cnt, d_off, c.ind, (T *)c.val, st);
    if (nL)
        hipLaunchKernelGGL((spgemm_run_fill<T>), dim3(nL), dim3(256), 0, st, lrows, sorted.ptr, sorted.ind,
                           (const T *)sorted.val, d_off, c.ind, (T *)c.val);
    SPAL_HIP_TRY(hipGetLastError());
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    return SPAL_OK;
}

int spgemm(int device, int elem_size, const Operand &A, const Operand &B, int route, int64_t lds_cap, hipStream_t st,
           Product &out) {
    uint32_t cap = route == 1 ? kMaxCap : lds_cap > 0 ? (uint32_t)std::min<int64_t>(lds_cap, kMaxCap) : kDefaultCap;
    return elem_size == 8 ? spgemm_t<double>(device, A, B, route, cap, st, out)
                          : spgemm_t<float>(device, A, B, route, cap, st, out);
}

std::string info_json(const Product &r, int route, double plan_ms, double ms) {
    char buf[640];
    std::string tiers;
    for (int t = 0; t < kTiers; ++t) {
        snprintf(buf, sizeof buf, "%s\"%s\": %u", t ? ", " : "", kTierNames[t], r.tier[t]);
        tiers += buf;
    }
    snprintf(buf, sizeof buf,
             "{\"route\": %d, \"tier_rows\": {%s}, \"products\": %llu, \"large_products\": %llu, \"nnz\": %llu, "
             "\"plan_ms\": %.3f, \"call_ms\": %.3f}",
             route, tiers.c_str(), (unsigned long long)r.products, (unsigned long long)r.large_products,
             (unsigned long long)r.c.nnz, plan_ms, ms);
    return buf;
}

// assert_eq!(self.ncols(), rhs.nrows()) of src/csr/ops/mul.rs:9 and src/csc/ops/mul.rs:9, then what the device needs
template <typename H>
int check_mul(const char *fn, const H *a, const H *b, H **out) {
    if (!a || !b || !out) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    if (a->ncols != b->nrows)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: ncols == rhs.nrows (left: %llu, right: %llu)",
                    (unsigned long long)a->ncols, (unsigned long long)b->nrows);
    return check_same_device_and_dtype(fn, a, b);
}

// C = a * b as the product L * R of the handles' arrays, into a handle of their type
template <typename H>
int product(const H *a, const H *b, const Operand &L, const Operand &R, void *stream, H **out) {
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    const auto t0 = std::chrono::steady_clock::now();
    Product r;
    SPAL_TRY(spgemm(a->device, a->elem_size, L, R, a->ops.spgemm_route, a->ops.spgemm_lds_cap, (hipStream_t)stream, r));
    const auto tp = std::chrono::steady_clock::now();
    // CSR: eager plan, like a handle built from host arrays.  This began as a workaround: a lazily planned handle reached
    // csr_blockwin_or_split re-entrantly (csr_form1_faster -> csr_launch -> csr_ensure_plan under the lock it held).  That
    // is fixed -- the planner launches through csr_launch_planned -- and eager planning stays as a choice: the plan's
    // cost shows as plan_ms, and the first product of the result pays nothing.
    SPAL_TRY(r.c.adopt(a->device, a->elem_size, a->nrows, b->ncols, out, true, false));
    (*out)->ops.spgemm_info = info_json(r, a->ops.spgemm_route, ms_since(tp), ms_since(t0));
    return SPAL_OK;
}

}  // namespace

int spgemm_option(const char *key, int64_t value, OpState &s, int *status) {
    if (!strcmp(key, "spgemm_route")) {
        *status = (value < 0 || value > 2)
                      ? fail(SPAL_ERR_INVALID_ARGUMENT, "spgemm_route must be 0 (auto), 1 (LDS tiers wherever they fit) or 2 (large-row tier)")
                      : SPAL_OK;
        if (*status == SPAL_OK) s.spgemm_route = (int)value;
        return 1;
    }
    if (!strcmp(key, "spgemm_lds_cap")) {
        *status = (value < 0 || value > (int64_t)kMaxCap)
                      ? fail(SPAL_ERR_INVALID_ARGUMENT, "spgemm_lds_cap must be 0 (default) or in [1, %u]", kMaxCap)
                      : SPAL_OK;
        if (*status == SPAL_OK) s.spgemm_lds_cap = value;
        return 1;
    }
    return 0;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_mul(spal_csr_t a, spal_csr_t b, void *stream, spal_csr_t *out) {
    SPAL_TRY(check_mul("spal_csr_mul", a, b, out));
    if (row_blocks(a) || row_blocks(b)) return refuse_row_blocks("spal_csr_mul");
    return product(a, b, operand_of(a), operand_of(b), stream, out);
}

// `impl Mul for &CscMatrix<T>`: the CSC arrays of A are the CSR arrays of A^T and (AB)^T = B^T A^T, so C's CSC arrays are
// the CSR product of lhs = B's arrays (p x n) and rhs = A's arrays (n x m).  k runs in the same order.  The reference
// sizes one workspace by the wrong extent here; this is the defined product where it would panic.
int spal_csc_mul(spal_csc_t a, spal_csc_t b, void *stream, spal_csc_t *out) {
    SPAL_TRY(check_mul("spal_csc_mul", a, b, out));
    return product(a, b, operand_of(b), operand_of(a), stream, out);   // B^T (p x n) times A^T (n x m)
}

}  // extern "C"
