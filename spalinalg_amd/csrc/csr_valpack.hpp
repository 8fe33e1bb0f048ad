// csr_valpack.hpp -- PACKED VALUES: the f64 values of a row of uniform length as fixed-point fields of one row block,
// for the sliding kernel's row-record form (csr_slide.hpp, csr_rowrec.hpp).
//
// Where every stored value of a matrix is an integer multiple of one power of two, v = k * 2^e with a small signed k
// (integer-valued matrices, values that came from f32 or from a fixed-point source, uniform random numbers drawn as
// m * 2^-52), a row of L values does not need L * 64 bits.  A row BLOCK of ND = 4 * (L / 2 - 1) dwords holds the L fields
// of W bits back to back, field k at bit k * W, each the two's complement of the value's k:
//     L = 12:  W = 53,  20 dwords (80 B instead of 96)
//     L = 14:  W = 54,  24 dwords (96 B instead of 112)
//     L = 16:  W = 54,  28 dwords (112 B instead of 128)
// Decoding splits k into hi = k >> 32 (signed) and lo = k & 0xffffffff: (double)hi * 2^32 + (double)lo is exact for
// |k| <= 2^53, and the product with 2^e is exact while 2^e is a normal number and 2^(e + 53) is finite (the plan
// checks): the decoded double is the stored value bit for bit.  -0.0, NaN, Inf and anything that is not a multiple of
// 2^e or does not fit W bits are not encodable; one such value and the matrix keeps its plain values alone.
//
// The array is [tile of 64 rows][NQ = L / 2 - 1][64 lanes] chunks of 16 bytes, lane = row: each of a tile's NQ loads
// is one 16-byte chunk per lane over 1 KB of contiguous memory.  Rows past the matrix's last get a block of zeros,
// which decodes to L values +0.0.  Every field sits at a compile-time place: no register is indexed dynamically.
//
// The codec below is plain C++ (host and device); the kernel part needs hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPAL_VALPACK_HD __host__ __device__ __forceinline__
#else
#define SPAL_VALPACK_HD inline
#endif

namespace spal {

constexpr int kValpackMaxDwords = 28;
constexpr bool valpack_length_ok(int L) { return L == 12 || L == 14 || L == 16; }
constexpr int valpack_width(int L) { return L == 12 ? 53 : 54; }
constexpr int valpack_chunks(int L) { return L / 2 - 1; }          // 16-byte chunks of a row block
constexpr int valpack_dwords(int L) { return 4 * valpack_chunks(L); }
// the quantum 2^e must be a normal double, and the largest magnitude a field holds times it finite
constexpr int kValpackMinExp = -1022, kValpackMaxExp = 1023 - 53;
constexpr bool valpack_exp_ok(int e) { return e >= kValpackMinExp && e <= kValpackMaxExp; }

SPAL_VALPACK_HD uint64_t valpack_bits_of(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return b;
}
SPAL_VALPACK_HD double valpack_double_of(uint64_t b) {
    double v;
    __builtin_memcpy(&v, &b, sizeof(v));
    return v;
}
// 2^e, e in [kValpackMinExp, 1023]
SPAL_VALPACK_HD double valpack_scale(int e) { return valpack_double_of((uint64_t)(e + 1023) << 52); }

// A finite non-zero double as mant * 2^ex with an odd or even integer mant < 2^53: returns false for zeros, NaN, Inf.
SPAL_VALPACK_HD bool valpack_split(uint64_t bits, uint64_t *mant, int *ex) {
    const uint32_t field = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t frac = bits & ((1ull << 52) - 1ull);
    if (field == 0x7ffu || (field == 0u && frac == 0ull)) return false;
    *mant = field ? (frac | (1ull << 52)) : frac;
    *ex = field ? (int)field - 1075 : -1074;
    return true;
}

// k of v = k * 2^e as a signed integer of at most `width` bits.  False when v is NaN, Inf, -0.0, no multiple of 2^e or
// out of range.
SPAL_VALPACK_HD bool valpack_quantize(double v, int e, int width, int64_t *k) {
    const uint64_t bits = valpack_bits_of(v);
    if (bits == 0ull) { *k = 0; return true; }
    uint64_t mant = 0;
    int ex = 0;
    if (!valpack_split(bits, &mant, &ex)) return false;       // NaN, Inf, -0.0
    const int shift = ex - e;
    uint64_t mag;
    if (shift < 0) {
        if (shift <= -64 || (mant & ((1ull << -shift) - 1ull)) != 0ull) return false;   // not a multiple of 2^e
        mag = mant >> -shift;
    } else {
        if (shift > 10) return false;                         // mant * 2^shift >= 2^63 is possible: out of any range here
        mag = mant << shift;
    }
    const uint64_t top = 1ull << (width - 1);
    const bool neg = (bits >> 63) != 0ull;
    if (neg ? mag > top : mag >= top) return false;
    *k = neg ? -(int64_t)mag : (int64_t)mag;                  // (mag <= 2^53)
    return true;
}

// vals: the row's L values as stored.  False (blk untouched) when one of them is not encodable with quantum 2^e.
template <int L>
SPAL_VALPACK_HD bool valpack_encode(const double *vals, int e, uint32_t *blk) {
    static_assert(valpack_length_ok(L) && L * valpack_width(L) <= 32 * valpack_dwords(L) &&
                      valpack_dwords(L) <= kValpackMaxDwords, "the block holds the fields");
    constexpr int W = valpack_width(L), ND = valpack_dwords(L);
    if (!valpack_exp_ok(e)) return false;
    uint32_t w[ND];
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < ND; ++q) w[q] = 0u;
    bool ok = true;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < L; ++k) {
        int64_t kk = 0;
        ok = valpack_quantize(vals[k], e, W, &kk) && ok;
        const uint64_t f = (uint64_t)kk & ((1ull << W) - 1ull);
        const int bit = k * W, d = bit >> 5, s = bit & 31;
        w[d] |= (uint32_t)(f << s);
        w[d + 1] |= (uint32_t)((f << s) >> 32);
        if (s + W > 64) w[d + 2] |= (uint32_t)(f >> (64 - s));
    }
    if (!ok) return false;
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < ND; ++q) blk[q] = w[q];
    return true;
}

// out[k] = field k times scale (= 2^e), k < L.
template <int L>
SPAL_VALPACK_HD void valpack_decode(const uint32_t *blk, double scale, double *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    constexpr int W = valpack_width(L);
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < L; ++k) {
        // in 32-bit pieces (funnel shifts by constants): lo = bits [bit, bit + 32) of the block, hi = the HB bits above
        const int bit = k * W, d = bit >> 5, s = bit & 31, HB = W - 32;
        const uint32_t lo = s ? (blk[d] >> s) | (blk[d + 1] << (32 - s)) : blk[d];     // k & 0xffffffff
        uint32_t hr = blk[d + 1] >> s;
        if (s + HB > 32) hr |= blk[d + 2] << (32 - s);
        const int32_t hi = (int32_t)(hr << (32 - HB)) >> (32 - HB);                    // k >> 32, sign-extended
        out[k] = ((double)hi * 4294967296.0 + (double)lo) * scale;
    }
}

}  // namespace spal

#if defined(__HIPCC__)
#include "csr_kernels.hpp"
#include "csr_rowrec.hpp"

namespace spal {

using valpack_chunk_t = __attribute__((ext_vector_type(4))) uint32_t;

// One tile's NQ block loads: chunk q of the row blocks of tile `tix`, this lane's row.  They land in t.v[0 ... NQ).
template <int L>
__device__ __forceinline__ void valpack_tile_load(StreamTile<double> &t, const valpack_chunk_t *__restrict__ blocks,
                                                  uint32_t tix, uint32_t lane) {
    constexpr int NQ = valpack_chunks(L);
    static_assert(NQ <= kStreamSteps && sizeof(valpack_chunk_t) == sizeof(t.v[0]), "a chunk per pair of values");
    const valpack_chunk_t *at = blocks + (size_t)tix * (NQ * 64u) + lane;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        t.v[q] = __builtin_bit_cast(typename Pair<double>::type, __builtin_nontemporal_load(at + q * 64));
}

// The tile's turn, a row per lane: lane r holds its whole row -- the record in t.c[0 ... NR), the block in
// t.v[0 ... NQ) -- decodes its L window positions and its L values, and forms the products and the sum exactly as
// stream_compute does for a row: the first product is assigned, then acc = acc + p_k for k ascending, every product
// and sum rounded on its own.  No strip, no transpose: nothing leaves the lane but y.
template <int L>
__device__ __forceinline__ void valpack_row_compute(const StreamTile<double> &t, const double *xw, uint32_t wmax, uint32_t R,
                                                    double scale, double *__restrict__ y, uint32_t row0, uint32_t nrows,
                                                    uint32_t lane, uint32_t nt_store) {
#pragma clang fp contract(off)
    constexpr int NQ = valpack_chunks(L);
    uint32_t pos[L], blk[4 * NQ];
    double v[L];
    rowrec_decode<L>(t.c, R, pos);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const valpack_chunk_t c = __builtin_bit_cast(valpack_chunk_t, t.v[q]);
        blk[4 * q] = c.x; blk[4 * q + 1] = c.y; blk[4 * q + 2] = c.z; blk[4 * q + 3] = c.w;
    }
    valpack_decode<L>(blk, scale, v);
    double acc = v[0] * xw[min(pos[0], wmax)];
#pragma unroll
    for (int k = 1; k < L; ++k) {
        const double p = v[k] * xw[min(pos[k], wmax)];
        acc = acc + p;
    }
    if (row0 + lane < min(row0 + 64u, nrows)) {
        if (nt_store) __builtin_nontemporal_store(acc, &y[row0 + lane]);
        else y[row0 + lane] = acc;
    }
}

}  // namespace spal
#endif
