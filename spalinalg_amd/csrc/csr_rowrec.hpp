// csr_rowrec.hpp -- ROW RECORDS: the columns of a row of uniform length as one Elias-Fano record, for the sliding
// kernel (csr_slide.hpp).
//
// A banded row of L ascending distinct columns inside a few thousand carries log2 C(4096, 14) = 132 bits, its 16-bit
// ring positions (col16) occupy 224.  A record of NR dwords (NR = 5 for L <= 14, 6 for L <= 16) holds the same
// positions.  With c[0] < ... < c[L-1], d[k] = c[k] - c[0] and R = ring_pages * 256:
//     bits  0 - 15   c[0] mod R
//     bits 16 - 55   H, 40 bits: bit (d[k] >> 8) + (k - 1) is set for k = 1 ... L-1   (the high parts, in unary)
//     bytes 7 ... 7 + L - 2   d[k] & 255
//     the rest       0
// A row is encodable when (d[L-1] >> 8) + L - 2 <= 39 and d[L-1] < R.  Decoding walks the set bits of H upwards: the
// k-th one, at bit b, gives position (c[0] mod R) + ((b - (k - 1)) << 8 | low[k]), less R once if that is R or more --
// exactly the col16 of the entry.  Every field sits at a compile-time place: no register is indexed dynamically.
//
// The array is [tile of 64 rows][NR][64 lanes] dwords, lane = row: each of a tile's NR loads is one dword per lane over
// 256 contiguous bytes.  Rows past the matrix's last get a PAD record (base 0, H = the low L-1 bits, lows 0), which
// decodes to L positions 0: the bit scan never sees zero and every decoded position lies in the window.
//
// The codec below is plain C++ (host and device); the kernel part needs hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPAL_ROWREC_HD __host__ __device__ __forceinline__
#else
#define SPAL_ROWREC_HD inline
#endif

namespace spal {

constexpr int kRowrecMinLen = 12, kRowrecMaxLen = 16;   // below 12 a record is no smaller than the row's col16
constexpr int kRowrecHighBits = 40;
constexpr int kRowrecMaxDwords = 6;
constexpr int rowrec_dwords(int L) { return L <= 14 ? 5 : 6; }
constexpr bool rowrec_length_ok(int L) { return L >= kRowrecMinLen && L <= kRowrecMaxLen && L % 2 == 0; }
// the widest row (last column - first) a record of L columns holds in a ring of R positions
constexpr uint32_t rowrec_max_span(int L, uint32_t R) {
    const uint32_t by_bits = ((uint32_t)(kRowrecHighBits - 1 - (L - 2)) << 8) | 255u;
    return R == 0u ? 0u : (by_bits < R - 1u ? by_bits : R - 1u);
}

// The pad record of rows that do not exist.
template <int L>
SPAL_ROWREC_HD void rowrec_pad(uint32_t *rec) {
    const uint64_t H = (1ull << (L - 1)) - 1ull;
    rec[0] = (uint32_t)(H << 16);
    rec[1] = (uint32_t)(H >> 16);
    for (int q = 2; q < rowrec_dwords(L); ++q) rec[q] = 0u;
}

// cols: the row's L columns as stored.  False (rec untouched) when they are not strictly ascending or the row is not
// encodable.
template <int L>
SPAL_ROWREC_HD bool rowrec_encode(const uint32_t *cols, uint32_t R, uint32_t *rec) {
    static_assert(L >= 2 && L - 1 <= kRowrecHighBits && 7 + L - 1 <= 4 * kRowrecMaxDwords, "the record's fields");
    constexpr int NR = rowrec_dwords(L);
    for (int k = 1; k < L; ++k)
        if (cols[k] <= cols[k - 1]) return false;
    const uint32_t span = cols[L - 1] - cols[0];
    if (R == 0u || R > 65536u || span >= R || (span >> 8) + (uint32_t)(L - 2) > (uint32_t)(kRowrecHighBits - 1)) return false;
    uint64_t H = 0;
    uint32_t w[kRowrecMaxDwords] = {0u, 0u, 0u, 0u, 0u, 0u};
    for (int k = 1; k < L; ++k) {
        const uint32_t d = cols[k] - cols[0];
        H |= 1ull << ((d >> 8) + (uint32_t)(k - 1));
        const int byte = 7 + (k - 1);
        w[byte >> 2] |= (d & 255u) << (8 * (byte & 3));
    }
    w[0] |= (cols[0] % R) | (uint32_t)(H << 16);
    w[1] |= (uint32_t)(H >> 16);          // 24 bits: byte 7 stays the first low byte
    for (int q = 0; q < NR; ++q) rec[q] = w[q];
    return true;
}

// pos[k] = c[k] mod R, k < L.  rec must be a record rowrec_encode or rowrec_pad made (H holds L - 1 set bits).
template <int L>
SPAL_ROWREC_HD void rowrec_decode(const uint32_t *rec, uint32_t R, uint32_t *pos) {
    const uint32_t base = rec[0] & 0xffffu;
    uint64_t H = (uint64_t)(rec[0] >> 16) | ((uint64_t)(rec[1] & 0xffffffu) << 16);
    pos[0] = base;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 1; k < L; ++k) {
        const uint32_t b = (uint32_t)__builtin_ctzll(H | (1ull << kRowrecHighBits));   // (a damaged record stays in range)
        H &= H - 1ull;
        const int byte = 7 + (k - 1);
        const uint32_t low = (rec[byte >> 2] >> (8 * (byte & 3))) & 255u;
        const uint32_t p = base + (((b - (uint32_t)(k - 1)) << 8) | low);
        pos[k] = p >= R ? p - R : p;
    }
}

}  // namespace spal

#if defined(__HIPCC__)
#include "csr_kernels.hpp"

namespace spal {

// One tile's NR record loads: dword q of the records of tile `tix`, this lane's row.  They land in t.c[0 ... NR).
template <typename T, int L>
__device__ __forceinline__ void rowrec_tile_load(StreamTile<T> &t, const uint32_t *__restrict__ rec, uint32_t tix,
                                                 uint32_t lane) {
    constexpr int NR = rowrec_dwords(L);
    const uint32_t *at = rec + (size_t)tix * (NR * 64u) + lane;
#pragma unroll
    for (int q = 0; q < NR; ++q) t.c[q] = __builtin_nontemporal_load(at + q * 64);
}

// The tile's turn: lane r decodes its row's L positions out of t.c[0 ... NR), writes them as L / 2 dwords at dword
// (L / 2) * r of the wave's product strip (free between two tiles; 7 * r for L = 14: an odd stride, no bank conflicts)
// and every lane reads back dword j * 64 + lane, j < L / 2: the t.c[j] that col16 would have delivered.  No lane
// computes with another lane's numbers; stream_compute then runs as for col16.
template <typename T, int L>
__device__ __forceinline__ void rowrec_expand(StreamTile<T> &t, uint32_t *strip, uint32_t R, uint32_t lane) {
    static_assert(L % 2 == 0 && L / 2 <= kStreamSteps && 64 * (L / 2) * 4 <= kStreamTileNnz * (int)sizeof(T), "the strip holds the tile");
    uint32_t pos[L];
    rowrec_decode<L>(t.c, R, pos);
    __builtin_amdgcn_wave_barrier();   // the strip was read by the previous tile's sums until here
#pragma unroll
    for (int i = 0; i < L / 2; ++i) strip[(L / 2) * lane + i] = pos[2 * i] | (pos[2 * i + 1] << 16);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L / 2; ++j) t.c[j] = strip[j * 64 + lane];
    __builtin_amdgcn_wave_barrier();   // ... and takes the products next
}

}  // namespace spal
#endif
