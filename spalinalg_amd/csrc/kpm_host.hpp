// kpm_host.hpp -- the host half of the KPM moments (spal_*_kpm_moments_*: DESIGN 3.29).  Plain C++, no device and no
// library call: the probe hash, the refusals of the arguments, the interval's scalars, the column tile, the chunk and
// the sizes of a call's scratch.  The text is in include/spal.h; tests/kpm_ref.py restates it in numpy bit for bit, and
// tests/cpp/test_kpm_asan.cpp compiles this header alone under the sanitizers.  (Not installed.)
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#pragma clang fp contract(off)

namespace spal {

constexpr uint64_t kKpmMaxDegree = 4096;
constexpr uint64_t kKpmMaxProbes = 256;
constexpr uint64_t kKpmDotTile = 1024;             // = kTile of krylov_kernels.hpp: dot's tiles, and the rows of a workgroup
constexpr int kKpmMaxTile = 8;                     // the widest instantiated column tile
constexpr unsigned kKpmProductBytes = 32 * 1024;   // LDS of a step's products: chunk * tile * sizeof(T) stays within it

// mix32 of the text (the colouring's): a bijection of the 32-bit words
inline uint32_t kpm_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// z[i, j] of the hashed probes: -1 when the top bit of mix32(h(i) + j) is set, else +1; only seed mod 2^32 enters
inline int kpm_probe_sign(uint64_t i, uint64_t j, uint64_t seed) {
    const uint32_t h = kpm_mix32((uint32_t)i + (uint32_t)seed);
    return kpm_mix32(h + (uint32_t)j) >> 31 ? -1 : 1;
}
template <typename T>
inline void kpm_probes(uint64_t n, uint64_t k, uint64_t seed, T *z, uint64_t ldz) {
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < k; ++j) z[i * ldz + j] = (T)kpm_probe_sign(i, j, seed);
}

// Why a call is refused: 0 = it is fine.  The order is the text's.
enum KpmRefusal {
    KPM_OK = 0, KPM_DEGREE, KPM_PROBES, KPM_MU_LEN, KPM_LDZ, KPM_Z_ROWS, KPM_AUTOMATIC, KPM_NOT_FINITE, KPM_EMPTY
};
inline const char *kpm_refusal_text(KpmRefusal r) {
    switch (r) {
    case KPM_DEGREE: return "degree must be 1 .. 4096";
    case KPM_PROBES: return "k must be 1 .. 256";
    case KPM_MU_LEN: return "mu_len must be (degree + 1) * k";
    case KPM_LDZ: return "ldz must be at least k";
    case KPM_Z_ROWS: return "z_rows must be the matrix's rows";
    case KPM_AUTOMATIC: return "automatic must be 0 or 1";
    case KPM_NOT_FINITE: return "lo and hi must be finite";
    case KPM_EMPTY: return "lo must be less than hi";
    default: return "";
    }
}

// has_z: the caller gave a block (ldz and z_rows are looked at only then; the _dev forms pass z_rows = nrows)
inline KpmRefusal kpm_check(uint64_t degree, uint64_t k, uint64_t mu_len, bool has_z, uint64_t z_rows, uint64_t ldz,
                            uint64_t nrows, int automatic, double lo, double hi) {
    if (degree < 1 || degree > kKpmMaxDegree) return KPM_DEGREE;
    if (k < 1 || k > kKpmMaxProbes) return KPM_PROBES;
    if (mu_len != (degree + 1) * k) return KPM_MU_LEN;
    if (has_z && ldz < k) return KPM_LDZ;
    if (has_z && z_rows != nrows) return KPM_Z_ROWS;
    if (automatic != 0 && automatic != 1) return KPM_AUTOMATIC;
    if (automatic) return KPM_OK;
    if (!std::isfinite(lo) || !std::isfinite(hi)) return KPM_NOT_FINITE;
    if (!(lo < hi)) return KPM_EMPTY;
    return KPM_OK;
}

// m = ceil(d / 2): the recurrence steps, = the products per column
inline uint64_t kpm_steps(uint64_t degree) { return (degree + 1) / 2; }

// a1 = T(1/e), a2 = T(2/e), cT = T(c) as in cheb_series
template <typename T>
struct KpmScalars {
    T a1, a2, cT;
};
template <typename T>
inline KpmScalars<T> kpm_scalars(double lo, double hi) {
    const double c = (lo + hi) / 2.0, e = (hi - lo) / 2.0;
    return {(T)(1.0 / e), (T)(2.0 / e), (T)c};
}

inline bool kpm_tile_valid(int64_t t) { return t == 0 || t == 1 || t == 2 || t == 4 || t == 8; }
// the option "kpm_tile", 0 (automatic) resolved: the narrowest tile that holds k, at most the widest
inline int kpm_tile_of(int64_t option, uint64_t k) {
    if (option) return (int)option;
    int t = 1;
    while (t < kKpmMaxTile && (uint64_t)t < k) t *= 2;
    return t;
}
// columns of the work blocks: k rounded up to whole tiles (the padding columns are computed and never returned)
inline uint64_t kpm_padded(uint64_t k, int tile) { return (k + (uint64_t)tile - 1) / (uint64_t)tile * (uint64_t)tile; }
// entries per chunk of the step: the option "cheb_chunk" (0 = 16 KiB of products per column), clipped so that the tile's
// products fit kKpmProductBytes; never below 256 (a tile of 8 f64 columns: 512)
inline unsigned kpm_chunk_of(unsigned option, int tile, size_t elem) {
    const unsigned want = option ? option : (unsigned)(16 * 1024 / elem);
    const unsigned fit = (unsigned)(kKpmProductBytes / ((size_t)tile * elem));
    return want < fit ? want : fit;
}

// elements of the scratch of ONE dot over n elements: the first level's tile sums and every level above
inline uint64_t kpm_dot_elems(uint64_t n) {
    uint64_t m = n ? (n + kKpmDotTile - 1) / kKpmDotTile : 1, total = m;
    while (m > 1) {
        m = (m + kKpmDotTile - 1) / kKpmDotTile;
        total += m;
    }
    return total;
}

// The device block of a call, in bytes from its start (every part 256-byte aligned): three work blocks of n x kp
// elements, three dots' scratch of kp columns, mu_0 and mu_1 of every column, and the moment table in doubles.
struct KpmLayout {
    size_t block[3], part[3], base, table, total;
    uint64_t kp, pe;
};
inline bool kpm_layout(uint64_t n, uint64_t k, int tile, uint64_t degree, size_t elem, KpmLayout *out) {
    const size_t lim = std::numeric_limits<size_t>::max() / 16;
    KpmLayout L{};
    L.kp = kpm_padded(k, tile);
    L.pe = kpm_dot_elems(n);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    if (n > lim / (L.kp * elem)) return false;
    const size_t blk = up((size_t)n * L.kp * elem), prt = up((size_t)L.pe * L.kp * elem);
    if (blk > lim / 4) return false;
    size_t at = 0;
    for (int i = 0; i < 3; ++i) { L.block[i] = at; at += blk; }
    for (int i = 0; i < 3; ++i) { L.part[i] = at; at += prt; }
    L.base = at;
    at += up((size_t)2 * L.kp * elem);
    L.table = at;
    at += up((size_t)(degree + 1) * k * sizeof(double));
    L.total = at;
    *out = L;
    return true;
}

}  // namespace spal
