// Stand-alone host program over the codec of spalinalg_amd/csrc/csr_rowrec.hpp (nothing else of the library): random and
// adversarial rows of 12, 14 and 16 columns -- decode(encode(row)) is the row's columns mod R, the unused part of a
// record is zero, the pad record decodes to zeros, and rows are refused exactly at the bounds the header documents.
// The expected positions are computed here, column by column, not by the header.  Prints "ok <cases>" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "csr_rowrec.hpp"

using namespace spal;

static long g_cases = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

// the documented bound, written out again: span < R and (span >> 8) + L - 2 <= 39
template <int L>
static bool encodable(const std::vector<uint32_t> &c, uint32_t R) {
    for (int k = 1; k < L; ++k)
        if (c[k] <= c[k - 1]) return false;
    const uint32_t span = c[L - 1] - c[0];
    return span < R && (span >> 8) + (uint32_t)(L - 2) <= 39u;
}

template <int L>
static void one_row(const std::vector<uint32_t> &c, uint32_t R, bool expect) {
    ++g_cases;
    constexpr int NR = rowrec_dwords(L);
    static_assert(NR == (L <= 14 ? 5 : 6), "5 dwords up to 14 columns, 6 up to 16");
    std::vector<uint32_t> rec(NR, 0xdeadbeefu);   // (exactly NR words: the sanitizer sees a write past them)
    CHECK(encodable<L>(c, R) == expect);
    const bool ok = rowrec_encode<L>(c.data(), R, rec.data());
    CHECK(ok == expect);
    if (!ok) {
        for (int q = 0; q < NR; ++q) CHECK(rec[q] == 0xdeadbeefu);   // refused: untouched
        return;
    }
    // the fields, bit by bit
    CHECK((rec[0] & 0xffffu) == c[0] % R);
    uint64_t H = (uint64_t)(rec[0] >> 16) | ((uint64_t)(rec[1] & 0xffffffu) << 16);
    CHECK(__builtin_popcountll(H) == L - 1);
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(rec.data());   // (little endian, as the device)
    for (int k = 1; k < L; ++k) {
        const uint32_t d = c[k] - c[0];
        CHECK((H >> ((d >> 8) + (uint32_t)(k - 1))) & 1u);
        CHECK(bytes[7 + k - 1] == (d & 255u));
    }
    for (int b = 7 + L - 1; b < 4 * NR; ++b) CHECK(bytes[b] == 0);
    std::vector<uint32_t> pos(L, 0xffffffffu);
    rowrec_decode<L>(rec.data(), R, pos.data());
    for (int k = 0; k < L; ++k) {
        CHECK(pos[k] == c[k] % R);
        // ... which is the col16 of the plan: (page % ring) * 256 + column inside the page
        CHECK(pos[k] == (((c[k] >> 8) % (R >> 8)) << 8 | (c[k] & 255u)));
    }
}

template <int L>
static std::vector<uint32_t> row_from(uint32_t c0, const std::vector<uint32_t> &d) {   // d: L - 1 ascending offsets
    std::vector<uint32_t> c(L, c0);
    for (int k = 1; k < L; ++k) c[k] = c0 + d[k - 1];
    return c;
}

template <int L>
static void adversarial(uint32_t R) {
    const uint32_t by_bits = ((uint32_t)(39 - (L - 2)) << 8) | 255u;
    const uint32_t top = by_bits < R - 1u ? by_bits : R - 1u;
    CHECK(rowrec_max_span(L, R) == top);
    std::vector<uint32_t> d(L - 1);
    const uint32_t firsts[] = {0u, 1u, 255u, 256u, R - 256u, R - 1u, R, R + 3u, 7u * R + 5u, 9999744u, 0xffffffffu - top};
    for (uint32_t c0 : firsts) {
        for (int k = 1; k < L; ++k) d[k - 1] = (uint32_t)k;                       // consecutive columns
        one_row<L>(row_from<L>(c0, d), R, true);
        for (int k = 1; k < L; ++k) d[k - 1] = (uint32_t)(17 * k);               // one page (when c0 starts one)
        one_row<L>(row_from<L>(c0, d), R, true);
        for (int k = 1; k < L; ++k) d[k - 1] = (uint32_t)k;                       // the widest row ...
        d[L - 2] = top;
        one_row<L>(row_from<L>(c0, d), R, true);
        d[L - 2] = top + 1u;                                                      // ... and one column more
        one_row<L>(row_from<L>(c0, d), R, false);
        for (int k = 1; k < L; ++k) d[k - 1] = top - (uint32_t)(L - 1 - k);       // all in the last page but the first
        one_row<L>(row_from<L>(c0, d), R, true);
        for (int k = 1; k < L; ++k) d[k - 1] = (uint32_t)k * (top / (uint32_t)(L - 1));   // spread evenly
        one_row<L>(row_from<L>(c0, d), R, true);
        for (int k = 1; k < L; ++k) d[k - 1] = (uint32_t)k * 256u;                // one column per page
        one_row<L>(row_from<L>(c0, d), R, d[L - 2] <= top);
        for (int k = 1; k < L; ++k) d[k - 1] = (uint32_t)k * 256u - 1u;           // low bytes 255
        one_row<L>(row_from<L>(c0, d), R, d[L - 2] <= top);
    }
    // not ascending: equal neighbours, a descent, at either end and in the middle
    for (int at : {1, L / 2, L - 1}) {
        for (int k = 1; k < L; ++k) d[k - 1] = (uint32_t)(3 * k);
        std::vector<uint32_t> c = row_from<L>(1000u, d);
        c[at] = c[at - 1];
        one_row<L>(c, R, false);
        c[at] = c[at - 1] - 1u;
        one_row<L>(c, R, false);
    }
    // the pad record: L zeros
    uint32_t pad[kRowrecMaxDwords] = {1u, 1u, 1u, 1u, 1u, 1u}, pos[L];
    rowrec_pad<L>(pad);
    rowrec_decode<L>(pad, R, pos);
    for (int k = 0; k < L; ++k) CHECK(pos[k] == 0u);
    for (int q = 2; q < rowrec_dwords(L); ++q) CHECK(pad[q] == 0u);
    ++g_cases;
}

template <int L>
static void random_rows(uint32_t R, std::mt19937_64 &rng, int n) {
    const uint32_t top = rowrec_max_span(L, R);
    for (int i = 0; i < n; ++i) {
        // spans around the bound as often as inside it
        const uint32_t span = (i % 4 == 0) ? top - (uint32_t)(rng() % 3) + (uint32_t)(rng() % 3)
                                           : (uint32_t)(L - 1) + (uint32_t)(rng() % (top - (uint32_t)(L - 1) + 1u));
        std::vector<uint32_t> d;
        while ((int)d.size() < L - 2) {   // L - 2 distinct offsets inside (0, span), then the span itself
            const uint32_t v = 1u + (uint32_t)(rng() % (span - 1u));
            bool seen = false;
            for (uint32_t w : d) seen = seen || w == v;
            if (!seen) d.push_back(v);
        }
        for (size_t a = 0; a < d.size(); ++a)
            for (size_t b = a + 1; b < d.size(); ++b)
                if (d[b] < d[a]) { const uint32_t t = d[a]; d[a] = d[b]; d[b] = t; }
        d.push_back(span);
        const uint32_t c0 = (uint32_t)(rng() % 10000000u);
        one_row<L>(row_from<L>(c0, d), R, span <= top);
    }
}

int main() {
    static_assert(!rowrec_length_ok(10) && rowrec_length_ok(12) && !rowrec_length_ok(13) && rowrec_length_ok(14) &&
                      rowrec_length_ok(16) && !rowrec_length_ok(18), "even lengths from 12 to 16");
    std::mt19937_64 rng(20240611u);
    // rings: the band of the benchmark (24 pages), one page more than a record's reach, the largest (255), small ones
    for (uint32_t pages : {8u, 17u, 24u, 27u, 28u, 29u, 30u, 64u, 255u}) {
        const uint32_t R = pages * 256u;
        adversarial<12>(R);
        adversarial<14>(R);
        adversarial<16>(R);
        random_rows<12>(R, rng, 2000);
        random_rows<14>(R, rng, 2000);
        random_rows<16>(R, rng, 2000);
    }
    printf("ok %ld\n", g_cases);
    return 0;
}
