// Stand-alone host program over the codec of spalinalg_amd/csrc/csr_valpack.hpp (nothing else of the library): rows of
// 12, 14 and 16 values k * 2^e -- random k, the bounds of the width, quanta 2^0, 2^-52, 2^-1000 and 2^900 -- encode,
// every field is read back bit by bit here (field k at bit k * W, two's complement), decode returns the stored doubles
// bit for bit, the block of zeros decodes to +0.0, and NaN, Inf, -0.0, a value that is no multiple of the quantum, one
// that needs W + 1 bits and a subnormal quantum are refused with the block untouched.  Prints "ok <cases>", returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "csr_valpack.hpp"

using namespace spal;

static long g_cases = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static uint64_t bits_of(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof(b));
    return b;
}

// bit `at` of the block, counted from bit 0 of dword 0
static uint32_t block_bit(const std::vector<uint32_t> &blk, int at) { return (blk[(size_t)at / 32] >> (at % 32)) & 1u; }

template <int L>
static void one_row(const std::vector<int64_t> &k, int e) {
    ++g_cases;
    constexpr int W = valpack_width(L), ND = valpack_dwords(L);
    static_assert(W == (L == 12 ? 53 : 54) && ND == 4 * (L / 2 - 1) && valpack_chunks(L) * 4 == ND, "the documented sizes");
    std::vector<double> v(L);
    for (int i = 0; i < L; ++i) v[i] = std::ldexp((double)k[i], e);   // exact: |k| <= 2^53, 2^e normal, the product finite
    std::vector<uint32_t> blk(ND, 0xdeadbeefu);   // (exactly ND words: the sanitizer sees a write past them)
    CHECK(valpack_encode<L>(v.data(), e, blk.data()));
    for (int i = 0; i < L; ++i) {
        uint64_t f = 0;
        for (int b = 0; b < W; ++b) f |= (uint64_t)block_bit(blk, i * W + b) << b;
        CHECK(f == ((uint64_t)k[i] & ((1ull << W) - 1ull)));
    }
    for (int b = L * W; b < 32 * ND; ++b) CHECK(block_bit(blk, b) == 0u);   // the rest is zero
    std::vector<double> out(L, -1.0);
    valpack_decode<L>(blk.data(), valpack_scale(e), out.data());
    for (int i = 0; i < L; ++i) CHECK(bits_of(out[i]) == bits_of(v[i]));
}

template <int L>
static void refused(std::vector<double> v, int e) {
    ++g_cases;
    constexpr int ND = valpack_dwords(L);
    std::vector<uint32_t> blk(ND, 0xdeadbeefu);
    CHECK(!valpack_encode<L>(v.data(), e, blk.data()));
    for (int q = 0; q < ND; ++q) CHECK(blk[q] == 0xdeadbeefu);   // untouched
}

template <int L>
static void at_exponent(int e, std::mt19937_64 &rng, int n) {
    constexpr int W = valpack_width(L);
    const int64_t top = (int64_t)((1ull << (W - 1)) - 1ull), bottom = -top - 1;
    CHECK(valpack_scale(e) == std::ldexp(1.0, e));
    // the bounds, every one at every place of the row, among small neighbours
    for (int64_t edge : {top, -top, bottom, (int64_t)0, (int64_t)1, (int64_t)-1}) {
        for (int at = 0; at < L; ++at) {
            std::vector<int64_t> k(L);
            for (int i = 0; i < L; ++i) k[i] = (i % 2) ? 1 : -1;
            k[at] = edge;
            one_row<L>(k, e);
        }
        one_row<L>(std::vector<int64_t>(L, edge), e);
    }
    // random k of every bit length
    for (int i = 0; i < n; ++i) {
        std::vector<int64_t> k(L);
        for (int j = 0; j < L; ++j) {
            const int bits = 1 + (int)(rng() % (uint64_t)(W - 1));
            const int64_t mag = (int64_t)(rng() & ((1ull << bits) - 1ull));
            k[j] = (rng() & 1ull) ? -mag : mag;
        }
        one_row<L>(k, e);
    }
    // refusals: each odd value at the first, a middle and the last place of an otherwise encodable row
    const double q = std::ldexp(1.0, e);
    const double odd[] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                          -std::numeric_limits<double>::infinity(), -0.0,
                          q * (1.0 / 3.0),                              // no multiple of the quantum
                          q * 0.5,                                      // half a quantum
                          std::ldexp(1.0, e + W - 1),                   // +2^(W-1): W + 1 bits
                          -std::ldexp(1.0, e + W - 1) - std::ldexp(1.0, e + 1)};   // -(2^(W-1) + 2): W + 1 bits (exact: W <= 54)
    for (double o : odd)
        for (int at : {0, L / 2, L - 1}) {
            std::vector<double> v(L, q);
            v[at] = o;
            refused<L>(v, e);
        }
}

template <int L>
static void pad_and_quanta() {
    constexpr int ND = valpack_dwords(L);
    // the pad block: zeros, which decode to +0.0 under any quantum
    std::vector<uint32_t> blk(ND, 0u);
    std::vector<double> out(L, -1.0);
    for (int e : {0, -52, -1000, 900}) {
        valpack_decode<L>(blk.data(), valpack_scale(e), out.data());
        for (int i = 0; i < L; ++i) CHECK(bits_of(out[i]) == 0ull);
        ++g_cases;
    }
    // +0.0 is a value like any other
    one_row<L>(std::vector<int64_t>(L, 0), -52);
    // a quantum that is not a normal double, and one whose largest field overflows: refused whatever the values
    CHECK(!valpack_exp_ok(-1023) && valpack_exp_ok(-1022) && valpack_exp_ok(970) && !valpack_exp_ok(971));
    refused<L>(std::vector<double>(L, 0.0), -1023);
    refused<L>(std::vector<double>(L, std::numeric_limits<double>::denorm_min()), -1074);   // a subnormal quantum
    refused<L>(std::vector<double>(L, std::ldexp(1.0, -1050)), -1050);
    refused<L>(std::vector<double>(L, std::ldexp(1.0, 1000)), 1000);
    // subnormal VALUES are no multiples of the smallest normal quantum
    refused<L>(std::vector<double>(L, std::ldexp(1.0, -1030)), -1022);
    one_row<L>(std::vector<int64_t>(L, 3), -1022);
}

int main() {
    static_assert(!valpack_length_ok(10) && valpack_length_ok(12) && !valpack_length_ok(13) && valpack_length_ok(14) &&
                      valpack_length_ok(16) && !valpack_length_ok(18), "even lengths from 12 to 16");
    std::mt19937_64 rng(20240917u);
    for (int e : {0, -52, -1000, 900}) {
        at_exponent<12>(e, rng, 5000);
        at_exponent<14>(e, rng, 5000);
        at_exponent<16>(e, rng, 5000);
    }
    pad_and_quanta<12>();
    pad_and_quanta<14>();
    pad_and_quanta<16>();
    printf("ok %ld\n", g_cases);
    return 0;
}
