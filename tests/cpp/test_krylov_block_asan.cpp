// Stand-alone host program for the sanitizers (address, undefined behaviour): no GPU, no Python.  It is linked with the
// host side of spal_krylov_block.hip, spal_krylov.hip and spal_host.cpp compiled under -fsanitize=address,undefined and
// drives what those do before any device work: the argument checking of the eight spal_*_krylov_block_* entry points,
// the "krylov_tile" option's validation, and spal_dot_* -- the host reduce the definition of every column's dot rests on.
// tests/test_krylov_block_sanitize.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "spal.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool refused(int status, const char *prefix, const char *text) {
    const std::string msg = spal_last_error();
    return status == SPAL_ERR_INVALID_ARGUMENT && msg.rfind(prefix, 0) == 0 && msg.find(text) != std::string::npos;
}

template <typename T, typename H, typename Host, typename Dev>
static void entry_points(const char *prefix, Host host, Dev dev) {
    // exactly as large as the calls claim: a read or write past them is the sanitizer's to report
    std::vector<T> b(4 * 3, T(1)), x(4 * 3, T(0));
    std::vector<spal_krylov_info> info(3);
    std::vector<unsigned char> zeros(1 << 16, 0);       // stands in for a handle in calls that end before it is looked at
    H fake = reinterpret_cast<H>(zeros.data());
    CHECK(refused(host(nullptr, 0, nullptr, 3, b.data(), 3, 4, x.data(), 3, 4, 1e-8, 5, info.data()), prefix, "null argument"));
    CHECK(refused(host(fake, 0, nullptr, 3, nullptr, 3, 4, x.data(), 3, 4, 1e-8, 5, info.data()), prefix, "null argument"));
    CHECK(refused(host(fake, 0, nullptr, 3, b.data(), 3, 4, nullptr, 3, 4, 1e-8, 5, info.data()), prefix, "null argument"));
    CHECK(refused(host(fake, 0, nullptr, 3, b.data(), 3, 4, x.data(), 3, 4, 1e-8, 5, nullptr), prefix, "null argument"));
    CHECK(refused(host(fake, 0, nullptr, 0, b.data(), 3, 4, x.data(), 3, 4, 1e-8, 5, info.data()), prefix, "k = 0"));
    CHECK(refused(host(fake, 0, nullptr, 3, b.data(), 2, 4, x.data(), 3, 4, 1e-8, 5, info.data()), prefix, "ldb = 2 is less than k = 3"));
    CHECK(refused(host(fake, 0, nullptr, 3, b.data(), 3, 4, x.data(), 1, 4, 1e-8, 5, info.data()), prefix, "ldx = 1 is less than k = 3"));
    CHECK(refused(host(fake, 9, nullptr, 3, b.data(), 3, 4, x.data(), 3, 4, 1e-8, 5, info.data()), prefix, "method = 9"));
    CHECK(refused(host(fake, 0, nullptr, 1ull << 32, b.data(), 1ull << 32, 4, x.data(), 1ull << 32, 4, 1e-8, 5, info.data()),
                  prefix, "does not fit 32 bits"));
    CHECK(refused(dev(nullptr, 1, nullptr, 3, b.data(), 3, x.data(), 3, 1e-8, 5, nullptr, info.data()), prefix, "null argument"));
    CHECK(refused(dev(fake, 1, nullptr, 0, b.data(), 3, x.data(), 3, 1e-8, 5, nullptr, info.data()), prefix, "k = 0"));
    CHECK(refused(dev(fake, 1, nullptr, 3, b.data(), 3, x.data(), 2, 1e-8, 5, nullptr, info.data()), prefix, "ldx = 2"));
    for (const T v : x) CHECK(v == T(0));               // nothing was written
}

// the definition of include/spal.h, restated: pad to tiles of 1024, halve every tile, reduce the tile sums
template <typename T>
static T reduce(std::vector<T> v) {
    const size_t c = v.empty() ? 1 : (v.size() + 1023) / 1024;
    v.resize(c * 1024, T(0));
    std::vector<T> sums(c);
    for (size_t tile = 0; tile < c; ++tile) {
        T *e = v.data() + tile * 1024;
        for (size_t h = 512; h >= 1; h /= 2)
            for (size_t t = 0; t < h; ++t) e[t] = e[t] + e[t + h];
        sums[tile] = e[0];
    }
    return c == 1 ? sums[0] : reduce(sums);
}

template <typename T, typename Dot>
static void host_reduce(Dot dot) {
    for (size_t n : {size_t(0), size_t(1), size_t(1023), size_t(1024), size_t(1025), size_t(1024 * 1024 + 1)}) {
        std::vector<T> a(n), b(n), p(n);                 // exactly n elements
        unsigned long long s = 88172645463325252ull + n;
        for (size_t i = 0; i < n; ++i) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            a[i] = T((double)(s % 2000001) / 1e6 - 1.0) * T(std::pow(10.0, (double)((s >> 40) % 13) - 6.0));
            b[i] = T((double)((s >> 20) % 2000001) / 1e6 - 1.0);
            p[i] = a[i] * b[i];
        }
        T got = T(7);
        CHECK(dot(a.data(), b.data(), n, &got) == SPAL_OK);
        const T want = reduce(p);
        CHECK(std::memcmp(&got, &want, sizeof(T)) == 0);
    }
    T out = T(0);
    CHECK(dot(nullptr, nullptr, 3, &out) == SPAL_ERR_INVALID_ARGUMENT);
}

int main() {
    entry_points<double, spal_csr_t>("spal_csr_krylov_block:", spal_csr_krylov_block_f64, spal_csr_krylov_block_dev_f64);
    entry_points<float, spal_csr_t>("spal_csr_krylov_block:", spal_csr_krylov_block_f32, spal_csr_krylov_block_dev_f32);
    entry_points<double, spal_csc_t>("spal_csc_krylov_block:", spal_csc_krylov_block_f64, spal_csc_krylov_block_dev_f64);
    entry_points<float, spal_csc_t>("spal_csc_krylov_block:", spal_csc_krylov_block_f32, spal_csc_krylov_block_dev_f32);
    std::vector<unsigned char> zeros(1 << 16, 0);
    for (long long bad : {3ll, -1ll, 64ll, 1ll << 40}) {
        CHECK(spal_csr_set_option(reinterpret_cast<spal_csr_t>(zeros.data()), "krylov_tile", bad) == SPAL_ERR_INVALID_ARGUMENT);
        CHECK(std::string(spal_last_error()).find("krylov_tile must be 0") != std::string::npos);
    }
    host_reduce<double>(spal_dot_f64);
    host_reduce<float>(spal_dot_f32);
    if (failures) return 1;
    printf("krylov block sanitize ok\n");
    return 0;
}
