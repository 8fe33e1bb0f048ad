// Stand-alone host program for the sanitizers (address, undefined behaviour): no GPU, no Python.  It is linked with the
// host side of spal_gmres_block.hip, spal_gmres.hip and spal_host.cpp compiled under -fsanitize=address,undefined and
// drives what those do before any device work: the argument checking of the eight spal_*_gmres_block_* entry points
// (and of spal_*_gmres_*, whose refusals they repeat), and the "krylov_tile" option's validation.
// tests/test_gmres_block_sanitize.py builds and runs it.
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
    CHECK(refused(host(nullptr, nullptr, 3, b.data(), 3, 4, x.data(), 3, 4, 5, 1e-8, 5, info.data()), prefix, "null argument"));
    CHECK(refused(host(fake, nullptr, 3, nullptr, 3, 4, x.data(), 3, 4, 5, 1e-8, 5, info.data()), prefix, "null argument"));
    CHECK(refused(host(fake, nullptr, 3, b.data(), 3, 4, nullptr, 3, 4, 5, 1e-8, 5, info.data()), prefix, "null argument"));
    CHECK(refused(host(fake, nullptr, 3, b.data(), 3, 4, x.data(), 3, 4, 5, 1e-8, 5, nullptr), prefix, "null argument"));
    CHECK(refused(host(fake, nullptr, 0, b.data(), 3, 4, x.data(), 3, 4, 5, 1e-8, 5, info.data()), prefix, "k = 0"));
    CHECK(refused(host(fake, nullptr, 3, b.data(), 2, 4, x.data(), 3, 4, 5, 1e-8, 5, info.data()), prefix, "ldb = 2 is less than k = 3"));
    CHECK(refused(host(fake, nullptr, 3, b.data(), 3, 4, x.data(), 1, 4, 5, 1e-8, 5, info.data()), prefix, "ldx = 1 is less than k = 3"));
    CHECK(refused(host(fake, nullptr, 3, b.data(), 3, 4, x.data(), 3, 4, 0, 1e-8, 5, info.data()), prefix, "restart = 0 must be 1 .. 256"));
    CHECK(refused(host(fake, nullptr, 3, b.data(), 3, 4, x.data(), 3, 4, 257, 1e-8, 5, info.data()), prefix, "restart = 257 must be"));
    CHECK(refused(host(fake, nullptr, 1ull << 32, b.data(), 1ull << 32, 4, x.data(), 1ull << 32, 4, 5, 1e-8, 5, info.data()),
                  prefix, "does not fit 32 bits"));
    CHECK(refused(dev(nullptr, nullptr, 3, b.data(), 3, x.data(), 3, 5, 1e-8, 5, nullptr, info.data()), prefix, "null argument"));
    CHECK(refused(dev(fake, nullptr, 0, b.data(), 3, x.data(), 3, 5, 1e-8, 5, nullptr, info.data()), prefix, "k = 0"));
    CHECK(refused(dev(fake, nullptr, 3, b.data(), 3, x.data(), 2, 5, 1e-8, 5, nullptr, info.data()), prefix, "ldx = 2"));
    CHECK(refused(dev(fake, nullptr, 3, b.data(), 3, x.data(), 3, 1000, 1e-8, 5, nullptr, info.data()), prefix, "restart = 1000"));
    for (const T v : x) CHECK(v == T(0));               // nothing was written
}

// the vector entry points' own null checks: the block calls refuse everything these refuse
template <typename T, typename H, typename Host, typename Dev>
static void vector_entry_points(const char *prefix, Host host, Dev dev) {
    std::vector<T> b(4, T(1)), x(4, T(0));
    spal_krylov_info info;
    std::vector<unsigned char> zeros(1 << 16, 0);
    H fake = reinterpret_cast<H>(zeros.data());
    CHECK(refused(host(nullptr, nullptr, b.data(), 4, x.data(), 4, 5, 1e-8, 5, &info), prefix, "null argument"));
    CHECK(refused(host(fake, nullptr, b.data(), 4, x.data(), 4, 5, 1e-8, 5, nullptr), prefix, "null argument"));
    CHECK(refused(dev(fake, nullptr, nullptr, x.data(), 5, 1e-8, 5, nullptr, &info), prefix, "null argument"));
    for (const T v : x) CHECK(v == T(0));
}

int main() {
    entry_points<double, spal_csr_t>("spal_csr_gmres_block:", spal_csr_gmres_block_f64, spal_csr_gmres_block_dev_f64);
    entry_points<float, spal_csr_t>("spal_csr_gmres_block:", spal_csr_gmres_block_f32, spal_csr_gmres_block_dev_f32);
    entry_points<double, spal_csc_t>("spal_csc_gmres_block:", spal_csc_gmres_block_f64, spal_csc_gmres_block_dev_f64);
    entry_points<float, spal_csc_t>("spal_csc_gmres_block:", spal_csc_gmres_block_f32, spal_csc_gmres_block_dev_f32);
    vector_entry_points<double, spal_csr_t>("spal_csr_gmres", spal_csr_gmres_f64, spal_csr_gmres_dev_f64);
    vector_entry_points<float, spal_csc_t>("spal_csc_gmres", spal_csc_gmres_f32, spal_csc_gmres_dev_f32);
    std::vector<unsigned char> zeros(1 << 16, 0);
    for (long long bad : {3ll, -1ll, 64ll, 1ll << 40}) {
        CHECK(spal_csr_set_option(reinterpret_cast<spal_csr_t>(zeros.data()), "krylov_tile", bad) == SPAL_ERR_INVALID_ARGUMENT);
        CHECK(std::string(spal_last_error()).find("krylov_tile must be 0") != std::string::npos);
    }
    if (failures) return 1;
    printf("gmres block sanitize ok\n");
    return 0;
}
