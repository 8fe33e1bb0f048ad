// Stand-alone host program for the sanitizers (address, undefined behaviour): no GPU, no Python.  It is linked with the
// host side of spal_eigsh.hip and spal_host.cpp compiled under -fsanitize=address,undefined and drives what those do
// before any device work: spal_eigsh_jacobi, the Jacobi text, on buffers of exactly the size the call claims, and the
// refusals of every spal_*_eigsh_* entry point that need no device.  tests/test_eigsh_sanitize.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "spal.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool refused(int status, const char *text) {
    return status == SPAL_ERR_INVALID_ARGUMENT && std::string(spal_last_error()).find(text) != std::string::npos;
}

// S = the m x m matrix with S[i][j] = 1 / (1 + |i - j|) + (i == j ? i : 0): symmetric, distinct eigenvalues
static void host_text(uint64_t m) {
    std::vector<double> s(m * m), theta(m), y(m * m);
    for (uint64_t i = 0; i < m; ++i)
        for (uint64_t j = 0; j < m; ++j) s[i * m + j] = 1.0 / (1.0 + (double)(i > j ? i - j : j - i)) + (i == j ? (double)i : 0.0);
    uint64_t sweeps = 99;
    CHECK(spal_eigsh_jacobi(m, s.data(), theta.data(), y.data(), &sweeps) == SPAL_OK);
    CHECK(sweeps < 12);
    double worst = 0.0, trace = 0.0, sum = 0.0;
    for (uint64_t i = 0; i < m; ++i) {
        trace += s[i * m + i];
        sum += theta[i];
        for (uint64_t c = 0; c < m; ++c) {   // (S Y - Y diag(theta))[i, c]
            double r = -y[i * m + c] * theta[c];
            for (uint64_t t = 0; t < m; ++t) r += s[i * m + t] * y[t * m + c];
            worst = std::fmax(worst, std::fabs(r));
        }
    }
    CHECK(worst <= 1e-13 * (double)(m + 1));
    CHECK(std::fabs(trace - sum) <= 1e-12 * (double)(m * m + 1));
    CHECK(spal_eigsh_jacobi(m, s.data(), theta.data(), y.data(), nullptr) == SPAL_OK);   // sweeps may be NULL
}

template <typename T, typename H, typename Host, typename Dev>
static void entry_refusals(Host host, Dev dev) {
    std::vector<unsigned char> zeros(1 << 16, 0);   // stands in for a handle in calls that end before it is looked at
    H fake = reinterpret_cast<H>(zeros.data());
    std::vector<T> theta(2, T(9)), resid(2, T(9)), x(12 * 2, T(9));
    spal_eigsh_info info;
    auto h = [&](H a, uint64_t k, int which, uint64_t ncv, double tol, T *th, T *rs, uint64_t ldx, spal_eigsh_info *inf) {
        return host(a, k, which, ncv, nullptr, 0, 0, tol, 3, th, k, rs, k, x.data(), ldx, 12, inf);
    };
    auto d = [&](H a, uint64_t k, int which, uint64_t ncv, double tol, T *th, T *rs, uint64_t ldx, spal_eigsh_info *inf) {
        return dev(a, k, which, ncv, nullptr, 0, tol, 3, th, rs, x.data(), ldx, nullptr, inf);
    };
    auto all = [&](auto f) {
        CHECK(refused(f(nullptr, 2, 0, 8, 1e-8, theta.data(), resid.data(), 2, &info), "null argument"));
        CHECK(refused(f(fake, 2, 0, 8, 1e-8, nullptr, resid.data(), 2, &info), "null argument"));
        CHECK(refused(f(fake, 2, 0, 8, 1e-8, theta.data(), nullptr, 2, &info), "null argument"));
        CHECK(refused(f(fake, 2, 0, 8, 1e-8, theta.data(), resid.data(), 2, nullptr), "null argument"));
        CHECK(refused(f(fake, 0, 0, 8, 1e-8, theta.data(), resid.data(), 2, &info), "k = 0"));
        CHECK(refused(f(fake, 2, 0, 2, 1e-8, theta.data(), resid.data(), 2, &info), "must be greater than k = 2"));
        CHECK(refused(f(fake, 2, 0, 257, 1e-8, theta.data(), resid.data(), 2, &info), "must be at most 256"));
        CHECK(refused(f(fake, 2, 2, 8, 1e-8, theta.data(), resid.data(), 2, &info), "which = 2"));
        CHECK(refused(f(fake, 2, 0, 8, -1.0, theta.data(), resid.data(), 2, &info), "must be finite and >= 0"));
        CHECK(refused(f(fake, 2, 0, 8, NAN, theta.data(), resid.data(), 2, &info), "must be finite and >= 0"));
        CHECK(refused(f(fake, 2, 0, 8, INFINITY, theta.data(), resid.data(), 2, &info), "must be finite and >= 0"));
        CHECK(refused(f(fake, 2, 0, 8, 1e-8, theta.data(), resid.data(), 1, &info), "ldx = 1 is less than k = 2"));
    };
    all(h);
    all(d);
    for (const T v : theta) CHECK(v == T(9));
    for (const T v : resid) CHECK(v == T(9));
    for (const T v : x) CHECK(v == T(9));
}

int main() {
    for (uint64_t m : {1, 2, 9, 24, 64}) host_text(m);
    std::vector<double> s(4, 1.0), out(4);
    CHECK(refused(spal_eigsh_jacobi(0, s.data(), out.data(), out.data(), nullptr), "m = 0"));
    CHECK(refused(spal_eigsh_jacobi(2, nullptr, out.data(), out.data(), nullptr), "null argument"));
    s[1] = 2.0;
    CHECK(refused(spal_eigsh_jacobi(2, s.data(), out.data(), out.data(), nullptr), "not symmetric"));
    s[1] = s[2] = NAN;
    CHECK(refused(spal_eigsh_jacobi(2, s.data(), out.data(), out.data(), nullptr), "not finite"));
    entry_refusals<double, spal_csr_t>(spal_csr_eigsh_f64, spal_csr_eigsh_dev_f64);
    entry_refusals<float, spal_csr_t>(spal_csr_eigsh_f32, spal_csr_eigsh_dev_f32);
    entry_refusals<double, spal_csc_t>(spal_csc_eigsh_f64, spal_csc_eigsh_dev_f64);
    entry_refusals<float, spal_csc_t>(spal_csc_eigsh_f32, spal_csc_eigsh_dev_f32);
    if (failures) return 1;
    printf("eigsh sanitize ok\n");
    return 0;
}
