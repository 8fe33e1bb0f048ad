// test_fsai_asan.cpp -- the host half of FSAI (spalinalg_amd/csrc/fsai_host.hpp) as a stand-alone program under
// -fsanitize=address,undefined: the text's Cholesky and back-substitution on exact-size buffers for m = 1 .. 64, in
// place and out of place, the rejected rows, and the option's range.  No library, no device.
#include "fsai_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace spal;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                        \
        }                                                                    \
    } while (0)

// the leading m x m block of the tridiagonal (-1, 4, -1) matrix with a -1 at distance 8: Poisson 8 x 8's
template <typename T>
static std::vector<T> poisson_lower(size_t m) {
    std::vector<T> b(m * (m + 1) / 2, T(0));
    for (size_t r = 0; r < m; ++r) {
        b[fsai_idx(r, r)] = T(4);
        if (r >= 1 && r % 8 != 0) b[fsai_idx(r, r - 1)] = T(-1);
        if (r >= 8) b[fsai_idx(r, r - 8)] = T(-1);
    }
    return b;
}

template <typename T>
static int rows() {
    for (size_t m : {1, 2, 3, 7, 13, 33, 64}) {
        const std::vector<T> b = poisson_lower<T>(m);   // exactly m (m + 1) / 2 values: one more read is out of bounds
        std::vector<T> c(b.size()), g(m), c2 = b, g2(m);
        CHECK(fsai_row_host<T>(m, b.data(), c.data(), g.data()) == 0);
        CHECK(fsai_row_host<T>(m, c2.data(), c2.data(), g2.data()) == 0);   // in place: the same values
        for (size_t t = 0; t < m; ++t) CHECK(g[t] == g2[t] && std::isfinite(g[t]));
        CHECK(g[m - 1] > T(0));
        // row m - 1 of G A Gt: g^T B g = 1 up to rounding (B symmetric, given by its lower triangle)
        double q = 0.0;
        for (size_t r = 0; r < m; ++r)
            for (size_t s = 0; s < m; ++s) q += (double)g[r] * (double)b[r >= s ? fsai_idx(r, s) : fsai_idx(s, r)] * (double)g[s];
        CHECK(std::fabs(q - 1.0) <= 8.0 * (double)m * (double)std::numeric_limits<T>::epsilon());
    }
    return 0;
}

template <typename T>
static int rejections() {
    const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
    std::vector<T> g(7), c(28);
    for (int which = 0; which < 6; ++which) {
        std::vector<T> b = poisson_lower<T>(7);
        T expect = T(0.5);   // 1 / sqrt(4)
        if (which == 0) b[fsai_idx(0, 0)] = T(-4);                      // a non-positive first pivot
        if (which == 1) b[fsai_idx(6, 6)] = T(-4), expect = T(1);       // a non-positive last pivot
        if (which == 2) b[fsai_idx(1, 0)] = T(-4);                      // a pivot made negative by cancellation: 4 - 4
        if (which == 3) b[fsai_idx(3, 1)] = nan;                        // a NaN entry
        if (which == 4) b[fsai_idx(6, 6)] = inf, expect = T(1);         // an Inf diagonal
        if (which == 5) b[fsai_idx(0, 0)] = T(0);                       // a zero pivot
        CHECK(fsai_row_host<T>(7, b.data(), c.data(), g.data()) == 1);
        for (size_t t = 0; t < 6; ++t) CHECK(g[t] == T(0));
        CHECK(g[6] == expect);
    }
    CHECK(fsai_reject_diag<T>(T(0)) == T(1) && fsai_reject_diag<T>(nan) == T(1) && fsai_reject_diag<T>(T(-1)) == T(1));
    CHECK(fsai_reject_diag<T>(T(16)) == T(0.25));
    return 0;
}

// f32: B = 2^-146 L Lt, L unit lower bidiagonal with -32 below the diagonal: every pivot is positive, g overflows
static int overflow() {
    const size_t m = 13;
    const float s = std::ldexp(1.0f, -146);
    std::vector<float> b(m * (m + 1) / 2, 0.0f), g(m);
    for (size_t r = 0; r < m; ++r) {
        b[fsai_idx(r, r)] = (r ? 1025.0f : 1.0f) * s;
        if (r) b[fsai_idx(r, r - 1)] = -32.0f * s;
    }
    CHECK(fsai_row_host<float>(m, b.data(), b.data(), g.data()) == 1);
    for (size_t t = 0; t + 1 < m; ++t) CHECK(g[t] == 0.0f);
    CHECK(std::isfinite(g[m - 1]) && g[m - 1] > 1e20f);
    return 0;
}

int main() {
    if (rows<double>() || rows<float>() || rejections<double>() || rejections<float>() || overflow()) return 1;
    if (!(fsai_cap_valid(1) && fsai_cap_valid(32) && fsai_cap_valid(64) && !fsai_cap_valid(0) && !fsai_cap_valid(65) &&
          !fsai_cap_valid(-1))) {
        std::printf("FAILED fsai_cap_valid\n");
        return 1;
    }
    std::printf("fsai sanitize ok\n");
    return 0;
}
