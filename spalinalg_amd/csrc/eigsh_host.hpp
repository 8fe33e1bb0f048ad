// eigsh_host.hpp -- the host half of spal_*_eigsh_* (thick-restart Lanczos): the projected problem.  Plain
// C++ on doubles, no device: cyclic Jacobi in a fixed order with a fixed stop rule, the ordering of the Ritz values, the
// residual estimates and the count of converged pairs.  Only + - * / sqrt, contraction off: the text of include/spal.h,
// which tests/eigsh_ref.py restates in numpy bit for bit.  (Not installed.)
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#pragma clang fp contract(off)

namespace spal {

constexpr unsigned kJacobiSweeps = 64;   // the cap; a sweep without a rotation ends the iteration (6 .. 10 in practice)

// S: m x m, symmetric, row-major, finite; on exit its diagonal holds the eigenvalues.  Y: m x m, row-major; on exit
// column i is the eigenvector of S[i, i].  Returns the sweeps that rotated.
inline unsigned eigsh_jacobi(uint64_t m, double *S, double *Y) {
    for (uint64_t i = 0; i < m; ++i)
        for (uint64_t j = 0; j < m; ++j) Y[i * m + j] = i == j ? 1.0 : 0.0;
    unsigned sweep = 0;
    for (; sweep < kJacobiSweeps; ++sweep) {
        bool rotated = false;
        for (uint64_t p = 0; p + 1 < m; ++p) {
            for (uint64_t q = p + 1; q < m; ++q) {
                const double apq = S[p * m + q];
                if (apq == 0.0) continue;
                const double app = S[p * m + p], aqq = S[q * m + q], g = std::fabs(apq);
                if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    S[p * m + q] = S[q * m + p] = 0.0;   // below the rounding of both diagonal entries
                    continue;
                }
                rotated = true;
                const double theta = (0.5 * (aqq - app)) / apq;
                double t = 1.0 / (std::fabs(theta) + std::sqrt((theta * theta) + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / std::sqrt((t * t) + 1.0), s = t * c;
                S[p * m + p] = app - (t * apq);
                S[q * m + q] = aqq + (t * apq);
                S[p * m + q] = S[q * m + p] = 0.0;
                for (uint64_t r = 0; r < m; ++r) {
                    if (r == p || r == q) continue;
                    const double a = S[r * m + p], b = S[r * m + q];
                    S[r * m + p] = S[p * m + r] = (c * a) - (s * b);
                    S[r * m + q] = S[q * m + r] = (s * a) + (c * b);
                }
                for (uint64_t r = 0; r < m; ++r) {
                    const double a = Y[r * m + p], b = Y[r * m + q];
                    Y[r * m + p] = (c * a) - (s * b);
                    Y[r * m + q] = (s * a) + (c * b);
                }
            }
        }
        if (!rotated) break;
    }
    return sweep;
}

// The Ritz pairs of one phase, ordered: theta[i], column i of Y (m x m, row-major), res[i] = |hn * Y[m - 1, i]|.
struct RitzPairs {
    std::vector<double> theta, Y, res;
    double scale = 0.0;   // max |theta|
    unsigned sweeps = 0;
};

// false: S holds a value that is not finite (reason 2).  S is m x m, row-major, and is destroyed.  which: 0 = LA
// (descending), 1 = SA (ascending); ties go by position.
inline bool eigsh_ritz(uint64_t m, double *S, double hn, int which, RitzPairs *out) {
    for (uint64_t i = 0; i < m * m; ++i)
        if (!std::isfinite(S[i])) return false;
    std::vector<double> Q(m * m);
    out->sweeps = eigsh_jacobi(m, S, Q.data());
    std::vector<uint64_t> order(m);
    for (uint64_t i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        return which == 0 ? S[a * m + a] > S[b * m + b] : S[a * m + a] < S[b * m + b];
    });
    out->theta.resize(m);
    out->res.resize(m);
    out->Y.resize(m * m);
    out->scale = 0.0;
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t o = order[i];
        out->theta[i] = S[o * m + o];
        out->scale = std::max(out->scale, std::fabs(out->theta[i]));
        for (uint64_t r = 0; r < m; ++r) out->Y[r * m + i] = Q[r * m + o];
        out->res[i] = std::fabs(hn * out->Y[(m - 1) * m + i]);
    }
    return true;
}

// the leading pairs among the first nk with res[i] <= tol * max |theta|
inline uint64_t eigsh_converged(const RitzPairs &p, uint64_t nk, double tol) {
    uint64_t c = 0;
    while (c < nk && p.res[c] <= tol * p.scale) ++c;
    return c;
}

inline uint64_t eigsh_keep(uint64_t k, uint64_t ncv) { return std::min(k + (ncv - k) / 2, ncv - 1); }

}  // namespace spal
