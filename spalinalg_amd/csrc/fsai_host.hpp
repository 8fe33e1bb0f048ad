// fsai_host.hpp -- the host half of FSAI (spal_*_fsai_setup: DESIGN 3.30).  Plain C++, no device and no library call:
// the text's Cholesky and back-substitution on ONE local system (what spal_fsai_row_* run), the rejected row, and the
// range of the option "fsai_max_row".  The text is in include/spal.h; tests/fsai_ref.py restates it in numpy bit for
// bit, and tests/cpp/test_fsai_asan.cpp compiles this header alone under the sanitizers.  (Not installed.)
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

namespace spal {

constexpr int64_t kFsaiCapDefault = 32, kFsaiCapMax = 64;   // the option "fsai_max_row": 1 .. 64
inline bool fsai_cap_valid(int64_t cap) { return cap >= 1 && cap <= kFsaiCapMax; }

// element (r, c), c <= r, of a lower triangle packed by rows
inline size_t fsai_idx(size_t r, size_t c) { return r * (r + 1) / 2 + c; }

// G[i, i] of a rejected row: 1 / sqrt(a_ii) where that is a finite number, else 1
template <typename T>
inline T fsai_reject_diag(T aii) {
    if (aii > T(0) && std::isfinite(aii)) {
        const T d = T(1) / std::sqrt(aii);
        if (std::isfinite(d)) return d;
    }
    return T(1);
}

// One row of the text: b = the packed lower triangle B (m (m + 1) / 2 values), c = as many values of scratch (b and c
// may be the same array), g = m values.  Returns 1 when the row is rejected: then g = (0, ..., 0, G[i, i]).
template <typename T>
inline int fsai_row_host(size_t m, const T *b, T *c, T *g) {
    const T aii = b[fsai_idx(m - 1, m - 1)];
    bool rejected = false;
    for (size_t j = 0; j < m && !rejected; ++j) {
        T d = b[fsai_idx(j, j)];
        for (size_t k = 0; k < j; ++k) d = d - (c[fsai_idx(j, k)] * c[fsai_idx(j, k)]);
        if (!(d > T(0) && std::isfinite(d))) {
            rejected = true;
            break;
        }
        const T cjj = std::sqrt(d);
        c[fsai_idx(j, j)] = cjj;
        for (size_t r = j + 1; r < m; ++r) {
            T t = b[fsai_idx(r, j)];
            for (size_t k = 0; k < j; ++k) t = t - (c[fsai_idx(r, k)] * c[fsai_idx(j, k)]);
            c[fsai_idx(r, j)] = t / cjj;
        }
    }
    if (!rejected) {
        g[m - 1] = T(1) / c[fsai_idx(m - 1, m - 1)];
        for (size_t t = m - 1; t-- > 0;) {
            T s = T(0);
            for (size_t u = t + 1; u < m; ++u) s = s + (c[fsai_idx(u, t)] * g[u]);
            g[t] = (T(0) - s) / c[fsai_idx(t, t)];
        }
        for (size_t t = 0; t < m; ++t)
            if (!std::isfinite(g[t])) rejected = true;
    }
    if (rejected) {
        for (size_t t = 0; t + 1 < m; ++t) g[t] = T(0);
        g[m - 1] = fsai_reject_diag<T>(aii);
    }
    return rejected ? 1 : 0;
}

}  // namespace spal
