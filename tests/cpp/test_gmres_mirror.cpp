// C++ host-mirror test of restarted GMRES (include/spalinalg.hpp: gmres).
//   ./test_gmres_mirror host   -- no GPU needed: the sequential text of include/spal.h restated here on the library's
//                                 dot() solves a dense system and the cyclic shift; gmres() is there for both formats
//                                 and types and panics on wrong shapes and restarts before any device call
//   ./test_gmres_mirror gpu    -- a nonsymmetric tridiagonal matrix against the restatement, its ILU(0) factor as M,
//                                 the cyclic shift (the lucky breakdown), maxit, the refusals
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "spalinalg.hpp"

using namespace spalinalg;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::string panic_text(const std::function<void()> &f) {
    try { f(); } catch (const Panic &p) { return p.what(); }
    return "";
}

// The text of include/spal.h, restated.  Every product is a statement of its own, so no compiler contracts it into an
// FMA.  mul: w = A v;  M^-1 is the identity.
template <typename T>
static Solution<T> gmres_text(const std::function<std::vector<T>(const std::vector<T> &)> &mul, const std::vector<T> &b,
                              std::vector<T> x, size_t m, double tol, size_t maxit) {
    const size_t n = b.size();
    const T bb = dot(b, b), thr = T(tol * tol) * bb;
    size_t it = 0;
    auto result = [&](int reason, T rr) { return Solution<T>{x, it, reason, (double)rr, (double)bb, 0.0}; };
    for (;;) {
        const std::vector<T> q = mul(x);
        std::vector<T> r(n);
        for (size_t i = 0; i < n; ++i) r[i] = b[i] - q[i];
        const T rr = dot(r, r);
        if (rr <= thr) return result(0, rr);
        if (!std::isfinite(rr)) return result(2, rr);
        if (it == maxit) return result(1, rr);
        const T beta = std::sqrt(rr);
        std::vector<std::vector<T>> V(1, std::vector<T>(n));
        for (size_t i = 0; i < n; ++i) V[0][i] = r[i] / beta;
        std::vector<T> g(m + 1, T(0)), cs(m, T(0)), sn(m, T(0)), H((m + 1) * m, T(0));
        g[0] = beta;
        size_t jj = 0;
        for (;;) {
            const size_t j = jj;
            std::vector<T> w = mul(V[j]), h(j + 2), c(j + 1);
            for (size_t k = 0; k <= j; ++k) h[k] = dot(V[k], w);
            for (size_t k = 0; k <= j; ++k)
                for (size_t i = 0; i < n; ++i) { const volatile T p = h[k] * V[k][i]; w[i] = w[i] - p; }
            for (size_t k = 0; k <= j; ++k) c[k] = dot(V[k], w);
            for (size_t k = 0; k <= j; ++k)
                for (size_t i = 0; i < n; ++i) { const volatile T p = c[k] * V[k][i]; w[i] = w[i] - p; }
            for (size_t k = 0; k <= j; ++k) h[k] = h[k] + c[k];
            const T hn = std::sqrt(dot(w, w));
            V.emplace_back(n);
            for (size_t i = 0; i < n; ++i) V[j + 1][i] = w[i] / hn;
            it += 1;
            h[j + 1] = hn;
            for (size_t k = 0; k < j; ++k) {
                const volatile T p0 = cs[k] * h[k], p1 = sn[k] * h[k + 1], p2 = cs[k] * h[k + 1], p3 = sn[k] * h[k];
                h[k] = p0 + p1;
                h[k + 1] = p2 - p3;
            }
            const volatile T s0 = h[j] * h[j], s1 = hn * hn;
            const T d = std::sqrt(s0 + s1);
            cs[j] = h[j] / d;
            sn[j] = hn / d;
            h[j] = d;
            g[j + 1] = -(sn[j] * g[j]);
            g[j] = cs[j] * g[j];
            for (size_t k = 0; k <= j; ++k) H[j * (m + 1) + k] = h[k];
            const T est = g[j + 1] * g[j + 1];
            jj = j + 1;
            if (!std::isfinite(est)) return result(2, est);   // x is what it was at the start of this cycle
            if (est <= thr || it == maxit || jj == m) break;
        }
        std::vector<T> y(jj);
        for (size_t k = jj; k-- > 0;) {   // column form
            y[k] = g[k] / H[k * (m + 1) + k];
            for (size_t l = 0; l < k; ++l) { const volatile T p = H[k * (m + 1) + l] * y[k]; g[l] = g[l] - p; }
        }
        for (size_t i = 0; i < n; ++i) {
            T u = y[0] * V[0][i];
            for (size_t k = 1; k < jj; ++k) { const volatile T p = y[k] * V[k][i]; u = u + p; }
            x[i] = x[i] + u;
        }
    }
}

template <typename T>
static std::function<std::vector<T>(const std::vector<T> &)> shift_mul() {
    return [](const std::vector<T> &v) {
        std::vector<T> w(v.size());
        for (size_t i = 0; i < v.size(); ++i) w[(i + 1) % v.size()] = v[i];
        return w;
    };
}

template <typename T>
static void host_text() {
    const double tol = sizeof(T) == 8 ? 1e-10 : 1e-5;
    // dense, diagonally dominant, not symmetric
    const size_t n = 40;
    std::vector<T> a(n * n), b(n);
    unsigned long long s = 88172645463325252ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return T((double)(s % 2000001) / 1e6 - 1.0); };
    for (size_t i = 0; i < n; ++i) {
        T sum = 0;
        for (size_t k = 0; k < n; ++k) { a[i * n + k] = next(); if (k != i) sum += std::fabs(a[i * n + k]); }
        a[i * n + i] = 1 + sum;
        b[i] = next();
    }
    auto mul = [&](const std::vector<T> &v) {
        std::vector<T> w(n, T(0));
        for (size_t i = 0; i < n; ++i)
            for (size_t k = 0; k < n; ++k) w[i] += a[i * n + k] * v[k];
        return w;
    };
    for (size_t restart : {size_t(1), size_t(5), size_t(30)}) {
        const Solution<T> r = gmres_text<T>(mul, b, std::vector<T>(n, T(0)), restart, tol, 200);
        CHECK(r.reason == 0 && r.iterations >= 1 && r.iterations <= 200);
        const std::vector<T> ax = mul(r.x);
        double rr = 0, bb = 0;
        for (size_t i = 0; i < n; ++i) { rr += ((double)b[i] - ax[i]) * ((double)b[i] - ax[i]); bb += (double)b[i] * b[i]; }
        CHECK(std::sqrt(rr) <= 2 * tol * std::sqrt(bb));
    }
    // the cyclic shift with b = e0: n steps, exact, and the NaN v_n of the lucky breakdown is never read
    std::vector<T> e0(8, T(0)), want(8, T(0));
    e0[0] = 1;
    want[7] = 1;
    const Solution<T> c8 = gmres_text<T>(shift_mul<T>(), e0, std::vector<T>(8, T(0)), 8, 1e-6, 200);
    CHECK(c8.reason == 0 && c8.iterations == 8 && c8.x == want && c8.residual_sq == 0.0);
    const Solution<T> c4 = gmres_text<T>(shift_mul<T>(), e0, std::vector<T>(8, T(0)), 4, 1e-6, 40);
    CHECK(c4.reason == 1 && c4.iterations == 40);
    const Solution<T> zero = gmres_text<T>([](const std::vector<T> &v) { return std::vector<T>(v.size(), T(0)); }, e0, want, 5, 1e-6, 200);
    CHECK(zero.reason == 2 && zero.iterations == 1 && zero.x == want);
    const Solution<T> none = gmres_text<T>(shift_mul<T>(), e0, std::vector<T>(8, T(0)), 8, 1e-6, 0);
    CHECK(none.reason == 1 && none.iterations == 0 && none.residual_sq == 1.0);
}

static void host_tests() {
    host_text<double>();
    host_text<float>();
    Solution<double> (CsrMatrix<double>::*a)(const std::vector<double> &, usize, const CsrMatrix<double> *,
                                             const std::vector<double> &, double, usize) const = &CsrMatrix<double>::gmres;
    Solution<float> (CscMatrix<float>::*b)(const std::vector<float> &, usize, const CscMatrix<float> *,
                                           const std::vector<float> &, double, usize) const = &CscMatrix<float>::gmres;
    CHECK(a && b);
    const CsrMatrix<double> R(2, 3, {0, 1, 2}, {0, 2}, {1, 2});
    CHECK(panic_text([&] { (void)R.gmres({1, 2}); }).find("not square (2 x 3)") != std::string::npos);
    const CscMatrix<float> S(2, 2, {0, 1, 2}, {0, 1}, {1, 2});
    CHECK(panic_text([&] { (void)S.gmres({1, 2, 3}); }).find("b.len() = 3") != std::string::npos);
    CHECK(panic_text([&] { (void)S.gmres({1, 2}, 30, nullptr, {1}); }).find("x0.len() = 1") != std::string::npos);
    CHECK(panic_text([&] { (void)S.gmres({1, 2}, 0); }).find("restart = 0 must be 1 .. 256") != std::string::npos);
    CHECK(panic_text([&] { (void)S.gmres({1, 2}, 257); }).find("restart = 257 must be 1 .. 256") != std::string::npos);
}

template <typename T>
static void gpu_tests() {
    // tridiag(-1, 2, -0.5): every row sum has at most three terms
    const std::vector<usize> ptr{0, 2, 5, 8, 11, 14, 16}, ind{0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5};
    const std::vector<T> val{2, -0.5, -1, 2, -0.5, -1, 2, -0.5, -1, 2, -0.5, -1, 2, -0.5, -1, 2};
    const std::vector<T> b{1, -2, 3, 0.5, 0, 7};
    const double tol = sizeof(T) == 8 ? 1e-12 : 1e-5;
    const CsrMatrix<T> A(6, 6, ptr, ind, val);
    auto mul = [&](const std::vector<T> &v) {
        std::vector<T> w(6, T(0));
        for (size_t i = 0; i < 6; ++i)
            for (usize e = ptr[i]; e < ptr[i + 1]; ++e) { const volatile T p = val[e] * v[ind[e]]; w[i] = w[i] + p; }
        return w;
    };
    const Solution<T> text = gmres_text<T>(mul, b, std::vector<T>(6, T(0)), 30, tol, 100);
    const Solution<T> got = A.gmres(b, 30, nullptr, {}, tol, 100);
    CHECK(text.reason == 0 && got.reason == 0 && got.iterations >= 1 && got.iterations <= 7 && got.rhs_sq == text.rhs_sq);
    for (size_t i = 0; i < 6; ++i) CHECK(std::fabs((double)got.x[i] - (double)text.x[i]) <= 100 * tol * 8);
    // by columns: the transpose's arrays
    const std::vector<T> valt{2, -1, -0.5, 2, -1, -0.5, 2, -1, -0.5, 2, -1, -0.5, 2, -1, -0.5, 2};
    const CscMatrix<T> Ac(6, 6, ptr, ind, valt);
    const Solution<T> gotc = Ac.gmres(b, 30, nullptr, {}, tol, 100);
    CHECK(gotc.reason == 0);
    for (size_t i = 0; i < 6; ++i) CHECK(std::fabs((double)gotc.x[i] - (double)text.x[i]) <= 100 * tol * 8);
    // ILU(0) of a tridiagonal matrix is its LU: M = A and one iteration
    const CsrMatrix<T> F = A.ilu0();
    const Solution<T> pre = A.gmres(b, 30, &F, {}, sizeof(T) == 8 ? 1e-10 : 1e-5, 100);
    CHECK(pre.reason == 0 && pre.iterations == 1);
    for (size_t i = 0; i < 6; ++i) CHECK(std::fabs((double)pre.x[i] - (double)text.x[i]) <= 1e-4);
    // restarts, maxit in the middle of a cycle, maxit = 0
    const Solution<T> two = A.gmres(b, 2, nullptr, {}, 0.0, 5);
    CHECK(two.reason == 1 && two.iterations == 5);
    const std::vector<T> x0{1, 1, 1, 1, 1, 1};
    const Solution<T> none = A.gmres(b, 30, nullptr, x0, tol, 0);
    CHECK(none.reason == 1 && none.iterations == 0 && none.x == x0);
    // the cyclic shift: BiCGStab breaks down, GMRES(8) takes 8 steps and is exact
    const std::vector<usize> sptr{0, 1, 2, 3, 4, 5, 6, 7, 8}, sind{7, 0, 1, 2, 3, 4, 5, 6};
    const CsrMatrix<T> S(8, 8, sptr, sind, std::vector<T>(8, T(1)));
    std::vector<T> e0(8, T(0)), want(8, T(0));
    e0[0] = 1;
    want[7] = 1;
    CHECK(S.solve(e0, Method::BiCgStab, nullptr, {}, 1e-6, 200).reason == 2);
    for (usize restart : {usize(8), usize(30)}) {
        const Solution<T> c = S.gmres(e0, restart, nullptr, {}, 1e-6, 200);
        CHECK(c.reason == 0 && c.iterations == 8 && c.x == want && c.residual_sq == 0.0);
    }
    const Solution<T> c4 = S.gmres(e0, 4, nullptr, {}, 1e-6, 40);
    const Solution<T> t4 = gmres_text<T>(shift_mul<T>(), e0, std::vector<T>(8, T(0)), 4, 1e-6, 40);
    CHECK(c4.reason == 1 && c4.iterations == 40 && c4.x == t4.x && c4.residual_sq == t4.residual_sq);
    CHECK(panic_text([&] { (void)A.gmres(b, 30, nullptr, {}, -1.0); }).find("must be >= 0") != std::string::npos);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    try {
        host_tests();
        if (gpu) {
            gpu_tests<double>();
            gpu_tests<float>();
        }
    } catch (const std::exception &e) {
        printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("gmres mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
