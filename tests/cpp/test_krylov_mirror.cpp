// C++ host-mirror test of the Krylov solvers and their dot product (include/spalinalg.hpp: solve, dot).
//   ./test_krylov_mirror host   -- no GPU needed: dot() against the definition written out here; solve() is there for
//                                  both formats and types and panics on wrong shapes before any device call
//   ./test_krylov_mirror gpu    -- tridiag(-1, 2, -1): CG, BiCGStab with its ILU(0) factor (the half-step exit), maxit
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

template <typename T>
static void host_dot() {
    for (size_t n : {size_t(0), size_t(1), size_t(1023), size_t(1024), size_t(1025), size_t(3 * 1024 * 1024 + 5)}) {
        std::vector<T> a(n), b(n), p(n);
        unsigned long long s = 88172645463325252ull + n;
        for (size_t i = 0; i < n; ++i) {   // xorshift: mixed magnitudes
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            a[i] = T((double)(s % 2000001) / 1e6 - 1.0) * T(std::pow(10.0, (double)((s >> 40) % 13) - 6.0));
            b[i] = T((double)((s >> 20) % 2000001) / 1e6 - 1.0);
            p[i] = a[i] * b[i];
        }
        const T got = dot(a, b), want = reduce(p);
        CHECK(std::memcmp(&got, &want, sizeof(T)) == 0);
    }
    const T z = dot(std::vector<T>{T(-0.0)}, std::vector<T>{T(1)});
    CHECK(z == T(0) && !std::signbit(z));
    CHECK(std::isnan(dot(std::vector<T>{T(1), T(NAN)}, std::vector<T>{T(1), T(1)})));
    CHECK(panic_text([] { (void)dot(std::vector<T>{1, 2}, std::vector<T>{1}); }).find("b.len() = 1") != std::string::npos);
}

static void host_tests() {
    host_dot<double>();
    host_dot<float>();
    Solution<double> (CsrMatrix<double>::*a)(const std::vector<double> &, Method, const CsrMatrix<double> *,
                                             const std::vector<double> &, double, usize) const = &CsrMatrix<double>::solve;
    Solution<float> (CscMatrix<float>::*b)(const std::vector<float> &, Method, const CscMatrix<float> *,
                                           const std::vector<float> &, double, usize) const = &CscMatrix<float>::solve;
    CHECK(a && b);
    const CsrMatrix<double> R(2, 3, {0, 1, 2}, {0, 2}, {1, 2});
    CHECK(panic_text([&] { (void)R.solve({1, 2}); }).find("not square (2 x 3)") != std::string::npos);
    const CscMatrix<float> S(2, 2, {0, 1, 2}, {0, 1}, {1, 2});
    CHECK(panic_text([&] { (void)S.solve({1, 2, 3}); }).find("b.len() = 3") != std::string::npos);
    CHECK(panic_text([&] { (void)S.solve({1, 2}, Method::Cg, nullptr, {1}); }).find("x0.len() = 1") != std::string::npos);
}

template <typename T>
static void gpu_tridiagonal() {
    const std::vector<usize> ptr{0, 2, 5, 8, 11, 14, 16}, ind{0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5};
    const std::vector<T> val{2, -1, -1, 2, -1, -1, 2, -1, -1, 2, -1, -1, 2, -1, -1, 2};
    const std::vector<T> b{0, 0, 0, 0, 0, 7}, want{1, 2, 3, 4, 5, 6};
    const double tol = sizeof(T) == 8 ? 1e-12 : 1e-5;
    const CsrMatrix<T> A(6, 6, ptr, ind, val);
    const CscMatrix<T> Ac(6, 6, ptr, ind, val);   // symmetric: the same arrays by columns
    auto close = [&](const std::vector<T> &x) {
        for (size_t i = 0; i < 6; ++i)
            if (std::fabs((double)x[i] - (double)want[i]) > 100 * tol * 6) return false;
        return true;
    };
    const Solution<T> cg = A.solve(b, Method::Cg, nullptr, {}, tol, 100);
    CHECK(cg.reason == 0 && cg.iterations >= 1 && cg.iterations <= 6 && close(cg.x) && cg.rhs_sq == 49.0);
    const Solution<T> cgc = Ac.solve(b, Method::Cg, nullptr, {}, tol, 100);
    CHECK(cgc.reason == 0 && cgc.iterations == cg.iterations && cgc.x == cg.x && cgc.residual_sq == cg.residual_sq);
    const CsrMatrix<T> F = A.ilu0();
    const Solution<T> bi = A.solve(b, Method::BiCgStab, &F, {}, tol, 100);
    CHECK(bi.reason == 0 && bi.iterations == 1 && close(bi.x));          // M = A exactly: the half-step exit
    const CscMatrix<T> Fc = Ac.ilu0();
    const Solution<T> bic = Ac.solve(b, Method::BiCgStab, &Fc, {}, tol, 100);
    CHECK(bic.reason == 0 && bic.iterations == 1 && bic.x == bi.x);
    const std::vector<T> x0{1, 1, 1, 1, 1, 1};
    const Solution<T> none = A.solve(b, Method::BiCgStab, nullptr, x0, tol, 0);
    CHECK(none.reason == 1 && none.iterations == 0 && none.x == x0);
    // r0 = b - A x0 = (-1, 0, 0, 0, 0, 6)
    CHECK(none.residual_sq == 37.0);
    const Solution<T> two = A.solve(b, Method::Cg, nullptr, {}, tol, 2);
    CHECK(two.reason == 1 && two.iterations == 2);
    CHECK(panic_text([&] { (void)A.solve(b, static_cast<Method>(7)); }).find("method = 7") != std::string::npos);
    CHECK(panic_text([&] { (void)A.solve(b, Method::Cg, nullptr, {}, -1.0); }).find("must be >= 0") != std::string::npos);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    try {
        host_tests();
        if (gpu) {
            gpu_tridiagonal<double>();
            gpu_tridiagonal<float>();
        }
    } catch (const std::exception &e) {
        printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("krylov mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
