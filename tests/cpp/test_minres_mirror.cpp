// C++ host-mirror test of MINRES (include/spalinalg.hpp: minres, minres_block) against the C ABI.
//   ./test_minres_mirror host   -- no GPU needed: the methods are there for both formats and types and panic on wrong
//                                  shapes and shifts before any device call
//   ./test_minres_mirror gpu    -- tridiag(-1, +-3, -1), symmetric and indefinite: the mirror returns what the C entry
//                                  points return, for a shift, a Jacobi preconditioner, maxit and a block
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

static void host_tests() {
    Solution<double> (CsrMatrix<double>::*a)(const std::vector<double> &, const CsrMatrix<double> *, double,
                                             const std::vector<double> &, double, usize) const = &CsrMatrix<double>::minres;
    BlockSolution<float> (CscMatrix<float>::*b)(const std::vector<float> &, usize, const CscMatrix<float> *, double,
                                                const std::vector<float> &, double, usize) const = &CscMatrix<float>::minres_block;
    CHECK(a && b);
    const CsrMatrix<double> R(2, 3, {0, 1, 2}, {0, 2}, {1, 2});
    CHECK(panic_text([&] { (void)R.minres({1, 2}); }).find("not square (2 x 3)") != std::string::npos);
    const CscMatrix<float> S(2, 2, {0, 1, 2}, {0, 1}, {1, -2});
    CHECK(panic_text([&] { (void)S.minres({1, 2, 3}); }).find("b.len() = 3") != std::string::npos);
    CHECK(panic_text([&] { (void)S.minres({1, 2}, nullptr, 0.0, {1}); }).find("x0.len() = 1") != std::string::npos);
    CHECK(panic_text([&] { (void)S.minres({1, 2}, nullptr, NAN); }).find("shift must be finite") != std::string::npos);
    CHECK(panic_text([&] { (void)S.minres_block({1, 2, 3, 4}, 2, nullptr, INFINITY); }).find("shift must be finite") != std::string::npos);
    CHECK(panic_text([&] { (void)S.minres_block({1, 2, 3, 4}, 2, nullptr, 0.0, {1}); }).find("X0.len() = 1") != std::string::npos);
    CHECK(!panic_text([&] { (void)S.minres_block({1, 2, 3}, 2); }).empty());
}

template <typename T> struct Entry;
template <> struct Entry<double> { static constexpr auto csr = spal_csr_minres_f64; };
template <> struct Entry<float> { static constexpr auto csr = spal_csr_minres_f32; };

template <typename T>
static void gpu_tridiagonal() {
    const std::vector<usize> ptr{0, 2, 5, 8, 11, 14, 16}, ind{0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5};
    const std::vector<T> val{3, -1, -1, -3, -1, -1, 3, -1, -1, -3, -1, -1, 3, -1, -1, -3};
    const std::vector<T> want{1, 2, 3, 4, 5, 6};
    const std::vector<T> b{1, -10, 3, -20, 5, -23};   // A want
    const double tol = sizeof(T) == 8 ? 1e-12 : 1e-5;
    const CsrMatrix<T> A(6, 6, ptr, ind, val);
    const CscMatrix<T> Ac(6, 6, ptr, ind, val);   // symmetric: the same arrays by columns
    auto close = [&](const std::vector<T> &x, const std::vector<T> &to) {
        for (size_t i = 0; i < 6; ++i)
            if (std::fabs((double)x[i] - (double)to[i]) > 100 * tol * 6) return false;
        return true;
    };
    const Solution<T> s = A.minres(b, nullptr, 0.0, {}, tol, 100);
    CHECK(s.reason == 0 && s.iterations >= 1 && s.iterations <= 6 && close(s.x, want));
    CHECK(s.rhs_sq == 1064.0);
    // the C entry point itself, on the mirror's own handle
    std::vector<T> x(6, T(0));
    spal_krylov_info info;
    CHECK(Entry<T>::csr(A.device_handle(), nullptr, 0.0, b.data(), 6, x.data(), 6, tol, 100, &info) == SPAL_OK);
    CHECK(x == s.x && info.iterations == s.iterations && info.reason == s.reason && info.residual_sq == s.residual_sq &&
          info.rhs_sq == s.rhs_sq);
    const Solution<T> sc = Ac.minres(b, nullptr, 0.0, {}, tol, 100);
    CHECK(sc.reason == 0 && sc.iterations == s.iterations && sc.x == s.x && sc.residual_sq == s.residual_sq);
    // (A - 0.5 I) want = b - 0.5 want
    std::vector<T> bs(6);
    for (size_t i = 0; i < 6; ++i) bs[i] = b[i] - T(0.5) * want[i];
    const Solution<T> sh = A.minres(bs, nullptr, 0.5, {}, tol, 100);
    CHECK(sh.reason == 0 && close(sh.x, want));
    CHECK(Entry<T>::csr(A.device_handle(), nullptr, 0.5, bs.data(), 6, (x.assign(6, T(0)), x.data()), 6, tol, 100, &info) == SPAL_OK);
    CHECK(x == sh.x && info.iterations == sh.iterations);
    // the exact start, maxit
    const Solution<T> start = A.minres(b, nullptr, 0.0, want, tol, 100);
    CHECK(start.reason == 0 && start.iterations == 0 && start.x == want && start.residual_sq == 0.0);
    const Solution<T> two = A.minres(b, nullptr, 0.0, {}, 0.0, 2);
    CHECK(two.reason == 1 && two.iterations == 2 && two.residual_sq < s.rhs_sq);
    // a block: columns b, 0, 2 b
    std::vector<T> B(18);
    for (size_t i = 0; i < 6; ++i) {
        B[3 * i] = b[i];
        B[3 * i + 1] = T(0);
        B[3 * i + 2] = 2 * b[i];
    }
    const BlockSolution<T> blk = A.minres_block(B, 3, nullptr, 0.0, {}, tol, 100);
    const BlockSolution<T> blkc = Ac.minres_block(B, 3, nullptr, 0.0, {}, tol, 100);
    CHECK(blk.columns.size() == 3 && blk.columns[1].iterations == 0 && blk.columns[1].reason == 0);
    CHECK(blk.columns[0].reason == 0 && blk.columns[2].reason == 0 && blkc.x == blk.x);
    for (size_t i = 0; i < 6; ++i) CHECK(std::fabs((double)blk.x[3 * i] - (double)want[i]) <= 100 * tol * 6 && blk.x[3 * i + 1] == T(0));
    CHECK(panic_text([&] { (void)A.minres(b, nullptr, 0.0, {}, -1.0); }).find("must be >= 0") != std::string::npos);
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
    printf("minres mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
