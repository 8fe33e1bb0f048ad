// C++ host-mirror test of GMRES on a block of right-hand sides (include/spalinalg.hpp: gmres_block).
//   ./test_gmres_block_mirror host   -- no GPU needed: gmres_block is there for both formats and types and panics on
//                                       wrong shapes and restarts before any device call
//   ./test_gmres_block_mirror gpu    -- a tridiagonal matrix that is not symmetric with four right-hand sides: every
//                                       column is gmres()'s result for it, bit for bit, among them a zero column
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
    BlockSolution<double> (CsrMatrix<double>::*a)(const std::vector<double> &, usize, usize, const CsrMatrix<double> *,
                                                  const std::vector<double> &, double, usize) const =
        &CsrMatrix<double>::gmres_block;
    BlockSolution<float> (CscMatrix<float>::*b)(const std::vector<float> &, usize, usize, const CscMatrix<float> *,
                                                const std::vector<float> &, double, usize) const =
        &CscMatrix<float>::gmres_block;
    CHECK(a && b);
    const CsrMatrix<double> R(2, 3, {0, 1, 2}, {0, 2}, {1, 2});
    CHECK(panic_text([&] { (void)R.gmres_block({1, 2, 3, 4}, 2); }).find("gmres_block: the matrix is not square (2 x 3)") !=
          std::string::npos);
    const CscMatrix<float> S(2, 2, {0, 1, 2}, {0, 1}, {1, 2});
    CHECK(panic_text([&] { (void)S.gmres_block({1, 2, 3, 4}, 0); }).find("k = 0") != std::string::npos);
    CHECK(panic_text([&] { (void)S.gmres_block({1, 2, 3}, 2); }).find("B.len() = 3 is not 2 rows of k = 2") != std::string::npos);
    CHECK(panic_text([&] { (void)S.gmres_block({1, 2, 3, 4}, 2, 30, nullptr, {1, 2}); }).find("X0.len() = 2") != std::string::npos);
    CHECK(panic_text([&] { (void)S.gmres_block({1, 2, 3, 4}, 2, 0); }).find("restart = 0 must be 1 .. 256") != std::string::npos);
    CHECK(panic_text([&] { (void)S.gmres_block({1, 2, 3, 4}, 2, 257); }).find("restart = 257 must be 1 .. 256") != std::string::npos);
}

template <typename T>
static CsrMatrix<T> tridiagonal(const CsrMatrix<T> *) {   // rows (-1, 3, -2)
    return CsrMatrix<T>(6, 6, {0, 2, 5, 8, 11, 14, 16}, {0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5},
                        {3, -2, -1, 3, -2, -1, 3, -2, -1, 3, -2, -1, 3, -2, -1, 3});
}
template <typename T>
static CscMatrix<T> tridiagonal(const CscMatrix<T> *) {   // the same matrix by columns: (-2, 3, -1) down a column
    return CscMatrix<T>(6, 6, {0, 2, 5, 8, 11, 14, 16}, {0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5},
                        {3, -1, -2, 3, -1, -2, 3, -1, -2, 3, -1, -2, 3, -1, -2, 3});
}

template <typename T, template <typename> class M>
static void gpu_tridiagonal() {
    const double tol = sizeof(T) == 8 ? 1e-12 : 1e-5;
    const M<T> A = tridiagonal<T>(static_cast<const M<T> *>(nullptr));
    const usize k = 4;
    // columns: (0 .. 0 7), zeros, A * (1 1 1 1 1 1) = (1 0 0 0 0 2), (1 2 3 4 5 6)
    const std::vector<std::vector<T>> cols{{0, 0, 0, 0, 0, 7}, {0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 2}, {1, 2, 3, 4, 5, 6}};
    std::vector<T> B(6 * k);
    for (usize i = 0; i < 6; ++i)
        for (usize j = 0; j < k; ++j) B[i * k + j] = cols[j][i];
    const M<T> F = A.ilu0();
    for (usize restart : {usize(2), usize(30)}) {
        for (const M<T> *pre : {static_cast<const M<T> *>(nullptr), &F}) {
            const BlockSolution<T> s = A.gmres_block(B, k, restart, pre, {}, tol, 100);
            CHECK(s.x.size() == 6 * k && s.columns.size() == k);
            for (usize j = 0; j < k; ++j) {
                const Solution<T> one = A.gmres(cols[j], restart, pre, {}, tol, 100);
                bool same = true;
                for (usize i = 0; i < 6; ++i) same = same && std::memcmp(&s.x[i * k + j], &one.x[i], sizeof(T)) == 0;
                CHECK(same);
                CHECK(s.columns[j].iterations == one.iterations && s.columns[j].reason == one.reason);
                CHECK(s.columns[j].residual_sq == one.residual_sq && s.columns[j].rhs_sq == one.rhs_sq);
                CHECK(s.columns[j].solve_ms == s.columns[0].solve_ms);
            }
            CHECK(s.columns[1].iterations == 0 && s.columns[1].reason == 0);     // the zero column stops at once
            CHECK(s.columns[0].reason == 0 && s.columns[0].iterations >= 1);
            if (pre) CHECK(s.columns[3].iterations == 1);                        // M = A exactly: a tridiagonal matrix has no fill
        }
    }
    // maxit = 0 from a start: nothing moves; r0 of column 0 = b - A x0 = (-1, 0, 0, 0, 0, 5)
    std::vector<T> X0(6 * k, T(1));
    const BlockSolution<T> none = A.gmres_block(B, k, 5, nullptr, X0, tol, 0);
    CHECK(none.x == X0 && none.columns[0].reason == 1 && none.columns[0].iterations == 0);
    CHECK(none.columns[0].residual_sq == 26.0 && none.columns[0].rhs_sq == 49.0);
    CHECK(panic_text([&] { (void)A.gmres_block(B, k, 5, nullptr, {}, -1.0); }).find("must be >= 0") != std::string::npos);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    try {
        host_tests();
        if (gpu) {
            gpu_tridiagonal<double, CsrMatrix>();
            gpu_tridiagonal<float, CsrMatrix>();
            gpu_tridiagonal<double, CscMatrix>();
            gpu_tridiagonal<float, CscMatrix>();
        }
    } catch (const std::exception &e) {
        printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("gmres block mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
