// C++ host-mirror test of the block triangular solves (include/spalinalg.hpp: solve_triangular_block,
// solve_triangular_block_sweeps).
//   ./test_trsm_mirror host   -- no GPU needed: a bad shape panics before any device call
//   ./test_trsm_mirror gpu    -- the hand example of include/spal.h's definitions, column by column, both formats and types
#include <cstdio>
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
    const CsrMatrix<double> a(2, 3, {0, 1, 2}, {0, 2}, {1.0, 2.0});
    CHECK(panic_text([&] { (void)a.solve_triangular_block({1.0, 2.0}, 1); }) ==
          "solve_triangular_block: the matrix is not square (2 x 3)");
    CHECK(panic_text([&] { (void)a.solve_triangular_block_sweeps({1.0, 2.0}, 1, true, false, 2); }) ==
          "solve_triangular_block_sweeps: the matrix is not square (2 x 3)");
    const CsrMatrix<double> b(2, 2, {0, 1, 2}, {0, 1}, {1.0, 2.0});
    CHECK(panic_text([&] { (void)b.solve_triangular_block({1.0, 2.0, 3.0, 4.0}, 0); }) ==
          "solve_triangular_block: k = 0 (B and X need at least one column)");
    CHECK(panic_text([&] { (void)b.solve_triangular_block({1.0, 2.0, 3.0}, 2); }) ==
          "solve_triangular_block: B.len() = 3 is not 2 rows of k = 2");
    CHECK(panic_text([&] { (void)b.solve_triangular_block_sweeps({1.0, 2.0, 3.0, 4.0, 5.0, 6.0}, 2, true, false, 1); }) ==
          "solve_triangular_block_sweeps: B.len() = 6 is not 2 rows of k = 2");
    const CscMatrix<float> c(3, 2, {0, 1, 2}, {0, 2}, {1.0f, 2.0f});
    CHECK(panic_text([&] { (void)c.solve_triangular_block({1.0f, 2.0f, 3.0f}, 1, false); }) ==
          "solve_triangular_block: the matrix is not square (3 x 2)");
    const CscMatrix<float> d(2, 2, {0, 1, 2}, {0, 1}, {1.0f, 2.0f});
    CHECK(panic_text([&] { (void)d.solve_triangular_block_sweeps({1.0f, 2.0f, 3.0f}, 2, true, false, 0); }) ==
          "solve_triangular_block_sweeps: B.len() = 3 is not 2 rows of k = 2");
}

template <typename T>
static std::vector<T> column(const std::vector<T> &X, usize k, usize j) {
    std::vector<T> c;
    for (usize i = 0; i * k + j < X.size(); ++i) c.push_back(X[i * k + j]);
    return c;
}

template <typename T>
static void gpu_hand_example() {
    // L = [[2,0,0,0],[1,1,0,0],[0,3,4,0],[1,0,2,2]]; the columns of B are b = [2,3,10,9], 2 b and [0,0,0,2].
    const std::vector<usize> ptr{0, 1, 3, 5, 8}, l_ind{0, 0, 1, 1, 2, 0, 2, 3};
    const std::vector<T> l_val{2, 1, 1, 3, 4, 1, 2, 2};
    const std::vector<usize> u_ptr{0, 3, 5, 7, 8}, u_ind{0, 1, 3, 1, 2, 2, 3, 3};
    const std::vector<T> u_val{2, 1, 1, 1, 3, 4, 2, 2};
    const std::vector<T> B{2, 4, 0, 3, 6, 0, 10, 20, 0, 9, 18, 2};
    const usize k = 3;
    const CsrMatrix<T> L(4, 4, ptr, l_ind, l_val);
    const CscMatrix<T> Lc(4, 4, u_ptr, u_ind, u_val);   // the CSC arrays of L are the CSR arrays of its transpose
    const std::vector<T> X = L.solve_triangular_block(B, k);
    CHECK((X == std::vector<T>{1, 2, 0, 2, 4, 0, 1, 2, 0, 3, 6, 1}));
    CHECK(Lc.solve_triangular_block(B, k) == X);
    for (usize j = 0; j < k; ++j) {
        const std::vector<T> bj = column(B, k, j);
        CHECK(column(X, k, j) == L.solve_triangular(bj));
        CHECK(column(L.solve_triangular_block(B, k, true, true), k, j) == L.solve_triangular(bj, true, true));
        for (std::uint64_t s = 0; s < 4; ++s) {
            CHECK(column(L.solve_triangular_block_sweeps(B, k, true, false, s), k, j) ==
                  L.solve_triangular_sweeps(bj, true, false, s));
            CHECK(column(Lc.solve_triangular_block_sweeps(B, k, true, false, s), k, j) ==
                  Lc.solve_triangular_sweeps(bj, true, false, s));
        }
    }
    CHECK(L.solve_triangular_block_sweeps(B, k, true, false, 1000000000) == X);   // clamped to n - 1
    // a row without a diagonal: refused unless the diagonal is taken as ones
    const CsrMatrix<T> M(2, 2, {0, 1, 2}, {0, 0}, {2, 1});
    CHECK(panic_text([&] { (void)M.solve_triangular_block({2, 3}, 1); }).find("row 1 stores no diagonal entry") !=
          std::string::npos);
    CHECK((M.solve_triangular_block({2, 3}, 1, true, true) == std::vector<T>{2, 1}));
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    try {
        host_tests();
        if (gpu) {
            gpu_hand_example<double>();
            gpu_hand_example<float>();
        }
    } catch (const std::exception &e) {
        printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("trsm mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
