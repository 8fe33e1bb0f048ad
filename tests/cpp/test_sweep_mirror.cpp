// C++ host-mirror test of the Jacobi sweeps on a triangle (include/spalinalg.hpp: solve_triangular_sweeps).
//   ./test_sweep_mirror host   -- no GPU needed: a shape mismatch panics before any device call
//   ./test_sweep_mirror gpu    -- the hand example of include/spal.h's definition, both formats and types
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
    CHECK(panic_text([&] { (void)a.solve_triangular_sweeps({1.0, 2.0}, true, false, 2); }) ==
          "solve_triangular_sweeps: the matrix is not square (2 x 3)");
    const CsrMatrix<double> b(2, 2, {0, 1, 2}, {0, 1}, {1.0, 2.0});
    CHECK(panic_text([&] { (void)b.solve_triangular_sweeps({1.0, 2.0, 3.0}, true, false, 2); }) ==
          "solve_triangular_sweeps: b.len() = 3 but the matrix has 2 rows");
    const CscMatrix<float> c(3, 2, {0, 1, 2}, {0, 2}, {1.0f, 2.0f});
    CHECK(panic_text([&] { (void)c.solve_triangular_sweeps({1.0f, 2.0f, 3.0f}, false, false, 0); }) ==
          "solve_triangular_sweeps: the matrix is not square (3 x 2)");
}

template <typename T>
static void gpu_hand_example() {
    // L = [[2,0,0,0],[1,1,0,0],[0,3,4,0],[1,0,2,2]], b = [2,3,10,9].  x0 = b / d = [1, 3, 2.5, 4.5];
    // x1 = [1, (3 - 1) / 1, (10 - 9) / 4, (9 - 1 - 5) / 2] = [1, 2, 0.25, 1.5];  x2 = [1, 2, (10 - 6) / 4, (9 - 1 - 0.5) / 2]
    // = [1, 2, 1, 3.75];  x3 = [1, 2, 1, 3], the substitution's result (4 levels).
    const std::vector<usize> ptr{0, 1, 3, 5, 8}, l_ind{0, 0, 1, 1, 2, 0, 2, 3};
    const std::vector<T> l_val{2, 1, 1, 3, 4, 1, 2, 2};
    const std::vector<usize> u_ptr{0, 3, 5, 7, 8}, u_ind{0, 1, 3, 1, 2, 2, 3, 3};
    const std::vector<T> u_val{2, 1, 1, 1, 3, 4, 2, 2};
    const std::vector<T> bl{2, 3, 10, 9};
    const std::vector<std::vector<T>> xs{{1, 3, 2.5, 4.5}, {1, 2, 0.25, 1.5}, {1, 2, 1, 3.75}, {1, 2, 1, 3}};
    const CsrMatrix<T> L(4, 4, ptr, l_ind, l_val);
    const CscMatrix<T> Lc(4, 4, u_ptr, u_ind, u_val);   // the CSC arrays of L are the CSR arrays of its transpose
    for (std::uint64_t s = 0; s < 4; ++s) {
        CHECK(L.solve_triangular_sweeps(bl, true, false, s) == xs[s]);
        CHECK(Lc.solve_triangular_sweeps(bl, true, false, s) == xs[s]);
    }
    CHECK(L.solve_triangular_sweeps(bl, true, false, 1000000000) == L.solve_triangular(bl));   // clamped to n - 1
    // unit diagonal: x0 = b, x1 = [2, 3 - 2, 10 - 9, 9 - 2 - 20] = [2, 1, 1, -13]
    CHECK((L.solve_triangular_sweeps(bl, true, true, 1) == std::vector<T>{2, 1, 1, -13}));
    CHECK((Lc.solve_triangular_sweeps(bl, true, true, 1) == std::vector<T>{2, 1, 1, -13}));
    CHECK((L.solve_triangular_sweeps(bl, false, false, 3) == xs[0]));   // its upper triangle is its diagonal
    // a row without a diagonal: refused unless the diagonal is taken as ones
    const CsrMatrix<T> M(2, 2, {0, 1, 2}, {0, 0}, {2, 1});
    CHECK(panic_text([&] { (void)M.solve_triangular_sweeps({2, 3}, true, false, 1); }).find("row 1 stores no diagonal entry") !=
          std::string::npos);
    CHECK((M.solve_triangular_sweeps({2, 3}, true, true, 1) == std::vector<T>{2, 1}));
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
    printf("sweep mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
