// C++ host-mirror test of the triangular solve (include/spalinalg.hpp: CsrMatrix / CscMatrix::solve_triangular).
//   ./test_trsv_mirror host   -- no GPU needed: a shape mismatch panics before any device call
//   ./test_trsv_mirror gpu    -- the hand example of include/spal.h's definition, both formats, types and triangles
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
    CHECK(panic_text([&] { (void)a.solve_triangular({1.0, 2.0}); }) == "solve_triangular: the matrix is not square (2 x 3)");
    const CsrMatrix<double> b(2, 2, {0, 1, 2}, {0, 1}, {1.0, 2.0});
    CHECK(panic_text([&] { (void)b.solve_triangular({1.0, 2.0, 3.0}); }) ==
          "solve_triangular: b.len() = 3 but the matrix has 2 rows");
    const CscMatrix<float> c(3, 2, {0, 1, 2}, {0, 2}, {1.0f, 2.0f});
    CHECK(panic_text([&] { (void)c.solve_triangular({1.0f, 2.0f, 3.0f}, false); }) ==
          "solve_triangular: the matrix is not square (3 x 2)");
}

template <typename T>
static void gpu_hand_example() {
    // L = [[2,0,0,0],[1,1,0,0],[0,3,4,0],[1,0,2,2]] and U = its transpose; both solves give x = [1,2,1,3]
    const std::vector<usize> ptr{0, 1, 3, 5, 8}, l_ind{0, 0, 1, 1, 2, 0, 2, 3};
    const std::vector<T> l_val{2, 1, 1, 3, 4, 1, 2, 2};
    const std::vector<usize> u_ptr{0, 3, 5, 7, 8}, u_ind{0, 1, 3, 1, 2, 2, 3, 3};
    const std::vector<T> u_val{2, 1, 1, 1, 3, 4, 2, 2};
    const std::vector<T> bl{2, 3, 10, 9}, bu{7, 5, 10, 6}, x{1, 2, 1, 3};
    const CsrMatrix<T> L(4, 4, ptr, l_ind, l_val), U(4, 4, u_ptr, u_ind, u_val);
    CHECK(L.solve_triangular(bl) == x);
    CHECK(U.solve_triangular(bu, false) == x);
    CHECK((L.solve_triangular(bl, true, true) == std::vector<T>{2, 1, 7, -7}));
    CHECK((U.solve_triangular(bu, false, true) == std::vector<T>{-10, 11, -2, 6}));
    CHECK((L.solve_triangular(bl, false) == std::vector<T>{1, 3, 2.5, 4.5}));   // its upper triangle is its diagonal
    // the CSC arrays of L are the CSR arrays of U, and the reverse
    const CscMatrix<T> Lc(4, 4, u_ptr, u_ind, u_val), Uc(4, 4, ptr, l_ind, l_val);
    CHECK(Lc.solve_triangular(bl) == x);
    CHECK(Uc.solve_triangular(bu, false) == x);
    CHECK((Lc.solve_triangular(bl, true, true) == std::vector<T>{2, 1, 7, -7}));
    // a row without a diagonal: refused unless the diagonal is taken as ones
    const CsrMatrix<T> M(2, 2, {0, 1, 2}, {0, 0}, {2, 1});
    CHECK(panic_text([&] { (void)M.solve_triangular({2, 3}); }).find("row 1 stores no diagonal entry") != std::string::npos);
    CHECK((M.solve_triangular({2, 3}, true, true) == std::vector<T>{2, 1}));
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
    printf("trsv mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
