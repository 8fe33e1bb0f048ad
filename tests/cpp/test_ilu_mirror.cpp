// C++ host-mirror test of ILU(0) (include/spalinalg.hpp: CsrMatrix / CscMatrix::ilu0).
//   ./test_ilu_mirror host   -- no GPU needed: the mirror compiles and the method is there for both formats and types
//   ./test_ilu_mirror gpu    -- the hand example of include/spal.h's definition and its two-solve application
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
    CsrMatrix<double> (CsrMatrix<double>::*a)() const = &CsrMatrix<double>::ilu0;
    CsrMatrix<float> (CsrMatrix<float>::*b)() const = &CsrMatrix<float>::ilu0;
    CscMatrix<double> (CscMatrix<double>::*c)() const = &CscMatrix<double>::ilu0;
    CscMatrix<float> (CscMatrix<float>::*d)() const = &CscMatrix<float>::ilu0;
    CHECK(a && b && c && d);
}

template <typename T>
static void gpu_hand_example() {
    // A = [[2,1,0,0],[4,1,3,0],[0,3,-4,-2],[0,0,20,-5]]  ->  L\U = [[2,1,.,.],[2,-1,3,.],[.,-3,5,-2],[.,.,4,3]]
    const std::vector<usize> ptr{0, 2, 5, 8, 10}, ind{0, 1, 0, 1, 2, 1, 2, 3, 2, 3};
    const std::vector<T> val{2, 1, 4, 1, 3, 3, -4, -2, 20, -5}, factor{2, 1, 2, -1, 3, -3, 5, -2, 4, 3};
    const std::vector<T> b{4, 9, -4, 5}, x{1, 2, 1, 3};   // b = A x
    const CsrMatrix<T> A(4, 4, ptr, ind, val);
    const CsrMatrix<T> F = A.ilu0();
    CHECK(F.rowptr() == ptr && F.colind() == ind && F.values() == factor);
    CHECK(A.values() == val);
    const std::vector<T> y = F.solve_triangular(b, true, true);
    CHECK((y == std::vector<T>{4, 1, -1, 9}));
    CHECK(F.solve_triangular(y, false) == x);
    // the same matrix by columns
    const std::vector<usize> cptr{0, 2, 5, 8, 10}, cind{0, 1, 0, 1, 2, 1, 2, 3, 2, 3};
    const std::vector<T> cval{2, 4, 1, 1, 3, 3, -4, 20, -2, -5}, cfactor{2, 2, 1, -1, -3, 3, 5, 4, -2, 3};
    const CscMatrix<T> Ac(4, 4, cptr, cind, cval);
    const CscMatrix<T> Fc = Ac.ilu0();
    CHECK(Fc.colptr() == cptr && Fc.rowind() == cind && Fc.values() == cfactor);
    CHECK(Fc.solve_triangular(Fc.solve_triangular(b, true, true), false) == x);
    // refusals: not square; a row without a diagonal, named
    const CsrMatrix<T> R(2, 3, {0, 1, 2}, {0, 2}, {1, 2});
    CHECK(panic_text([&] { (void)R.ilu0(); }).find("not square (2 x 3)") != std::string::npos);
    const CsrMatrix<T> M(2, 2, {0, 1, 2}, {0, 0}, {2, 1});
    CHECK(panic_text([&] { (void)M.ilu0(); }).find("row 1 stores no diagonal entry") != std::string::npos);
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
    printf("ilu mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
