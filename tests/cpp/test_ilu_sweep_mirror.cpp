// C++ host-mirror test of ILU(0) by row sweeps (include/spalinalg.hpp: CsrMatrix / CscMatrix::ilu0(sweeps)).
//   ./test_ilu_sweep_mirror host   -- no GPU needed: the overload is there for both formats and types beside ilu0(), and
//                                     a matrix that is not square panics before any device call
//   ./test_ilu_sweep_mirror gpu    -- the hand example of include/spal.h's definition, pass by pass, CSR and CSC
#include <cstdint>
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
    CsrMatrix<double> (CsrMatrix<double>::*a)(std::uint64_t) const = &CsrMatrix<double>::ilu0;
    CsrMatrix<float> (CsrMatrix<float>::*b)(std::uint64_t) const = &CsrMatrix<float>::ilu0;
    CscMatrix<double> (CscMatrix<double>::*c)(std::uint64_t) const = &CscMatrix<double>::ilu0;
    CscMatrix<float> (CscMatrix<float>::*d)(std::uint64_t) const = &CscMatrix<float>::ilu0;
    CsrMatrix<double> (CsrMatrix<double>::*e)() const = &CsrMatrix<double>::ilu0;   // the exact call keeps its signature
    CHECK(a && b && c && d && e);
    const CsrMatrix<double> R(2, 3, {0, 1, 2}, {0, 2}, {1.0, 2.0});
    CHECK(panic_text([&] { (void)R.ilu0(2); }) == "ilu0: the matrix is not square (2 x 3)");
    CHECK(panic_text([&] { (void)R.ilu0(0); }) == "ilu0: the matrix is not square (2 x 3)");
    const CscMatrix<float> C(3, 2, {0, 1, 2}, {0, 2}, {1.0f, 2.0f});
    CHECK(panic_text([&] { (void)C.ilu0(1); }) == "ilu0: the matrix is not square (3 x 2)");
}

template <typename T>
static void gpu_hand_example() {
    // A = [[2,1,0,0],[4,1,3,0],[0,3,-4,-2],[0,0,20,-5]], four levels.  Pass 1 reads A's rows: row 1 = [4/2, 1 - 2*1, 3],
    // row 2 = [3/1, -4 - 3*3, -2], row 3 = [20/-4, -5 - (-5)(-2)].  Pass 2 reads pass 1's: row 2 = [3/-1, -4 - (-3)*3, -2],
    // row 3 = [20/-13, -5 - (20/-13)(-2)].  Pass 3 is the factor L\U = [[2,1,.,.],[2,-1,3,.],[.,-3,5,-2],[.,.,4,3]].
    const std::vector<usize> ptr{0, 2, 5, 8, 10}, ind{0, 1, 0, 1, 2, 1, 2, 3, 2, 3};
    const std::vector<T> val{2, 1, 4, 1, 3, 3, -4, -2, 20, -5}, factor{2, 1, 2, -1, 3, -3, 5, -2, 4, 3};
    const T w = T(20) / T(-13);
    const std::vector<std::vector<T>> passes{val,
                                             {2, 1, 2, -1, 3, 3, -13, -2, -5, -15},
                                             {2, 1, 2, -1, 3, -3, 5, -2, w, T(-5) - w * T(-2)},
                                             factor};
    const CsrMatrix<T> A(4, 4, ptr, ind, val);
    for (std::uint64_t s = 0; s < 4; ++s) {
        const CsrMatrix<T> F = A.ilu0(s);
        CHECK(F.rowptr() == ptr && F.colind() == ind && F.values() == passes[s]);
    }
    CHECK(A.ilu0(3).values() == A.ilu0().values());
    CHECK(A.ilu0(2).values() != factor);
    CHECK(A.ilu0(1000000000000ull).values() == factor);   // clamped to n - 1
    CHECK(A.values() == val);
    // the swept factor applied by sweeps: b = A [1, 2, 1, 3]; three sweeps per triangle are the two solves here
    const std::vector<T> b{4, 9, -4, 5}, x{1, 2, 1, 3};
    const CsrMatrix<T> F = A.ilu0(3);
    const std::vector<T> y = F.solve_triangular_sweeps(b, true, true, 3);
    CHECK((y == std::vector<T>{4, 1, -1, 9}));
    CHECK(F.solve_triangular_sweeps(y, false, false, 3) == x);
    // the same matrix by columns
    const std::vector<usize> cptr{0, 2, 5, 8, 10}, cind{0, 1, 0, 1, 2, 1, 2, 3, 2, 3};
    const std::vector<T> cval{2, 4, 1, 1, 3, 3, -4, 20, -2, -5}, cfactor{2, 2, 1, -1, -3, 3, 5, 4, -2, 3};
    const std::vector<T> cpass1{2, 2, 1, -1, 3, 3, -13, -5, -2, -15};
    const CscMatrix<T> Ac(4, 4, cptr, cind, cval);
    CHECK(Ac.ilu0(0).values() == cval);
    const CscMatrix<T> F1 = Ac.ilu0(1);
    CHECK(F1.colptr() == cptr && F1.rowind() == cind && F1.values() == cpass1);
    CHECK(Ac.ilu0(3).values() == cfactor && Ac.ilu0(2).values() != cfactor);
    // refusals: a row without a diagonal, named
    const CsrMatrix<T> M(2, 2, {0, 1, 2}, {0, 0}, {2, 1});
    CHECK(panic_text([&] { (void)M.ilu0(2); }).find("row 1 stores no diagonal entry") != std::string::npos);
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
    printf("ilu sweep mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
