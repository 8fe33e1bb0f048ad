// C++ host-mirror test of the multicolour ordering (include/spalinalg.hpp: colour_greedy, perm_from_colours and
// CsrMatrix / CscMatrix::colour, permute, multicolour, ordering, to_order, from_order).
//   ./test_colour_mirror host   -- no GPU needed: the host text on the hand example, the methods exist for both formats
//   ./test_colour_mirror gpu    -- the hand example of tests/colour_ref.py on the device
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

// edges 0-1, 0-2, 1-2, 2-3, 3-4; (1,0), (3,2) and (4,3) stored in one direction only; keys at seed 0 order the
// vertices 4, 2, 1, 3, 0
static const std::vector<usize> kPtr{0, 2, 4, 7, 9, 11}, kInd{0, 2, 0, 2, 0, 1, 2, 2, 3, 3, 4};
static const std::vector<usize> kColours{2, 1, 0, 1, 0}, kPerm{2, 4, 1, 3, 0};
// P A P^T with values 0 .. 10 in A's order
static const std::vector<usize> kPermPtr{0, 3, 5, 7, 9, 11}, kPermInd{0, 2, 4, 1, 3, 0, 4, 0, 3, 0, 4};

template <typename T>
static std::vector<T> values_of(const std::vector<int> &v) { return std::vector<T>(v.begin(), v.end()); }

static void host_tests() {
    const Colouring c = colour_greedy(5, kPtr, kInd, 0);
    CHECK(c.colours == kColours && c.ncolours == 3);
    CHECK(perm_from_colours(c.colours) == kPerm);
    CHECK(colour_greedy(5, kPtr, kInd, 7).ncolours == 3);   // a triangle needs three, whatever the order
    CHECK(panic_text([&] { (void)colour_greedy(5, kPtr, {0, 2, 0, 2, 0, 1, 2, 2, 3, 3, 5}, 0); }).find("stores column 5") !=
          std::string::npos);
    CHECK(panic_text([&] { (void)perm_from_colours({0, 9}); }).find("colour[1] = 9") != std::string::npos);
    Colouring (CsrMatrix<double>::*a)(usize) const = &CsrMatrix<double>::colour;
    CsrMatrix<float> (CsrMatrix<float>::*b)(const std::vector<usize> &) const = &CsrMatrix<float>::permute;
    CscMatrix<double> (CscMatrix<double>::*m)(usize) const = &CscMatrix<double>::multicolour;
    Ordering (CscMatrix<float>::*o)() const = &CscMatrix<float>::ordering;
    std::vector<double> (CsrMatrix<double>::*t)(const std::vector<double> &) const = &CsrMatrix<double>::to_order;
    std::vector<float> (CscMatrix<float>::*f)(const std::vector<float> &) const = &CscMatrix<float>::from_order;
    CHECK(a && b && m && o && t && f);
}

template <typename T>
static void gpu_hand_example() {
    const std::vector<T> val = values_of<T>({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10});
    const std::vector<T> pval = values_of<T>({6, 5, 4, 10, 9, 3, 2, 7, 8, 1, 0});
    const CsrMatrix<T> A(5, 5, kPtr, kInd, val);
    const Colouring c = A.colour();
    CHECK(c.colours == kColours && c.ncolours == 3 && c.rounds == 3);
    const CsrMatrix<T> B = A.permute(kPerm);
    CHECK(B.rowptr() == kPermPtr && B.colind() == kPermInd && B.values() == pval);
    CHECK(B.ordering().perm == kPerm && B.ordering().ncolours == 0);
    const CsrMatrix<T> M = A.multicolour();
    CHECK(M.rowptr() == kPermPtr && M.colind() == kPermInd && M.values() == pval);
    CHECK(M.ordering().perm == kPerm && M.ordering().ncolours == 3);
    const std::vector<T> v = values_of<T>({10, 11, 12, 13, 14});
    CHECK(M.to_order(v) == values_of<T>({12, 14, 11, 13, 10}));
    CHECK(M.from_order(M.to_order(v)) == v);
    // the same matrix by columns: the CSC arrays of A are the CSR arrays of A^T
    const std::vector<usize> cptr{0, 3, 4, 8, 10, 11}, cind{0, 1, 2, 2, 0, 1, 2, 3, 3, 4, 4};
    const std::vector<T> cval = values_of<T>({0, 2, 4, 5, 1, 3, 6, 7, 8, 9, 10});
    const CscMatrix<T> Ac(5, 5, cptr, cind, cval);
    CHECK(Ac.colour().colours == kColours);
    const CscMatrix<T> Mc = Ac.multicolour();
    CHECK(Mc.ordering().perm == kPerm && Mc.ordering().ncolours == 3);
    const CsrMatrix<T> back = CsrMatrix<T>::from(Mc);
    CHECK(back.rowptr() == kPermPtr && back.colind() == kPermInd && back.values() == pval);
    // refusals: not square; no permutation, the first offending position named; a matrix without an ordering
    const CsrMatrix<T> R(2, 3, {0, 1, 2}, {0, 2}, {1, 2});
    CHECK(panic_text([&] { (void)R.multicolour(); }).find("not square (2 x 3)") != std::string::npos);
    CHECK(panic_text([&] { (void)A.permute({0, 1, 1, 3, 4}); }).find("perm[2] = 1 repeats") != std::string::npos);
    CHECK(panic_text([&] { (void)A.permute({0, 1, 2, 5, 4}); }).find("perm[3] = 5 is out of range") != std::string::npos);
    CHECK(panic_text([&] { (void)A.ordering(); }).find("no ordering") != std::string::npos);
    CHECK(panic_text([&] { (void)A.to_order(v); }).find("no ordering") != std::string::npos);
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
    printf("colour mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
