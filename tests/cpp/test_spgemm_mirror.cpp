// C++ host-mirror test of the sparse x sparse product (include/spalinalg.hpp: operator* of CsrMatrix / CscMatrix).
//   ./test_spgemm_mirror host   -- no GPU needed: a dimension mismatch panics before any device call
//   ./test_spgemm_mirror gpu    -- the reference's known-answer test src/csc/ops/mul.rs:67-95 (G5) on the device
#include <cstdio>
#include <functional>
#include <vector>

#include "spalinalg.hpp"

using namespace spalinalg;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool panics(const std::function<void()> &f) {
    try { f(); } catch (const Panic &) { return true; }
    return false;
}

static void host_tests() {
    const CsrMatrix<double> a(2, 3, {0, 1, 2}, {0, 2}, {1.0, 2.0});
    const CsrMatrix<double> b(4, 2, {0, 1, 1, 1, 2}, {0, 1}, {1.0, 2.0});
    CHECK(panics([&] { (void)(a * b); }));     // assert_eq!(self.ncols(), rhs.nrows()), mul.rs:9
    const CscMatrix<double> c(2, 3, {0, 1, 1, 2}, {0, 1}, {1.0, 2.0});
    const CscMatrix<double> d(4, 2, {0, 1, 2}, {0, 3}, {1.0, 2.0});
    CHECK(panics([&] { (void)(c * d); }));
}

static void gpu_tests() {
    // G5 (src/csc/ops/mul.rs:67-95)
    const CscMatrix<double> lhs(5, 3, {0, 3, 4, 6}, {0, 1, 4, 3, 1, 2}, {1.0, -5.0, 4.0, 3.0, 7.0, 2.0});
    const CscMatrix<double> rhs(3, 4, {0, 3, 4, 5, 6}, {0, 1, 2, 2, 0, 1}, {1.0, -5.0, 7.0, 3.0, -2.0, 4.0});
    const CscMatrix<double> out = lhs * rhs;
    CHECK(out.nrows() == 5 && out.ncols() == 4);
    CHECK((out.colptr() == std::vector<usize>{0, 5, 7, 10, 11}));
    CHECK((out.rowind() == std::vector<usize>{0, 1, 2, 3, 4, 1, 2, 0, 1, 4, 3}));
    CHECK((out.values() == std::vector<double>{1.0, 44.0, 14.0, -15.0, 4.0, 21.0, 6.0, -2.0, 10.0, -8.0, 12.0}));
    // the same product in CSR form: the operands and the result converted on the device
    const CsrMatrix<double> a = CsrMatrix<double>::from(lhs), b = CsrMatrix<double>::from(rhs);
    const CsrMatrix<double> c = a * b;
    const CscMatrix<double> back = CscMatrix<double>::from(c);
    CHECK(back.colptr() == out.colptr() && back.rowind() == out.rowind() && back.values() == out.values());
    // f32
    const CscMatrix<float> lf(5, 3, {0, 3, 4, 6}, {0, 1, 4, 3, 1, 2}, {1.f, -5.f, 4.f, 3.f, 7.f, 2.f});
    const CscMatrix<float> rf(3, 4, {0, 3, 4, 5, 6}, {0, 1, 2, 2, 0, 1}, {1.f, -5.f, 7.f, 3.f, -2.f, 4.f});
    const CscMatrix<float> of = lf * rf;
    CHECK((of.values() == std::vector<float>{1.f, 44.f, 14.f, -15.f, 4.f, 21.f, 6.f, -2.f, 10.f, -8.f, 12.f}));
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    try {
        host_tests();
        if (gpu) gpu_tests();
    } catch (const std::exception &e) {
        printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("spgemm mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
