// C++ host-mirror test of A + B, A - B and -A (include/spalinalg.hpp: operator+ / operator- of CsrMatrix / CscMatrix).
//   ./test_spadd_mirror host   -- no GPU needed: a shape mismatch panics before any device call
//   ./test_spadd_mirror gpu    -- the reference's six known-answer tests (src/csr/ops/{add,sub,neg}.rs,
//                                 src/csc/ops/{add,sub,neg}.rs) on the device
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
    const CsrMatrix<double> b(3, 3, {0, 1, 1, 2}, {0, 1}, {1.0, 2.0});
    const CsrMatrix<double> c(2, 4, {0, 1, 2}, {0, 3}, {1.0, 2.0});
    CHECK(panic_text([&] { (void)(a + b); }) == "assertion failed: nrows == rhs.nrows (left: 2, right: 3)");
    CHECK(panic_text([&] { (void)(a - c); }) == "assertion failed: ncols == rhs.ncols (left: 3, right: 4)");
    const CscMatrix<double> d(2, 3, {0, 1, 1, 2}, {0, 1}, {1.0, 2.0});
    const CscMatrix<double> e(4, 3, {0, 1, 2, 2}, {0, 3}, {1.0, 2.0});
    CHECK(panic_text([&] { (void)(d + e); }) == "assertion failed: nrows == rhs.nrows (left: 2, right: 4)");
    CHECK(panic_text([&] { (void)(d - e); }) == "assertion failed: nrows == rhs.nrows (left: 2, right: 4)");
}

template <typename T>
static void gpu_kats() {
    // src/csr/ops/add.rs:82-106, sub.rs:82-109
    const CsrMatrix<T> lhs(4, 4, {0, 1, 3, 4, 7}, {0, 0, 2, 1, 1, 2, 3}, {1, 2, 3, 4, 5, 6, 7});
    const CsrMatrix<T> rhs(4, 4, {0, 2, 3, 4, 5}, {0, 2, 2, 3, 1}, {2, 4, 8, 10, 6});
    const CsrMatrix<T> s = lhs + rhs, d = lhs - rhs;
    CHECK(s.nrows() == 4 && s.ncols() == 4);
    CHECK((s.rowptr() == std::vector<usize>{0, 2, 4, 6, 9}));
    CHECK((s.colind() == std::vector<usize>{0, 2, 0, 2, 1, 3, 1, 2, 3}));
    CHECK((s.values() == std::vector<T>{3, 4, 2, 11, 4, 10, 11, 6, 7}));
    CHECK(d.rowptr() == s.rowptr() && d.colind() == s.colind());
    CHECK((d.values() == std::vector<T>{-1, -4, 2, -5, 4, -10, -1, 6, 7}));
    // src/csr/ops/neg.rs:25-36
    const CsrMatrix<T> m(2, 1, {0, 1, 2}, {0, 0}, {1, 2});
    const CsrMatrix<T> n = -m;
    CHECK(n.nrows() == 2 && n.ncols() == 1);
    CHECK((n.rowptr() == std::vector<usize>{0, 1, 2}) && (n.colind() == std::vector<usize>{0, 0}));
    CHECK((n.values() == std::vector<T>{-1, -2}));
    // src/csc/ops/add.rs:77-101, sub.rs:77-104
    const CscMatrix<T> cl(4, 4, {0, 2, 4, 6, 7}, {0, 1, 2, 3, 1, 3, 3}, {1, 2, 4, 5, 3, 6, 7});
    const CscMatrix<T> cr(4, 4, {0, 1, 2, 4, 5}, {0, 3, 0, 1, 2}, {2, 6, 4, 8, 10});
    const CscMatrix<T> cs = cl + cr, cd = cl - cr;
    CHECK((cs.colptr() == std::vector<usize>{0, 2, 4, 7, 9}));
    CHECK((cs.rowind() == std::vector<usize>{0, 1, 2, 3, 0, 1, 3, 2, 3}));
    CHECK((cs.values() == std::vector<T>{3, 2, 4, 11, 4, 11, 6, 10, 7}));
    CHECK(cd.colptr() == cs.colptr() && cd.rowind() == cs.rowind());
    CHECK((cd.values() == std::vector<T>{-1, 2, 4, -1, -4, -5, 6, -10, 7}));
    // src/csc/ops/neg.rs:25-36
    const CscMatrix<T> cm(1, 2, {0, 1, 2}, {0, 0}, {1, 2});
    const CscMatrix<T> cn = -cm;
    CHECK(cn.nrows() == 1 && cn.ncols() == 2);
    CHECK((cn.colptr() == std::vector<usize>{0, 1, 2}) && (cn.rowind() == std::vector<usize>{0, 0}));
    CHECK((cn.values() == std::vector<T>{-1, -2}));
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    try {
        host_tests();
        if (gpu) {
            gpu_kats<double>();
            gpu_kats<float>();
        }
    } catch (const std::exception &e) {
        printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("spadd mirror %s ok\n", gpu ? "gpu" : "host");
    return 0;
}
