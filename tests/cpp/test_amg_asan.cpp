// Stand-alone host program for the sanitizers (address, undefined behaviour): no GPU, no Python.  It is linked with the
// host side of spal_amg.hip and spal_host.cpp compiled under -fsanitize=address,undefined and drives what those do before
// any device work: spal_amg_aggregate, the aggregation text, on buffers of exactly the size the call claims, and the
// refusals of every spal_amg_* / spal_*_amg_setup entry point that need no device.  tests/test_amg_sanitize.py builds and
// runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "spal.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool refused(int status, const char *text) {
    return status == SPAL_ERR_INVALID_ARGUMENT && std::string(spal_last_error()).find(text) != std::string::npos;
}

// the pattern of a path of n vertices with its diagonal
static void path(uint64_t n, std::vector<uint64_t> &rowptr, std::vector<uint64_t> &colind) {
    rowptr.assign(1, 0);
    colind.clear();
    for (uint64_t i = 0; i < n; ++i) {
        if (i) colind.push_back(i - 1);
        colind.push_back(i);
        if (i + 1 < n) colind.push_back(i + 1);
        rowptr.push_back(colind.size());
    }
}

static void host_text() {
    std::vector<uint64_t> rp, ci;
    path(8, rp, ci);
    std::vector<uint64_t> agg(8, 99);
    uint64_t nagg = 99;
    CHECK(spal_amg_aggregate(8, rp.data(), ci.data(), 0, agg.data(), &nagg) == SPAL_OK);
    CHECK(nagg == 4 && agg == (std::vector<uint64_t>{0, 1, 1, 2, 2, 2, 3, 3}));
    // seed 2^32 + 7 behaves as seed 7
    std::vector<uint64_t> a7(8), a7w(8);
    uint64_t n7 = 0, n7w = 0;
    CHECK(spal_amg_aggregate(8, rp.data(), ci.data(), 7, a7.data(), &n7) == SPAL_OK);
    CHECK(spal_amg_aggregate(8, rp.data(), ci.data(), (1ull << 32) + 7, a7w.data(), &n7w) == SPAL_OK);
    CHECK(n7 == n7w && a7 == a7w);
    // a star stored in one direction only: one aggregate
    std::vector<uint64_t> srp{0, 8}, sci{1, 2, 3, 4, 5, 6, 7, 8};
    srp.resize(10, 8);
    std::vector<uint64_t> sagg(9, 99);
    CHECK(spal_amg_aggregate(9, srp.data(), sci.data(), 0, sagg.data(), &nagg) == SPAL_OK);
    CHECK(nagg == 1 && sagg == std::vector<uint64_t>(9, 0));
    // n = 0: nothing is read through colind or written through agg
    const uint64_t zero = 0;
    CHECK(spal_amg_aggregate(0, &zero, nullptr, 0, nullptr, &nagg) == SPAL_OK && nagg == 0);
    // no entries at all: every vertex an aggregate of its own
    std::vector<uint64_t> erp(4, 0), eagg(3, 99);
    CHECK(spal_amg_aggregate(3, erp.data(), nullptr, 0, eagg.data(), &nagg) == SPAL_OK);
    CHECK(nagg == 3 && eagg == (std::vector<uint64_t>{0, 1, 2}));
    // refusals: agg stays untouched
    std::vector<uint64_t> keep(8, 99);
    CHECK(refused(spal_amg_aggregate(8, nullptr, ci.data(), 0, keep.data(), &nagg), "null array"));
    CHECK(refused(spal_amg_aggregate(8, rp.data(), ci.data(), 0, nullptr, &nagg), "null array"));
    CHECK(refused(spal_amg_aggregate(8, rp.data(), ci.data(), 0, keep.data(), nullptr), "null array"));
    CHECK(refused(spal_amg_aggregate(8, rp.data(), nullptr, 0, keep.data(), &nagg), "null array"));
    std::vector<uint64_t> bad = rp;
    bad[0] = 1;
    CHECK(refused(spal_amg_aggregate(8, bad.data(), ci.data(), 0, keep.data(), &nagg), "rowptr[0] = 1"));
    bad = rp;
    bad[3] = bad[4] + 1;
    CHECK(refused(spal_amg_aggregate(8, bad.data(), ci.data(), 0, keep.data(), &nagg), "rowptr is not sorted"));
    std::vector<uint64_t> badc = ci;
    badc.back() = 8;
    CHECK(refused(spal_amg_aggregate(8, rp.data(), badc.data(), 0, keep.data(), &nagg), "stores column 8"));
    CHECK(keep == std::vector<uint64_t>(8, 99));
}

template <typename H, typename Setup>
static void setup_refusals(Setup setup) {
    std::vector<unsigned char> zeros(1 << 16, 0);   // stands in for a handle in calls that end before it is looked at
    H fake = reinterpret_cast<H>(zeros.data());
    spal_amg_params d;
    CHECK(spal_amg_default_params(&d) == SPAL_OK);
    CHECK(d.seed == 0 && d.max_levels == 16 && d.coarse_rows == 64 && d.nu == 2 && d.coarse_sweeps == 16 && d.gamma == 1);
    CHECK(d.omega == 2.0 / 3.0 && d.alpha == 1.0);
    spal_amg_t out = reinterpret_cast<spal_amg_t>(zeros.data());
    CHECK(refused(setup(nullptr, &d, nullptr, &out), "null argument"));
    CHECK(refused(setup(fake, nullptr, nullptr, &out), "null argument"));
    CHECK(refused(setup(fake, &d, nullptr, nullptr), "null argument"));
    struct Bad { const char *field; void (*set)(spal_amg_params &); };
    const Bad bad[] = {
        {"max_levels", [](spal_amg_params &p) { p.max_levels = 0; }},  {"max_levels", [](spal_amg_params &p) { p.max_levels = 33; }},
        {"nu", [](spal_amg_params &p) { p.nu = 0; }},                  {"nu", [](spal_amg_params &p) { p.nu = 17; }},
        {"coarse_sweeps", [](spal_amg_params &p) { p.coarse_sweeps = 0; }},
        {"coarse_sweeps", [](spal_amg_params &p) { p.coarse_sweeps = 1025; }},
        {"gamma", [](spal_amg_params &p) { p.gamma = 0; }},            {"gamma", [](spal_amg_params &p) { p.gamma = 3; }},
        {"omega", [](spal_amg_params &p) { p.omega = 0.0; }},          {"omega", [](spal_amg_params &p) { p.omega = NAN; }},
        {"omega", [](spal_amg_params &p) { p.omega = INFINITY; }},     {"alpha", [](spal_amg_params &p) { p.alpha = -1.0; }},
        {"alpha", [](spal_amg_params &p) { p.alpha = NAN; }},
    };
    for (const Bad &b : bad) {
        spal_amg_params p = d;
        b.set(p);
        out = reinterpret_cast<spal_amg_t>(zeros.data());
        CHECK(refused(setup(fake, &p, nullptr, &out), b.field));
        CHECK(out == nullptr);
    }
}

static void handle_refusals() {
    std::vector<double> b(4, 1.0), x(4, 0.0);
    std::vector<float> bf(4, 1.f), xf(4, 0.f);
    std::vector<uint64_t> agg(4, 99);
    char buf[64];
    spal_csr_t copy = nullptr;
    CHECK(spal_amg_default_params(nullptr) == SPAL_ERR_INVALID_ARGUMENT);
    CHECK(spal_amg_destroy(nullptr) == SPAL_OK);
    CHECK(refused(spal_amg_describe(nullptr, buf, sizeof buf), "null argument"));
    CHECK(refused(spal_amg_set_option(nullptr, "amg_tail_rows", 0), "null argument"));
    CHECK(refused(spal_amg_level_csr(nullptr, 0, &copy), "null argument"));
    CHECK(refused(spal_amg_aggregates(nullptr, 0, agg.data(), 4), "null argument"));
    CHECK(refused(spal_amg_apply_f64(nullptr, b.data(), 4, x.data(), 4), "handle is NULL"));
    CHECK(refused(spal_amg_apply_f32(nullptr, bf.data(), 4, xf.data(), 4), "handle is NULL"));
    CHECK(refused(spal_amg_apply_dev_f64(nullptr, b.data(), x.data(), nullptr), "handle is NULL"));
    CHECK(refused(spal_amg_apply_dev_f32(nullptr, bf.data(), xf.data(), nullptr), "handle is NULL"));
    // the solvers: g is not NULL
    std::vector<unsigned char> zeros(1 << 16, 0);
    spal_krylov_info info;
    CHECK(refused(spal_csr_krylov_amg_f64(reinterpret_cast<spal_csr_t>(zeros.data()), 0, nullptr, b.data(), 4, x.data(), 4, 1e-8, 5, &info),
                  "null argument"));
    CHECK(refused(spal_csc_krylov_amg_dev_f32(reinterpret_cast<spal_csc_t>(zeros.data()), 0, nullptr, bf.data(), xf.data(), 1e-8, 5,
                                              nullptr, &info), "null argument"));
    for (const double v : x) CHECK(v == 0.0);
    for (const uint64_t v : agg) CHECK(v == 99);
}

int main() {
    host_text();
    setup_refusals<spal_csr_t>(spal_csr_amg_setup);
    setup_refusals<spal_csc_t>(spal_csc_amg_setup);
    handle_refusals();
    if (failures) return 1;
    printf("amg sanitize ok\n");
    return 0;
}
