// Stand-alone host program for the sanitizers (address, undefined behaviour): no GPU, no Python, no library.  It compiles
// spalinalg_amd/csrc/cheb_host.hpp alone under -fsanitize=address,undefined and runs the host half of the Chebyshev series
// and of eigsh near sigma: the delta filter's coefficients on buffers of exactly degree + 1 doubles, the
// interval logic, and every refusal the new entry points decide before a device is touched (they call these functions).
// tests/test_near_sanitize.py builds and runs it.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "cheb_host.hpp"

using namespace spal;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// sum_i coef_i T_i(x) by the recurrence, in long double
static long double series_at(const double *coef, uint64_t d, long double x) {
    long double t0 = 1.0L, t1 = x, s = coef[0] + coef[1] * x;
    for (uint64_t i = 2; i <= d; ++i) {
        const long double t2 = 2.0L * x * t1 - t0;
        s += coef[i] * t2;
        t0 = t1;
        t1 = t2;
    }
    return s;
}

// the coefficients into a heap buffer of exactly d + 1 doubles: one write past it is the sanitizer's to find
static void delta(uint64_t d, double gamma) {
    std::unique_ptr<double[]> coef(new double[d + 1]);
    CHECK(cheb_delta_coefficients(d, gamma, coef.get()) == CHEB_SERIES_OK);
    for (uint64_t i = 0; i <= d; ++i) CHECK(std::isfinite(coef[i]));
    CHECK(fabsl(series_at(coef.get(), d, gamma) - 1.0L) <= 1e-12L);          // rho(gamma) = 1
    if (d <= 256)
        for (int j = -8; j <= 8; ++j) CHECK(series_at(coef.get(), d, j / 8.0L) >= -1e-12L);   // Fejer: rho >= 0 on [-1, 1]
    CHECK(cheb_series_check(d, -1.0, 1.0, coef.get(), d + 1) == CHEB_SERIES_OK);
    const ChebSeries<float> s = cheb_series_scalars<float>(0.0, 4.0, coef.get(), d + 1);
    CHECK(s.k.size() == d + 1 && s.a1 == 0.5f && s.a2 == 1.0f && s.cT == 2.0f);
    for (uint64_t i = 0; i <= d; ++i) CHECK(s.k[i] == (float)coef[i]);
}

int main() {
    const double edge = 1.0 - DBL_EPSILON;                                   // 1 - 2^-52
    for (uint64_t d : {1, 2, 3, 64, 4096})
        for (double gamma : {0.0, 0.5, -0.5, edge, -edge}) delta(d, gamma);

    // the coefficient function's refusals; a refused call writes nothing
    double one[2] = {7.0, 7.0};
    CHECK(cheb_delta_coefficients(0, 0.0, one) == CHEB_SERIES_DEGREE);
    CHECK(cheb_delta_coefficients(4097, 0.0, one) == CHEB_SERIES_DEGREE);
    CHECK(cheb_delta_coefficients(UINT64_MAX, 0.0, one) == CHEB_SERIES_DEGREE);
    CHECK(cheb_delta_coefficients(0, NAN, one) == CHEB_SERIES_DEGREE);       // the degree comes first
    for (double g : {1.0, -1.0, 1.5, -2.0, (double)NAN, (double)INFINITY, -(double)INFINITY})
        CHECK(cheb_delta_coefficients(1, g, one) == CHEB_DELTA_GAMMA);
    CHECK(one[0] == 7.0 && one[1] == 7.0);

    // the series' refusals, in the text's order
    const double good[3] = {1.0, 0.5, -0.0}, nan_c[3] = {1.0, NAN, 0.0}, inf_c[3] = {INFINITY, 0.0, 0.0};
    CHECK(cheb_series_check(2, 0.0, 1.0, good, 3) == CHEB_SERIES_OK);
    CHECK(cheb_series_check(0, 0.0, 1.0, good, 1) == CHEB_SERIES_DEGREE);
    CHECK(cheb_series_check(4097, 0.0, 1.0, good, 4098) == CHEB_SERIES_DEGREE);   // the buffer is not read
    CHECK(cheb_series_check(UINT64_MAX, 0.0, 1.0, good, 0) == CHEB_SERIES_DEGREE);
    CHECK(cheb_series_check(2, 0.0, 1.0, good, 2) == CHEB_SERIES_LEN);
    CHECK(cheb_series_check(2, 0.0, 1.0, good, 4) == CHEB_SERIES_LEN);            // ... nor here: 4 > its 3 doubles
    CHECK(cheb_series_check(2, 0.0, 1.0, nullptr, 4) == CHEB_SERIES_LEN);
    CHECK(cheb_series_check(2, NAN, 1.0, good, 3) == CHEB_SERIES_NOT_FINITE);
    CHECK(cheb_series_check(2, 0.0, INFINITY, good, 3) == CHEB_SERIES_NOT_FINITE);
    CHECK(cheb_series_check(2, 1.0, 1.0, good, 3) == CHEB_SERIES_EMPTY);
    CHECK(cheb_series_check(2, 2.0, 1.0, good, 3) == CHEB_SERIES_EMPTY);
    CHECK(cheb_series_check(2, 0.0, 1.0, nan_c, 3) == CHEB_SERIES_COEF);
    CHECK(cheb_series_check(2, 0.0, 1.0, inf_c, 3) == CHEB_SERIES_COEF);
    CHECK(cheb_series_check(2, -DBL_MAX, DBL_MAX, good, 3) == CHEB_SERIES_OK);
    {   // e = (hi - lo)/2 overflows for the widest interval: a1 = a2 = 0, finite; nothing here divides by zero
        const ChebSeries<double> s = cheb_series_scalars<double>(-DBL_MAX, DBL_MAX, good, 3);
        CHECK(s.a1 == 0.0 && s.a2 == 0.0 && s.cT == 0.0 && std::signbit(s.k[2]));
    }

    // eigsh near sigma: what is refused before the matrix is looked at
    CHECK(cheb_near_check(2, 1.0, 1, 0.0, 0.0) == CHEB_SERIES_OK);            // automatic: lo and hi are ignored
    CHECK(cheb_near_check(4096, 1.0, 1, NAN, NAN) == CHEB_SERIES_OK);
    CHECK(cheb_near_check(1, 1.0, 1, 0.0, 0.0) == CHEB_NEAR_DEGREE);
    CHECK(cheb_near_check(0, 1.0, 1, 0.0, 0.0) == CHEB_NEAR_DEGREE);
    CHECK(cheb_near_check(4097, 1.0, 1, 0.0, 0.0) == CHEB_NEAR_DEGREE);
    CHECK(cheb_near_check(16, NAN, 1, 0.0, 0.0) == CHEB_NEAR_SIGMA);
    CHECK(cheb_near_check(16, INFINITY, 0, 0.0, 4.0) == CHEB_NEAR_SIGMA);
    CHECK(cheb_near_check(16, 1.0, 0, 0.0, 4.0) == CHEB_SERIES_OK);
    CHECK(cheb_near_check(16, 1.0, 0, NAN, 4.0) == CHEB_SERIES_NOT_FINITE);
    CHECK(cheb_near_check(16, 1.0, 0, 0.0, INFINITY) == CHEB_SERIES_NOT_FINITE);
    CHECK(cheb_near_check(16, 1.0, 0, 4.0, 0.0) == CHEB_SERIES_EMPTY);
    CHECK(cheb_near_check(16, 1.0, 0, 1.0, 1.0) == CHEB_SERIES_EMPTY);
    CHECK(cheb_near_check(16, 0.0, 0, 0.0, 4.0) == CHEB_NEAR_SIGMA);          // strictly inside
    CHECK(cheb_near_check(16, 4.0, 0, 0.0, 4.0) == CHEB_NEAR_SIGMA);
    CHECK(cheb_near_check(16, -1.0, 0, 0.0, 4.0) == CHEB_NEAR_SIGMA);
    CHECK(cheb_near_check(16, std::nextafter(0.0, 1.0), 0, 0.0, 4.0) == CHEB_SERIES_OK);
    for (int r = CHEB_SERIES_OK; r <= CHEB_NEAR_SIGMA; ++r) CHECK(cheb_series_refusal_text((ChebSeriesRefusal)r) != nullptr);
    CHECK(cheb_series_refusal_text(CHEB_SERIES_OK)[0] == '\0' && cheb_series_refusal_text(CHEB_NEAR_SIGMA)[0] == 's');

    // the automatic interval and the filter on it
    double lo = 0.0, hi = 0.0, gamma = 9.0;
    cheb_near_auto_interval(0.0, 4.0, &lo, &hi);
    CHECK(lo == -4.0 / 1024 && hi == 4.0 + 4.0 / 1024);
    cheb_near_auto_interval(3.0, 3.0, &lo, &hi);                              // Gershgorin's interval is one point
    CHECK(lo == 3.0 && hi == 3.0);
    {
        std::vector<double> coef(65, 7.0);
        CHECK(cheb_near_filter(64, 3.0, 3.0, 3.0, &gamma, coef.data()) == CHEB_NEAR_SIGMA && gamma == 9.0 && coef[0] == 7.0);
        cheb_near_auto_interval(0.0, 4.0, &lo, &hi);
        CHECK(cheb_near_filter(64, 4.5, lo, hi, &gamma, coef.data()) == CHEB_NEAR_SIGMA);
        CHECK(cheb_near_filter(64, hi, lo, hi, &gamma, coef.data()) == CHEB_NEAR_SIGMA && coef[64] == 7.0);
        CHECK(cheb_near_filter(64, 2.0, lo, hi, &gamma, coef.data()) == CHEB_SERIES_OK && gamma == 0.0);
        CHECK(cheb_near_filter(64, 4.001, lo, hi, &gamma, coef.data()) == CHEB_SERIES_OK && gamma < 1.0);
        CHECK(fabsl(series_at(coef.data(), 64, gamma) - 1.0L) <= 1e-12L);
        // sigma strictly inside, but so near lo that gamma rounds to -1: the coefficient function refuses it
        CHECK(cheb_near_filter(64, 0.0, -1.0, 1e300, &gamma, coef.data()) == CHEB_DELTA_GAMMA && gamma == -1.0);
    }

    if (failures) return 1;
    printf("near sanitize ok\n");
    return 0;
}
