// Stand-alone host program for the sanitizers (address, undefined behaviour): no GPU, no Python, no library.  It compiles
// spalinalg_amd/csrc/cheb_host.hpp alone under -fsanitize=address,undefined and runs the coefficient recurrence, the
// interval rule and the argument checks of the Chebyshev filter on edge arguments.  tests/test_cheb_sanitize.py builds and
// runs it.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "cheb_host.hpp"

using namespace spal;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// T_d(x) for |x| >= 1 by the recurrence in long double
static long double cheb_t(unsigned d, long double x) {
    long double t0 = 1.0L, t1 = x;
    if (d == 0) return t0;
    for (unsigned i = 2; i <= d; ++i) {
        const long double t2 = 2.0L * x * t1 - t0;
        t0 = t1;
        t1 = t2;
    }
    return t1;
}

// The recurrence with the coefficients on one scalar a (a 1 x 1 matrix) in double: t_d = T_d((a-c)/e) / T_d((a0-c)/e).
template <typename T>
static double scalar_apply(const ChebCoeffs<T> &k, double a) {
    double t0 = 1.0, t1 = (double)k.alpha[0] * (a - (double)k.cT);
    for (size_t i = 1; i < k.alpha.size(); ++i) {
        const double t2 = (double)k.alpha[i] * (a * t1 - (double)k.cT * t1) - (double)k.beta[i] * t0;
        t0 = t1;
        t1 = t2;
    }
    return t1;
}

template <typename T>
static void coefficients(double lo, double hi, double a0, double rel) {
    for (uint64_t d : {1, 2, 3, 8, 17, 256}) {
        CHECK(cheb_check(d, lo, hi, a0) == CHEB_OK);
        const ChebCoeffs<T> k = cheb_coefficients<T>(d, lo, hi, a0);
        CHECK(k.alpha.size() == d && k.beta.size() == d);
        CHECK(k.beta[0] == T(0));
        for (uint64_t i = 0; i < d; ++i) {
            CHECK(std::isfinite((double)k.alpha[i]) && std::isfinite((double)k.beta[i]));
            CHECK(std::fabs((double)k.beta[i]) <= 1.0);   // s_{i-1} * s_i, |s| < 1
        }
        if (d <= 17) {
            CHECK(std::fabs(scalar_apply(k, a0) - 1.0) <= rel * (double)d);   // p(a0) = 1
            const long double c = ((long double)lo + hi) / 2, e = ((long double)hi - lo) / 2;
            const double bound = (double)(1.0L / fabsl(cheb_t((unsigned)d, ((long double)a0 - c) / e)));
            for (double a : {lo, hi, (double)c, lo + 0.3 * (hi - lo)})
                CHECK(std::fabs(scalar_apply(k, a)) <= bound * (1.0 + rel * (double)d) + rel);   // small on the interval
        }
    }
}

int main() {
    // the refusals, in the text's order
    CHECK(cheb_check(0, 0.0, 1.0, 2.0) == CHEB_DEGREE);
    CHECK(cheb_check(257, 0.0, 1.0, 2.0) == CHEB_DEGREE);
    CHECK(cheb_check(UINT64_MAX, 0.0, 1.0, 2.0) == CHEB_DEGREE);
    CHECK(cheb_check(0, NAN, 1.0, 2.0) == CHEB_DEGREE);             // the degree comes first
    CHECK(cheb_check(1, NAN, 1.0, 2.0) == CHEB_NOT_FINITE);
    CHECK(cheb_check(1, 0.0, INFINITY, 2.0) == CHEB_NOT_FINITE);
    CHECK(cheb_check(1, 0.0, 1.0, -INFINITY) == CHEB_NOT_FINITE);
    CHECK(cheb_check(1, 1.0, 1.0, 2.0) == CHEB_EMPTY);
    CHECK(cheb_check(1, 2.0, 1.0, 3.0) == CHEB_EMPTY);
    CHECK(cheb_check(256, 0.0, 1.0, 0.0) == CHEB_A0_INSIDE);
    CHECK(cheb_check(256, 0.0, 1.0, 1.0) == CHEB_A0_INSIDE);
    CHECK(cheb_check(256, 0.0, 1.0, 0.5) == CHEB_A0_INSIDE);
    CHECK(cheb_check(256, -0.0, 1.0, 0.0) == CHEB_A0_INSIDE);        // -0.0 <= +0.0
    CHECK(cheb_check(256, 0.0, 1.0, std::nextafter(1.0, 2.0)) == CHEB_OK);
    CHECK(cheb_check(1, -DBL_MAX, DBL_MAX, 0.0) == CHEB_A0_INSIDE);
    for (int r = CHEB_OK; r <= CHEB_A0_INSIDE; ++r) CHECK(cheb_refusal_text((ChebRefusal)r) != nullptr);
    CHECK(cheb_refusal_text(CHEB_DEGREE)[0] == 'd' && cheb_refusal_text(CHEB_OK)[0] == '\0');

    // the coefficients: wide and narrow gaps, both sides, large offsets, tiny intervals
    coefficients<double>(0.0, 3.9, 4.0, 1e-12);
    coefficients<double>(0.1, 4.0, 0.0, 1e-12);
    coefficients<double>(-3.0, -1.0, -0.5, 1e-12);
    coefficients<double>(1e6, 1e6 + 1.0, 1e6 + 2.0, 1e-8);
    coefficients<double>(0.0, 1e-300, 2e-300, 1e-12);
    coefficients<float>(0.0, 3.9, 4.0, 1e-4);
    coefficients<float>(0.1, 4.0, 0.0, 1e-4);
    {   // a0 one ulp outside: s_1 is one ulp below 1, nothing overflows at degree 256, f32 included
        const double a0 = std::nextafter(1.0, 2.0);
        const ChebCoeffs<float> k = cheb_coefficients<float>(256, 0.0, 1.0, a0);
        for (size_t i = 0; i < 256; ++i) CHECK(std::isfinite(k.alpha[i]) && std::fabs(k.beta[i]) <= 1.0f);
        CHECK(k.cT == 0.5f);
    }

    // the interval rule
    double lo = -1.0, hi = -1.0;
    CHECK(cheb_auto_interval(0, 0.0, 4.0, 3.5, &lo, &hi) && lo == 0.0 && hi == 3.5);
    CHECK(cheb_auto_interval(1, 0.0, 4.0, 0.25, &lo, &hi) && lo == 0.25 && hi == 4.0);
    lo = hi = -1.0;
    CHECK(!cheb_auto_interval(0, 0.0, 4.0, 4.0, &lo, &hi));
    CHECK(!cheb_auto_interval(0, 0.0, 4.0, 0.0, &lo, &hi));
    CHECK(!cheb_auto_interval(1, 0.0, 4.0, -1.0, &lo, &hi));
    CHECK(!cheb_auto_interval(1, 0.0, 4.0, NAN, &lo, &hi));
    CHECK(!cheb_auto_interval(0, 3.0, 3.0, 3.0, &lo, &hi));          // Gershgorin's interval is one point
    CHECK(lo == -1.0 && hi == -1.0);                                 // a degenerate cut writes nothing
    CHECK(cheb_a0(0, -2.0, 5.0) == 5.0 && cheb_a0(1, -2.0, 5.0) == -2.0);
    CHECK(cheb_scale(-7.0, 5.0) == 7.0 && cheb_scale(-2.0, 5.0) == 5.0 && cheb_scale(0.0, 0.0) == 0.0);
    CHECK(cheb_wanted_side(0, 0.0, 3.0, 4.0) && !cheb_wanted_side(0, 0.0, 3.0, -1.0) && !cheb_wanted_side(0, 0.0, 3.0, 3.0));
    CHECK(cheb_wanted_side(1, 1.0, 4.0, 0.0) && !cheb_wanted_side(1, 1.0, 4.0, 5.0) && !cheb_wanted_side(1, 1.0, 4.0, 1.0));

    // tol = 0
    CHECK(cheb_tol<double>(0.0) == 256.0 * DBL_EPSILON && cheb_tol<float>(0.0) == 256.0 * (double)FLT_EPSILON);
    CHECK(cheb_tol<double>(1e-8) == 1e-8 && cheb_tol<float>(1e-300) == 1e-300);

    if (failures) return 1;
    printf("cheb sanitize ok\n");
    return 0;
}
