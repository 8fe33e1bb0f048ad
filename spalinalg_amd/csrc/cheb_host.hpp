// cheb_host.hpp -- the host half of the Chebyshev filter (spal_*_cheb_apply_*, spal_*_eigsh_filtered_*: DESIGN 3.26).
// Plain C++ on doubles, no device and no library call: the coefficients of the three-term recurrence, the refusals of a
// degree and an interval, the rule that turns a warm-up's cut into the interval, and what tol = 0 stands for.  Only
// + - * / on doubles and one conversion to T at the end, contraction off: the text of include/spal.h, which
// tests/cheb_ref.py restates in numpy bit for bit.  tests/cpp/test_cheb_asan.cpp compiles this header alone under the
// sanitizers.  (Not installed.)
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#pragma clang fp contract(off)

namespace spal {

constexpr uint64_t kChebMaxDegree = 256;

// Why an interval is refused: 0 = it is fine.  The order is the text's.
enum ChebRefusal { CHEB_OK = 0, CHEB_DEGREE, CHEB_NOT_FINITE, CHEB_EMPTY, CHEB_A0_INSIDE };

inline ChebRefusal cheb_check(uint64_t degree, double lo, double hi, double a0) {
    if (degree < 1 || degree > kChebMaxDegree) return CHEB_DEGREE;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(a0)) return CHEB_NOT_FINITE;
    if (!(lo < hi)) return CHEB_EMPTY;
    if (lo <= a0 && a0 <= hi) return CHEB_A0_INSIDE;
    return CHEB_OK;
}
inline const char *cheb_refusal_text(ChebRefusal r) {
    switch (r) {
    case CHEB_DEGREE: return "degree must be 1 .. 256";
    case CHEB_NOT_FINITE: return "lo, hi and a0 must be finite";
    case CHEB_EMPTY: return "lo must be less than hi";
    case CHEB_A0_INSIDE: return "a0 must lie outside [lo, hi]";
    default: return "";
    }
}

// alpha[i - 1], beta[i - 1] for step i = 1 .. degree, and cT.  The arguments have passed cheb_check.
//   c = (lo+hi)/2;  e = (hi-lo)/2;  s_1 = e/(a0 - c);  s_i = 1/(2/s_1 - s_{i-1})
//   alpha_1 = T(s_1/e), beta_1 = 0;  alpha_i = T((2*s_i)/e), beta_i = T(s_{i-1}*s_i);  cT = T(c)
// |s_1| < 1 because a0 is outside the interval, and then |s_i| < 1 for every i: p(a0) = 1, nothing grows with the degree.
template <typename T>
struct ChebCoeffs {
    std::vector<T> alpha, beta;
    T cT = T(0);
};
template <typename T>
inline ChebCoeffs<T> cheb_coefficients(uint64_t degree, double lo, double hi, double a0) {
    ChebCoeffs<T> k;
    const double c = (lo + hi) / 2.0, e = (hi - lo) / 2.0;
    const double s1 = e / (a0 - c);
    k.alpha.reserve(degree);
    k.beta.reserve(degree);
    k.alpha.push_back((T)(s1 / e));
    k.beta.push_back(T(0));
    double sp = s1;
    for (uint64_t i = 2; i <= degree; ++i) {
        const double s = 1.0 / (2.0 / s1 - sp);
        k.alpha.push_back((T)((2.0 * s) / e));
        k.beta.push_back((T)(sp * s));
        sp = s;
    }
    k.cT = (T)c;
    return k;
}

// The far end of the wanted side (which: 0 = LA, 1 = SA) and the scale of the residual test.
inline double cheb_a0(int which, double glo, double ghi) { return which == 0 ? ghi : glo; }
inline double cheb_scale(double glo, double ghi) { return std::fmax(std::fabs(glo), std::fabs(ghi)); }

// The automatic interval from the warm-up's k-th Ritz value: [glo, cut] for LA, [cut, ghi] for SA.  false: the cut is
// degenerate (glo < cut < ghi does not hold, NaN included) and the warm-up's result stands.
inline bool cheb_auto_interval(int which, double glo, double ghi, double cut, double *lo, double *hi) {
    if (!(glo < cut && cut < ghi)) return false;
    *lo = which == 0 ? glo : cut;
    *hi = which == 0 ? cut : ghi;
    return true;
}

// A caller's interval for filtered eigsh: a0 strictly outside it ON THE WANTED SIDE (above for LA, below for SA).
inline bool cheb_wanted_side(int which, double lo, double hi, double a0) { return which == 0 ? a0 > hi : a0 < lo; }

// tol = 0 stands for 256 eps of the element type: a TRUE residual does not reach eps * scale (DESIGN 3.26 has the floors
// the text reaches on the test matrices: 66 eps * scale at worst).
template <typename T>
inline double cheb_tol(double tol) { return tol > 0.0 ? tol : 256.0 * (double)std::numeric_limits<T>::epsilon(); }

}  // namespace spal
