// cheb_host.hpp -- the host half of the Chebyshev filter (spal_*_cheb_apply_*, spal_*_eigsh_filtered_*: DESIGN 3.26).
// Plain C++ on doubles, no device and no library call: the coefficients of the three-term recurrence, the refusals of a
// degree and an interval, the rule that turns a warm-up's cut into the interval, and what tol = 0 stands for.  Only
// + - * / on doubles and one conversion to T at the end, contraction off: the text of include/spal.h, which
// tests/cheb_ref.py restates in numpy bit for bit.  tests/cpp/test_cheb_asan.cpp compiles this header alone under the
// sanitizers.  Below them the host half of the Chebyshev series and of eigsh near sigma: the delta filter's
// coefficients, the interval and the refusals; tests/cpp/test_near_asan.cpp does the same for those.  (Not installed.)
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

// ---- the Chebyshev series and eigsh near sigma (spal_*_cheb_series_*, spal_*_eigsh_near_*: DESIGN 3.28) ----------------
constexpr uint64_t kChebSeriesMaxDegree = 4096;

// Why a series or a delta filter is refused: 0 = it is fine.  The order is the text's.
enum ChebSeriesRefusal {
    CHEB_SERIES_OK = 0, CHEB_SERIES_DEGREE, CHEB_SERIES_LEN, CHEB_SERIES_NOT_FINITE, CHEB_SERIES_EMPTY, CHEB_SERIES_COEF,
    CHEB_DELTA_GAMMA, CHEB_DELTA_NRM, CHEB_NEAR_DEGREE, CHEB_NEAR_SIGMA
};
inline const char *cheb_series_refusal_text(ChebSeriesRefusal r) {
    switch (r) {
    case CHEB_SERIES_DEGREE: return "degree must be 1 .. 4096";
    case CHEB_SERIES_LEN: return "coef_len must be degree + 1";
    case CHEB_SERIES_NOT_FINITE: return "lo and hi must be finite";
    case CHEB_SERIES_EMPTY: return "lo must be less than hi";
    case CHEB_SERIES_COEF: return "every coefficient must be finite";
    case CHEB_DELTA_GAMMA: return "gamma must lie strictly inside (-1, 1)";
    case CHEB_DELTA_NRM: return "the filter's value at gamma is zero or not finite";
    case CHEB_NEAR_DEGREE: return "degree must be 2 .. 4096";
    case CHEB_NEAR_SIGMA: return "sigma must lie strictly inside the interval";
    default: return "";
    }
}

// coef may be null only when the caller has refused that already
inline ChebSeriesRefusal cheb_series_check(uint64_t degree, double lo, double hi, const double *coef, uint64_t coef_len) {
    if (degree < 1 || degree > kChebSeriesMaxDegree) return CHEB_SERIES_DEGREE;
    if (coef_len != degree + 1) return CHEB_SERIES_LEN;
    if (!std::isfinite(lo) || !std::isfinite(hi)) return CHEB_SERIES_NOT_FINITE;
    if (!(lo < hi)) return CHEB_SERIES_EMPTY;
    for (uint64_t i = 0; i < coef_len; ++i)
        if (!std::isfinite(coef[i])) return CHEB_SERIES_COEF;
    return CHEB_SERIES_OK;
}

// The series' scalars: a1 = T(1/e), a2 = T(2/e), cT = T(c), k[i] = T(coef[i]).  The arguments have passed cheb_series_check.
template <typename T>
struct ChebSeries {
    std::vector<T> k;
    T a1 = T(0), a2 = T(0), cT = T(0);
};
template <typename T>
inline ChebSeries<T> cheb_series_scalars(double lo, double hi, const double *coef, uint64_t coef_len) {
    ChebSeries<T> s;
    const double c = (lo + hi) / 2.0, e = (hi - lo) / 2.0;
    s.a1 = (T)(1.0 / e);
    s.a2 = (T)(2.0 / e);
    s.cT = (T)c;
    s.k.resize(coef_len);
    for (uint64_t i = 0; i < coef_len; ++i) s.k[i] = (T)coef[i];
    return s;
}

// The Fejer-damped delta function at gamma (the text of include/spal.h): coef[0 .. degree], only + - * / on doubles.
//   m_0 = 1;  m_1 = gamma;  m_i = ((2*gamma)*m_{i-1}) - m_{i-2};   g_i = double(d+1-i)/double(d+1)
//   u_0 = g_0*m_0;  u_i = g_i*(2*m_i);   nrm = (..((0 + u_0*m_0) + u_1*m_1) ..) + u_d*m_d;   coef_i = u_i/nrm
// coef is written only when the call is not refused.
inline ChebSeriesRefusal cheb_delta_coefficients(uint64_t degree, double gamma, double *coef) {
    if (degree < 1 || degree > kChebSeriesMaxDegree) return CHEB_SERIES_DEGREE;
    if (!(gamma > -1.0 && gamma < 1.0)) return CHEB_DELTA_GAMMA;
    std::vector<double> u(degree + 1);
    const double d1 = (double)(degree + 1), g2 = 2.0 * gamma;
    double mp = 1.0, m = gamma, nrm = 0.0;   // m_{i-1}, m_i
    u[0] = (d1 / d1) * 1.0;
    nrm = nrm + u[0] * 1.0;
    for (uint64_t i = 1; i <= degree; ++i) {
        if (i >= 2) {
            const double mn = (g2 * m) - mp;
            mp = m;
            m = mn;
        }
        u[i] = ((double)(degree + 1 - i) / d1) * (2.0 * m);
        nrm = nrm + u[i] * m;
    }
    if (!std::isfinite(nrm) || nrm == 0.0) return CHEB_DELTA_NRM;
    for (uint64_t i = 0; i <= degree; ++i) coef[i] = u[i] / nrm;
    return CHEB_SERIES_OK;
}

// eigsh near sigma: what needs no matrix.  A given interval is checked here; an automatic one after Gershgorin.
inline ChebSeriesRefusal cheb_near_check(uint64_t degree, double sigma, int automatic, double lo, double hi) {
    if (degree < 2 || degree > kChebSeriesMaxDegree) return CHEB_NEAR_DEGREE;
    if (!std::isfinite(sigma)) return CHEB_NEAR_SIGMA;
    if (automatic) return CHEB_SERIES_OK;
    if (!std::isfinite(lo) || !std::isfinite(hi)) return CHEB_SERIES_NOT_FINITE;
    if (!(lo < hi)) return CHEB_SERIES_EMPTY;
    if (!(lo < sigma && sigma < hi)) return CHEB_NEAR_SIGMA;
    return CHEB_SERIES_OK;
}

// The automatic interval: Gershgorin's, widened by 1/1024 of its width on either side.
inline void cheb_near_auto_interval(double glo, double ghi, double *lo, double *hi) {
    const double m = (ghi - glo) / 1024.0;
    *lo = glo - m;
    *hi = ghi + m;
}

// gamma = (sigma - c)/e and the filter's coefficients on [lo, hi] (degree + 1 doubles).  The interval is finite and not
// empty; refuses a sigma that is not strictly inside, and what cheb_delta_coefficients refuses.
inline ChebSeriesRefusal cheb_near_filter(uint64_t degree, double sigma, double lo, double hi, double *gamma, double *coef) {
    if (!(lo < sigma && sigma < hi)) return CHEB_NEAR_SIGMA;
    const double c = (lo + hi) / 2.0, e = (hi - lo) / 2.0;
    *gamma = (sigma - c) / e;
    return cheb_delta_coefficients(degree, *gamma, coef);
}

}  // namespace spal
