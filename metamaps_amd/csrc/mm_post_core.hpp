// The arithmetic of K8 (mapping qualities, mapWrap.h:215-356) and of K9's problem set-up and stop rule (fEM.h:262-275, :624-639), as one text for
// the kernels of mm_post.hip and for a host build (tests/test_post_core.cpp via g++): DESIGN.md section 2, "K8 / K9 arithmetic".
//
// parse6(v): the reference prints identities and mapping qualities with 6 significant digits (ostream default, "%g") and reads them back with
// std::stod.  parse6 restates that round trip in arithmetic.  Its contract, held by tests/test_post_core.py:
//   * finite for every finite v: never NaN, never infinite.  NaN and the infinities are returned as they are, 0 as 0, the sign is kept.
//   * 0 < |v| < DBL_MIN gives 0 (of v's sign), and so does every v whose 6-digit text lies below DBL_MIN (DBL_MIN itself: "2.22507e-308"):
//     stod throws out_of_range on a denormal and the reference takes 0 (fEM.h:269-275).
//   * 1e-17 <= |v| < 1e28 (the scale is 10^s with s <= 22, an exact double): BIT-EQUAL to strtod of the "%g" text.  x = |v| * 10^t is one
//     correctly rounded product (quotient) and the fma gives the sign of what that rounding dropped, so the nearest integer of the EXACT scaled
//     value is taken, ties to even as glibc's printf does; the six-digit integer is then scaled back by one correctly rounded division
//     (product) of two exact numbers, which is what strtod returns for the text.
//   * DBL_MIN <= |v| < 1e-17 and |v| >= 1e28: the scale is split into two factors from tables, 10^(s mod 22) (exact) and 10^(22 * (s / 22))
//     (the double nearest to it: within half an ulp; no pow(), so host and device agree to the bit).  The six digits are those of the text
//     unless the scaled value lies within two ulps (2.4e-16 relative) of a tie, and the result is scaled back by at most two correctly rounded
//     divisions and one factor that is half an ulp off: at most 4 * 2^-53 relative from the text's double.
#pragma once
#include <cfloat>
#include <cmath>
#include <stdint.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mm {

MM_HD double pow10_int(int t) {
  const double tab[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  if (t >= 0 && t <= 22) return tab[t];
  return pow(10.0, (double)t);
}
// |v| scaled by 10^s or 10^-s, 0 <= s <= 329: one exact factor up to 22, beyond that a second one, 10^(22 j) (exact for j = 1)
MM_HD double pow10_22(int j) {
  const double tab[15] = {1e0, 1e22, 1e44, 1e66, 1e88, 1e110, 1e132, 1e154, 1e176, 1e198, 1e220, 1e242, 1e264, 1e286, 1e308};
  return tab[j < 14 ? j : 14];
}
MM_HD double parse6_up(double a, int s) { return s <= 22 ? a * pow10_int(s) : a * pow10_int(s % 22) * pow10_22(s / 22); }
MM_HD double parse6_down(double a, int s) { return s <= 22 ? a / pow10_int(s) : a / pow10_int(s % 22) / pow10_22(s / 22); }

MM_HD double parse6(double v) {
  if (v == 0.0 || !(v == v)) return v;
  const double a = fabs(v);
  if (a > DBL_MAX) return v;
  if (a < DBL_MIN) return v < 0 ? -0.0 : 0.0;                    // stod throws out_of_range → reference uses 0, fEM.h:269-275
  int e = (int)floor(log10(a));
  {                                                              // fix log10 rounding at decade boundaries
    double pe = e >= 0 ? pow10_int(e) : 1.0 / pow10_int(-e);
    if (a < pe) --e; else if (a >= pe * 10.0) ++e;
  }
  int t = 5 - e;
  const int s = t >= 0 ? t : -t;
  double x, rest = 0.0;                                           // rest: the sign of (exact scaled value - x), where the scale is exact
  if (t >= 0) { x = parse6_up(a, s); if (s <= 22) rest = fma(a, pow10_int(s), -x); }
  else { x = parse6_down(a, s); if (s <= 22) rest = fma(-x, pow10_int(s), a); }
  double d = rint(x);                                            // half to even
  if (rest != 0.0 && fabs(x - d) == 0.5) d = floor(x) + (rest > 0 ? 1.0 : 0.0);   // x is a tie, the exact value is not
  if (d >= 1e6) { d /= 10.0; t -= 1; }
  double r = t >= 0 ? parse6_down(d, t) : parse6_up(d, -t);
  if (r < DBL_MIN) r = 0.0;                                      // the text is a denormal
  return v < 0 ? -r : r;
}

// float math of Stat::j2md (map_stats.hpp:44) and the identity of computeMap.hpp:406,411
MM_HD float dev_identity(int shared, int s, int k) {
  float j = (float)(1.0 * shared / s);
  float md;
  if (j == 0) md = 1.0f;
  else if (j == 1) md = 0.0f;
  else md = (float)((-1.0 / k) * log(2.0 * j / (double)(1 + j)));
  return 100 * (1 - md);
}

MM_HD double dev_binom_pmf(int n, double p, int k) {             // boost pdf(binomial), mapWrap.h:340
  if (k < 0 || k > n) return 0.0;
  if (p == 0) return k == 0 ? 1.0 : 0.0;
  if (p == 1) return k == n ? 1.0 : 0.0;
  if (n == 0) return 1.0;
  if (k == 0) return pow(1 - p, (double)n);
  if (k == n) return pow(p, (double)k);
  return exp(lgamma((double)n + 1) - lgamma((double)k + 1) - lgamma((double)(n - k) + 1) + k * log(p) + (n - k) * log1p(-p));
}

// the success probability of a read's binomial: its best identity (a fraction, from the 6-digit text) -> p (mapWrap.h:261-266, :335-339)
MM_HD double mapq_success_p(double best_identity, int read_len, int k) {
  const double maxid = exp(-(1 - best_identity));                 // :261
  const int nk = read_len - k + 1;                                // :266
  const double surv = pow(maxid, (double)k);                      // :335
  const double es = round(surv * nk);
  const double eu = nk + (nk - es);
  return es / eu;
}

// the EM's stop rule after iteration `it` (0-based) with log-likelihood ll, ll_prev that of the iteration before (fEM.h:624-639)
MM_HD bool em_stop_now(long long it, double ll, double ll_prev) { return it > 0 && (ll - ll_prev) <= 1 && (1 - ll / ll_prev) < 0.0001; }

}  // namespace mm
