// Extreme eigenvalues of a symmetric tridiagonal matrix of order k <= 64 and the eigenvector of the smallest one: the host side of the
// Lanczos estimate of lambda_min(H + J' Sigma J) (lanczos.hip).  Header-only, no device code, no allocation:
// okkt_debug_tridiag_eig exports it and the host sanitizer driver calls it.
//
//   T = tridiag(beta_0 .. beta_k-2; alpha_0 .. alpha_k-1; beta_0 .. beta_k-2)
//
// The eigenvalues come from bisection on the Sturm count of T scaled by a power of two (so squares of the off-diagonal neither
// overflow nor lose anything to the scaling), each to the last bit the count can resolve: an absolute error of a few ulps of ||T||.
// The vector belongs to the first unreduced block (split at the off-diagonal entries that are exactly zero) that attains theta_min.
// Its shift is the lower end of theta_min's final bisection interval, where the count is zero, i.e. where the pivots of the block's
// L D L' are all positive: inverse iteration with that factorisation needs no pivoting.  The start vector carries the sign pattern of
// the eigenvector (after the similarity that makes every off-diagonal entry negative the vector of the smallest eigenvalue is
// positive), so it is never orthogonal to it.
#pragma once
#include <cmath>
#include <cstdint>

namespace okkt {

constexpr int kTriMax = 64;

namespace tri_detail {
// the number of eigenvalues of a[lo..hi) / b[lo..hi-1) below x
inline int sturm_count(const double* a, const double* b, int lo, int hi, double x) {
  int cnt = 0;
  double q = 1.0;
  for (int i = lo; i < hi; ++i) {
    const double off = i > lo ? b[i - 1] : 0.0;
    if (q == 0.0) q = 1e-300;   // (scaled entries are <= 1: the quotient stays finite)
    q = (a[i] - x) - (i > lo ? (off * off) / q : 0.0);
    if (q < 0.0) ++cnt;
  }
  return cnt;
}
// the interval [lo_out, hi_out] of adjacent doubles (or equal ones) around eigenvalue `idx` (ascending, 0-based) of the block
inline void bisect(const double* a, const double* b, int lo, int hi, int idx, double glo, double ghi, double* lo_out, double* hi_out) {
  if (hi - lo == 1) { *lo_out = *hi_out = a[lo]; return; }   // a block of one: the entry itself
  double l = glo, h = ghi;   // count(l) <= idx < count(h)
  for (int it = 0; it < 2200; ++it) {
    const double mid = l + 0.5 * (h - l);
    if (!(mid > l && mid < h)) break;
    if (sturm_count(a, b, lo, hi, mid) <= idx) l = mid; else h = mid;
  }
  *lo_out = l;
  *hi_out = h;
}
}  // namespace tri_detail

// Returns 0; 1 when k is out of range or an entry is not finite (the outputs are then untouched); 2 when the inverse iteration left
// the finite range (theta_min and theta_max are set, s_out is not a vector to trust).  s_out: k doubles, unit 2-norm, its largest
// entry positive.
inline int tridiag_extreme(int k, const double* alpha, const double* beta, double* theta_min, double* theta_max, double* s_out) {
  if (k < 1 || k > kTriMax || !alpha || (k > 1 && !beta)) return 1;
  double big = 0.0;
  for (int i = 0; i < k; ++i) { if (!std::isfinite(alpha[i])) return 1; big = std::fmax(big, std::fabs(alpha[i])); }
  for (int i = 0; i + 1 < k; ++i) { if (!std::isfinite(beta[i])) return 1; big = std::fmax(big, std::fabs(beta[i])); }
  if (big == 0.0) {
    *theta_min = 0.0; *theta_max = 0.0;
    for (int i = 0; i < k; ++i) s_out[i] = i == 0 ? 1.0 : 0.0;
    return 0;
  }
  int ex = 0;
  (void)std::frexp(big, &ex);   // big = f * 2^ex, f in [0.5, 1): the scaled entries are below 1 in magnitude
  double a[kTriMax], b[kTriMax];
  for (int i = 0; i < k; ++i) a[i] = std::ldexp(alpha[i], -ex);
  for (int i = 0; i + 1 < k; ++i) b[i] = std::ldexp(beta[i], -ex);
  b[k - 1] = 0.0;
  // Gershgorin: every eigenvalue of the scaled matrix lies in [-3, 3]
  const double glo = -4.0, ghi = 4.0;
  double tmax_h = glo;
  // the blocks between exact zeros of the off-diagonal: the extreme eigenvalues of each, the first block that attains the minimum
  int best_lo = 0, best_hi = k;
  double best_l = 0.0, best_h = 0.0;
  bool have = false;
  for (int lo = 0; lo < k;) {
    int hi = lo + 1;
    while (hi < k && b[hi - 1] != 0.0) ++hi;
    double l, h;
    tri_detail::bisect(a, b, lo, hi, 0, glo, ghi, &l, &h);
    if (!have || h < best_h) { have = true; best_lo = lo; best_hi = hi; best_l = l; best_h = h; }
    tri_detail::bisect(a, b, lo, hi, hi - lo - 1, glo, ghi, &l, &h);
    tmax_h = std::fmax(tmax_h, h);
    lo = hi;
  }
  *theta_min = std::ldexp(best_h, ex);
  *theta_max = std::ldexp(tmax_h, ex);
  // inverse iteration in the block at the shift best_l (count = 0: positive pivots)
  for (int i = 0; i < k; ++i) s_out[i] = 0.0;
  const int lo = best_lo, nb = best_hi - best_lo;
  double q[kTriMax], x[kTriMax];
  const double kFloor = std::ldexp(1.0, -100);
  {
    double prev = 1.0;
    for (int i = 0; i < nb; ++i) {
      const double off = i > 0 ? b[lo + i - 1] : 0.0;
      double v = (a[lo + i] - best_l) - (i > 0 ? (off * off) / prev : 0.0);
      if (!(v > kFloor)) v = kFloor;   // a pivot that rounding took to zero or below: far under one ulp of the scaled ||T||
      q[i] = prev = v;
    }
    double sgn = 1.0;
    for (int i = 0; i < nb; ++i) {
      if (i > 0 && b[lo + i - 1] > 0.0) sgn = -sgn;
      x[i] = sgn * (1.0 + 0.25 * (double)((i * 37) % 16) / 16.0);
    }
  }
  for (int it = 0; it < 4; ++it) {
    // the right-hand side has norm 2^-500, a pivot is 2^-100 at least: a chain of fifteen floored pivots still stays finite
    double nrm = 0.0;
    for (int i = 0; i < nb; ++i) nrm = std::fmax(nrm, std::fabs(x[i]));
    if (!(nrm > 0.0)) { x[0] = 1.0; nrm = 1.0; }
    for (int i = 0; i < nb; ++i) x[i] = std::ldexp(x[i] / nrm, -500);
    for (int i = 1; i < nb; ++i) x[i] = x[i] - (b[lo + i - 1] / q[i - 1]) * x[i - 1];
    for (int i = 0; i < nb; ++i) x[i] = x[i] / q[i];
    for (int i = nb - 2; i >= 0; --i) x[i] = x[i] - (b[lo + i] / q[i]) * x[i + 1];
    bool fin = true;
    for (int i = 0; i < nb; ++i) fin = fin && std::isfinite(x[i]);
    if (!fin) return 2;
  }
  double mx = 0.0;
  int imx = 0;
  for (int i = 0; i < nb; ++i) if (std::fabs(x[i]) > mx) { mx = std::fabs(x[i]); imx = i; }
  if (!(mx > 0.0)) { x[0] = 1.0; mx = 1.0; imx = 0; }
  const double flip = x[imx] < 0.0 ? -1.0 : 1.0;
  double ss = 0.0;
  for (int i = 0; i < nb; ++i) { x[i] = flip * (x[i] / mx); ss += x[i] * x[i]; }
  const double inv = 1.0 / std::sqrt(ss);
  for (int i = 0; i < nb; ++i) s_out[lo + i] = x[i] * inv;
  return 0;
}

}  // namespace okkt
