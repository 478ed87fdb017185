// All eigenvalues and eigenvectors of a dense symmetric matrix of order m <= 128: the host side of the block Krylov-Schur method of
// okkt_eigs (api_eigs.cpp), which runs it on the projected matrix G = V' Op V after every sweep.  Header-only,
// no device code, no allocation: okkt_debug_sym_eig exports it and the host sanitizer driver calls it.
//
// Cyclic Jacobi by rows: a sweep visits the pairs (p, q), p < q, in the order p = 0 .. m-2, q = p+1 .. m-1, which depends on m alone.
// A pair is rotated when |a_pq| exceeds the threshold 2^-54 ||A||_F / m; the iteration ends with the first sweep that rotates nothing,
// i.e. when off(A) <= 2^-54 ||A||_F, or after kSymEigSweeps sweeps (return code 2).  Only the upper triangle of the input is read.
//
// Error.  A rotation is computed to a few units of roundoff u = 2^-53 and a sweep is m - 1 sets of disjoint rotations; each set
// perturbs A backward by at most 6 u ||A||_2 (Wilkinson, The Algebraic Eigenvalue Problem, ch. 3 sections 20-25, two-sided application),
// a sweep by 6 (m - 1) u ||A||_2 = 3 (m - 1) 2^-52 ||A||_2, and the entries left behind add sqrt(m) 2^-54 ||A||_2 at most.  With at most
// kSymEigSweeps = 20 sweeps every eigenvalue is within 61 m 2^-52 ||A||_2 of a true one, and ||S'S - I||_2 obeys a bound of the same form
// (the accumulated rotations carry the same 6 u per set).  Measured errors are a few units of 2^-52 ||A||_2.
//
// Output order: |theta| descending; of two values of equal modulus the positive one first; equal values keep the order of their
// diagonal positions.  Column j of S (s[i * m + j], row-major) is the unit eigenvector of theta[j].
#pragma once
#include <cmath>
#include <cstdint>

namespace okkt {

constexpr int kSymEigMax = 128;
constexpr int kSymEigSweeps = 20;

// Returns 0; 1 when m is out of range, a pointer is NULL or an entry of the upper triangle is not finite (the outputs are then
// untouched); 2 when kSymEigSweeps sweeps did not bring every off-diagonal entry under the threshold (the outputs hold the current
// diagonal and rotations).  a: m x m, row-major, leading dimension lda >= m (not modified).  theta: m.  s: m x m, row-major.
// work: m x m doubles.
inline int sym_eig(int m, const double* a, int lda, double* theta, double* s, double* work) {
  if (m < 1 || m > kSymEigMax || !a || !theta || !s || !work || lda < m) return 1;
  double fro2 = 0.0;
  for (int i = 0; i < m; ++i)
    for (int j = i; j < m; ++j) {
      const double v = a[(size_t)i * lda + j];
      if (!std::isfinite(v)) return 1;
    }
  // scale by a power of two so that the squares neither overflow nor vanish
  double big = 0.0;
  for (int i = 0; i < m; ++i)
    for (int j = i; j < m; ++j) big = std::fmax(big, std::fabs(a[(size_t)i * lda + j]));
  int ex = 0;
  if (big > 0.0) (void)std::frexp(big, &ex);
  double* A = work;
  for (int i = 0; i < m; ++i)
    for (int j = i; j < m; ++j) {
      const double v = std::ldexp(a[(size_t)i * lda + j], -ex);
      A[(size_t)i * m + j] = v;
      A[(size_t)j * m + i] = v;
      fro2 += (i == j ? 1.0 : 2.0) * v * v;
    }
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) s[(size_t)i * m + j] = i == j ? 1.0 : 0.0;
  const double thr = std::ldexp(std::sqrt(fro2), -54) / (double)m;
  int rc = big > 0.0 && m > 1 ? 2 : 0;
  for (int sweep = 0; sweep < kSymEigSweeps && rc == 2; ++sweep) {
    int rotated = 0;
    for (int p = 0; p + 1 < m; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = A[(size_t)p * m + q];
        if (!(std::fabs(apq) > thr)) continue;
        ++rotated;
        const double app = A[(size_t)p * m + p], aqq = A[(size_t)q * m + q];
        // tan of the rotation angle: the smaller root of t^2 + 2 zeta t - 1 = 0 (Rutishauser)
        const double zeta = (aqq - app) / (2.0 * apq);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), sn = t * c;
        for (int k = 0; k < m; ++k) {   // columns p and q
          const double akp = A[(size_t)k * m + p], akq = A[(size_t)k * m + q];
          A[(size_t)k * m + p] = c * akp - sn * akq;
          A[(size_t)k * m + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < m; ++k) {   // rows p and q
          const double apk = A[(size_t)p * m + k], aqk = A[(size_t)q * m + k];
          A[(size_t)p * m + k] = c * apk - sn * aqk;
          A[(size_t)q * m + k] = sn * apk + c * aqk;
        }
        A[(size_t)p * m + q] = 0.0;
        A[(size_t)q * m + p] = 0.0;
        for (int k = 0; k < m; ++k) {
          const double skp = s[(size_t)k * m + p], skq = s[(size_t)k * m + q];
          s[(size_t)k * m + p] = c * skp - sn * skq;
          s[(size_t)k * m + q] = sn * skp + c * skq;
        }
      }
    if (rotated == 0) rc = 0;
  }
  // the order of the output: insertion sort of the positions (stable), then the columns of S permuted through the work matrix
  int ord[kSymEigMax];
  double d[kSymEigMax];
  for (int i = 0; i < m; ++i) { d[i] = std::ldexp(A[(size_t)i * m + i], ex); ord[i] = i; }
  auto before = [&](int x, int y) {   // x strictly before y
    const double ax = std::fabs(d[x]), ay = std::fabs(d[y]);
    if (ax != ay) return ax > ay;
    return d[x] > d[y];
  };
  for (int i = 1; i < m; ++i) {
    const int x = ord[i];
    int j = i;
    while (j > 0 && before(x, ord[j - 1])) { ord[j] = ord[j - 1]; --j; }
    ord[j] = x;
  }
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) A[(size_t)i * m + j] = s[(size_t)i * m + ord[j]];
  for (int i = 0; i < m * m; ++i) s[i] = A[i];
  for (int j = 0; j < m; ++j) theta[j] = d[ord[j]];
  return rc;
}

}  // namespace okkt
