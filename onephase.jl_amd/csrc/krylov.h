// Vector kernels of GMRES-based iterative refinement (krylov.hip): the Gram-Schmidt passes over the basis
// V of each active system, the norms and the combination V y.  Up to four systems share every pass; each system's sums run in an
// order that depends on n alone, so a system gives the same bits whichever slot it has and however many systems share the pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace okkt {

constexpr int kKryMaxRestart = 64;          // restart cap of okkt_solve_gmres
constexpr int kKryCol = kKryMaxRestart + 2; // doubles per system in a Hessenberg column buffer (h_0j .. h_j+1,j, padded)

// One set of up to four systems: basis vector i of the system in slot s at v[s] + i * vstride; w[s] its current vector.
struct KrySet {
  const double* v[4];
  double* w[4];
  int64_t vstride;
};
// scale: dst[s] = src[s] / *div[s] (div in device memory)
struct KryScale {
  const double* src[4];
  double* dst[4];
  const double* div[4];
};
// combine: u[s] = sum_{i < m[s]} y[s][i] v_i (i ascending)
struct KryCombine {
  const double* v[4];
  double* u[4];
  int64_t vstride;
  int m[4];
  double y[4][kKryMaxRestart];
};

// The handle's workspace (allocated on the first okkt_solve_gmres after an analysis, grown for a larger restart, released with the
// analysis).  Slots: up to four systems of one group.  V is [restart + 1][4][n]; the others are [4][n].
struct KrylovWork {
  int64_t n = 0;
  int restart = 0;             // the restart V was allocated for
  int nb = 0;                  // workgroups per system of the reduction passes (a function of n alone)
  double* V = nullptr;
  double* W = nullptr;         // the operator product A F^-1 v_j, then its orthogonalised form
  double* Z = nullptr;         // F^-1 v_j of the active systems, packed; F^-1 V y at the end of a cycle
  double* P = nullptr;         // the solve's input when the active systems are not a prefix of the slots
  double* B = nullptr;         // the group's right-hand sides
  double* R = nullptr;         // outer residuals
  double* U = nullptr;         // V y of the systems whose cycle made a correction, packed
  double* XP = nullptr;        // the iterate before the last correction
  double* zero = nullptr;      // n zeros: the right-hand side of the operator product
  double* part = nullptr;      // per-workgroup partials: [4][kKryCol][nb]
  double* h1 = nullptr;        // first Gram-Schmidt coefficients [4][kKryCol]
  double* h2 = nullptr;        // second (reorthogonalisation) coefficients [4][kKryCol]
  double* col = nullptr;       // the Hessenberg column (h1 + h2 and h_j+1,j at index nv), or the outer norm at index 0 [4][kKryCol]
  double* om = nullptr;        // (omega, |r|_inf) of the outer residual [4][2] and of the operator product [4][2]
  int64_t bytes = 0;
};

std::string krylov_alloc(int64_t n, int restart, KrylovWork& K);
void krylov_release(KrylovWork& K);

// enqueue functions: no allocation, no synchronisation.  nr systems in slots 0..nr-1 of the set.
// h1 = V^T w (neg: w holds -w and is read negated) for the nv basis vectors; ends in K.h1
void krylov_dots_enqueue(const KrylovWork& K, const KrySet& S, int nr, int nv, bool neg, hipStream_t st);
// w = (neg ? -w : w) - V h1; h2 = V^T w; ends in K.h2
void krylov_orth_dots_enqueue(const KrylovWork& K, const KrySet& S, int nr, int nv, bool neg, hipStream_t st);
// w = w - V h2; K.col[s] = h1 + h2 (nv entries) and ||w||_2 at index nv
void krylov_orth_norm_enqueue(const KrylovWork& K, const KrySet& S, int nr, int nv, hipStream_t st);
// K.col[s * kKryCol] = ||w[s]||_2 (S.v unused)
void krylov_norm_enqueue(const KrylovWork& K, const KrySet& S, int nr, hipStream_t st);
void krylov_scale_enqueue(int64_t n, const KryScale& S, int nr, hipStream_t st);
void krylov_combine_enqueue(int64_t n, const KryCombine& C, int nr, hipStream_t st);

}  // namespace okkt
