// Dense symmetric-indefinite factorisation of the Schur complement and its solves (dense_ldlt.hip):
// P S P' = L D L' with Bunch-Kaufman partial pivoting (alpha = (1 + sqrt 17) / 8, the pivot choice of LAPACK's dsytrf, lower variant),
// L unit lower triangular, D block diagonal with 1 x 1 and 2 x 2 blocks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace okkt {

constexpr int kDlNB = 32;       // panel width (a panel ends one column early rather than split a 2 x 2 pivot)
constexpr int kDlSB = 64;       // block of the substitutions
constexpr int kDlIB = 32;       // block of the inverse (a block ends one column early rather than split a 2 x 2 pivot)
static_assert(kDlIB <= kDlNB, "the inverse keeps W_j of one block step in the panel buffer W");

// what the panel kernel leaves for the launches behind it and for the host
struct DenseLdltState {
  int next;                     // first column not yet eliminated
  int j0;                       // first column of the panel eliminated last
  long long cnt[4];             // pivots: positive, negative, zero, non-finite
};

struct DenseLdltWork {
  int64_t ns = 0;
  double* F = nullptr;          // ns x ns, column-major: unit L below the diagonal with EVERY interchange applied to every column, D on it
  double* W = nullptr;          // ns x kDlNB: L D of the current panel
  double* X = nullptr;          // 3 x 4 x ns: the solves' two work vectors for up to four right-hand sides, r2 / x2 of the fused solve
  int* ipiv = nullptr;          // dsytrf's convention, 1-based
  int* ptype = nullptr;         // 0: 1 x 1 pivot, 1 / 2: first / second column of a 2 x 2 pivot
  int* perm = nullptr;          // row i of P S P' is row perm[i] of S
  DenseLdltState* st = nullptr;
  // the inverse, allocated by the first dense_ldlt_inverse_enqueue
  double* Zt = nullptr;         // ns x ns: the inverse of P S P', both triangles
  double* Pt = nullptr;         // one kDlIB x kDlIB part of W_j' Z_Bj per 16 rows below the block
  int* blk = nullptr;           // [0]: number of blocks nb, [1 + j]: first column of block j, [1 + nb]: ns
  unsigned long long* nonfinite = nullptr;   // non-finite entries of the inverse handed out last
  bool valid = false;           // a factorisation completed
  bool own = false;             // it is of the S the handle assembled (stale after the next okkt_factor_schur)
  int64_t factor_seq = 0;       // the handle's factor_seq it was made at
  long long cnt[4] = {0, 0, 0, 0};
  int64_t seq = 0;              // the handle's count of okkt_schur_factor calls it was made at
  long long inv_nonfinite = 0;  // non-finite entries of the inverse okkt_schur_get_inverse handed out last
};

std::string dense_ldlt_alloc(DenseLdltWork& D, int64_t ns);
void dense_ldlt_release(DenseLdltWork& D);
// factor the lower triangle held in D.F (leading dimension ns) in place; counts -> D.cnt (synchronises the stream)
std::string dense_ldlt_factor(DenseLdltWork& D, hipStream_t st);
// x2 (ns x nr, leading dimension ns) = S^-1 r2; R = 1, 2 or 4 right-hand sides travel together (nr <= R).  r2 may alias x2
std::string dense_ldlt_solve_enqueue(DenseLdltWork& D, const double* d_r2, double* d_x2, int nr, int R, hipStream_t st);
// Z (ns x ns, leading dimension ld >= ns, both triangles, bitwise mirror images) = S^-1 from the stored factor; the number of its
// non-finite entries is left in D.nonfinite (device).  The panel buffer D.W is overwritten.  No synchronisation
std::string dense_ldlt_inverse_enqueue(DenseLdltWork& D, double* d_Z, int64_t ld, hipStream_t st);

}  // namespace okkt
