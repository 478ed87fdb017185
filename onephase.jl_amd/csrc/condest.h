// Condition estimation and forward error bounds (condest.hip): the device work of the Higham-Tisseur
// block 1-norm estimator around the multi-right-hand-side solves (api_condest.cpp drives it from the host).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "refine.h"

namespace okkt {

constexpr int kCondestMaxT = 4;     // columns of the estimator's block (one solve pass carries them all)
constexpr int kCondestItmax = 5;

// Layout of the small read-back buffer `out` (doubles)
constexpr int kCdY = 0;        // after Y: [0, 4) column 1-norms, [4] non-finite flag, [5, 21) S'S, [21, 37) S'S_old, [37, 53) S(0:4, :)
constexpr int kCdZ = 64;       // after Z: [64, 68) top values, [68, 72) their rows, [72, 76) top unused values, [76, 80) rows,
                               //          [80] h(ind_best), [81] non-finite flag
constexpr int kCdN = 96;       // [96] ||F||_1, [97] non-finite flag of F, [98] ||x||_inf (forward error)
constexpr int kCdOut = 128;

struct CondestWork {
  int64_t n = 0, nb = 0;       // rows, 256-row blocks of the row kernels
  double* X = nullptr;         // [4 n] the block the next Y = op X is formed from
  double* Y = nullptr;         // [4 n] Y, then Z (the solve output)
  double* S[2] = {nullptr, nullptr};   // [4 n] sign blocks: the current one and the previous one
  double* SF = nullptr;        // [4 n] diag(f) S: the right-hand sides of Z (forward-error operator only)
  double* R = nullptr;         // [4 n] residuals of a batch (forward error)
  double* DEN = nullptr;       // [4 n] their denominators (|A||x| + |b|)
  double* f = nullptr;         // [n] forward-error weights
  double* shift = nullptr;     // [n] diagonal shift of the factorisation, original order
  uint32_t* used = nullptr;    // [(n + 31) / 32] bitmap of the unit vectors already used
  double* part = nullptr;      // [nb * 40] per-block partials
  double* out = nullptr;       // [kCdOut] device side of the read-back buffer
  std::vector<void*> allocs;
};

// The fixed generator of the +-1 columns: entry i of the column of draw d and head class c.  Rows 0 .. H-1 (H = min(n, 4)) carry
// the class: row 0 is +1, row r >= 1 is -1 exactly when bit r-1 of c is set; two columns of different classes are never parallel.
// Rows i >= H: the sign bit of splitmix64's finaliser of (d << 32) ^ i.
__host__ __device__ inline uint64_t cd_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline double cd_sign(uint64_t draw, int cls, int64_t i, int64_t H) {
  if (i < H) return (i == 0 || !((cls >> (i - 1)) & 1)) ? 1.0 : -1.0;
  return (cd_mix((draw << 32) ^ (uint64_t)i) >> 63) ? -1.0 : 1.0;
}

struct CdIdx { int64_t i[4]; };

// host work and uploads (hipMalloc): not enqueue functions
std::string condest_alloc(int64_t n, CondestWork& W);
void condest_release(CondestWork& W);
// enqueue functions: no allocation, no synchronisation
// ||F||_1 into out[kCdN] (and its non-finite flag): F = the gathered values of M (refine_gather_enqueue first) + diag(shift), the
// shift taken from the factorisation's permuted diagadd
void condest_norm1_enqueue(const RefineMap& M, CondestWork& W, const double* diagadd_perm, const int* perm, hipStream_t st);
// the starting block: column 0 = 1/n, column j = generator(draw j, class j) / n
void condest_start_enqueue(CondestWork& W, int t, hipStream_t st);
// Y (= op X before the row weights): the column 1-norms of diag(f) Y, S[cur] = sign(diag(f) Y), SF = diag(f) S[cur] when f,
// the +-1 dot products within S[cur] and against S[cur ^ 1] (has_old), the first four rows of S[cur]
void condest_ystats_enqueue(CondestWork& W, int t, int cur, bool has_old, const double* f, hipStream_t st);
// column a of S[cur] (and SF) from the generator
void condest_resample_enqueue(CondestWork& W, int cur, int a, uint64_t draw, int cls, const double* f, hipStream_t st);
// Z: h_i = max_j |Z_ij|, the top t rows by (h desc, row asc), the top t of the rows not yet used, h(ind_best)
void condest_zstats_enqueue(CondestWork& W, int t, int64_t ind_best, hipStream_t st);
// X = [e_ind0 .. e_ind(t-1)], the rows marked as used
void condest_scatter_enqueue(CondestWork& W, int t, const CdIdx& ind, hipStream_t st);
// forward error: f_i = |r_i| + (nz_i + 1) eps den_i (nz_i: entries of row i of the full symmetric A), ||x||_inf into out[kCdN + 2]
void condest_fweights_enqueue(const RefineMap& M, CondestWork& W, const double* r, const double* den, const double* x, hipStream_t st);

}  // namespace okkt
