// Vector kernels of the block shift-invert Krylov-Schur method (eigs.hip): the hashed start block, the block
// Gram-Schmidt passes over the basis V, norms and scaling, the compression X = V S of a restart, the Ritz residual norms and the
// vectors of pencil mode.  No atomics: every sum runs over per-workgroup partials in an order that depends on n alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace okkt {

constexpr int kEigMaxBasis = 128;   // columns of V (max_basis of okkt_eigs)
constexpr int kEigMaxNev = 32;
constexpr int kEigMaxBlock = 4;     // = kMaxRhs of the solves: one pass over L per sweep
constexpr int kEigMaxKeep = kEigMaxNev + kEigMaxBlock;   // columns a restart keeps
constexpr int kEigRows = 512;       // rows one workgroup of a reduction pass covers (until the cap of kEigMaxWg workgroups)
constexpr int kEigMaxWg = 256;      // workgroups of a reduction pass
constexpr int kEigOut = 96;         // doubles of the small result buffer: Ritz residuals [0, 32), block norms [32, 64), true residuals [64, 96)

// The handle's workspace (allocated on the first okkt_eigs after an analysis, grown for a longer vector or a larger basis, released
// with the analysis).  Vectors of the operator have length len (nlead in pencil mode, else dim) and leading dimension ld = dim.
struct EigsWork {
  int64_t dim = 0;
  int mb = 0;                  // the basis V was allocated for
  int nb = 0;                  // workgroups of a reduction pass over len rows (set per call: a function of len alone)
  double* base = nullptr;
  double* V[2] = {nullptr, nullptr};    // the basis, [mb][dim]; a restart compresses from one into the other
  double* OV[2] = {nullptr, nullptr};   // Op V, the same way
  double* Q = nullptr;         // the next block, [4][dim]
  double* P = nullptr;         // pencil mode: the padded right-hand sides [4][dim]; the right-hand sides lambda B v of the residuals
  double* Y = nullptr;         // pencil mode: the solutions [4][dim]; the residuals
  double* X = nullptr;         // the returned vectors, [32][dim]
  double* part = nullptr;      // per-workgroup partials: [(mb * 4 + 32)][kEigMaxWg]
  double* c1 = nullptr;        // coefficients [mb][4]: V' W, the projected matrix's new columns and the first Gram-Schmidt pass
  double* c2 = nullptr;        // the second pass
  double* sd = nullptr;        // S of the host's eigen-solver, [mb][kEigMaxKeep]
  double* out = nullptr;       // norms and residual norms, [kEigOut]
  int64_t bytes = 0;
};

std::string eigs_alloc(int64_t dim, int mb, EigsWork& W);
void eigs_release(EigsWork& W);
inline int eigs_workgroups(int64_t len) {
  const int64_t nb = (len + kEigRows - 1) / kEigRows;
  return (int)(nb < 1 ? 1 : (nb > kEigMaxWg ? kEigMaxWg : nb));
}
// the start vector's entry: splitmix64 of (seed, column, row) mapped to an odd multiple of 2^-53 in (-1, 1)
__host__ __device__ inline uint64_t eigs_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// enqueue functions: no allocation, no synchronisation.  Columns have leading dimension W.dim; len rows take part.
// dst[c][i] = hash(seed, col0 + c, i), c < p
void eigs_fill_enqueue(const EigsWork& W, int64_t len, double* dst, int p, uint64_t seed, uint64_t col0, hipStream_t st);
// c1 = V' Wc for nv basis vectors and p columns (each basis vector read once for all p columns); c1[v * 4 + c]
void eigs_project_enqueue(const EigsWork& W, int64_t len, const double* V, int nv, const double* Wc, int p, hipStream_t st);
// Wc -= V c1, then c2 = V' Wc
void eigs_orth_project_enqueue(const EigsWork& W, int64_t len, const double* V, int nv, double* Wc, int p, hipStream_t st);
// Wc -= V c2 (nv = 0: nothing subtracted), then out[off + c] = ||Wc_c||_2
void eigs_orth_norm_enqueue(const EigsWork& W, int64_t len, const double* V, int nv, double* Wc, int p, int off, hipStream_t st);
// dst = src / out[off]
void eigs_scale_enqueue(const EigsWork& W, int64_t len, const double* src, double* dst, int off, hipStream_t st);
// out-of-place X = V S for the first keep columns of sd (leading dimension kEigMaxKeep), m basis vectors; cnt (1 or 2) pairs (in, out)
void eigs_compress_enqueue(const EigsWork& W, int64_t len, int m, int keep, const double* in0, double* out0, const double* in1, double* out1,
                           int cnt, hipStream_t st);
// out[j] = ||OV s_j - theta_j V s_j||_2 for j < k, s_j the columns of sd, theta at sd + kEigMaxBasis * kEigMaxKeep
void eigs_ritz_enqueue(const EigsWork& W, int64_t len, int m, int k, const double* V, const double* OV, hipStream_t st);
// pencil mode: P[c] = [x[c]; 0] (len rows of x, dim rows of P); dst[c][0 .. len) = Y[c][0 .. len)
void eigs_pad_enqueue(const EigsWork& W, int64_t len, const double* x, int p, hipStream_t st);
void eigs_restrict_enqueue(const EigsWork& W, int64_t len, double* dst, int p, hipStream_t st);
// P[c] = lam[c] * B v[c] (B = diag(I_len, 0)), c < p
struct EigsLam { double lam[4]; };
void eigs_lambda_b_enqueue(const EigsWork& W, int64_t len, const double* v, int p, const EigsLam& L, hipStream_t st);
// each of the nvec columns of v (dim rows): scaled to unit 2-norm of its leading len rows, the entry of largest modulus among them
// (lowest index among ties) positive
void eigs_finish_enqueue(const EigsWork& W, int64_t len, double* v, int nvec, hipStream_t st);

}  // namespace okkt
