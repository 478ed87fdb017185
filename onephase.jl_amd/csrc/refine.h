// Extra-precise residuals for iterative refinement (refine.hip): r = b - A x in double-double for the symmetric matrix
// whose lower triangle the analysed CSC holds, the denominators (|A||x| + |b|)_i and the componentwise backward error.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace okkt {

// Row-wise full-symmetric map of the caller's input pattern (built on the first residual / refine call after an analysis).
// Every (row, column) pair of the symmetric matrix is one entry; its value is gathered from nzval through src (the first
// input entry of the pair) and, for pairs that the input lists more than once, summed in input order by the dup lists.
struct RefineMap {
  bool ready = false;
  int64_t n = 0, nnz = 0, nnz_in = 0;
  int64_t* rowptr = nullptr;   // [n + 1]
  int* col = nullptr;          // [nnz]
  int64_t* src = nullptr;      // [nnz] index into nzval
  double* vals = nullptr;      // [nnz] the values of one call, row order (the 8-byte-per-entry workspace)
  int64_t ndup = 0;            // entries whose value is a sum of several input entries
  int64_t *dup_e = nullptr, *dup_ptr = nullptr, *dup_src = nullptr;
  int lpr = 4;                 // lanes per short row
  int64_t long_min = 0;        // rows with more entries than this get a workgroup each
  int64_t nb_short = 0, nlong = 0;
  int* long_rows = nullptr;    // [nlong]
  double* part = nullptr;      // per-workgroup partial maxima: [(nb_short + nlong) * 8]
  double* nz_stage = nullptr;  // [nnz_in] host-side nzval staging (host entry points only, allocated on first use)
  std::vector<void*> allocs;
};

// one batch of up to four right-hand sides; om[q] receives (omega, ||r||_inf)
struct ResidSet {
  const double* b[4];
  const double* x[4];
  double* r[4];
  double* om[4];
};
// optional per-row denominators (|A||x|)_i + |b_i| of the same pass (refine_residual_den_enqueue)
struct DenSet {
  double* d[4];
};
// masked correction: xp[q] = x[q]; x[q] += d[q]
struct UpdateSet {
  double* x[4];
  double* xp[4];
  const double* d[4];
};

// host work and uploads (hipMalloc): not an enqueue function
std::string refine_map_build(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t base, RefineMap& M);
std::string refine_stage_alloc(RefineMap& M);
void refine_map_release(RefineMap& M);
// enqueue functions: no allocation, no synchronisation
void refine_gather_enqueue(const RefineMap& M, const double* d_nzval, hipStream_t st);
void refine_residual_enqueue(const RefineMap& M, const ResidSet& S, int nr, hipStream_t st);
// the same pass, storing the denominators as well (r and omega bitwise as refine_residual_enqueue gives them)
void refine_residual_den_enqueue(const RefineMap& M, const ResidSet& S, const DenSet& D, int nr, hipStream_t st);
void refine_update_enqueue(int64_t n, const UpdateSet& U, int nr, hipStream_t st);

}  // namespace okkt
