// Symmetric equilibration before the static-pivot factorisation (scaling.hip): F~ = S F S with a positive
// diagonal S, computed on the device by Jacobi sweeps of Ruiz's infinity-norm iteration over the refinement's row map and rounded to
// powers of two, or given by the caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/okkt.h"
#include "refine.h"

namespace okkt {

constexpr int kScaleDefaultSweeps = 10;
constexpr int kScaleMaxSweeps = 64;
constexpr int kScaleExpMax = 510;      // exponents of the rounded scaling are clamped to [-510, 510]
constexpr int kScaleOut = 4;           // the small read of a factorisation: rowmax_min, rowmax_max, zero_rows, rows with a non-zero maximum

struct ScalingWork {
  // configuration (okkt_set_scaling): kept across analyses
  int mode = OKKT_SCALE_NONE;
  int sweeps = kScaleDefaultSweeps;
  std::vector<double> user;      // USER: the caller's vector, original order
  // device state of one analysis (scaling_alloc / scaling_release)
  bool ready = false;
  int64_t n = 0, nnz_in = 0;
  double* s[2] = {nullptr, nullptr};   // the two buffers the sweeps alternate between
  double* rmax = nullptr;              // [n] row maxima of |S F S| with the final s
  int* expo = nullptr;                 // [n] e_i of the rounded s_i = 2^e_i (RUIZ)
  double* shift = nullptr;             // [n] the factorisation's diagonal shift, original order
  double* dadd = nullptr;              // [n] the scaled shift s_i^2 diagadd_i, permuted order (what the scaled assembly adds)
  int *erow = nullptr, *ecol = nullptr;   // [nnz_in] row and column of every input entry
  double* vals = nullptr;              // [nnz_in] the scaled values the factorisation reads
  double* part = nullptr;              // per-workgroup partials of the extrema, kScaleOut each
  double* out = nullptr;               // [kScaleOut]
  int64_t nb_part = 0;
  bool user_uploaded = false;          // s[0] holds `user`
  std::vector<void*> allocs;
  // the current factor
  bool valid = false;                  // the handle's factor is that of S F S with s_cur
  double* s_cur = nullptr;             // the scaling of the current factor (one of s[0], s[1])
  okkt_scaling_info info = {0, 0, 0.0, 0.0, 0};
};

// host work and allocation (first scaled factorisation after an analysis): the per-entry indices from the analysed pattern
std::string scaling_alloc(ScalingWork& W, int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t base);
void scaling_release(ScalingWork& W);     // device state only: the configuration stays
// enqueue functions: no allocation, no synchronisation.
// The whole scaling phase of one factorisation: the shift to original order, the values gathered into M's row order (d_nzval: the
// caller's values), the sweeps (RUIZ) and the rounding, the row maxima with the final s and their extrema into W.out, the scaled
// values into W.vals and the scaled shift into W.dadd.  W.s_cur is the scaling afterwards.
void scaling_enqueue(ScalingWork& W, const RefineMap& M, const double* d_nzval, const double* diagadd_perm, const int* perm, hipStream_t st);

}  // namespace okkt
