// The factor as an operator (factor_ops.hip): y = L x, y = L^T x, L D L^T x and |L||D||L^T||x| from the stored
// panels, the copies that stop and restart a solve between its two sweeps, the quadratic form z' D z, and the device work of
// okkt_factor_error.  The state lives on the solver handle (FactorOpsWork), not in DevPlan: the factorisation and solve kernels are
// unchanged by it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "numeric.h"
#include "symbolic.h"

namespace okkt {

constexpr int kFoThreads = 256;        // workgroup of the big-front kernels and of the vector passes
constexpr int kFoSmallMax = 136;       // largest front order of the one-wave kernels (the clamp of Numeric::small_max)
constexpr int kFoLtCols = 8;           // L^T x, big fronts: pivot columns per work item ...
constexpr int kFoLtRows = 1024;        // ... and front rows per work item (the gathered x of the rows sits in LDS: 4 x 1024 doubles)
constexpr int kFoLRows = 256;          // L x, big fronts: front rows per work item (one per thread) ...
constexpr int kFoLCols = 512;          // ... and pivot columns per work item (their x sits in LDS: 4 x 512 doubles)
constexpr int kFoRedBlocks = 256;      // partial records of the reductions (quadratic form, factor error)
constexpr int kFoMaxProbes = 8;

// a small front (f <= small_max): one wave
struct FoSmall { int64_t L; int64_t rows; int f, k, col0, s; };
static_assert(sizeof(FoSmall) == 32, "host and device agree on the record");
// L^T x, big fronts: columns [c0, c0 + nc) of the front at L against front rows [r0, r1); column c0 + i writes partial record part + i * nch
struct FoLtBig { int64_t L; int64_t rows; int f, c0, nc, r0, r1, nch; int64_t part; };
static_assert(sizeof(FoLtBig) == 48, "host and device agree on the record");
// ... and the sum of a column's nch partial records (ascending rows), plus x itself (the unit diagonal)
struct FoLtMerge { int64_t part; int out, nch; };
static_assert(sizeof(FoLtMerge) == 16, "host and device agree on the record");
// L x, big fronts: rows [r0, r1) of the front at L against its pivot columns [c0, c0 + nc); row i writes partial part + i
struct FoLBig { int64_t L; int64_t part; int f, col0, c0, nc, r0, r1; };
static_assert(sizeof(FoLBig) == 40, "host and device agree on the record");
// ... and per block of rows: v itself on the pivot rows, the column blocks' partials in ascending order, then the children's
// contribution vectors through the inverted extend-add lists (DevPlan::ea_ptr / ea_pos from gcb on); pivot rows go to y, the rows
// below to the front's contribution vector at cv
struct FoLMerge { int64_t part; int64_t gcb; int64_t cv; int f, k, col0, r0; };
static_assert(sizeof(FoLMerge) == 40, "host and device agree on the record");

// the work-item lists of one analysis (host side; plain C++, run under the sanitizers by asan_driver.cpp)
struct FoPlan {
  std::vector<FoSmall> small;            // by level of the supernodal tree, ascending
  std::vector<FoLtBig> lt_big;
  std::vector<FoLtMerge> lt_merge;
  std::vector<FoLBig> l_big;             // by level
  std::vector<FoLMerge> l_merge;         // by level
  std::vector<int64_t> small_off, l_big_off, l_merge_off;   // [nlevels + 1] the levels' ranges in the three lists
  int64_t lt_parts = 0;                  // partial records of L^T x
  int64_t l_parts = 0;                   // partial sums of L x: the largest level's
  int64_t entries = 0;                   // entries of L below the diagonal that one product reads
};

// front_pos: the panel bases (Numeric::front_pos_host); bigcol_base: DevPlan::bigcol_base (the first extend-add list of a front, -1
// where it has none).  Returns "" or an error message.
inline std::string factor_ops_build_plan(const Symbolic& S, const std::vector<int64_t>& front_pos, const std::vector<int64_t>& bigcol_base, int small_max, FoPlan& P) {
  P = FoPlan();
  if ((int64_t)front_pos.size() < (int64_t)S.nsuper || (int64_t)bigcol_base.size() < (int64_t)S.nsuper) return "factor products: the panel bases do not cover the supernodes";
  if (small_max > kFoSmallMax) return "factor products: small_front_max is beyond the one-wave kernels";
  P.small_off.assign((size_t)S.nlevels + 1, 0);
  P.l_big_off.assign((size_t)S.nlevels + 1, 0);
  P.l_merge_off.assign((size_t)S.nlevels + 1, 0);
  for (int l = 0; l < S.nlevels; ++l) {
    int64_t lparts = 0;
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; ++q) {
      const int s = S.level_sn[q];
      const int64_t f64 = S.row_ptr[s + 1] - S.row_ptr[s];
      const int col0 = S.sn_col0[s], k = S.sn_col0[s + 1] - col0;
      if (f64 > INT32_MAX || k > f64 || k < 1) return "factor products: a front's shape is out of range";
      const int f = (int)f64;
      P.entries += (int64_t)f * k - (int64_t)k * (k + 1) / 2;
      if (f <= small_max) {
        P.small.push_back({front_pos[s], S.row_ptr[s], f, k, col0, s});
        continue;
      }
      if (bigcol_base[s] < 0) return "factor products: a front above small_front_max has no extend-add lists";
      // L^T x: groups of kFoLtCols columns, the rows below the group's first column in chunks of kFoLtRows
      for (int c0 = 0; c0 < k; c0 += kFoLtCols) {
        const int nc = std::min(kFoLtCols, k - c0);
        const int nch = std::max(1, (f - (c0 + 1) + kFoLtRows - 1) / kFoLtRows);
        for (int ch = 0; ch < nch; ++ch) {
          const int r0 = c0 + 1 + ch * kFoLtRows;
          P.lt_big.push_back({front_pos[s], S.row_ptr[s], f, c0, nc, std::min(r0, f), std::min(f, r0 + kFoLtRows), nch, P.lt_parts + ch});
        }
        for (int i = 0; i < nc; ++i) P.lt_merge.push_back({P.lt_parts + (int64_t)i * nch, col0 + c0 + i, nch});
        P.lt_parts += (int64_t)nc * nch;
      }
      // L x: blocks of kFoLRows rows against blocks of kFoLCols columns; a block that lies on or above the diagonal is left out
      const int ncb = (k + kFoLCols - 1) / kFoLCols;
      for (int r0 = 0; r0 < f; r0 += kFoLRows) {
        const int r1 = std::min(f, r0 + kFoLRows);
        for (int cb = 0; cb < ncb; ++cb) {
          const int c0 = cb * kFoLCols;
          if (r1 - 1 <= c0) break;
          P.l_big.push_back({front_pos[s], lparts + (int64_t)cb * f, f, col0, c0, std::min(kFoLCols, k - c0), r0, r1});
        }
        P.l_merge.push_back({lparts, bigcol_base[s], S.cv_pos[s], f, k, col0, r0});
      }
      lparts += (int64_t)ncb * f;
    }
    P.l_parts = std::max(P.l_parts, lparts);
    P.small_off[(size_t)l + 1] = (int64_t)P.small.size();
    P.l_big_off[(size_t)l + 1] = (int64_t)P.l_big.size();
    P.l_merge_off[(size_t)l + 1] = (int64_t)P.l_merge.size();
  }
  if ((int64_t)P.lt_big.size() > INT32_MAX || (int64_t)P.l_big.size() > INT32_MAX || (int64_t)P.small.size() > INT32_MAX)
    return "factor products: too many work items for one launch";
  return "";
}

// per block of the reductions
struct FoQuad { double pos_h[4], pos_l[4], neg_h[4], neg_l[4]; };
struct FoErr { double eta, norm_f, norm_a; long long row; };

struct FactorOpsWork {
  bool planned = false;
  int64_t analysis = -1;          // okkt_solver_s::n_analyze_calls the lists belong to
  const double* arena = nullptr;  // ... and the front arena (a new device plan gets a new one)
  int64_t n = 0, bytes = 0;
  int nlevels = 0;
  std::vector<int64_t> small_off, l_big_off, l_merge_off;
  int64_t n_small = 0, n_lt_big = 0, n_lt_merge = 0;
  FoSmall* small = nullptr;
  FoLtBig* lt_big = nullptr;
  FoLtMerge* lt_merge = nullptr;
  FoLBig* l_big = nullptr;
  FoLMerge* l_merge = nullptr;
  double* lt_part = nullptr;      // [4][lt_parts]
  double* l_part = nullptr;       // [4][l_parts]
  int64_t lt_parts = 0, l_parts = 0;
  double* wa = nullptr;           // [4][n] vectors in factor order: the operand of a product ...
  double* wb = nullptr;           // [4][n] ... and its result
  FoQuad* quad = nullptr;         // [kFoRedBlocks + 1] partial records of the quadratic form, then the result
  // okkt_factor_error: allocated on its first call
  double* ev = nullptr;           // 17 blocks of n doubles (their layout: factor_ops_error_init below)
  double* eom = nullptr;          // (omega, |r|) pairs of the residual passes (not used further)
  FoErr* err = nullptr;           // [kFoRedBlocks] per-block records of a batch of probes
  std::vector<void*> allocs;
};

// host lists and allocations for the current analysis
std::string factor_ops_setup(const Symbolic& S, const Numeric& N, FactorOpsWork& W);
std::string factor_ops_error_alloc(FactorOpsWork& W);
void factor_ops_release(FactorOpsWork& W);

// Everything below is enqueued on N.stream (no allocation, no synchronisation).  R = 1, 2 or 4 columns are carried, nr <= R of them the
// caller's; the others are zero.
// z of the forward sweep (DevPlan::zwork) -> d_z (factor order, columns `stride` apart) / back, the columns beyond nr zero
void factor_ops_z_out(const Numeric& N, double* d_z, int64_t stride, int nr);
void factor_ops_z_in(const Numeric& N, const double* d_z, int64_t stride, int nr, int R);
// q[r] = (sum over d_j > 0, sum over d_j < 0) of d_j z_j^2 for the z in zwork, into W.quad[kFoRedBlocks] (pos_h / neg_h)
void factor_ops_quadform(const Numeric& N, FactorOpsWork& W, int nr);
// dst[q][j] (W.wa or W.wb) = x[q][j] (perm = false, factor order) or x[q][perm[j]] / s[perm[j]] (perm = true; d_scale NULL: no
// division); abs: |.|
void factor_ops_load(const Numeric& N, FactorOpsWork& W, double* dst, const double* d_x, int64_t stride, int nr, int R, bool perm, const double* d_scale, bool abs);
// the reverse from `src` (W.wa or W.wb)
void factor_ops_store(const Numeric& N, const FactorOpsWork& W, const double* src, double* d_y, int64_t stride, int nr, bool perm, const double* d_scale);
// W.wb = L^T W.wa / W.wa = L W.wb (abs: with |L|); W.wb = D W.wb (abs: |D|)
std::string factor_ops_lt(const Numeric& N, FactorOpsWork& W, int R, bool abs);
std::string factor_ops_l(const Numeric& N, FactorOpsWork& W, int R, bool abs);
void factor_ops_d(const Numeric& N, FactorOpsWork& W, int R, bool abs);
// okkt_factor_error, the layout of W.ev in blocks of n doubles: 0 ones, 1 zeros, 2 |F0| e (F0: the values without the factorisation's
// diagonal shift), 3 ABS_LDLT e, 4 scratch, 5 .. 8 the probes of a batch, 9 .. 12 their LDLT products, 13 .. 16 the differences
// LDLT v - F0 v.  init: ones, zeros and the probes p0 .. p0 + np - 1 (entry i of probe p: fo_probe(p, i), i the original index)
void factor_ops_error_init(FactorOpsWork& W, int p0, int np, hipStream_t st);
// per block, into W.err: max over the batch's np probes and the rows of |shift v - dif| / (|F0| e + |shift| + ABS e) by (value, lowest
// row), max of |F0| e + |shift|, max of ABS e
void factor_ops_error_reduce(const Numeric& N, FactorOpsWork& W, int np, hipStream_t st);

__host__ __device__ inline uint64_t fo_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline double fo_probe(int p, int64_t i) { return (fo_mix(((uint64_t)p << 32) ^ (uint64_t)i) >> 63) ? -1.0 : 1.0; }

}  // namespace okkt
