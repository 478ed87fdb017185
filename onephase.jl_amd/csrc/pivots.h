// Threshold pivot report (pivots.hip): g_j = max_i |L_ij| over the stored rows below the diagonal of every pivot
// column and the row that attains it, from one read of the factor's panels.  The state lives on the solver handle (PivotWork), not in
// DevPlan: the factorisation and solve kernels are unchanged by it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "numeric.h"
#include "symbolic.h"

namespace okkt {

constexpr int kPvThreads = 256;          // workgroup of every kernel of the report
constexpr int kPvWaves = kPvThreads / 64;   // small fronts per workgroup: one wave each
constexpr int kPvChunkRows = 2048;       // rows of a big front's column that one workgroup scans (8 rows per thread)
constexpr int kPvCountBlocks = 256;      // partial records of the count over g

// a small front (f <= small_max): one wave loops over its k columns
struct PvSmall { int64_t L; int64_t rows; int f, k, col0, pad; };
static_assert(sizeof(PvSmall) == 32, "host and device agree on the record");
// one chunk of one column of a big front: rows [r0, r1) of the column whose top (front row 0) is arena entry `col`; part < 0: the
// chunk is the whole column and writes the result, else it writes partial record `part`
struct PvBig { int64_t col; int64_t rows; int r0, r1, out, part; };
static_assert(sizeof(PvBig) == 32, "host and device agree on the record");
// a column of more than one chunk: its partial records part0 .. part0 + nparts - 1 in ascending row order
struct PvMerge { int64_t rows; int part0, nparts, out, pad; };
static_assert(sizeof(PvMerge) == 24, "host and device agree on the record");
// one block's share of the count over g
struct PvCount { long long rejected, nonfinite, max_idx; double max_g; };

// the work-item lists of one analysis (host side; plain C++, run under the sanitizers by asan_driver.cpp)
struct PvPlan {
  std::vector<PvSmall> small;
  std::vector<PvBig> big;
  std::vector<PvMerge> merge;
  int64_t nparts = 0;        // partial records
  int64_t ncols = 0;         // pivot columns covered (n - nschur)
  int64_t entries = 0;       // entries of L read
};

// front_pos: the panel bases (Numeric::front_pos_host); skip_sn: the Schur front (-1: none), which is not scanned.
// Returns "" or an error message.
inline std::string pivot_build_items(const Symbolic& S, const std::vector<int64_t>& front_pos, int small_max, int skip_sn, PvPlan& P) {
  P = PvPlan();
  if ((int64_t)front_pos.size() < (int64_t)S.nsuper) return "pivot report: the panel bases do not cover the supernodes";
  for (int s = 0; s < S.nsuper; ++s) {
    if (s == skip_sn) continue;
    const int64_t f64 = S.row_ptr[s + 1] - S.row_ptr[s];
    const int col0 = S.sn_col0[s], k = S.sn_col0[s + 1] - col0;
    if (f64 > INT32_MAX || k > f64) return "pivot report: a front's shape is out of range";
    const int f = (int)f64;
    P.ncols += k;
    P.entries += (int64_t)f * k - (int64_t)k * (k + 1) / 2;
    if (f <= small_max) {
      P.small.push_back({front_pos[s], S.row_ptr[s], f, k, col0, 0});
      continue;
    }
    for (int lc = 0; lc < k; ++lc) {
      const int64_t col = front_pos[s] + (int64_t)lc * f;     // 64-bit: lc * f passes 2^31 on the largest fronts
      const int lo = lc + 1;
      const int nch = std::max(1, (f - lo + kPvChunkRows - 1) / kPvChunkRows);
      if (nch == 1) {
        P.big.push_back({col, S.row_ptr[s], lo, f, col0 + lc, -1});
        continue;
      }
      if (P.nparts + nch > INT32_MAX) return "pivot report: too many partial records";
      P.merge.push_back({S.row_ptr[s], (int)P.nparts, nch, col0 + lc, 0});
      for (int c = 0; c < nch; ++c)
        P.big.push_back({col, S.row_ptr[s], lo + c * kPvChunkRows, std::min(f, lo + (c + 1) * kPvChunkRows), col0 + lc, (int)(P.nparts + c)});
      P.nparts += nch;
    }
  }
  return "";
}

struct PivotWork {
  bool planned = false;
  int64_t analysis = -1;          // okkt_solver_s::n_analyze_calls the lists belong to
  const double* arena = nullptr;  // ... and the front arena (a new device plan gets a new one)
  int64_t factor_seq = -1;        // the factorisation g was scanned from (-1: none)
  int64_t n = 0, nschur = 0, bytes = 0;
  int64_t n_small = 0, n_big = 0, n_merge = 0;
  double* g = nullptr;            // [n] original order
  int64_t* partner = nullptr;     // [n] original order, original indices
  PvSmall* small = nullptr;
  PvBig* big = nullptr;
  PvMerge* merge = nullptr;
  double* part_v = nullptr;       // partial records: value, front row
  int* part_r = nullptr;
  PvCount* count = nullptr;       // [kPvCountBlocks]
  // the last report
  double u = 0, seconds_device = 0;
  int64_t rejected = 0, nonfinite_cols = 0, max_col = -1;
  double max_multiplier = 0;
  // host copy of g / partner for okkt_get_rejected_pivots (fetched on its first call after a scan)
  int64_t host_seq = -1;
  std::vector<double> g_host;
  std::vector<int64_t> partner_host;
  std::vector<void*> allocs;
};

// host lists and allocations for the current analysis
std::string pivots_setup(const Symbolic& S, const Numeric& N, PivotWork& W);
void pivots_release(PivotWork& W);
// g and the partners from the factor in N, on `st` (no synchronisation)
std::string pivots_scan_enqueue(const Numeric& N, PivotWork& W, hipStream_t st);
// the per-block counts of g against 1 / u into W.count, on `st` (no synchronisation)
void pivots_count_enqueue(const PivotWork& W, double inv_u, hipStream_t st);

}  // namespace okkt
