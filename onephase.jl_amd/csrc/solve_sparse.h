// Sparse right-hand sides: the units a workgroup runs, the reach of a batch in the supernodal forest
// (solve_sparse_host.cpp, host) and the launches of a pruned solve (solve_sparse.hip, gfx950).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "numeric.h"
#include "symbolic.h"

namespace okkt {

// fronts of at most this many rows are "small" (one workgroup, the front in LDS): numeric_setup's rule
inline int small_front_limit(const SymbolicOptions& o) { return std::max(32, std::min(o.small_front_max, 136)); }

// The units of the schedules (numeric_setup builds its levels from them, the reach activates them whole): a big front is a unit of
// its own, a task of small fronts is the index range task_lo[root] .. root.  unit_root[s]: the root of the unit that holds front s;
// ulevel[root]: height of the unit in the tree of units; schur_sn: the Schur front (a unit that no schedule holds), -1 outside Schur mode
struct FrontUnits {
  std::vector<int> task_lo, unit_root, ulevel;
  int schur_sn = -1;
  bool use_tasks = true, parted_tasks = true;
};
void form_front_units(const Symbolic& S, int small_max, FrontUnits& U);

// prepare kinds of k_sp_prepare's items
enum { kSpZeroX = 0, kSpZeroZ = 1, kSpZeroCv = 2 };
constexpr int kSpChunk = 4096;      // entries of one item (a front's pivot columns or contribution vector, per right-hand side)

// what one batch activates, counted (okkt_sparse_info's fields) and listed
struct SparseSets {
  int64_t fwd_reach = 0, bwd_reach = 0, fwd_run = 0, bwd_run = 0, fringe = 0, fringe_entries = 0;
  int64_t fwd_panel_bytes = 0, bwd_panel_bytes = 0;
  bool fwd_full = false, bwd_full = false;
  std::vector<int> fwd_units, bwd_units;      // roots of the active units (unordered)
  std::vector<int> fwd_fronts, bwd_only_fronts, fringe_fronts;   // fronts the forward sweep runs; fronts the backward sweep runs that it did not; the fringe
};

// Per analysis: the units, epoch-stamped marks (a batch costs O(active), not O(nsuper)), and -- with a device plan -- where every unit
// stands in the schedules, the pinned list buffer and its device twin
struct SparseWork {
  int64_t analysis = -1;            // h->n_analyze_calls the host tables were built for
  FrontUnits U;
  std::vector<int> fmark, bmark, frun, brun;      // [nsuper] epoch stamps: in the forward / backward closure, run by the forward / backward sweep
  std::vector<int> colmark;                       // [n] epoch stamps of the rows of one column of b (duplicates)
  int epoch = 0, col_epoch = 0;
  int64_t factor_panel_bytes = 0;
  // device side (solve_sparse.hip)
  int64_t plan_analysis = -1;
  const void* plan_arena = nullptr;
  std::vector<int> unit_pos;        // [nsuper] roots: index in sched (small classes) or nsched + index in ssched (big fronts); -1 otherwise
  std::vector<int> unit_level;      // [nsuper] roots: level of the schedule
  std::vector<signed char> unit_kind;   // [nsuper] roots: 0..2 small class, 3 thin, 4 wide; -1 otherwise
  int nsched = 0;
  int* pinned = nullptr;            // one batch's lists, packed
  int* d_lists = nullptr;
  int64_t cap = 0;                  // ints of either
  int* d_xsel = nullptr;            // the requested rows of a call: permuted positions
  int64_t xsel_cap = 0;
  double* d_ones = nullptr;         // unit values of okkt_get_inverse_columns
  int64_t ones_cap = 0;
  hipEvent_t copied = nullptr;      // behind the list copy of the last batch: the pinned buffer is free again
  bool copy_pending = false;
};

void sparse_host_setup(const Symbolic& S, const SymbolicOptions& opts, SparseWork& W);
// rows: permuted indices of the non-zeros (nb of them, any order, duplicates allowed) and of the requested entries (x_all: every entry)
void sparse_reach(const Symbolic& S, SparseWork& W, const int* b_rows, int64_t nb, const int* x_rows, int64_t nx, bool x_all, SparseSets& out);

// device side
std::string sparse_plan_setup(const Symbolic& S, Numeric& N, SparseWork& W);
void sparse_release(SparseWork& W);
// the non-zeros of one batch, column after column: permuted positions, col[q] .. col[q + 1] the entries of column q (col[q] = count beyond the batch)
struct SparseScatter { const int* pos; int count; int col[kMaxRhs + 1]; };
// one batch: lists -> device, prepare, scatter (d_val: the batch's values in the order of sc.pos), the two sweeps (pruned or ordinary).
// The caller gathers.
std::string sparse_batch_enqueue(const Symbolic& S, Numeric& N, SparseWork& W, const SparseSets& A, const SparseScatter& sc, const double* d_val, const double* d_scale, int R);
// d_out[q * stride + t] = scale[perm[pos[t]]] * xwork[q][pos[t]], t < nx, q < nr (d_xsel: the nx permuted positions)
void sparse_gather_enqueue(const Numeric& N, const int* d_xsel, int64_t nx, double* d_out, int64_t stride, int nr, const double* d_scale);

// solve.hip: the sweeps over a view of the schedule -- sublists of the level lists with the levels' bounds
struct SweepLists {
  const std::vector<LevelSchedule>* levels;
  const std::vector<SolveLevel>* slevels;
  const int* sched;       // device list the segments' offsets index
  const int* ssched;      // ... and the solve levels'
};
std::string solve_fwd_enqueue_lists(Numeric& N, const SweepLists& V, int R);
std::string solve_bwd_enqueue_lists(Numeric& N, const SweepLists& V, int R);

}  // namespace okkt
