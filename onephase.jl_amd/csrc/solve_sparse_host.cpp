// Sparse right-hand sides, host side: the units of the schedules and the reach of a batch.
//
// A solve with a sparse b and a few wanted entries of x only has to visit two sets of supernodes: the closure, under the supernodal
// parent relation, of the supernodes that hold the permuted non-zero rows (forward sweep) and the closure of those that hold the wanted
// rows (backward sweep).  Everything else is exactly zero or never read.  What runs is a UNIT -- a big front, or a task of small
// fronts that one workgroup runs whole -- so the sets are rounded up to units; the FRINGE is every front that does not run in the
// forward sweep but whose parent does: the parent gathers its contribution vector, which has to read zero.
#include "solve_sparse.h"

#include <algorithm>
#include <cstdlib>

namespace okkt {

// Tasks: a workgroup runs a whole subtree of small fronts, children before parents (numeric_setup states the rule and why).
void form_front_units(const Symbolic& S, int small_max, FrontUnits& U) {
  const int ns = S.nsuper;
  const bool parted = S.nparts > 1 && (int)S.sn_owner.size() == ns;
  static const bool parted_tasks = !(getenv("OKKT_PARTED_TASKS") && atoi(getenv("OKKT_PARTED_TASKS")) == 0);
  const bool use_tasks = (!parted || parted_tasks) && !(getenv("OKKT_TASKS") && atoi(getenv("OKKT_TASKS")) == 0);
  U.parted_tasks = parted_tasks;
  U.use_tasks = use_tasks;
  // plans of the level-structure dissection (banded systems) are all small fronts and nothing but launch latency: finer tasks
  // (12 front units, ratio 1.1) cut the hanging chain at the CUTEst size from 0.19 + 0.15 ms to 0.11 + 0.10 ms, N_h = 20 000 from
  // 0.37 + 0.29 to 0.24 + 0.19 ms (round 3 sweep); the general plans keep the coarser round-2 setting
  const bool level_nd = S.ordering_used == 4 && S.max_front <= small_max;   // the banded plans: all small fronts (a mesh-like system ordered by the level structure keeps the general setting)
  const double task_abs = getenv("OKKT_TASK_ABS") ? atof(getenv("OKKT_TASK_ABS")) : (level_nd ? 12.0 : 48.0);
  const double task_ratio = getenv("OKKT_TASK_RATIO") ? atof(getenv("OKKT_TASK_RATIO")) : (level_nd ? 1.1 : 1.5);
  std::vector<int>&task_lo = U.task_lo, &unit_root = U.unit_root, &ulevel = U.ulevel;
  task_lo.assign(ns, 0);
  unit_root.assign(ns, 0);
  ulevel.assign(ns, 0);
  auto fof = [&](int s2) { return (int)(S.row_ptr[s2 + 1] - S.row_ptr[s2]); };
  // forbid[s]: front s is a unit of its own (neither the root nor a member of a multi-front task); see the second pass below
  std::vector<char> forbid(ns, 0);
  // Schur mode: the last supernode is the Schur front -- a unit of its own that no schedule holds (assembled by numeric_factor_enqueue
  // behind the interior, never factored, left out of the solve sweeps)
  U.schur_sn = S.nschur > 0 ? ns - 1 : -1;
  if (U.schur_sn >= 0) forbid[U.schur_sn] = 1;
  auto form_units = [&]() {
    std::fill(ulevel.begin(), ulevel.end(), 0);
    std::vector<char> allsmall(ns), assigned(ns, 0);
    std::vector<int> first(ns);
    std::vector<double> ctot(ns), cpath(ns), cmaxchild(ns, 0.0);
    for (int s2 = 0; s2 < ns; ++s2) {
      const int f = fof(s2), k = S.sn_col0[s2 + 1] - S.sn_col0[s2];
      allsmall[s2] = f <= small_max && !forbid[s2];
      first[s2] = s2;
      ctot[s2] = 1.0 + (double)f * f * k / 8192.0;
      cpath[s2] = ctot[s2];
    }
    for (int s2 = 0; s2 < ns; ++s2) {           // children before parents
      cpath[s2] += cmaxchild[s2];
      const int p2 = S.sn_parent[s2];
      if (p2 < 0) continue;
      if (!allsmall[s2] || (parted && S.sn_owner[s2] != S.sn_owner[p2])) allsmall[p2] = 0;      // "all small" also means "all of one part"
      first[p2] = std::min(first[p2], first[s2]);
      ctot[p2] += ctot[s2];
      cmaxchild[p2] = std::max(cmaxchild[p2], cpath[s2]);
    }
    for (int s2 = ns - 1; s2 >= 0; --s2) {      // parents before children: the largest admissible subtrees win
      if (assigned[s2]) continue;
      task_lo[s2] = s2;
      unit_root[s2] = s2;
      assigned[s2] = 1;
      if (!use_tasks || !allsmall[s2] || !(ctot[s2] <= task_abs || ctot[s2] <= task_ratio * cpath[s2])) continue;
      task_lo[s2] = first[s2];
      for (int t = first[s2]; t < s2; ++t) { assigned[t] = 1; unit_root[t] = s2; task_lo[t] = t; }
    }
    for (int s2 = 0; s2 < ns; ++s2) {           // level of a unit = height in the tree of units
      const int p2 = S.sn_parent[s2];
      if (p2 < 0 || unit_root[p2] == unit_root[s2]) continue;
      ulevel[unit_root[p2]] = std::max(ulevel[unit_root[p2]], ulevel[unit_root[s2]] + 1);
    }
  };
  form_units();
  {
    // Second pass (round 6).  A level WITHOUT big fronts whose tasks are nearly all one-wave tasks (fronts of at most 32 rows) but for
    // a handful with a mid-size front ran that handful in launches of its own -- one 256-thread workgroup for 67 us of the
    // factorisation's critical path and 21 + 19 us of every solve at the metric size (53 869 one-wave tasks and ONE task with a
    // front of 65 .. 128 rows in level 0).  Those mid-size fronts become units of their own: they move up to the level above their
    // children, where the rule of numeric_setup's build() lets them join the big fronts of that level; what is left of their subtrees
    // is one-wave tasks like everything around it.
    static const int lone_max = getenv("OKKT_FOLD_LONE") ? atoi(getenv("OKKT_FOLD_LONE")) : 3;
    int nl = 0;
    for (int s2 = 0; s2 < ns; ++s2) if (unit_root[s2] == s2) nl = std::max(nl, ulevel[s2] + 1);
    std::vector<int> nbig(nl, 0), nmid(nl, 0), nwave(nl, 0);
    auto unit_maxf = [&](int s2) { int f = 0; for (int t = task_lo[s2]; t <= s2; ++t) f = std::max(f, fof(t)); return f; };
    for (int s2 = 0; s2 < ns; ++s2) {
      if (unit_root[s2] != s2) continue;
      const int f = unit_maxf(s2);
      ++(f <= 32 ? nwave : (f <= small_max ? nmid : nbig))[ulevel[s2]];
    }
    bool any = false;
    if (lone_max > 0 && use_tasks && !parted)
      for (int s2 = 0; s2 < ns; ++s2) {
        if (unit_root[s2] != s2) continue;
        const int l = ulevel[s2];
        if (nbig[l] != 0 || nmid[l] == 0 || nmid[l] > lone_max || nwave[l] < 64 || unit_maxf(s2) <= 32) continue;
        for (int t = task_lo[s2]; t <= s2; ++t) if (fof(t) > 32) { forbid[t] = 1; any = true; }
      }
    if (any) form_units();
  }
}

void sparse_host_setup(const Symbolic& S, const SymbolicOptions& opts, SparseWork& W) {
  const int ns = S.nsuper;
  form_front_units(S, small_front_limit(opts), W.U);
  W.fmark.assign(ns, 0);
  W.bmark.assign(ns, 0);
  W.frun.assign(ns, 0);
  W.brun.assign(ns, 0);
  W.colmark.assign((size_t)S.n, 0);
  W.epoch = 0;
  W.col_epoch = 0;
  W.factor_panel_bytes = 0;
  for (int s = 0; s < ns; ++s) W.factor_panel_bytes += (int64_t)(S.row_ptr[s + 1] - S.row_ptr[s]) * (S.sn_col0[s + 1] - S.sn_col0[s]) * 8;
}

namespace {
// closure of the supernodes of `rows` under the parent relation, rounded up to units: mark (closure) and run (what the launches visit)
// are stamped with W.epoch; returns the closure's size, appends the units' roots and the fronts they hold
int64_t close_up(const Symbolic& S, const FrontUnits& U, const int* rows, int64_t n, int epoch, std::vector<int>& mark, std::vector<int>& run, std::vector<int>& units,
                 std::vector<int>* fronts, int64_t* n_run, int64_t* bytes) {
  int64_t reach = 0;
  for (int64_t t = 0; t < n; ++t) {
    for (int s = S.col2sn[rows[t]]; s >= 0 && mark[s] != epoch; s = S.sn_parent[s]) {
      mark[s] = epoch;
      ++reach;
      if (run[s] == epoch) continue;
      const int u = U.unit_root[s];
      units.push_back(u);
      for (int v = U.task_lo[u]; v <= u; ++v) {
        run[v] = epoch;
        ++*n_run;
        *bytes += (int64_t)(S.row_ptr[v + 1] - S.row_ptr[v]) * (S.sn_col0[v + 1] - S.sn_col0[v]) * 8;
        if (fronts) fronts->push_back(v);
      }
    }
  }
  return reach;
}
}  // namespace

void sparse_reach(const Symbolic& S, SparseWork& W, const int* b_rows, int64_t nb, const int* x_rows, int64_t nx, bool x_all, SparseSets& A) {
  const int ns = S.nsuper;
  A = SparseSets();
  if (++W.epoch == 0x7fffffff) {      // the stamps start over
    std::fill(W.fmark.begin(), W.fmark.end(), 0); std::fill(W.bmark.begin(), W.bmark.end(), 0);
    std::fill(W.frun.begin(), W.frun.end(), 0); std::fill(W.brun.begin(), W.brun.end(), 0);
    W.epoch = 1;
  }
  const int ep = W.epoch;
  A.fwd_reach = close_up(S, W.U, b_rows, nb, ep, W.fmark, W.frun, A.fwd_units, &A.fwd_fronts, &A.fwd_run, &A.fwd_panel_bytes);
  A.fwd_full = A.fwd_run == ns;
  // the fringe: children of the fronts that run which do not run themselves
  for (int v : A.fwd_fronts)
    for (int64_t c = S.child_ptr[v]; c < S.child_ptr[v + 1]; ++c) {
      const int ch = S.children[c];
      if (W.frun[ch] == ep) continue;
      A.fringe_fronts.push_back(ch);
      ++A.fringe;
      A.fringe_entries += (S.row_ptr[ch + 1] - S.row_ptr[ch]) - (S.sn_col0[ch + 1] - S.sn_col0[ch]);
    }
  if (x_all) {
    A.bwd_full = true;
    A.bwd_reach = A.bwd_run = ns;
    A.bwd_panel_bytes = W.factor_panel_bytes;
    if (!A.fwd_full)
      for (int s = 0; s < ns; ++s) if (W.frun[s] != ep) A.bwd_only_fronts.push_back(s);
    return;
  }
  std::vector<int> bfronts;
  A.bwd_reach = close_up(S, W.U, x_rows, nx, ep, W.bmark, W.brun, A.bwd_units, &bfronts, &A.bwd_run, &A.bwd_panel_bytes);
  A.bwd_full = A.bwd_run == ns;
  for (int v : bfronts) if (W.frun[v] != ep) A.bwd_only_fronts.push_back(v);
}

}  // namespace okkt
