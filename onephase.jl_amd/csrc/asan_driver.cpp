// Host-side sanitizer run (make asan): the orderings, the symbolic analysis and the dataflow queue builder under AddressSanitizer and
// UndefinedBehaviorSanitizer on small synthetic patterns -- a banded KKT (level-structure dissection), a 3-D grid, a small-world graph
// (multilevel dissection with its helper threads) and an arrow matrix -- and the work-item lists of the pivot report (pivots.h) on each
// of them and on a front tall enough for several chunks per column.  No device code, no HIP call.  SURVEY.md section 5 (host-side
// sanitizer build); GPU sanitizers are not available on this pool.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "numeric.h"
#include "pivots.h"
#include "symbolic.h"

using namespace okkt;

static void csc_lower(int n, const std::set<std::pair<int, int>>& e, std::vector<int64_t>& cp, std::vector<int64_t>& ri) {
  std::vector<std::vector<int>> cols(n);
  for (auto& p : e) cols[std::min(p.first, p.second)].push_back(std::max(p.first, p.second));
  cp.assign(n + 1, 0); ri.clear();
  for (int j = 0; j < n; ++j) { ri.push_back(j); for (int r : cols[j]) if (r != j) ri.push_back(r); cp[j + 1] = (int64_t)ri.size(); }
}

static int run(const char* name, int n, const std::set<std::pair<int, int>>& e, int ordering) {
  std::vector<int64_t> cp, ri;
  csc_lower(n, e, cp, ri);
  SymbolicOptions o;
  o.ordering = ordering;
  Symbolic S;
  const std::string err = analyze_pattern(n, cp.data(), ri.data(), 0, o, nullptr, S);
  if (!err.empty()) { fprintf(stderr, "%s (ordering %d): %s\n", name, ordering, err.c_str()); return 1; }
  // the dataflow queues of the three largest fronts as one level, both forms
  std::vector<DfFront> fronts;
  for (int s = 0; s < (int)S.sn_col0.size() - 1 && fronts.size() < 3; ++s) {
    const int k = S.sn_col0[s + 1] - S.sn_col0[s], f = (int)(S.row_ptr[s + 1] - S.row_ptr[s]);
    if (f > 128) fronts.push_back({s, f, k});
  }
  size_t ntask = 0;
  if (!fronts.empty()) {
    std::vector<DfTask> q;
    double model = 0;
    df_build_queue(fronts, 64, 4, 1, true, true, q, &model, true);
    ntask = q.size();
    df_build_queue(fronts, 96, 2, 2, false, false, q, &model, false);
  }
  // the work-item lists of the pivot report: every pivot column once, every chunk inside its column's rows below the diagonal, the
  // chunks of a column contiguous and in ascending order; once with the last supernode left out (Schur mode)
  std::vector<int64_t> fpos(S.nsuper + 1, 0);
  for (int s = 0; s < S.nsuper; ++s)
    fpos[s + 1] = fpos[s] + (S.row_ptr[s + 1] - S.row_ptr[s]) * (int64_t)(S.sn_col0[s + 1] - S.sn_col0[s]);
  for (int skip : {-1, S.nsuper - 1}) {
    PvPlan P;
    const std::string pe = pivot_build_items(S, fpos, 128, skip, P);
    if (!pe.empty()) { fprintf(stderr, "%s (ordering %d): %s\n", name, ordering, pe.c_str()); return 1; }
    std::vector<int> seen(n, 0), next_row(n, -1);
    int64_t entries = 0;
    bool ok = true;
    for (const PvSmall& q : P.small) {
      ok = ok && q.f <= 128 && q.k <= q.f && q.L >= 0 && q.L + (int64_t)q.f * q.k <= fpos[S.nsuper];
      for (int lc = 0; lc < q.k; ++lc) { ++seen[q.col0 + lc]; entries += q.f - lc - 1; }
    }
    std::vector<int> part_owner(P.nparts, -1);
    for (const PvBig& q : P.big) {
      const int s = S.col2sn[q.out], f = (int)(S.row_ptr[s + 1] - S.row_ptr[s]), lc = q.out - S.sn_col0[s];
      ok = ok && f > 128 && q.col == fpos[s] + (int64_t)lc * f && q.rows == S.row_ptr[s] && q.r0 <= q.r1 && q.r1 <= f && q.r1 - q.r0 <= kPvChunkRows;
      ok = ok && q.r0 == (next_row[q.out] < 0 ? lc + 1 : next_row[q.out]);
      next_row[q.out] = q.r1;
      entries += q.r1 - q.r0;
      if (q.part < 0) ++seen[q.out];
      else { ok = ok && q.part < P.nparts && part_owner[q.part] < 0; if (ok) part_owner[q.part] = q.out; }
    }
    for (const PvMerge& q : P.merge) {
      ++seen[q.out];
      ok = ok && q.nparts > 1 && q.part0 >= 0 && q.part0 + q.nparts <= P.nparts;
      for (int c = 0; ok && c < q.nparts; ++c) ok = part_owner[q.part0 + c] == q.out;
    }
    const int ncov = skip < 0 ? n : S.sn_col0[skip];
    for (int c = 0; c < n; ++c) {
      ok = ok && seen[c] == (c < ncov ? 1 : 0);
      if (c < ncov && next_row[c] >= 0) { const int s = S.col2sn[c]; ok = ok && next_row[c] == (int)(S.row_ptr[s + 1] - S.row_ptr[s]); }
    }
    ok = ok && entries == P.entries && P.ncols == ncov;
    if (!ok) { fprintf(stderr, "%s (ordering %d): the pivot-report items do not tile the factor (skip %d)\n", name, ordering, skip); return 1; }
  }
  printf("%-12s ordering %d: n %d nnz(L) %lld supernodes %zu, %zu dataflow tasks\n", name, ordering, n, (long long)S.nnzL, S.sn_col0.size() - 1, ntask);
  return 0;
}

int main() {
  int bad = 0;
  std::mt19937 rng(5);
  {   // banded KKT with one dense row
    const int n = 3000;
    std::set<std::pair<int, int>> e;
    for (int i = 0; i < n; ++i) for (int d = 1; d <= 3; ++d) if (i + d < n) e.insert({i, i + d});
    for (int i = 0; i < n; i += 2) e.insert({i, n - 1});
    for (int o : {0, 3, 4}) bad += run("banded", n, e, o);
  }
  {   // 3-D grid 14^3
    const int g = 14, n = g * g * g;
    std::set<std::pair<int, int>> e;
    auto id = [&](int x, int y, int z) { return (x * g + y) * g + z; };
    for (int x = 0; x < g; ++x) for (int y = 0; y < g; ++y) for (int z = 0; z < g; ++z) {
      if (x + 1 < g) e.insert({id(x, y, z), id(x + 1, y, z)});
      if (y + 1 < g) e.insert({id(x, y, z), id(x, y + 1, z)});
      if (z + 1 < g) e.insert({id(x, y, z), id(x, y, z + 1)});
    }
    for (int o : {0, 3, 4, 5}) bad += run("grid", n, e, o);
  }
  {   // small world: a band plus random long edges (the shape of the metric workload), large enough for the threaded dissection
    const int n = 12000;
    std::set<std::pair<int, int>> e;
    for (int i = 0; i < n; ++i) for (int d = 1; d <= 12; d += 3) if (i + d < n) e.insert({i, i + d});
    for (int t = 0; t < n / 4; ++t) { const int a = (int)(rng() % n), b = (int)(rng() % n); if (a != b) e.insert({a, b}); }
    for (int o : {0, 5}) bad += run("small-world", n, e, o);
  }
  {   // the same shape at 24 000: the sizes from which the cut statistics and the induced subgraphs go to helper threads as well
    const int n = 24000;
    std::set<std::pair<int, int>> e;
    for (int i = 0; i < n; ++i) for (int d = 1; d <= 12; d += 3) if (i + d < n) e.insert({i, i + d});
    for (int t = 0; t < n / 4; ++t) { const int a = (int)(rng() % n), b = (int)(rng() % n); if (a != b) e.insert({a, b}); }
    bad += run("small-world-24k", n, e, 5);
  }
  {   // arrow
    const int n = 600;
    std::set<std::pair<int, int>> e;
    for (int i = 0; i + 1 < n; ++i) { e.insert({i, n - 1}); e.insert({i, i + 1}); }
    for (int o : {0, 1, 3}) bad += run("arrow", n, e, o);
  }
  {   // a full column under natural ordering: one front of 2300 rows, its leading columns in two chunks of the pivot report
    const int n = 2300;
    std::set<std::pair<int, int>> e;
    for (int i = 1; i < n; ++i) e.insert({0, i});
    bad += run("full-column", n, e, 1);
  }
  if (bad) { fprintf(stderr, "%d case(s) failed\n", bad); return 1; }
  printf("asan driver: all cases clean\n");
  return 0;
}
