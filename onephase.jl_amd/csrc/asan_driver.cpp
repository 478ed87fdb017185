// Host-side sanitizer run (make asan): the orderings, the symbolic analysis and the dataflow queue builder under AddressSanitizer and
// UndefinedBehaviorSanitizer on small synthetic patterns -- a banded KKT (level-structure dissection), a 3-D grid, a small-world graph
// (multilevel dissection with its helper threads) and an arrow matrix -- and the work-item lists of the pivot report (pivots.h) on each
// of them and on a front tall enough for several chunks per column, and the flat records of the staged big-front assembly
// (asm_pieces.h) on each of them and under a front of three chunks, and the tridiagonal solver of the Lanczos estimate
// (lanczos_tridiag.h), and the dense symmetric eigen-solver of okkt_eigs (sym_eig.h), and the sets of the sparse right-hand sides
// (solve_sparse_host.cpp), and the grids of the uniform batches (batch_host.cpp), and the host arithmetic behind the reductions of the
// step-side functions (ls_finish.h).  No device code, no HIP call.  SURVEY.md section 5 (host-side
// sanitizer build); GPU sanitizers are not available on this pool.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "asm_pieces.h"
#include "factor_ops.h"
#include "lanczos_tridiag.h"
#include "numeric.h"
#include "pivots.h"
#include "solve_sparse.h"
#include "batch.h"
#include "batch_schur.h"
#include "kkt_items_seq.h"
#include "ls_finish.h"
#include "../../include/okkt.h"
#include "sym_eig.h"
#include "symbolic.h"

using namespace okkt;

// The tridiagonal solver of okkt_kkt_min_eig (lanczos_tridiag.h) on the shapes its arrays are indexed hardest by: orders 1, 2 and 64
// (its stack arrays are exactly 64 long), a zero off-diagonal entry in the middle and at both ends, entries 300 decades apart, the zero
// matrix, and the refused orders 0 and 65.  Checks the residual of the returned pair against the matrix.
static int check_tridiag() {
  int bad = 0;
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  auto one = [&](int k, std::vector<double> a, std::vector<double> b, const char* name) {
    double tmin = 0.0, tmax = 0.0;
    std::vector<double> s((size_t)k, 0.0);   // exactly k long: a write past it is caught
    const int rc = tridiag_extreme(k, a.data(), b.data(), &tmin, &tmax, s.data());
    if (rc != 0) { fprintf(stderr, "tridiag %s: rc %d\n", name, rc); ++bad; return; }
    double scale = 0.0, r2 = 0.0, s2 = 0.0;
    for (int i = 0; i < k; ++i) scale = std::max(scale, std::abs(a[i]));
    for (int i = 0; i + 1 < k; ++i) scale = std::max(scale, std::abs(b[i]));
    if (scale == 0.0) scale = 1.0;
    for (int i = 0; i < k; ++i) {
      double r = (a[i] / scale) * s[i] - (tmin / scale) * s[i];
      if (i > 0) r += (b[i - 1] / scale) * s[i - 1];
      if (i + 1 < k) r += (b[i] / scale) * s[i + 1];
      r2 += r * r; s2 += s[i] * s[i];
    }
    if (!(tmin <= tmax) || std::abs(s2 - 1.0) > 1e-12 || !(std::sqrt(r2) <= 1e-9)) {
      fprintf(stderr, "tridiag %s: theta %g %g, |s|^2 %g, residual %g\n", name, tmin, tmax, s2, std::sqrt(r2));
      ++bad;
    }
  };
  for (int k : {1, 2, 3, 17, 63, 64}) {
    std::vector<double> a((size_t)k), b((size_t)std::max(k - 1, 1));   // the solver reads k - 1 off-diagonal entries, no more
    for (double& v : a) v = 10.0 * u(rng);
    for (double& v : b) v = u(rng);
    one(k, a, b, "random");
    if (k >= 3) {
      b[(size_t)(k / 2)] = 0.0; one(k, a, b, "zero in the middle");
      b[0] = 0.0; b[(size_t)(k - 2)] = 0.0; one(k, a, b, "zeros at the ends");
    }
    for (double& v : b) v = 0.0;
    one(k, a, b, "diagonal");
    for (double& v : a) v = 0.0;
    one(k, a, b, "zero");
  }
  one(6, {1e150, -1e-150, 2.0, -1e150, 1e-150, 1.0}, {1e-150, 1.0, 1e100, 1e-150, 1e149}, "300 decades");
  {
    double a[65] = {0}, t0 = 0.0, t1 = 0.0, s[65];
    if (tridiag_extreme(0, a, a, &t0, &t1, s) != 1 || tridiag_extreme(65, a, a, &t0, &t1, s) != 1) { fprintf(stderr, "tridiag: order 0 / 65 not refused\n"); ++bad; }
  }
  if (!bad) printf("tridiag      orders 1 .. 64, split, scaled and refused cases clean\n");
  return bad;
}

// The attempt sequencing of the delta loop over the items of a KKT batch (kkt_items_seq.h): items that pass at delta = 0, after three
// attempts, beyond delta_max (status 0) and with a previous delta, stepped as okkt_kkt_items_ipopt_strategy steps
// them (an attempt succeeds when delta >= need).  Checks the counts against a serial walk of the same sequence per item, that the number
// of rounds is the largest count, and that an item leaves the active list exactly once.
static int check_items_loop() {
  int bad = 0;
  okkt_kkt_pars P = default_kkt_pars();
  P.delta_max = 1e3; P.delta_dec = 1.0 / 3.0;
  // item 6 starts from a large previous delta: it passes delta_max at its third attempt and leaves with status 0 while items 1 and 4
  // are still making attempts (item 1 succeeds at its fourth)
  const double dmin[] = {0.5, 0.5, -2.0, -2.0, 0.5, 0.25, 0.5};
  const double prev[] = {0.0, 0.0, 0.0, 0.3, 0.0, 7.0, 900.0};
  const double need[] = {0.0, 1e-5, 4.0, 0.01, 1e9, 1.0, 1e9};
  const int B = 7;
  {   // a NaN diag_min: every attempt is NaN, none ends the loop, and the sequence is used up after max_it attempts (error("max it"))
    DeltaSeq s;
    s.start(NAN, 0.0, P);
    double d = 0.0;
    bool lp = false;
    int cnt = 0;
    while (s.next(P, &d, &lp)) { ++cnt; if (d == d || !lp) { ++bad; break; } }
    if (cnt != P.max_it) { fprintf(stderr, "items loop: the NaN sequence gave %d attempts\n", cnt); ++bad; }
  }
  std::vector<DeltaSeq> seq(B);
  std::vector<double> cand(B, 0.0), delta(B, 0.0);
  std::vector<char> in_loop(B, 0);
  std::vector<int32_t> flags(B, 0), status(B, -1), nfac(B, 0), left(B, 0);
  for (int b = 0; b < B; ++b) seq[b].start(dmin[b], prev[b], P);
  ItemsLoop L;
  L.start(B);
  int rounds = 0;
  while (!L.active.empty() && rounds < 1000) {
    const std::vector<int32_t> before = L.active;
    for (const int32_t b : L.active) {
      bool lp = false;
      if (!seq[b].next(P, &cand[b], &lp)) { ++bad; break; }
      in_loop[b] = lp;
      flags[b] = cand[b] >= need[b] ? 1 : 0;
    }
    ++rounds;
    L.close_round(cand.data(), in_loop.data(), flags.data(), P.delta_max, status.data(), nfac.data(), delta.data());
    for (const int32_t b : before)
      if (std::find(L.active.begin(), L.active.end(), b) == L.active.end()) ++left[b];
  }
  int max_fac = 0;
  for (int b = 0; b < B; ++b) {
    // the serial walk of one item
    DeltaSeq s;
    s.start(dmin[b], prev[b], P);
    int nf = 0, st = -1;
    double d = 0.0;
    bool lp = false;
    while (s.next(P, &d, &lp)) {
      ++nf;
      if (d >= need[b]) { st = 1; break; }
      if (lp && d > P.delta_max) { st = 0; break; }
    }
    if (nf != nfac[b] || st != status[b] || d != delta[b] || left[b] != 1) {
      fprintf(stderr, "items loop: item %d: %d attempts (serial %d), status %d (%d), left %d times\n", b, nfac[b], nf, status[b], st, left[b]);
      ++bad;
    }
    max_fac = std::max(max_fac, nf);
  }
  if (status[6] != 0 || nfac[6] != 3 || status[1] != 1 || nfac[1] != 4 || rounds <= nfac[6]) { fprintf(stderr, "items loop: the early failure: status %d after %d attempts\n", status[6], nfac[6]); ++bad; }
  if (rounds != max_fac || status[4] != 0 || status[0] != 1 || nfac[0] != 1) { fprintf(stderr, "items loop: %d rounds, largest count %d\n", rounds, max_fac); ++bad; }
  return bad;
}

// The sequence all three delta loops step (DeltaSeq), against delta_strategy.jl:37-114 evaluated by hand with the default parameters
// (start 1e-6, min 1e-12, max 1e50, inc 8, dec 1/pi, zero 0): the attempt at delta_zero outside the loop (tau = 1.5 diag_min > 0), an
// attempt that a caller skips (it is consumed: the next one is delta * inc all the same), the first attempt of the loop above
// delta_max (1e-6 * 8^63 = 1e-6 * 2^189 = 7.8e50; 8^62 gives 9.8e49), and the first attempts with tau < 0
static int check_delta_seq() {
  int bad = 0;
  const okkt_kkt_pars P = default_kkt_pars();
  double d = -1.0;
  bool lp = true;
  auto expect = [&](DeltaSeq& s, double want, bool want_loop, const char* what) {
    if (!s.next(P, &d, &lp) || d != want || lp != want_loop) { fprintf(stderr, "delta seq: %s: (%.17g, %d), expected (%.17g, %d)\n", what, d, (int)lp, want, (int)want_loop); ++bad; }
  };
  DeltaSeq s;
  s.start(0.5, 0.0, P);
  expect(s, 0.0, false, "the attempt at delta_zero");
  expect(s, 1e-6, true, "i = 1: delta_start - tau with tau = 0 (this one is skipped, not factored)");
  expect(s, 8e-6, true, "i = 2 after the skipped attempt");
  for (int i = 3; i <= 63; ++i) {
    if (!s.next(P, &d, &lp) || !lp || d > P.delta_max) { fprintf(stderr, "delta seq: i = %d: %.17g is above delta_max or outside the loop\n", i, d); ++bad; break; }
  }
  expect(s, std::ldexp(1e-6, 189), true, "i = 64: the first attempt above delta_max");
  if (!(d > P.delta_max)) { fprintf(stderr, "delta seq: i = 64 is not above delta_max\n"); ++bad; }
  s.start(-2.0, 0.0, P);
  expect(s, 3.000001, true, "tau = -3, no previous delta: delta_start - tau");
  expect(s, 24.000008, true, "then delta * inc");
  s.start(-2.0, 0.3, P);
  expect(s, 3.000000000001, true, "tau = -3, previous delta 0.3: max(delta_min - tau, 0.3 / pi)");
  s.start(-2.0, 30.0, P);
  expect(s, 30.0 * (1.0 / M_PI), true, "tau = -3, previous delta 30: 30 * dec");
  if (!bad) printf("delta seq    zero-first, skipped, above delta_max and tau < 0 attempts as delta_strategy.jl gives them\n");
  return bad;
}

// The dense symmetric eigen-solver of okkt_eigs (sym_eig.h) with outputs and work of exactly m and m x m entries: orders 1, 2, 127 and
// 128 (its stack arrays are exactly 128 long), a leading dimension above m, graded, diagonal and zero matrices, and the refused orders 0
// and 129.  Checks A S = S theta and the order of the output.
static int check_sym_eig() {
  int bad = 0;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  auto one = [&](int m, int lda, const std::vector<double>& a, const char* name) {
    std::vector<double> theta((size_t)m), s((size_t)m * m), work((size_t)m * m);
    const int rc = sym_eig(m, a.data(), lda, theta.data(), s.data(), work.data());
    if (rc != 0) { fprintf(stderr, "sym_eig %s m=%d: rc %d\n", name, m, rc); ++bad; return; }
    double scale = 0.0, worst = 0.0;
    for (int i = 0; i < m; ++i) for (int j = i; j < m; ++j) scale = std::max(scale, std::abs(a[(size_t)i * lda + j]));
    if (scale == 0.0) scale = 1.0;
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i) {
        double r = -(theta[j] / scale) * s[(size_t)i * m + j];
        for (int k = 0; k < m; ++k) r += (a[(size_t)std::min(i, k) * lda + std::max(i, k)] / scale) * s[(size_t)k * m + j];
        worst = std::max(worst, std::abs(r));
      }
    bool ordered = true;
    for (int j = 0; j + 1 < m; ++j) ordered = ordered && std::abs(theta[j]) >= std::abs(theta[j + 1]);
    if (!ordered || !(worst <= 1e-11)) { fprintf(stderr, "sym_eig %s m=%d: residual %g, ordered %d\n", name, m, worst, (int)ordered); ++bad; }
  };
  for (int m : {1, 2, 3, 17, 127, 128}) {
    const int lda = m + (m % 3);
    std::vector<double> a((size_t)m * lda, 0.0);
    for (int i = 0; i < m; ++i) for (int j = i; j < m; ++j) a[(size_t)i * lda + j] = u(rng);
    one(m, lda, a, "random");
    for (int i = 0; i < m; ++i) for (int j = i; j < m; ++j) a[(size_t)i * lda + j] *= std::pow(10.0, -7.0 * (i + j) / (2.0 * m));
    one(m, lda, a, "graded");
    for (int i = 0; i < m; ++i) for (int j = i + 1; j < m; ++j) a[(size_t)i * lda + j] = 0.0;
    one(m, lda, a, "diagonal");
    std::fill(a.begin(), a.end(), 0.0);
    one(m, lda, a, "zero");
  }
  {
    std::vector<double> a(129 * 129, 1.0), t(129), s(129 * 129), w(129 * 129);
    if (sym_eig(0, a.data(), 1, t.data(), s.data(), w.data()) != 1 || sym_eig(129, a.data(), 129, t.data(), s.data(), w.data()) != 1) {
      fprintf(stderr, "sym_eig: order 0 / 129 not refused\n"); ++bad;
    }
  }
  if (!bad) printf("sym_eig      orders 1 .. 128, graded, diagonal, zero and refused cases clean\n");
  return bad;
}

static void csc_lower(int n, const std::set<std::pair<int, int>>& e, std::vector<int64_t>& cp, std::vector<int64_t>& ri) {
  std::vector<std::vector<int>> cols(n);
  for (auto& p : e) cols[std::min(p.first, p.second)].push_back(std::max(p.first, p.second));
  cp.assign(n + 1, 0); ri.clear();
  for (int j = 0; j < n; ++j) { ri.push_back(j); for (int r : cols[j]) if (r != j) ri.push_back(r); cp[j + 1] = (int64_t)ri.size(); }
}

// The records of the staged assembly against a plain enumeration: for every column of every big front (more than 128 rows here) the
// items are the columns jj of its children, ascending, with rel[jj] = the column; the pieces of the column's chunks must tile the rows
// jj .. rc - 1 of every item exactly once, chunk after chunk, keep the order of the items inside every chunk, and none may be empty.
// The A entries of the chunks of a column must tile the column's entries.
static bool check_asm_pieces(const Symbolic& S, int chunk) {
  const int ns = S.nsuper;
  std::vector<char> big(ns, 0);
  std::vector<int64_t> cb_base(ns, 0);
  int64_t top = 0;
  for (int s = 0; s < ns; ++s) {
    const int64_t f = S.row_ptr[s + 1] - S.row_ptr[s], k = S.sn_col0[s + 1] - S.sn_col0[s];
    big[s] = f > 128;
    cb_base[s] = top + k * f + k;
    top += f * f + (s & 1);      // odd and even bases
  }
  AsmPlan A;
  if (!asm_build_pieces(S, big, cb_base, chunk, A).empty()) return false;
  std::vector<std::vector<int>> kids(ns);
  for (int c = 0; c < ns; ++c) if (S.sn_parent[c] >= 0) kids[S.sn_parent[c]].push_back(c);
  int64_t items = 0, pieces = 0;
  for (int p = 0; p < ns; ++p) {
    if (!big[p]) { if (A.unit_base[p] != -1) return false; continue; }
    const int64_t f = S.row_ptr[p + 1] - S.row_ptr[p];
    const int nchunks = (int)((f + chunk - 1) / chunk);
    for (int64_t pc = 0; pc < f; ++pc) {
      // the items of the column
      std::vector<int> ic, ijj, done;
      for (int c : kids[p]) {
        const int* rb = S.rel.data() + S.rel_ptr[c];
        const int* re = S.rel.data() + S.rel_ptr[c + 1];
        const int* it = std::lower_bound(rb, re, (int)pc);
        if (it != re && *it == pc) { ic.push_back(c); ijj.push_back((int)(it - rb)); }
      }
      done = ijj;       // per item: the next row a piece has to start at
      items += (int64_t)ic.size();
      int64_t a_next = -1;
      for (int t = 0; t < nchunks; ++t) {
        const AsmUnit& U = A.units[(size_t)(A.unit_base[p] + (int64_t)t * f + pc)];
        const int64_t r0 = std::max<int64_t>(pc, (int64_t)t * chunk), r1 = std::min<int64_t>(f, (int64_t)(t + 1) * chunk);
        if (r0 >= r1) { if (U.np != 0 || U.na != 0) return false; continue; }
        if (U.np < 0 || U.piece0 < 0 || U.piece0 + U.np > (int64_t)A.pieces.size()) return false;
        // A entries: one range, in the chunk, contiguous from chunk to chunk
        if (U.na < 0 || U.a0 < S.aent_ptr[p] || U.a0 + U.na > S.aent_ptr[p + 1]) return false;
        for (int64_t e = U.a0; e < U.a0 + U.na; ++e) if (S.aent_dst[e] < pc * f + r0 || S.aent_dst[e] >= pc * f + r1) return false;
        if (a_next >= 0 && U.a0 != a_next) return false;
        a_next = U.a0 + U.na;
        int q = 0;      // next item that may own a piece of this chunk
        for (int i = 0; i < U.np; ++i, ++pieces) {
          const AsmPiece& R = A.pieces[(size_t)(U.piece0 + i)];
          if (R.n <= 0) return false;
          // the first item from q on with a row in the chunk
          for (; q < (int)ic.size(); ++q) {
            const int c = ic[q];
            const int rc = (int)(S.rel_ptr[c + 1] - S.rel_ptr[c]);
            if (done[q] < rc && S.rel[S.rel_ptr[c] + done[q]] < r1) break;
          }
          if (q == (int)ic.size()) return false;
          const int c = ic[q];
          const int64_t fc = S.row_ptr[c + 1] - S.row_ptr[c];
          const int rc = (int)(S.rel_ptr[c + 1] - S.rel_ptr[c]);
          int hi = done[q];
          while (hi < rc && S.rel[S.rel_ptr[c] + hi] < r1) ++hi;
          if (S.rel[S.rel_ptr[c] + done[q]] < r0) return false;
          if (R.src != cb_base[c] + (int64_t)ijj[q] * fc + done[q] || R.rel != S.rel_ptr[c] + done[q] || R.n != hi - done[q]) return false;
          done[q] = hi;
          ++q;
        }
        // no item with rows in this chunk was left out
        for (int j = 0; j < (int)ic.size(); ++j) {
          const int c = ic[j];
          const int rc = (int)(S.rel_ptr[c + 1] - S.rel_ptr[c]);
          if (done[j] < rc && S.rel[S.rel_ptr[c] + done[j]] < r1) return false;
        }
      }
      for (int j = 0; j < (int)ic.size(); ++j) if (done[j] != (int)(S.rel_ptr[ic[j] + 1] - S.rel_ptr[ic[j]])) return false;
      // every A entry of the column in one of its chunks
      if (a_next >= 0) {
        const int64_t* dst = S.aent_dst.data();
        const int64_t lo = std::lower_bound(dst + S.aent_ptr[p], dst + S.aent_ptr[p + 1], pc * f + pc) - dst;
        const int64_t hi = std::lower_bound(dst + S.aent_ptr[p], dst + S.aent_ptr[p + 1], (pc + 1) * f) - dst;
        const AsmUnit& U0 = A.units[(size_t)(A.unit_base[p] + (pc / chunk) * f + pc)];
        if (U0.a0 != lo || a_next != hi) return false;
      }
    }
  }
  return items == A.items && pieces == (int64_t)A.pieces.size();
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
  // the work-item lists of the factor products (factor_ops.h): every column of L once on either side, the items of L^T x and of L x
  // each tiling the entries below the diagonal, partial records inside their buffers, children on lower levels than their parents
  {
    std::vector<int64_t> gcb(S.nsuper, -1);
    int64_t nbig = 0;
    for (int s = 0; s < S.nsuper; ++s) {
      const int64_t f = S.row_ptr[s + 1] - S.row_ptr[s];
      if (f > 128) { gcb[s] = nbig; nbig += f; }
    }
    FoPlan P;
    const std::string fe = factor_ops_build_plan(S, fpos, gcb, 128, P);
    if (!fe.empty()) { fprintf(stderr, "%s (ordering %d): %s\n", name, ordering, fe.c_str()); return 1; }
    bool ok = (int)P.small_off.size() == S.nlevels + 1 && P.small_off.back() == (int64_t)P.small.size() && P.l_big_off.back() == (int64_t)P.l_big.size() &&
              P.l_merge_off.back() == (int64_t)P.l_merge.size();
    std::vector<int> seen(n, 0);
    int64_t e_small = 0, e_lt = 0, e_l = 0;
    for (const FoSmall& q : P.small) {
      ok = ok && q.f <= 128 && q.k <= q.f && q.s >= 0 && q.s < S.nsuper && q.L == fpos[q.s] && q.col0 == S.sn_col0[q.s];
      for (int lc = 0; lc < q.k; ++lc) { ++seen[q.col0 + lc]; e_small += q.f - lc - 1; }
    }
    for (const FoLtMerge& q : P.lt_merge) { ++seen[q.out]; ok = ok && q.nch >= 1 && q.part >= 0 && q.part + q.nch <= P.lt_parts; }
    for (const FoLtBig& q : P.lt_big) {
      ok = ok && q.nc >= 1 && q.nc <= kFoLtCols && q.r0 <= q.r1 && q.r1 <= q.f && q.r1 - q.r0 <= kFoLtRows && q.r0 >= std::min(q.c0 + 1, q.f) &&
           q.part >= 0 && q.part + (int64_t)(q.nc - 1) * q.nch < P.lt_parts;
      for (int c = 0; c < q.nc; ++c) e_lt += std::max(0, q.r1 - std::max(q.r0, q.c0 + c + 1));
    }
    for (const FoLBig& q : P.l_big) {
      ok = ok && q.nc >= 1 && q.nc <= kFoLCols && q.r0 < q.r1 && q.r1 <= q.f && q.r1 - q.r0 <= kFoLRows && q.part >= 0 && q.part + q.r1 <= P.l_parts;
      for (int j = q.c0; j < q.c0 + q.nc; ++j) e_l += std::max(0, q.r1 - std::max(q.r0, j + 1));
    }
    for (const FoLMerge& q : P.l_merge) ok = ok && q.gcb >= 0 && q.gcb + q.f <= nbig && q.r0 < q.f && q.part + (int64_t)((q.k + kFoLCols - 1) / kFoLCols) * q.f <= P.l_parts;
    for (int c = 0; c < n; ++c) ok = ok && seen[c] == 1;
    for (int s = 0; s < S.nsuper; ++s) if (S.sn_parent[s] >= 0) ok = ok && S.sn_level[s] < S.sn_level[S.sn_parent[s]];
    ok = ok && e_small + e_lt == P.entries && e_small + e_l == P.entries;
    if (!ok) { fprintf(stderr, "%s (ordering %d): the factor-product items do not tile the factor\n", name, ordering); return 1; }
  }
  // the records of the staged assembly, with the library's chunks and with one small enough for several chunks on every pattern
  for (int chunk : {512, 1024, 48})
    if (!check_asm_pieces(S, chunk)) { fprintf(stderr, "%s (ordering %d): the assembly pieces do not tile the extend-add items (chunk %d)\n", name, ordering, chunk); return 1; }
  // the sets of the sparse right-hand sides (solve_sparse_host.cpp): what runs is closed under the parent relation and made of whole
  // units, the fringe is exactly the children of running fronts that do not run, the counts add up; repeated batches on one set of marks
  {
    SparseWork W;
    sparse_host_setup(S, o, W);
    std::mt19937 rng(n + ordering);
    for (int trial = 0; trial < 8; ++trial) {
      std::vector<int> b(trial == 7 ? n : 1 + (int)(rng() % 5)), x(trial % 2 ? 1 + (int)(rng() % 5) : 0);
      for (size_t t = 0; t < b.size(); ++t) b[t] = trial == 7 ? (int)t : (int)(rng() % n);
      for (int& v : x) v = (int)(rng() % n);
      SparseSets A;
      sparse_reach(S, W, b.data(), (int64_t)b.size(), x.data(), (int64_t)x.size(), x.empty(), A);
      std::vector<char> fr(S.nsuper, 0), br(S.nsuper, 0);
      for (int s : A.fwd_fronts) fr[s] = 1;
      for (int s = 0; s < S.nsuper; ++s) br[s] = A.bwd_full || W.brun[s] == W.epoch;
      bool ok = (int64_t)A.fwd_fronts.size() == A.fwd_run && A.fwd_run >= A.fwd_reach && A.bwd_run >= A.bwd_reach && A.fwd_full == (A.fwd_run == S.nsuper);
      for (int v : b) ok = ok && fr[S.col2sn[v]];
      for (int v : x) ok = ok && br[S.col2sn[v]];
      int64_t fringe = 0, fentries = 0, bonly = 0;
      for (int s = 0; s < S.nsuper; ++s) {
        const int p = S.sn_parent[s];
        if (fr[s]) ok = ok && (p < 0 || fr[p]) && fr[W.U.unit_root[s]];
        if (br[s]) ok = ok && (p < 0 || br[p]) && br[W.U.unit_root[s]];
        if (!fr[s] && p >= 0 && fr[p]) { ++fringe; fentries += (S.row_ptr[s + 1] - S.row_ptr[s]) - (S.sn_col0[s + 1] - S.sn_col0[s]); }
        if (br[s] && !fr[s]) ++bonly;
      }
      ok = ok && fringe == A.fringe && fentries == A.fringe_entries && fringe == (int64_t)A.fringe_fronts.size() && bonly == (int64_t)A.bwd_only_fronts.size();
      if (trial == 7) ok = ok && A.fwd_full && A.fringe == 0;
      if (!ok) { fprintf(stderr, "%s (ordering %d): the sets of a sparse solve are not closed or miscounted (trial %d)\n", name, ordering, trial); return 1; }
    }
  }
  // the grids of a uniform batch (batch_host.cpp): with a limit that every front passes, every level holds at least one task, the levels
  // hold every task once and no level's largest front exceeds the plan's; one row less and the plan is refused, nothing counted
  {
    BatchShape B, C;
    batch_shape(S, (int)S.max_front, B);
    batch_shape(S, (int)S.max_front - 1, C);
    int64_t cnt = 0;
    bool ok = B.reason == OKKT_BATCH_OK && B.levels >= 1 && (int)B.level_cnt.size() == B.levels && (int)B.level_maxf.size() == B.levels && B.tasks <= S.nsuper;
    for (int l = 0; ok && l < B.levels; ++l) {
      ok = B.level_cnt[l] >= 1 && B.level_maxf[l] >= 1 && B.level_maxf[l] <= S.max_front;
      cnt += B.level_cnt[l];
    }
    ok = ok && cnt == B.tasks && C.reason == OKKT_BATCH_BIG_FRONTS && C.tasks == 0 && C.levels == 0;
    ok = ok && batch_slot_doubles(S, S.arena_doubles, 4) - batch_slot_doubles(S, S.arena_doubles, 1) == 3 * (2 * S.n + S.sum_r) &&
         batch_arena_stride(S, S.arena_doubles) % 2 == 0 && batch_arena_stride(S, S.arena_doubles) >= S.arena_doubles + 512 + 2 * S.max_front;
    if (!ok) { fprintf(stderr, "%s (ordering %d): the grids of a batch do not hold every task once\n", name, ordering); return 1; }
  }
  // the grids of a scenario batch (batch_host.cpp): without a set the plan is refused for that; with the last three variables held back the
  // Schur front is the last supernode and in no level -- with a limit that every interior front passes every interior unit is a task, one row
  // less and the interior is refused, and a set above the bound of the assembly is refused behind the interior's fronts
  if (n > 8) {
    SchurBatchShape Q;
    schur_batch_shape(S, (int)S.max_front, Q);
    bool ok = Q.reason == OKKT_SBATCH_NO_SET && Q.tasks == 0;
    const int64_t idx[3] = {n - 3, n - 2, n - 1};
    Symbolic T;
    const std::string e2 = analyze_pattern(n, cp.data(), ri.data(), 0, o, nullptr, T, idx, 3);
    if (!e2.empty()) { fprintf(stderr, "%s (ordering %d), Schur set: %s\n", name, ordering, e2.c_str()); return 1; }
    int maxf = 0;
    for (int s = 0; s + 1 < T.nsuper; ++s) maxf = std::max(maxf, (int)(T.row_ptr[s + 1] - T.row_ptr[s]));
    SchurBatchShape A, C;
    schur_batch_shape(T, maxf, A);
    schur_batch_shape(T, maxf - 1, C);
    ok = ok && T.nschur == 3 && A.reason == OKKT_SBATCH_OK && A.ns == 3 && A.max_front == maxf && A.levels >= 1 && A.tasks >= A.levels && A.tasks <= T.nsuper - 1;
    ok = ok && C.reason == OKKT_SBATCH_BIG_FRONTS && C.tasks == 0 && C.levels == 0;
    ok = ok && schur_batch_item_doubles(3, 4) == 12 + 1 && schur_batch_shared_doubles(3) >= 2 * 9;
    if (!ok) { fprintf(stderr, "%s (ordering %d): the grids of a scenario batch are miscounted\n", name, ordering); return 1; }
  }
  printf("%-12s ordering %d: n %d nnz(L) %lld supernodes %zu, %zu dataflow tasks\n", name, ordering, n, (long long)S.nnzL, S.sn_col0.size() - 1, ntask);
  return 0;
}

// The host arithmetic behind the reductions of the step-side functions (ls_finish.h), stepped once on what a launch can return: ordinary
// numbers, NaN in either argument of Julia's min / max, a zero norm under a fractional exponent, the non-finite bounds that fall back to
// (0, -1), a reset interval whose ub stays at -1, no constraints (m = 0: no complementarity penalty) and a NaN least-squares step.
static int check_ls_finish() {
  int bad = 0;
  auto fail = [&](const char* what) { fprintf(stderr, "ls_finish: %s\n", what); ++bad; };
  if (jl_min(1.0, 2.0) != 1.0 || jl_max(1.0, 2.0) != 2.0 || !std::isnan(jl_min(NAN, 1.0)) || !std::isnan(jl_min(1.0, NAN)) || !std::isnan(jl_max(NAN, 1.0)) ||
      !std::isnan(jl_max(1.0, NAN)) || jl_min(-INFINITY, 1.0) != -INFINITY)
    fail("jl_min / jl_max");
  if (thres_scalar(4.0, 0.5) != 8.0 || thres_scalar(0.0, 0.5) != 0.0 || !std::isnan(thres_scalar(NAN, 0.5)) || thres_scalar(INFINITY, 0.5) != INFINITY) fail("thres_scalar");
  if (step_from_ratio(4.0) != 0.25 || step_from_ratio(INFINITY) != 0.0 || !std::isnan(step_from_ratio(NAN))) fail("step_from_ratio");
  double lb = 0.0, ub = 0.0;
  { const double r[4] = {0.25, 0.75, -1.0, 2.0}; dual_range_finish(r, &lb, &ub); if (lb != 0.25 || ub != 0.5) fail("dual range, ordinary"); }
  { const double r[4] = {0.25, 0.75, -1.0, 1.0}; dual_range_finish(r, &lb, &ub); if (lb != 0.25 || ub != 0.75) fail("dual range, ratio 1"); }
  { const double r[4] = {INFINITY, 0.75, -1.0, 2.0}; dual_range_finish(r, &lb, &ub); if (lb != 0.0 || ub != -1.0) fail("dual range, lb = Inf"); }
  { const double r[4] = {0.25, NAN, -1.0, 2.0}; dual_range_finish(r, &lb, &ub); if (lb != 0.0 || ub != -1.0) fail("dual range, ub = NaN"); }
  { const double r[4] = {0.0, -1.0, 16.0, 1.0}; dual_range_finish(r, &lb, &ub); if (lb != 0.0 || ub != -1.0) fail("dual range, behind a reset"); }
  { const double r[4] = {0.25, 0.75, -1.0, NAN}; dual_range_finish(r, &lb, &ub); if (lb != 0.25 || !std::isnan(ub)) fail("dual range, NaN ratio"); }
  double out[4];
  { const double rm[3] = {2.0, 3.0, 4.0}, rn[2] = {-1.0, 6.0};
    predicted_reduction_finish(5, rm, rn, 0.5, 0.5, out);
    if (out[0] != 0.5 * -1.0 + 0.25 * 0.5 * 8.0 || out[1] != 3.0 || out[2] != 4.0 || out[3] != out[0] + (64.0 - 27.0) / 0.25) fail("predicted reduction");
    predicted_reduction_finish(0, rm, rn, 0.0, 0.5, out);
    if (out[3] != out[0]) fail("predicted reduction, m = 0"); }
  { const double rm[3] = {2.0, 3.0, NAN}, rn[2] = {-1.0, 6.0};
    predicted_reduction_finish(5, rm, rn, 0.5, 1.0, out);
    if (out[1] != 3.0 || !std::isnan(out[2]) || !std::isnan(out[3]) || out[0] != -1.0 + 0.5 * 8.0) fail("predicted reduction, NaN"); }
  if (dual_small_step(0.25, 0.75, 0.5) != 0.5 || dual_small_step(0.25, 0.75, 2.0) != 0.75 || dual_small_step(0.25, 0.1, 2.0) != 0.25) fail("dual_small_step");
  { const double rn[2] = {1.0, 2.0}, rm[2] = {2.0, 2.0};
    if (dual_step_finish(rn, rm, 1.0, 0.1) != 0.75 || dual_step_finish(rn, rm, 0.5, 0.1) != 0.5 || dual_step_finish(rn, rm, 1.0, 0.9) != 0.9) fail("dual_step_finish"); }
  { const double rn[2] = {0.0, 0.0}, rm[2] = {0.0, 0.0};
    if (!std::isnan(dual_step_finish(rn, rm, 1.0, 0.1))) fail("dual_step_finish, 0 / 0"); }
  if (!bad) printf("ls_finish    min / max, threshold, dual range, predicted reduction and dual step clean\n");
  return bad;
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
  {   // three leaf cliques under a separator of 2300 nodes that their elimination makes dense (natural ordering): a root front of three
      // 1024-row chunks whose children's contribution blocks cover every row, every second row and a scattered third of the rows
    const int nl = 30, nsep = 2300, n = 3 * nl + nsep;
    std::set<std::pair<int, int>> e;
    for (int g = 0; g < 3; ++g) {
      for (int i = 0; i < nl; ++i) for (int j = i + 1; j < nl; ++j) e.insert({g * nl + i, g * nl + j});
      for (int i = 0; i < nl; ++i)
        for (int r = 0; r < nsep; ++r)
          if (g == 0 || r == 0 || (g == 1 && r % 2 == 1) || (g == 2 && (r % 3 == 2 || (r > 1020 && r < 1030)))) e.insert({g * nl + i, 3 * nl + r});
    }
    bad += run("three-chunks", n, e, 1);
  }
  bad += check_tridiag();
  bad += check_sym_eig();
  bad += check_items_loop();
  bad += check_delta_seq();
  bad += check_ls_finish();
  if (bad) { fprintf(stderr, "%d case(s) failed\n", bad); return 1; }
  printf("asan driver: all cases clean\n");
  return 0;
}
