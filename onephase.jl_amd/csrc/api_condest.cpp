// C ABI, linear-solver level: condition estimation and forward error bounds (condest.hip), on the plain route and
// through the Schur route (section 8.10): the Higham-Tisseur estimator's host side, the two drivers and their entry points.
#include <cmath>
#include <cstring>

#include "api_internal.h"

using namespace okkt;

namespace okkt {

// device, analysis, no partition, a complete factorisation; the refinement map and the estimator's blocks
static int condest_ready(okkt_solver_s* h, bool schur_route = false) {
  if (schur_route) {
    int rc = schur_route_ready(h);
    if (rc != OKKT_OK) return rc;
  } else {
    if (schur_mode(h)) return schur_refuse(h, "the condition estimate / forward error bound");
    int rc = refine_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (!h->numeric_ready || !h->factored)
      return solver_set_error(h, OKKT_ERR_INVALID, "condition estimate called before a complete factorisation (none yet, or an early exit stopped it)");
  }
  std::string e = condest_alloc(h->S.n, h->cd);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "condition estimator blocks: " + e);
  return OKKT_OK;
}

// Higham-Tisseur Algorithm 2.4 for op = diag(f) F^-1 (f NULL: F^-1), op' = F^-1 diag(f), t columns (1 <= t <= min(n, 4)).  Y = op X and
// Z = op' S are one solve pass each, every pass followed by one read of the small buffer W.out (first: its copy at the first read,
// which carries what was enqueued before the estimate: ||F||_1, ||x||_inf).  est: the estimate (Inf for status 3).
static int condest_run(okkt_solver_s* h, bool schur_route, int t, const double* f, double* est_out, int* iters_out, int* solves_out,
                       int* status_out, double* first) {
  CondestWork& W = h->cd;
  const int64_t n = h->S.n;
  const int64_t H = std::min<int64_t>(n, 4);
  hipStream_t st = h->stream;
  double out[kCdOut];
  bool have_first = false;
  auto read = [&]() -> int {
    int rc = stream_read(h, out, W.out, sizeof(out), "condition estimate");
    if (rc != OKKT_OK) return rc;
    if (!have_first && first) std::memcpy(first, out, sizeof(out));
    have_first = true;
    return OKKT_OK;
  };
  h->cd_hist.clear();
  int rc = hip_check(h, hipMemsetAsync(W.used, 0, (size_t)((n + 31) / 32) * 4, st), "condition estimate");
  if (rc != OKKT_OK) return rc;
  condest_start_enqueue(W, t, st);
  // the class of a +-1 column: its first H entries, normalised to a leading +1 (condest.h)
  auto cls_of = [&](int a) {
    int c = 0;
    for (int64_t r = 1; r < H; ++r)
      if (out[kCdY + 37 + a * 4 + r] != out[kCdY + 37 + a * 4]) c |= 1 << (r - 1);
    return c;
  };
  const int ncls = 1 << (H - 1);
  double est = 0.0, est_old = 0.0;
  int64_t ind_best = -1;
  int64_t ind[4] = {-1, -1, -1, -1};
  int cls_old[4] = {0, 0, 0, 0};
  int cur = 0, solves = 0, iters = 0, status = 1;
  bool has_old = false;
  uint64_t next_draw = (uint64_t)t;
  const double dn = (double)n;
  for (int k = 1;; ++k) {
    if ((rc = route_solve_enqueue(h, schur_route, W.X, W.Y, t)) != OKKT_OK) return rc;    // Y = F^-1 X
    ++solves;
    condest_ystats_enqueue(W, t, cur, has_old, f, st);
    if ((rc = read()) != OKKT_OK) return rc;
    if (out[kCdY + 4] != 0.0) { status = 3; est = INFINITY; break; }
    int jb = 0;
    for (int j = 1; j < t; ++j)
      if (out[kCdY + j] > out[kCdY + jb]) jb = j;
    const double e = out[kCdY + jb];
    if ((e > est_old || k == 2) && k >= 2) ind_best = ind[jb];
    if (k >= 2 && e <= est_old) { est = est_old; status = 0; break; }
    est = est_old = e;
    if (k > kCondestItmax) { status = 1; break; }
    // every column of S parallel to a column of S_old: converged
    auto par_old = [&](int a) {
      if (!has_old) return false;
      for (int c = 0; c < t; ++c)
        if (std::fabs(out[kCdY + 21 + a * 4 + c]) == dn) return true;
      return false;
    };
    bool all_par = has_old;
    for (int a = 0; a < t && all_par; ++a) all_par = par_old(a);
    if (all_par) { status = 0; break; }
    // a column parallel to an earlier one or to one of S_old: replaced by a generator column of a head class no other column has
    int cls[4] = {0, 0, 0, 0};
    bool repl[4] = {false, false, false, false};
    for (int a = 0; a < t; ++a) cls[a] = cls_of(a);
    if (t > 1)
      for (int a = 0; a < t; ++a) {
        bool par = par_old(a);
        for (int b = 0; b < a && !par; ++b) par = !repl[b] && std::fabs(out[kCdY + 5 + a * 4 + b]) == dn;
        if (!par) continue;
        for (int c = 0; c < ncls; ++c) {
          bool taken = false;
          for (int b = 0; b < t; ++b) taken = taken || (b != a && cls[b] == c) || (has_old && cls_old[b] == c);
          if (taken) continue;
          condest_resample_enqueue(W, cur, a, next_draw++, c, f, st);
          cls[a] = c;
          repl[a] = true;
          break;
        }
      }
    for (int a = 0; a < t; ++a) cls_old[a] = cls[a];
    if ((rc = route_solve_enqueue(h, schur_route, f ? W.SF : W.S[cur], W.Y, t)) != OKKT_OK) return rc;   // Z = F^-1 diag(f) S
    ++solves;
    ++iters;
    condest_zstats_enqueue(W, t, k >= 2 ? ind_best : -1, st);
    if ((rc = read()) != OKKT_OK) return rc;
    if (out[kCdZ + 17] != 0.0) { status = 3; est = INFINITY; break; }
    if (k >= 2 && out[kCdZ] == out[kCdZ + 16]) { status = 0; break; }
    auto used = [&](int64_t i) { return std::find(h->cd_hist.begin(), h->cd_hist.end(), i) != h->cd_hist.end(); };
    auto row = [&](int off) -> int64_t {
      const double v = out[off];
      return (v >= 0.0 && v < dn) ? (int64_t)v : -1;
    };
    CdIdx nx;
    bool stop = false;
    if (t > 1) {
      bool all_used = true;
      for (int r = 0; r < t; ++r) { const int64_t i = row(kCdZ + 4 + r); all_used = all_used && i >= 0 && used(i); }
      if (all_used) { status = 0; break; }
      for (int r = 0; r < t; ++r) {
        ind[r] = row(kCdZ + 12 + r);
        if (ind[r] < 0) stop = true;      // fewer than t unused rows are left
      }
    } else {
      ind[0] = row(kCdZ + 4);
      stop = ind[0] < 0;
    }
    if (stop) { status = 0; break; }
    for (int r = 0; r < 4; ++r) nx.i[r] = r < t ? ind[r] : -1;
    condest_scatter_enqueue(W, t, nx, st);
    for (int r = 0; r < t; ++r) h->cd_hist.push_back(ind[r]);
    has_old = true;
    cur ^= 1;
  }
  *est_out = est;
  *iters_out = iters;
  *solves_out = solves;
  *status_out = status;
  return OKKT_OK;
}

int solver_condest_device(okkt_solver_s* h, const double* d_nzval, int32_t t, okkt_condest_info* info, bool schur_route) {
  int rc = condest_ready(h, schur_route);
  if (rc != OKKT_OK) return rc;
  okkt_condest_info I;
  std::memset(&I, 0, sizeof(I));
  const int64_t n = h->S.n;
  h->cd_hist.clear();
  if (n == 0) { if (info) *info = I; return OKKT_OK; }
  t = t <= 0 ? 2 : std::min<int32_t>(t, kCondestMaxT);
  t = (int32_t)std::min<int64_t>(t, n);
  hipStream_t st = h->stream;
  refine_gather_enqueue(h->rf, d_nzval, st);
  condest_norm1_enqueue(h->rf, h->cd, h->N.d.diagadd, h->N.d.perm, st);
  double first[kCdOut], est = 0.0;
  if ((rc = condest_run(h, schur_route, t, nullptr, &est, &I.iterations, &I.solves, &I.status, first)) != OKKT_OK) return rc;
  I.norm1 = first[kCdN];
  I.inv_norm1 = est;
  I.cond1 = I.status == 3 ? INFINITY : I.norm1 * est;
  if (info) *info = I;
  return OKKT_OK;
}

int solver_forward_error_device(okkt_solver_s* h, const double* d_nzval, const double* d_b, const double* d_x, int64_t nrhs, double* ferr_out,
                                double* berr_out, bool schur_route) {
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  int rc = condest_ready(h, schur_route);
  if (rc != OKKT_OK) return rc;
  const int64_t n = h->S.n;
  h->cd_hist.clear();
  if (nrhs == 0) return OKKT_OK;
  if (n == 0) {
    for (int64_t q = 0; q < nrhs; ++q) { ferr_out[q] = 0.0; if (berr_out) berr_out[q] = 0.0; }
    return OKKT_OK;
  }
  if ((rc = refine_work(h, 0, 2 * nrhs)) != OKKT_OK) return rc;
  CondestWork& W = h->cd;
  hipStream_t st = h->stream;
  const int t = (int)std::min<int64_t>(2, n);
  refine_gather_enqueue(h->rf, d_nzval, st);
  for (int64_t q0 = 0; q0 < nrhs; q0 += 4) {
    const int nr = (int)std::min<int64_t>(4, nrhs - q0);
    ResidSet S;
    DenSet D;
    for (int s = 0; s < 4; ++s) {
      const int k = std::min(s, nr - 1);
      const int64_t q = q0 + k;
      S.b[s] = d_b + q * n; S.x[s] = d_x + q * n; S.r[s] = W.R + (int64_t)k * n; S.om[s] = h->rf_om + 2 * q;
      D.d[s] = W.DEN + (int64_t)k * n;
    }
    refine_residual_den_enqueue(h->rf, S, D, nr, st);   // r and (|A||x| + |b|) of the refinement's residual pass
    for (int k = 0; k < nr; ++k) {
      const int64_t q = q0 + k;
      condest_fweights_enqueue(h->rf, W, W.R + (int64_t)k * n, W.DEN + (int64_t)k * n, d_x + q * n, st);
      double first[kCdOut], est = 0.0;
      int iters = 0, solves = 0, status = 0;
      if ((rc = condest_run(h, schur_route, t, W.f, &est, &iters, &solves, &status, first)) != OKKT_OK) return rc;
      const double xn = first[kCdN + 2];
      ferr_out[q] = status == 3 ? INFINITY : (xn > 0.0 ? est / xn : (xn == 0.0 ? est : NAN));
    }
  }
  std::vector<double> om((size_t)(2 * nrhs));
  if ((rc = stream_read(h, om.data(), h->rf_om, om.size() * sizeof(double), "forward error")) != OKKT_OK) return rc;
  if (berr_out) for (int64_t q = 0; q < nrhs; ++q) berr_out[q] = om[(size_t)(2 * q)];
  return OKKT_OK;
}

}  // namespace okkt

// okkt_condest_dev / okkt_condest and their twins through the Schur route
static int condest_dev_entry(okkt_handle h, bool schur_route, const double* d_nzval, int32_t t, okkt_condest_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  if (!d_nzval && h->S.nnz_in > 0) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "the condition estimate", [&] { return solver_condest_device(h, d_nzval, t, info, schur_route); });
}

static int condest_host_entry(okkt_handle h, bool schur_route, const double* nzval, int32_t t, okkt_condest_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  if (!nzval && h->S.nnz_in > 0) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "the condition estimate", [&]() -> int {
    int rc = condest_ready(h, schur_route);
    if (rc == OKKT_OK) rc = stage_nzval(h, nzval, "nzval upload");
    return rc != OKKT_OK ? rc : solver_condest_device(h, h->rf.nz_stage, t, info, schur_route);
  });
}

// okkt_forward_error_dev / okkt_forward_error and their twins through the Schur route
static int ferr_dev_entry(okkt_handle h, bool schur_route, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs, double* ferr_out,
                          double* berr_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs > 0 && (!d_rhs || !d_x || !ferr_out || (!d_nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "the forward error bound", [&] { return solver_forward_error_device(h, d_nzval, d_rhs, d_x, nrhs, ferr_out, berr_out, schur_route); });
}

static int ferr_host_entry(okkt_handle h, bool schur_route, const double* nzval, const double* rhs, const double* x, int64_t nrhs, double* ferr_out,
                           double* berr_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!rhs || !x || !ferr_out || (!nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "the forward error bound", [&]() -> int {
    int rc = condest_ready(h, schur_route);
    if (rc != OKKT_OK) return rc;
    const int64_t len = nrhs * h->S.n;
    if ((rc = stage_nzval(h, nzval, "forward error upload")) != OKKT_OK) return rc;
    if ((rc = refine_work(h, 2 * len, 2 * nrhs)) != OKKT_OK) return rc;
    double* db = h->rf_work;
    double* dxv = db + len;
    if ((rc = stage_upload(h, db, rhs, len, "forward error upload")) != OKKT_OK) return rc;
    if ((rc = stage_upload(h, dxv, x, len, "forward error upload")) != OKKT_OK) return rc;
    return solver_forward_error_device(h, h->rf.nz_stage, db, dxv, nrhs, ferr_out, berr_out, schur_route);
  });
}

extern "C" {

int okkt_condest_dev(okkt_handle h, const double* d_nzval, int32_t t, okkt_condest_info* info) { return condest_dev_entry(h, false, d_nzval, t, info); }
int okkt_schur_condest_dev(okkt_handle h, const double* d_nzval, int32_t t, okkt_condest_info* info) { return condest_dev_entry(h, true, d_nzval, t, info); }
int okkt_condest(okkt_handle h, const double* nzval, int32_t t, okkt_condest_info* info) { return condest_host_entry(h, false, nzval, t, info); }
int okkt_schur_condest(okkt_handle h, const double* nzval, int32_t t, okkt_condest_info* info) { return condest_host_entry(h, true, nzval, t, info); }

int64_t okkt_condest_indices(okkt_handle h, int64_t* ind_out, int64_t cap) {
  if (!h || (cap > 0 && !ind_out)) return OKKT_ERR_INVALID;
  const int64_t cnt = (int64_t)h->cd_hist.size();
  for (int64_t i = 0; i < std::min(cnt, cap); ++i) ind_out[i] = h->cd_hist[(size_t)i];
  return cnt;
}

int okkt_forward_error_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs, double* ferr_out,
                           double* berr_out) {
  return ferr_dev_entry(h, false, d_nzval, d_rhs, d_x, nrhs, ferr_out, berr_out);
}

int okkt_schur_forward_error_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs, double* ferr_out,
                                 double* berr_out) {
  return ferr_dev_entry(h, true, d_nzval, d_rhs, d_x, nrhs, ferr_out, berr_out);
}

int okkt_forward_error(okkt_handle h, const double* nzval, const double* rhs, const double* x, int64_t nrhs, double* ferr_out,
                       double* berr_out) {
  return ferr_host_entry(h, false, nzval, rhs, x, nrhs, ferr_out, berr_out);
}

int okkt_schur_forward_error(okkt_handle h, const double* nzval, const double* rhs, const double* x, int64_t nrhs, double* ferr_out,
                             double* berr_out) {
  return ferr_host_entry(h, true, nzval, rhs, x, nrhs, ferr_out, berr_out);
}

}  // extern "C"
