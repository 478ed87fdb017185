// C ABI, linear-solver level: residuals and refinement with extra-precise residuals (refine.hip), on the plain
// route and through the Schur set (section 8.9), and GMRES-based refinement (krylov.hip, section 8.6): the drivers and their entry points.
#include <cmath>
#include <cstring>

#include "api_internal.h"

using namespace okkt;

namespace okkt {

int route_solve_enqueue(okkt_solver_s* h, bool schur_route, const double* d_rhs, double* d_sol, int64_t nrhs) {
  return schur_route ? schur_dense_sweeps(h, d_rhs, d_sol, nrhs, true, false) : solver_solve_enqueue(h, d_rhs, d_sol, nrhs, false);
}

int refine_ready(okkt_solver_s* h, bool need_factor) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  if (h->S.nparts > 1) return refuse_partitioned(h);
  if (need_factor) {
    if (schur_mode(h)) return schur_refuse(h, "refinement");
    if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
    if (!h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "refinement called before a factorisation");
  }
  return ensure_row_map(h, "refinement map");
}

int refine_work(okkt_solver_s* h, int64_t len, int64_t nom) {
  auto grow = [&](double** p, int64_t* have, int64_t want) -> bool {
    if (*have >= want) return true;
    (void)hipStreamSynchronize(h->stream);
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    if (hipMalloc((void**)p, (size_t)std::max<int64_t>(want, 2) * sizeof(double)) != hipSuccess) { *p = nullptr; return false; }
    *have = want;
    return true;
  };
  if (!grow(&h->rf_work, &h->rf_work_len, len) || !grow(&h->rf_om, &h->rf_om_len, nom))
    return solver_set_error(h, OKKT_ERR_ALLOC, "refinement work vectors: hipMalloc failed");
  return OKKT_OK;
}

static double nan_max(double a, double b) { return (a != a || b != b) ? NAN : std::max(a, b); }

// r = b - A x and omega for nrhs right-hand sides (device pointers, checked handle); omega_out host [nrhs] or NULL
static int residual_device(okkt_solver_s* h, const double* d_nzval, const double* d_b, const double* d_x, double* d_r, int64_t nrhs,
                           double* omega_out) {
  const int64_t n = h->S.n;
  int rc = refine_work(h, 0, 2 * nrhs);
  if (rc != OKKT_OK) return rc;
  hipStream_t st = h->stream;
  refine_gather_enqueue(h->rf, d_nzval, st);
  for (int64_t q0 = 0; q0 < nrhs; q0 += 4) {
    const int nr = (int)std::min<int64_t>(4, nrhs - q0);
    ResidSet S;
    for (int s = 0; s < 4; ++s) {
      const int64_t q = q0 + std::min(s, nr - 1);
      S.b[s] = d_b + q * n; S.x[s] = d_x + q * n; S.r[s] = d_r + q * n; S.om[s] = h->rf_om + 2 * q;
    }
    refine_residual_enqueue(h->rf, S, nr, st);
  }
  std::vector<double> om((size_t)(2 * nrhs));
  if ((rc = stream_read(h, om.data(), h->rf_om, om.size() * sizeof(double), "residual")) != OKKT_OK) return rc;
  if (omega_out) for (int64_t q = 0; q < nrhs; ++q) omega_out[q] = om[(size_t)(2 * q)];
  return OKKT_OK;
}

// the refinement loop over one of two solves: the factor of the whole matrix (solver_solve_enqueue), or, schur_route, the fused
// whole-system sweeps of okkt_schur_solve
static int refine_loop(okkt_solver_s* h, bool schur_route, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                       double tol, okkt_refine_info* info, double* omega_out, void (*lap)(void*, int), void* lap_ctx, int* n_solves_out) {
  if (n_solves_out) *n_solves_out = 0;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (max_steps < 0) return solver_set_error(h, OKKT_ERR_INVALID, "max_steps < 0");
  int rc = schur_route ? schur_refine_ready(h) : refine_ready(h, true);
  if (rc != OKKT_OK) return rc;
  auto solve = [&](const double* src, double* dst, int64_t cnt) { return route_solve_enqueue(h, schur_route, src, dst, cnt); };
  if (!(tol > 0.0)) tol = std::ldexp(1.0, -52);
  const int64_t n = h->S.n;
  okkt_refine_info I;
  std::memset(&I, 0, sizeof(I));
  if (nrhs == 0 || n == 0) {
    if (info) *info = I;
    if (omega_out) for (int64_t q = 0; q < nrhs; ++q) omega_out[q] = 0.0;
    return OKKT_OK;
  }
  if ((rc = refine_work(h, 4 * nrhs * n, 2 * nrhs)) != OKKT_OK) return rc;
  double* B = h->rf_work;            // the right-hand sides (rhs may alias sol)
  double* R = B + nrhs * n;          // residuals of the active right-hand sides, packed
  double* D = R + nrhs * n;          // their corrections, packed
  double* XP = D + nrhs * n;         // the iterate before the last correction, per right-hand side
  hipStream_t st = h->stream;
  auto mark = [&](int tag) { if (lap) lap(lap_ctx, tag); };
  int nsolves = 0;
  if ((rc = hip_check(h, hipMemcpyAsync(B, d_rhs, (size_t)(nrhs * n) * sizeof(double), hipMemcpyDeviceToDevice, st), "refinement rhs copy")) != OKKT_OK) return rc;
  refine_gather_enqueue(h->rf, d_nzval, st);
  mark(1);
  if ((rc = solve(B, d_sol, nrhs)) != OKKT_OK) return rc;   // x = F \ b: the batches of okkt_solve / okkt_schur_solve
  nsolves += (int)nrhs;
  mark(0);
  const size_t Q = (size_t)nrhs;
  std::vector<double> w0(Q, 0.0), wprev(Q, 0.0), rprev(Q, 0.0), wbest(Q, 0.0), rbest(Q, 0.0), om(2 * Q);
  std::vector<int> steps(Q, 0), status(Q, 0);
  std::vector<int64_t> act(Q);
  for (size_t q = 0; q < Q; ++q) act[q] = (int64_t)q;
  for (int it = 0; !act.empty(); ++it) {
    // omega of every active right-hand side; slot k of R belongs to act[k]
    for (size_t k0 = 0; k0 < act.size(); k0 += 4) {
      const int nr = (int)std::min<size_t>(4, act.size() - k0);
      ResidSet S;
      for (int s = 0; s < 4; ++s) {
        const size_t k = k0 + (size_t)std::min(s, nr - 1);
        const int64_t q = act[k];
        S.b[s] = B + q * n; S.x[s] = d_sol + q * n; S.r[s] = R + (int64_t)k * n; S.om[s] = h->rf_om + 2 * q;
      }
      refine_residual_enqueue(h->rf, S, nr, st);
    }
    if ((rc = stream_read(h, om.data(), h->rf_om, 2 * Q * sizeof(double), "refinement residual")) != OKKT_OK) return rc;    // the one device-to-host read of a step
    mark(1);
    std::vector<int64_t> next, next_slot;
    for (size_t k = 0; k < act.size(); ++k) {
      const size_t q = (size_t)act[k];
      const double w = om[2 * q], ri = om[2 * q + 1];
      if (it == 0) w0[q] = w;
      // the previous iterate is the better one: back to it (the last correction is undone)
      auto restore = [&]() -> int {
        wbest[q] = wprev[q]; rbest[q] = rprev[q]; --steps[q];
        return hip_check(h, hipMemcpyAsync(d_sol + (int64_t)q * n, XP + (int64_t)q * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st), "refinement restore");
      };
      if (!std::isfinite(w) || !std::isfinite(ri)) {
        status[q] = 3;
        if (it > 0) { if ((rc = restore()) != OKKT_OK) return rc; }
        else { wbest[q] = w; rbest[q] = ri; }
      } else if (w <= tol) {
        status[q] = 0; wbest[q] = w; rbest[q] = ri;
      } else if (it > 0 && w > 0.5 * wprev[q]) {
        status[q] = 2;
        if (w > wprev[q]) { if ((rc = restore()) != OKKT_OK) return rc; }
        else { wbest[q] = w; rbest[q] = ri; }
      } else if (it >= max_steps) {
        status[q] = 1; wbest[q] = w; rbest[q] = ri;
      } else {
        wprev[q] = w; rprev[q] = ri;
        next.push_back((int64_t)q);
        next_slot.push_back((int64_t)k);
      }
    }
    if (next.empty()) break;
    // the residuals of the right-hand sides that go on, to the front of R (slot k' <= k: nothing unread is overwritten)
    for (size_t k = 0; k < next.size(); ++k)
      if (next_slot[k] != (int64_t)k) {
        rc = hip_check(h, hipMemcpyAsync(R + (int64_t)k * n, R + next_slot[k] * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st), "refinement compaction");
        if (rc != OKKT_OK) return rc;
      }
    mark(1);
    if ((rc = solve(R, D, (int64_t)next.size())) != OKKT_OK) return rc;   // d = F \ r
    nsolves += (int)next.size();
    mark(0);
    // masked correction: only the right-hand sides that go on are touched (no solve of a zero rhs: 0 * NaN is not 0)
    for (size_t k0 = 0; k0 < next.size(); k0 += 4) {
      const int nr = (int)std::min<size_t>(4, next.size() - k0);
      UpdateSet U;
      for (int s = 0; s < 4; ++s) {
        const size_t k = k0 + (size_t)std::min(s, nr - 1);
        const int64_t q = next[k];
        U.x[s] = d_sol + q * n; U.xp[s] = XP + q * n; U.d[s] = D + (int64_t)k * n;
      }
      refine_update_enqueue(n, U, nr, st);
    }
    for (int64_t q : next) ++steps[(size_t)q];
    act.swap(next);
  }
  for (size_t q = 0; q < Q; ++q) {
    if (q == 0) { I.omega0 = w0[q]; I.omega = wbest[q]; I.resid_inf = rbest[q]; }
    else { I.omega0 = nan_max(I.omega0, w0[q]); I.omega = nan_max(I.omega, wbest[q]); I.resid_inf = nan_max(I.resid_inf, rbest[q]); }
    I.steps = std::max(I.steps, steps[q]);
    I.status = std::max(I.status, status[q]);
    if (omega_out) omega_out[q] = wbest[q];
  }
  if (info) *info = I;
  if (n_solves_out) *n_solves_out = nsolves;
  return hip_check(h, hipStreamSynchronize(st), "refinement");
}

int solver_refine_device(okkt_solver_s* h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                         double tol, okkt_refine_info* info, double* omega_out, void (*lap)(void*, int), void* lap_ctx, int* n_solves_out) {
  return refine_loop(h, false, d_nzval, d_rhs, d_sol, nrhs, max_steps, tol, info, omega_out, lap, lap_ctx, n_solves_out);
}

// ---- GMRES-based iterative refinement (krylov.hip) ---------------------------------------------

namespace {
constexpr double kGmresInnerTol = OKKT_GMRES_INNER_TOL;

// the host side of one right-hand side's GMRES cycle: the rotated Hessenberg columns, the rotations and the rotated beta e_1
struct GmresCycle {
  std::vector<double> H;     // column j at j * kKryCol: R's column after the rotations
  std::vector<double> cs, sn, g;
  double beta = 0;
  int m = 0;                 // columns kept (the correction uses V[0..m))
  int cap = 0;               // iterations this cycle may take
  bool live = false;
};

// take column j (h[0..j+1]) into the cycle; false when the cycle ends with it (the column is kept only if it is usable)
bool gmres_take_column(GmresCycle& c, int j, const double* h) {
  for (int i = 0; i <= j + 1; ++i)
    if (!std::isfinite(h[i])) return false;    // not kept: the correction uses the columns before it
  double* col = c.H.data() + (size_t)j * kKryCol;
  for (int i = 0; i <= j + 1; ++i) col[i] = h[i];
  for (int i = 0; i < j; ++i) {
    const double t = c.cs[(size_t)i] * col[i] + c.sn[(size_t)i] * col[i + 1];
    col[i + 1] = -c.sn[(size_t)i] * col[i] + c.cs[(size_t)i] * col[i + 1];
    col[i] = t;
  }
  const double d = std::hypot(col[j], col[j + 1]);
  if (!(d > 0.0) || !std::isfinite(d)) return false;
  c.cs[(size_t)j] = col[j] / d;
  c.sn[(size_t)j] = col[j + 1] / d;
  col[j] = d;
  col[j + 1] = 0.0;
  c.g[(size_t)j + 1] = -c.sn[(size_t)j] * c.g[(size_t)j];
  c.g[(size_t)j] = c.cs[(size_t)j] * c.g[(size_t)j];
  c.m = j + 1;
  const bool happy = !(h[j + 1] > 0.0);
  return !(std::fabs(c.g[(size_t)j + 1]) <= kGmresInnerTol * c.beta || c.m >= c.cap || happy);
}

// y = R^-1 g[0..m) by back substitution
void gmres_solve_y(const GmresCycle& c, double* y) {
  for (int i = c.m - 1; i >= 0; --i) {
    double s = c.g[(size_t)i];
    for (int k = i + 1; k < c.m; ++k) s -= c.H[(size_t)k * kKryCol + i] * y[k];
    y[i] = s / c.H[(size_t)i * kKryCol + i];
  }
}
}  // namespace

int solver_gmres_device(okkt_solver_s* h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                        int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out, bool schur_route) {
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (max_iters < 0) return solver_set_error(h, OKKT_ERR_INVALID, "max_iters < 0");
  if (restart > kKryMaxRestart) return solver_set_error(h, OKKT_ERR_INVALID, "restart > 64");
  if (restart <= 0) restart = 30;
  int rc = schur_route ? schur_route_ready(h) : refine_ready(h, true);
  if (rc != OKKT_OK) return rc;
  if (!(tol > 0.0)) tol = std::ldexp(1.0, -52);
  const int64_t n = h->S.n;
  okkt_gmres_info I;
  std::memset(&I, 0, sizeof(I));
  if (nrhs == 0 || n == 0) {
    I.work_bytes = h->kr.bytes;
    if (info) *info = I;
    if (omega_out) for (int64_t q = 0; q < nrhs; ++q) omega_out[q] = 0.0;
    return OKKT_OK;
  }
  std::string e = krylov_alloc(n, restart, h->kr);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "GMRES workspace: " + e);
  const KrylovWork& K = h->kr;
  hipStream_t st = h->stream;
  const int64_t vstride = 4 * n;    // V is [restart + 1][4][n]
  refine_gather_enqueue(h->rf, d_nzval, st);
  const size_t Q = (size_t)nrhs;
  std::vector<double> w0(Q, 0.0), wbest(Q, 0.0), rbest(Q, 0.0);
  std::vector<int> iters(Q, 0), cycles(Q, 0), status(Q, 0);
  std::vector<double> rd(4 * kKryCol + 16);     // the one read of a step: K.col and, behind it, K.om
  int nsolves = 0;
  for (int64_t q0 = 0; q0 < nrhs; q0 += 4) {
    const int G = (int)std::min<int64_t>(4, nrhs - q0);
    double* X = d_sol + q0 * n;                  // system g of the group: column q0 + g
    if ((rc = hip_check(h, hipMemcpyAsync(K.B, d_rhs + q0 * n, (size_t)(G * n) * sizeof(double), hipMemcpyDeviceToDevice, st), "GMRES rhs copy")) != OKKT_OK) return rc;
    if ((rc = route_solve_enqueue(h, schur_route, K.B, X, G)) != OKKT_OK) return rc;   // x = F \ b: okkt_solve's / okkt_schur_solve's batch
    ++nsolves;
    double wprev[4] = {0, 0, 0, 0}, rprev[4] = {0, 0, 0, 0};
    std::vector<int> act;                        // systems of the group that go on; outer slot k belongs to act[k]
    for (int g = 0; g < G; ++g) act.push_back(g);
    GmresCycle cyc[4];
    for (int it = 0; !act.empty(); ++it) {
      const int na = (int)act.size();
      ResidSet S;
      KrySet NS;
      for (int s = 0; s < 4; ++s) {
        const int k = std::min(s, na - 1), g = act[(size_t)k];
        S.b[s] = K.B + g * n; S.x[s] = X + g * n; S.r[s] = K.R + k * n; S.om[s] = K.om + 2 * k;
        NS.v[s] = K.V; NS.w[s] = K.R + k * n;
      }
      NS.vstride = vstride;
      refine_residual_enqueue(h->rf, S, na, st);
      krylov_norm_enqueue(K, NS, na, st);        // ||r||_2 to K.col[k][0]
      if ((rc = stream_read(h, rd.data(), K.col, rd.size() * sizeof(double), "GMRES residual")) != OKKT_OK) return rc;    // the one device-to-host read of an outer step
      const double* om = rd.data() + 4 * kKryCol;
      std::vector<int> next, next_slot;
      for (int k = 0; k < na; ++k) {
        const int g = act[(size_t)k];
        const size_t q = (size_t)(q0 + g);
        const double w = om[2 * k], ri = om[2 * k + 1], beta = rd[(size_t)k * kKryCol];
        if (it == 0) w0[q] = w;
        auto restore = [&]() -> int {      // the previous iterate is the better one: the last correction is undone
          wbest[q] = wprev[g]; rbest[q] = rprev[g];
          return hip_check(h, hipMemcpyAsync(X + g * n, K.XP + g * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st), "GMRES restore");
        };
        if (!std::isfinite(w) || !std::isfinite(ri) || !std::isfinite(beta)) {
          status[q] = 3;
          if (it > 0) { if ((rc = restore()) != OKKT_OK) return rc; }
          else { wbest[q] = w; rbest[q] = ri; }
        } else if (w <= tol) {
          status[q] = 0; wbest[q] = w; rbest[q] = ri;
        } else if (it > 0 && w > 0.5 * wprev[g]) {
          status[q] = 2;
          if (w > wprev[g]) { if ((rc = restore()) != OKKT_OK) return rc; }
          else { wbest[q] = w; rbest[q] = ri; }
        } else if (iters[q] >= max_iters) {
          status[q] = 1; wbest[q] = w; rbest[q] = ri;
        } else {
          wprev[g] = w; rprev[g] = ri;
          next.push_back(g);
          next_slot.push_back(k);
        }
      }
      if (next.empty()) break;
      // one GMRES cycle for the systems that go on; cycle slot c belongs to next[c].  v_0 = r / ||r||_2
      const int C = (int)next.size();
      KryScale SC;
      for (int s = 0; s < 4; ++s) {
        const int c = std::min(s, C - 1);
        SC.src[s] = K.R + next_slot[(size_t)c] * n; SC.dst[s] = K.V + c * n; SC.div[s] = K.col + (size_t)next_slot[(size_t)c] * kKryCol;
      }
      for (int c = 0; c < C; ++c) {
        const size_t q = (size_t)(q0 + next[(size_t)c]);
        GmresCycle& cy = cyc[c];
        cy.H.assign((size_t)restart * kKryCol, 0.0);
        cy.cs.assign((size_t)restart, 0.0); cy.sn.assign((size_t)restart, 0.0); cy.g.assign((size_t)restart + 1, 0.0);
        cy.beta = rd[(size_t)next_slot[(size_t)c] * kKryCol];
        cy.g[0] = cy.beta;
        cy.m = 0;
        cy.cap = std::min(restart, max_iters - iters[q]);
        cy.live = true;
        ++cycles[q];
      }
      krylov_scale_enqueue(n, SC, C, st);
      for (int j = 0;; ++j) {
        std::vector<int> live;
        for (int c = 0; c < C; ++c) if (cyc[c].live) live.push_back(c);
        if (live.empty()) break;
        const int nl = (int)live.size();
        const double* Vj = K.V + (int64_t)j * vstride;
        const double* zin = Vj;               // the live systems' v_j, contiguous when they are a prefix of the slots
        if (live.back() != nl - 1) {
          for (int k = 0; k < nl; ++k) {
            rc = hip_check(h, hipMemcpyAsync(K.P + k * n, Vj + live[(size_t)k] * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st), "GMRES pack");
            if (rc != OKKT_OK) return rc;
          }
          zin = K.P;
        }
        if ((rc = route_solve_enqueue(h, schur_route, zin, K.Z, nl)) != OKKT_OK) return rc;   // z = F^-1 v_j
        ++nsolves;
        ResidSet OS;
        KrySet AS;
        for (int s = 0; s < 4; ++s) {
          const int k = std::min(s, nl - 1);
          OS.b[s] = K.zero; OS.x[s] = K.Z + k * n; OS.r[s] = K.W + k * n; OS.om[s] = K.om + 8 + 2 * k;
          AS.v[s] = K.V + live[(size_t)k] * n; AS.w[s] = K.W + k * n;
        }
        AS.vstride = vstride;
        refine_residual_enqueue(h->rf, OS, nl, st);   // W = 0 - A z: -(A z) in double-double, rounded once
        krylov_dots_enqueue(K, AS, nl, j + 1, true, st);
        krylov_orth_dots_enqueue(K, AS, nl, j + 1, true, st);
        krylov_orth_norm_enqueue(K, AS, nl, j + 1, st);
        if ((rc = stream_read(h, rd.data(), K.col, (size_t)nl * kKryCol * sizeof(double), "GMRES iteration")) != OKKT_OK) return rc;    // the one device-to-host read of an iteration
        KryScale NV;
        int nn = 0;
        for (int k = 0; k < nl; ++k) {
          const int c = live[(size_t)k];
          GmresCycle& cy = cyc[c];
          const bool more = gmres_take_column(cy, j, rd.data() + (size_t)k * kKryCol);
          ++iters[(size_t)(q0 + next[(size_t)c])];
          if (!more) { cy.live = false; continue; }
          NV.src[nn] = K.W + k * n; NV.dst[nn] = K.V + (int64_t)(j + 1) * vstride + c * n; NV.div[nn] = K.col + (size_t)k * kKryCol + (j + 1);
          ++nn;
        }
        for (int s = nn; s < 4; ++s) { NV.src[s] = NV.src[0]; NV.dst[s] = NV.dst[0]; NV.div[s] = NV.div[0]; }
        if (nn > 0) krylov_scale_enqueue(n, NV, nn, st);   // v_j+1 = w / h_j+1,j
      }
      // x += F^-1 (V y) for the systems whose cycle kept a column
      KryCombine CB;
      CB.vstride = vstride;
      std::vector<int> upd;
      for (int c = 0; c < C; ++c) {
        if (cyc[c].m == 0) continue;
        const int e2 = (int)upd.size();
        CB.v[e2] = K.V + c * n; CB.u[e2] = K.U + e2 * n; CB.m[e2] = cyc[c].m;
        gmres_solve_y(cyc[c], CB.y[e2]);
        upd.push_back(c);
      }
      const int ne = (int)upd.size();
      if (ne > 0) {
        for (int s = ne; s < 4; ++s) { CB.v[s] = CB.v[0]; CB.u[s] = CB.u[0]; CB.m[s] = 0; }
        krylov_combine_enqueue(n, CB, ne, st);
        if ((rc = route_solve_enqueue(h, schur_route, K.U, K.Z, ne)) != OKKT_OK) return rc;   // d = F^-1 (V y)
        ++nsolves;
        UpdateSet U;
        for (int s = 0; s < 4; ++s) {
          const int k = std::min(s, ne - 1), g = next[(size_t)upd[(size_t)k]];
          U.x[s] = X + g * n; U.xp[s] = K.XP + g * n; U.d[s] = K.Z + k * n;
        }
        refine_update_enqueue(n, U, ne, st);
      }
      act.swap(next);
    }
  }
  for (size_t q = 0; q < Q; ++q) {
    if (q == 0) { I.omega0 = w0[q]; I.omega = wbest[q]; I.resid_inf = rbest[q]; }
    else { I.omega0 = nan_max(I.omega0, w0[q]); I.omega = nan_max(I.omega, wbest[q]); I.resid_inf = nan_max(I.resid_inf, rbest[q]); }
    I.iterations = std::max(I.iterations, iters[q]);
    I.cycles = std::max(I.cycles, cycles[q]);
    I.status = std::max(I.status, status[q]);
    if (omega_out) omega_out[q] = wbest[q];
  }
  I.solves = nsolves;
  I.work_bytes = K.bytes;
  if (info) *info = I;
  return hip_check(h, hipStreamSynchronize(st), "GMRES");
}
}  // namespace okkt

// the host-pointer form of a solve with refinement: nzval and the right-hand sides staged, body(d_nzval, d_rhs = d_sol), the solutions back
template <class F>
static int staged_solve(okkt_solver_s* h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, const char* upload, F&& body) {
  const int64_t len = h->S.n * nrhs;
  if (len == 0) return body(nullptr, nullptr);
  int rc = stage_nzval(h, nzval, upload);
  if (rc == OKKT_OK) rc = stage_reserve(h, len);
  if (rc == OKKT_OK) rc = stage_upload(h, h->d_rhs_stage, rhs, len, upload);
  if (rc == OKKT_OK) rc = body(h->rf.nz_stage, h->d_rhs_stage);
  if (rc == OKKT_OK) rc = stage_download(h, sol, h->d_rhs_stage, len, "sol download failed");
  return rc;
}

// okkt_solve_refine_dev / okkt_solve_refine and their twins through the Schur set
static int refine_dev_entry(okkt_handle h, bool schur_route, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                            double tol, okkt_refine_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs > 0 && (!d_rhs || !d_sol || (!d_nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, schur_route ? "okkt_schur_solve_refine_dev" : "okkt_solve_refine_dev",
               [&] { return refine_loop(h, schur_route, d_nzval, d_rhs, d_sol, nrhs, max_steps, tol, info, omega_out, nullptr, nullptr, nullptr); });
}

static int refine_host_entry(okkt_handle h, bool schur_route, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t max_steps,
                             double tol, okkt_refine_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (max_steps < 0) return solver_set_error(h, OKKT_ERR_INVALID, "max_steps < 0");
  if (nrhs > 0 && (!rhs || !sol || (!nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, schur_route ? "okkt_schur_solve_refine" : "okkt_solve_refine", [&]() -> int {
    int rc = schur_route ? schur_refine_ready(h) : refine_ready(h, true);
    if (rc != OKKT_OK) return rc;
    return staged_solve(h, nzval, rhs, sol, nrhs, "refinement upload", [&](const double* d_nzval, double* d_x) {
      return refine_loop(h, schur_route, d_nzval, d_x, d_x, nrhs, max_steps, tol, info, omega_out, nullptr, nullptr, nullptr);
    });
  });
}

// okkt_solve_gmres_dev / okkt_solve_gmres and their twins through the Schur route
static int gmres_dev_entry(okkt_handle h, bool schur_route, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                           int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs > 0 && (!d_rhs || !d_sol || (!d_nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, schur_route ? "okkt_schur_solve_gmres_dev" : "okkt_solve_gmres_dev",
               [&] { return solver_gmres_device(h, d_nzval, d_rhs, d_sol, nrhs, restart, max_iters, tol, info, omega_out, schur_route); });
}

static int gmres_host_entry(okkt_handle h, bool schur_route, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t restart,
                            int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (max_iters < 0) return solver_set_error(h, OKKT_ERR_INVALID, "max_iters < 0");
  if (restart > kKryMaxRestart) return solver_set_error(h, OKKT_ERR_INVALID, "restart > 64");
  if (nrhs > 0 && (!rhs || !sol || (!nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, schur_route ? "okkt_schur_solve_gmres" : "okkt_solve_gmres", [&]() -> int {
    int rc = schur_route ? schur_route_ready(h) : refine_ready(h, true);
    if (rc != OKKT_OK) return rc;
    return staged_solve(h, nzval, rhs, sol, nrhs, "GMRES upload", [&](const double* d_nzval, double* d_x) {
      return solver_gmres_device(h, d_nzval, d_x, d_x, nrhs, restart, max_iters, tol, info, omega_out, schur_route);
    });
  });
}

extern "C" {

int okkt_residual_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, double* d_r, int64_t nrhs,
                      double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_residual_dev", [&]() -> int {
    int rc = refine_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (nrhs == 0) return OKKT_OK;
    if ((!d_nzval && h->S.nnz_in > 0) || !d_rhs || !d_x || !d_r) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
    return residual_device(h, d_nzval, d_rhs, d_x, d_r, nrhs, omega_out);
  });
}

int okkt_residual(okkt_handle h, const double* nzval, const double* rhs, const double* x, double* r, int64_t nrhs, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_residual", [&]() -> int {
    int rc = refine_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (nrhs == 0) return OKKT_OK;
    if ((!nzval && h->S.nnz_in > 0) || !rhs || !x || !r) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
    const int64_t len = nrhs * h->S.n;
    if ((rc = stage_nzval(h, nzval, "residual upload")) != OKKT_OK) return rc;
    if ((rc = refine_work(h, 3 * len, 2 * nrhs)) != OKKT_OK) return rc;
    double* db = h->rf_work;
    double* dxv = db + len;
    double* dr = dxv + len;
    if ((rc = stage_upload(h, db, rhs, len, "residual upload")) != OKKT_OK) return rc;
    if ((rc = stage_upload(h, dxv, x, len, "residual upload")) != OKKT_OK) return rc;
    if ((rc = residual_device(h, h->rf.nz_stage, db, dxv, dr, nrhs, omega_out)) != OKKT_OK) return rc;
    return stage_download(h, r, dr, len, "residual download failed");
  });
}

int okkt_debug_row_map(okkt_handle h, int64_t out[6]) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_debug_row_map", [&]() -> int {
    int rc = refine_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (!out) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
    const RefineMap& M = h->rf;
    out[0] = M.lpr; out[1] = M.long_min; out[2] = M.nb_short; out[3] = M.nlong; out[4] = M.ndup; out[5] = M.nnz;
    return OKKT_OK;
  });
}

int okkt_solve_refine_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                          double tol, okkt_refine_info* info, double* omega_out) {
  return refine_dev_entry(h, false, d_nzval, d_rhs, d_sol, nrhs, max_steps, tol, info, omega_out);
}

int okkt_schur_solve_refine_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                                double tol, okkt_refine_info* info, double* omega_out) {
  return refine_dev_entry(h, true, d_nzval, d_rhs, d_sol, nrhs, max_steps, tol, info, omega_out);
}

int okkt_solve_refine(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t max_steps, double tol,
                      okkt_refine_info* info, double* omega_out) {
  return refine_host_entry(h, false, nzval, rhs, sol, nrhs, max_steps, tol, info, omega_out);
}

int okkt_schur_solve_refine(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t max_steps, double tol,
                            okkt_refine_info* info, double* omega_out) {
  return refine_host_entry(h, true, nzval, rhs, sol, nrhs, max_steps, tol, info, omega_out);
}

int okkt_solve_gmres_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                         int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_dev_entry(h, false, d_nzval, d_rhs, d_sol, nrhs, restart, max_iters, tol, info, omega_out);
}

int okkt_schur_solve_gmres_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                               int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_dev_entry(h, true, d_nzval, d_rhs, d_sol, nrhs, restart, max_iters, tol, info, omega_out);
}

int okkt_solve_gmres(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t restart, int32_t max_iters,
                     double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_host_entry(h, false, nzval, rhs, sol, nrhs, restart, max_iters, tol, info, omega_out);
}

int okkt_schur_solve_gmres(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t restart, int32_t max_iters,
                           double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_host_entry(h, true, nzval, rhs, sol, nrhs, restart, max_iters, tol, info, omega_out);
}

}  // extern "C"
