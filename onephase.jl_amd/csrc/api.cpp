// C ABI, linear-solver level (include/okkt.h): the entry points a
// `linear_solver_HIP <: abstract_linear_system_solver` binds in place of linear_solver_JULIA
// (/root/reference/src/linear_system_solvers/julia.jl).  No exception leaves this file.
#include <algorithm>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "solver.h"

using namespace okkt;

// the Schur route of the refinement loop (defined with the Schur-mode entry points below)
extern "C" {
static int schur_refine_ready(okkt_solver_s* h);
static int schur_dense_sweeps(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs, bool whole, bool sync = true);
}

namespace okkt {

int solver_set_error(okkt_solver_s* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

static int ensure_device(okkt_solver_s* h) {
  if (h->opts.host_symbolic_only) return solver_set_error(h, OKKT_ERR_NO_DEVICE, "handle was created with host_symbolic_only");
  if (h->device_ready) {
    if (hipSetDevice(h->device) != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, "hipSetDevice failed");
    return OKKT_OK;
  }
  return solver_set_error(h, OKKT_ERR_NO_DEVICE, "no HIP device");
}

int solver_ensure_numeric(okkt_solver_s* h) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  if (h->numeric_ready) return OKKT_OK;
  h->N.part_id = h->part_id;
  h->N.stream_masked = h->stream_masked;     // before the set-up: the lanes of the plan are given streams there
  h->N.stream_panel = h->stream_panel;
  h->N.stream_aux = h->stream_aux;
  if (const char* fl = getenv("OKKT_FLOW")) h->N.flow = atoi(fl);   // read by the set-up
  if (const char* df = getenv("OKKT_DATAFLOW")) h->N.dataflow = atoi(df);
  if (const char* sf = getenv("OKKT_SOLVE_FLOW")) h->N.solve_flow = atoi(sf);   // read by the set-up (it sizes the partial-product buffers)
  if (const char* sw = getenv("OKKT_SOLVE_FUSE_WIDE_MAX")) h->N.solve_fuse_wide_max = atoi(sw);   // read by the set-up (the experiment keeps the explicit inverses for every front)
  std::string e = numeric_setup(h->S, h->sopts, h->stream, h->N);
  if (const char* sh = getenv("OKKT_SPLIT_HEAD")) h->N.split_head = atoi(sh);
  if (const char* d2 = getenv("OKKT_DIAG2")) h->N.diag2 = atoi(d2);
  if (const char* fd = getenv("OKKT_FUSE_DIAG_TRSM")) h->N.fuse_diag_trsm = atoi(fd);
  if (const char* ss = getenv("OKKT_SOLVE_SPLIT_SMALL")) h->N.solve_split_small = atoi(ss);
  if (const char* su = getenv("OKKT_SOLVE_FUSE")) h->N.solve_fuse = atoi(su);
  if (const char* mt = getenv("OKKT_LA_MIN_TILES")) h->N.la_min_tiles = atoi(mt);
  if (!e.empty()) { numeric_release(h->N); return solver_set_error(h, OKKT_ERR_HIP, e); }
  h->numeric_ready = true;
  return OKKT_OK;
}

// A scaling is on: the refusals, the length of a caller's vector, and on the first scaled factorisation after
// an analysis the row map of the pattern (the one the refinement calls build) and the workspace
static int scaling_prepare(okkt_solver_s* h) {
  ScalingWork& W = h->sc;
  if (schur_mode(h)) return solver_set_error(h, OKKT_ERR_INVALID, "a scaling is set: Schur mode cannot factor a scaled matrix (okkt_set_scaling with OKKT_SCALE_NONE first)");
  if (h->S.nparts > 1) return solver_set_error(h, OKKT_ERR_INVALID, "a scaling is set: a partitioned handle cannot factor a scaled matrix (okkt_set_scaling with OKKT_SCALE_NONE first)");
  if (W.mode == OKKT_SCALE_USER && (int64_t)W.user.size() != h->S.n)
    return solver_set_error(h, OKKT_ERR_INVALID, "the scaling vector of okkt_set_scaling was given for another dimension than the analysed one");
  if (!h->rf.ready) {
    std::string e = refine_map_build(h->S.n, h->pat_colptr.data(), h->pat_rowval.data(), h->pat_colptr[0], h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, "scaling: row map: " + e);
  }
  if (!W.ready) {
    std::string e = scaling_alloc(W, h->S.n, h->pat_colptr.data(), h->pat_rowval.data(), h->pat_colptr[0]);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "scaling workspace: " + e);
  }
  if (W.mode == OKKT_SCALE_USER && !W.user_uploaded && W.n > 0) {
    hipError_t he = hipMemcpyAsync(W.s[0], W.user.data(), (size_t)W.n * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("scaling vector upload: ") + hipGetErrorString(he));
    W.user_uploaded = true;
  }
  return OKKT_OK;
}

int solver_factor_device(okkt_solver_s* h, const double* d_vals, int64_t n, int64_t m, int sym_kind,
                         okkt_inertia* out, bool zero_tol) {
  int rc = solver_ensure_numeric(h);
  if (rc != OKKT_OK) return rc;
  const bool scaled = h->sc.mode != OKKT_SCALE_NONE;
  const int64_t order = h->S.n - h->S.nschur;     // the pivots factored: A11's in Schur mode (its front is assembled, not factored)
  if (n < 0 || m < 0 || n + m != order) return solver_set_error(h, OKKT_ERR_INVALID, "n + m does not match the analysed dimension");
  if (sym_kind != OKKT_SYM_DEFINITE && sym_kind != OKKT_SYM_SYMMETRIC) return solver_set_error(h, OKKT_ERR_INVALID, "unknown sym_kind");
  if (sym_kind == OKKT_SYM_DEFINITE && m != 0) return solver_set_error(h, OKKT_ERR_INVALID, ":definite requires m == 0 (julia.jl:30)");
  const double tol = (sym_kind == OKKT_SYM_DEFINITE || zero_tol) ? 0.0 : h->opts.inertia_tol;
  h->factored = false;
  ++h->factor_seq;     // a selected inverse of the previous factor is stale from here on
  h->sc.valid = false;
  if (scaled && (rc = scaling_prepare(h)) != OKKT_OK) return rc;     // (behind the argument checks: it may overwrite the previous factor's s)
  h->N.early_check = h->early_exit && h->S.nschur == 0;
  h->N.early_device = h->early_exit && h->last_failed;   // the previous factorisation failed the inertia: this one is a retry
  h->N.early_n = n;
  h->N.early_m = m;
  (void)hipEventRecord(h->ev0, h->stream);
  std::string e;
  double sc_out[kScaleOut] = {0.0, 0.0, 0.0, 0.0};
  if (scaled) {
    // s, then S F S into the workspace; the assembly adds the scaled shift.  The unscaled shift stays the handle's (okkt_condest reads it)
    scaling_enqueue(h->sc, h->rf, d_vals, h->N.d.diagadd, h->N.d.perm, h->stream);
    double* const shift = h->N.d.diagadd;
    h->N.d.diagadd = h->sc.dadd;
    e = numeric_factor_enqueue(h->N, h->sc.vals, tol);
    h->N.d.diagadd = shift;
  } else {
    e = numeric_factor_enqueue(h->N, d_vals, tol);
  }
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
  (void)hipEventRecord(h->ev1, h->stream);
  if (scaled && h->sc.n > 0 && hipMemcpyAsync(sc_out, h->sc.out, sizeof(sc_out), hipMemcpyDeviceToHost, h->stream) != hipSuccess)
    return solver_set_error(h, OKKT_ERR_HIP, "scaling: read of the row-maximum extrema failed");
  unsigned long long cnt[6];
  e = numeric_read_counts(h->N, h->stream, cnt);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, std::string("numeric factorisation failed: ") + e);
  if (cnt[5] != 0)      // distinct from an inertia failure: callers of the delta loop must not shift and retry on it
    return solver_set_error(h, OKKT_ERR_INTERNAL, "a hand-off inside a launch timed out: the pivot counts are incomplete and there is no factor");
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_factor_ms = ms;
  okkt_inertia in;
  in.pos = (int64_t)cnt[0]; in.neg = (int64_t)cnt[1]; in.zero = (int64_t)cnt[2]; in.nonfinite = (int64_t)cnt[3];
  if (out) *out = in;
  h->a11_inertia = in;
  h->last_failed = true;
  if (h->N.early_exited || cnt[4] != 0) return 0;   // wrong inertia decided before the end: counts are partial, no factor to solve with
  h->factored = true;
  if (scaled) {
    h->sc.valid = true;
    h->sc.info.mode = h->sc.mode;
    h->sc.info.sweeps = h->sc.mode == OKKT_SCALE_RUIZ ? h->sc.sweeps : 0;
    h->sc.info.rowmax_min = sc_out[3] > 0.0 ? sc_out[0] : 0.0;
    h->sc.info.rowmax_max = sc_out[1];
    h->sc.info.zero_rows = (int64_t)sc_out[2];
  }
  if (in.pos + in.neg + in.zero + in.nonfinite != order)
    return solver_set_error(h, OKKT_ERR_INTERNAL, "pivot counts do not add up to the matrix order");
  if (in.nonfinite > 0) return 0;                       // julia.jl:77-89
  const int flag = sym_kind == OKKT_SYM_DEFINITE ? (in.pos == n ? 1 : 0)   // PosDefException <=> some pivot <= 0
                                                 : ((in.pos == n && in.neg == m) ? 1 : 0);   // linear_system_solvers.jl:73-74
  h->last_failed = flag == 0;
  return flag;
}

int solver_solve_enqueue(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs, bool accumulate) {
  int rc = solver_ensure_numeric(h);
  if (rc != OKKT_OK) return rc;
  if (!h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "solve called before a factorisation");
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  // a scaled factor: x = S F~^-1 S b, the two multiplications inside the permutation gather and scatter
  const double* sc = h->sc.valid ? h->sc.s_cur : nullptr;
  // batches of up to kMaxRhs right-hand sides: one pass over L per batch (R = 1, 2 or 4 kernels; three are padded to four)
  for (int64_t r = 0; r < nrhs;) {
    const int nr = (int)std::min<int64_t>(nrhs - r, kMaxRhs);
    const int R = nr >= 3 ? 4 : nr;
    solve_permute_in(h->N, d_rhs + r * h->S.n, h->S.n, nr, R, sc);
    std::string e = numeric_solve_enqueue(h->N, R);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    solve_permute_out(h->N, d_sol + r * h->S.n, h->S.n, nr, R, accumulate, sc);
    r += nr;
  }
  return OKKT_OK;
}

int solver_solve_device(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs) {
  (void)hipEventRecord(h->ev0, h->stream);
  int rc = solver_solve_enqueue(h, d_rhs, d_sol, nrhs, false);
  if (rc != OKKT_OK) return rc;
  (void)hipEventRecord(h->ev1, h->stream);
  hipError_t he = hipStreamSynchronize(h->stream);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("solve failed: ") + hipGetErrorString(he));
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_solve_ms = ms;
  return OKKT_OK;
}

// A^-1 for the drivers that run on either route: the factor of the whole matrix, or, schur_route, the fused
// whole-system sweeps of okkt_schur_solve.  No synchronisation
static int route_solve_enqueue(okkt_solver_s* h, bool schur_route, const double* d_rhs, double* d_sol, int64_t nrhs) {
  return schur_route ? ::schur_dense_sweeps(h, d_rhs, d_sol, nrhs, true, false) : solver_solve_enqueue(h, d_rhs, d_sol, nrhs, false);
}

// the Schur route's gate: a device, then the rules of okkt_schur_solve_refine
static int schur_route_ready(okkt_solver_s* h) {
  int rc = ensure_device(h);
  return rc != OKKT_OK ? rc : ::schur_refine_ready(h);
}

// ---- refinement with extra-precise residuals (refine.hip) ------------------------------------

void solver_refine_release(okkt_solver_s* h) {
  refine_map_release(h->rf);
  condest_release(h->cd);
  selinv_release(h->sl);
  pivots_release(h->pv);
  krylov_release(h->kr);
  dense_ldlt_release(h->dl);
  scaling_release(h->sc);
  h->cd_hist.clear();
  if (h->rf_work) (void)hipFree(h->rf_work);
  if (h->rf_om) (void)hipFree(h->rf_om);
  h->rf_work = nullptr; h->rf_work_len = 0;
  h->rf_om = nullptr; h->rf_om_len = 0;
}

// device, analysis, no partition; the row map of the pattern on the first call after an analysis
static int refine_ready(okkt_solver_s* h, bool need_factor) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  if (h->S.nparts > 1)
    return solver_set_error(h, OKKT_ERR_INVALID, "residuals and refinement are not available on a partitioned handle (okkt_dist_set_partition with nparts > 1)");
  if (need_factor) {
    if (schur_mode(h)) return schur_refuse(h, "refinement");
    if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
    if (!h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "refinement called before a factorisation");
  }
  if (!h->rf.ready) {
    std::string e = refine_map_build(h->S.n, h->pat_colptr.data(), h->pat_rowval.data(), h->pat_colptr[0], h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, "refinement map: " + e);
  }
  return OKKT_OK;
}

// work vectors of the handle: len doubles and nom (omega, |r|) pairs' doubles (grown, never shrunk until the next analysis)
static int refine_work(okkt_solver_s* h, int64_t len, int64_t nom) {
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
  hipError_t he = hipMemcpyAsync(om.data(), h->rf_om, (size_t)(2 * nrhs) * sizeof(double), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("residual: ") + hipGetErrorString(he));
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
  int rc = schur_route ? ::schur_refine_ready(h) : refine_ready(h, true);
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
  hipError_t he = hipMemcpyAsync(B, d_rhs, (size_t)(nrhs * n) * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("refinement rhs copy: ") + hipGetErrorString(he));
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
    he = hipMemcpyAsync(om.data(), h->rf_om, 2 * Q * sizeof(double), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);    // the one device-to-host read of a step
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("refinement residual: ") + hipGetErrorString(he));
    mark(1);
    std::vector<int64_t> next, next_slot;
    for (size_t k = 0; k < act.size(); ++k) {
      const size_t q = (size_t)act[k];
      const double w = om[2 * q], ri = om[2 * q + 1];
      if (it == 0) w0[q] = w;
      // the previous iterate is the better one: back to it (the last correction is undone)
      auto restore = [&]() -> int {
        hipError_t e2 = hipMemcpyAsync(d_sol + (int64_t)q * n, XP + (int64_t)q * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e2 != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("refinement restore: ") + hipGetErrorString(e2));
        wbest[q] = wprev[q]; rbest[q] = rprev[q]; --steps[q];
        return OKKT_OK;
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
        he = hipMemcpyAsync(R + (int64_t)k * n, R + next_slot[k] * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("refinement compaction: ") + hipGetErrorString(he));
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
  he = hipStreamSynchronize(st);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("refinement: ") + hipGetErrorString(he));
  return OKKT_OK;
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
  auto hip_fail = [&](hipError_t he, const char* what) { return solver_set_error(h, OKKT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(he)); };
  refine_gather_enqueue(h->rf, d_nzval, st);
  const size_t Q = (size_t)nrhs;
  std::vector<double> w0(Q, 0.0), wbest(Q, 0.0), rbest(Q, 0.0);
  std::vector<int> iters(Q, 0), cycles(Q, 0), status(Q, 0);
  std::vector<double> rd(4 * kKryCol + 16);     // the one read of a step: K.col and, behind it, K.om
  int nsolves = 0;
  for (int64_t q0 = 0; q0 < nrhs; q0 += 4) {
    const int G = (int)std::min<int64_t>(4, nrhs - q0);
    double* X = d_sol + q0 * n;                  // system g of the group: column q0 + g
    hipError_t he = hipMemcpyAsync(K.B, d_rhs + q0 * n, (size_t)(G * n) * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "GMRES rhs copy");
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
      he = hipMemcpyAsync(rd.data(), K.col, rd.size() * sizeof(double), hipMemcpyDeviceToHost, st);
      if (he == hipSuccess) he = hipStreamSynchronize(st);    // the one device-to-host read of an outer step
      if (he != hipSuccess) return hip_fail(he, "GMRES residual");
      const double* om = rd.data() + 4 * kKryCol;
      std::vector<int> next, next_slot;
      for (int k = 0; k < na; ++k) {
        const int g = act[(size_t)k];
        const size_t q = (size_t)(q0 + g);
        const double w = om[2 * k], ri = om[2 * k + 1], beta = rd[(size_t)k * kKryCol];
        if (it == 0) w0[q] = w;
        auto restore = [&]() -> int {      // the previous iterate is the better one: the last correction is undone
          hipError_t e2 = hipMemcpyAsync(X + g * n, K.XP + g * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st);
          if (e2 != hipSuccess) return hip_fail(e2, "GMRES restore");
          wbest[q] = wprev[g]; rbest[q] = rprev[g];
          return OKKT_OK;
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
            he = hipMemcpyAsync(K.P + k * n, Vj + live[(size_t)k] * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st);
            if (he != hipSuccess) return hip_fail(he, "GMRES pack");
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
        he = hipMemcpyAsync(rd.data(), K.col, (size_t)nl * kKryCol * sizeof(double), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);    // the one device-to-host read of an iteration
        if (he != hipSuccess) return hip_fail(he, "GMRES iteration");
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
  hipError_t he = hipStreamSynchronize(st);
  if (he != hipSuccess) return hip_fail(he, "GMRES");
  return OKKT_OK;
}

// ---- condition estimation and forward error bounds (condest.hip) -----------------------------

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
    hipError_t he = hipMemcpyAsync(out, W.out, sizeof(out), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("condition estimate: ") + hipGetErrorString(he));
    if (!have_first && first) std::memcpy(first, out, sizeof(out));
    have_first = true;
    return OKKT_OK;
  };
  h->cd_hist.clear();
  hipError_t he = hipMemsetAsync(W.used, 0, (size_t)((n + 31) / 32) * 4, st);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("condition estimate: ") + hipGetErrorString(he));
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
  int cur = 0, solves = 0, iters = 0, status = 1, rc;
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
  hipError_t he = hipMemcpyAsync(om.data(), h->rf_om, (size_t)(2 * nrhs) * sizeof(double), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("forward error: ") + hipGetErrorString(he));
  if (berr_out) for (int64_t q = 0; q < nrhs; ++q) berr_out[q] = om[(size_t)(2 * q)];
  return OKKT_OK;
}

int solver_set_scaling(okkt_solver_s* h, int mode, int32_t sweeps, const double* s_user) {
  if (mode != OKKT_SCALE_NONE && mode != OKKT_SCALE_RUIZ && mode != OKKT_SCALE_USER)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_scaling: unknown mode");
  if (mode == OKKT_SCALE_NONE) {      // the current factor, if scaled, stays what it is until the next factorisation
    h->sc.mode = OKKT_SCALE_NONE;
    return OKKT_OK;
  }
  if (schur_mode(h))
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_scaling: the handle is in Schur mode, which does not factor a scaled matrix (clear the set with okkt_set_schur, ns = 0)");
  if (h->analyzed && h->S.nparts > 1)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_scaling: the handle is partitioned (okkt_dist_set_partition with nparts > 1), a partitioned factorisation is not scaled");
  if (mode == OKKT_SCALE_RUIZ) {
    if (sweeps > kScaleMaxSweeps) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_scaling: sweeps > 64");
    h->sc.mode = OKKT_SCALE_RUIZ;
    h->sc.sweeps = sweeps <= 0 ? kScaleDefaultSweeps : sweeps;
    return OKKT_OK;
  }
  if (!s_user) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_scaling: OKKT_SCALE_USER needs the vector s_user (it is NULL)");
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_scaling: OKKT_SCALE_USER reads dim entries: okkt_analyze has not been called");
  for (int64_t i = 0; i < h->S.n; ++i)
    if (!(s_user[i] > 0.0) || !std::isfinite(s_user[i]))
      return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_scaling: s_user[" + std::to_string(i) + "] is not finite and positive");
  h->sc.user.assign(s_user, s_user + h->S.n);
  h->sc.user_uploaded = false;
  h->sc.mode = OKKT_SCALE_USER;
  return OKKT_OK;
}

}  // namespace okkt

extern "C" {

const char* okkt_version(void) {
  // (log=0: the product library; log=1: libonephase_kkt_log.so, whose dataflow kernel carries the task-log instrumentation)
  static const std::string v = std::string("onephase-kkt-mi355x 0.1 (gfx950; dataflow kernel: ") + okkt::df_build_flags() + ")";
  return v.c_str();
}

int okkt_default_opts(okkt_opts* o) {
  if (!o) return OKKT_ERR_INVALID;
  std::memset(o, 0, sizeof(*o));
  SymbolicOptions d;
  o->device = -1;
  o->host_symbolic_only = 0;
  o->ordering = 0;
  o->relax_always = d.relax_always;
  o->relax_small = d.relax_small;
  o->relax_mid = d.relax_mid;
  o->relax_small_frac = d.relax_small_frac;
  o->relax_mid_frac = d.relax_mid_frac;
  o->relax_any_frac = d.relax_any_frac;
  o->inertia_tol = 1e-20;
  o->small_front_max = 128;
  o->panel_nb = 128;
  o->early_exit = 0;
  o->schur_dense_rows = 0;
  return OKKT_OK;
}

// Stream sets are pooled per (device, look-ahead, reserved CUs) for the life of the process: a handle takes a set and
// gives it back in okkt_destroy.  Measured on MI355X: streams created after another set was destroyed (a second handle
// in the same process) ran the look-ahead schedule 13 % slower (62.9 vs 54.6 ms on the Schur-shape S-metric system)
// -- the runtime's hardware-queue assignment of later streams differs -- while a reused set keeps the first timing.
struct StreamSet {
  int device = -1, la = 0, reserved = 0, seq = 0;   // seq: order of creation in this process (1, 2, ...)
  hipStream_t stream = nullptr, masked = nullptr, panel = nullptr, aux = nullptr;
};
// heap objects that are never destructed: no static-destruction order to get wrong at process exit
static std::mutex& pool_mutex() { static std::mutex* m = new std::mutex; return *m; }
static std::vector<StreamSet>& pool_free() { static std::vector<StreamSet>* v = new std::vector<StreamSet>; return *v; }
static std::vector<StreamSet>& pool_all() { static std::vector<StreamSet>* v = new std::vector<StreamSet>; return *v; }
static bool g_pool_closed = false;

// At exit every stream of the pool is destroyed (in use or not): CU-masked and priority streams that are still alive
// when rocprofv3's tool library tears down crash it (exit code 139 after the traces were written); the handler is
// registered at the first okkt_create, i.e. after HIP's and the profiler's own, so it runs before them.
static void pool_close() {
  std::lock_guard<std::mutex> lock(pool_mutex());
  g_pool_closed = true;
  for (const StreamSet& set : pool_all()) {
    if (hipSetDevice(set.device) != hipSuccess) continue;
    for (hipStream_t q : {set.aux, set.panel, set.masked, set.stream})
      if (q) { (void)hipStreamSynchronize(q); (void)hipStreamDestroy(q); }
  }
  pool_all().clear();
  pool_free().clear();
}

static bool take_stream_set(int device, int la, int reserved, StreamSet* out) {
  std::lock_guard<std::mutex> lock(pool_mutex());
  std::vector<StreamSet>& fr = pool_free();
  // the OLDEST matching set: later sets share the hardware queues of the earlier ones (a part of the sharded model measured on
  // the third set of a process ran 2.5x slower than on the first), so a lone handle should always get the first one back
  long best = -1;
  for (size_t q = 0; q < fr.size(); ++q)
    if (fr[q].device == device && fr[q].la == la && fr[q].reserved == reserved && (best < 0 || fr[q].seq < fr[(size_t)best].seq)) best = (long)q;
  if (best < 0) return false;
  *out = fr[(size_t)best];
  fr.erase(fr.begin() + best);
  return true;
}
static int pool_size();
static void register_stream_set(const StreamSet& set) {
  std::lock_guard<std::mutex> lock(pool_mutex());
  static bool registered = false;
  if (!registered) { registered = true; (void)atexit(pool_close); }
  pool_all().push_back(set);
  pool_all().back().seq = (int)pool_all().size();
}
static int pool_size() { std::lock_guard<std::mutex> lock(pool_mutex()); return (int)pool_all().size(); }
static void give_stream_set(const StreamSet& set) {
  std::lock_guard<std::mutex> lock(pool_mutex());
  if (!g_pool_closed) pool_free().push_back(set);
}

int okkt_create(okkt_handle* out, const okkt_opts* opts) {
  if (!out) return OKKT_ERR_INVALID;
  *out = nullptr;
  okkt_solver_s* h = new (std::nothrow) okkt_solver_s();
  if (!h) return OKKT_ERR_ALLOC;
  okkt_opts def;
  okkt_default_opts(&def);
  h->opts = opts ? *opts : def;
  okkt_opts& o = h->opts;
  if (o.relax_always <= 0) o.relax_always = def.relax_always;
  if (o.relax_small <= 0) o.relax_small = def.relax_small;
  if (o.relax_mid <= 0) o.relax_mid = def.relax_mid;
  if (o.relax_small_frac <= 0) o.relax_small_frac = def.relax_small_frac;
  if (o.relax_mid_frac <= 0) o.relax_mid_frac = def.relax_mid_frac;
  if (o.relax_any_frac <= 0) o.relax_any_frac = def.relax_any_frac;
  if (o.inertia_tol < 0) o.inertia_tol = def.inertia_tol;
  if (o.small_front_max <= 0) o.small_front_max = def.small_front_max;
  if (o.panel_nb <= 0) o.panel_nb = def.panel_nb;
  h->sopts.ordering = o.ordering;
  h->sopts.relax_always = o.relax_always;
  h->sopts.relax_small = o.relax_small;
  h->sopts.relax_mid = o.relax_mid;
  h->sopts.relax_small_frac = o.relax_small_frac;
  h->sopts.relax_mid_frac = o.relax_mid_frac;
  h->sopts.relax_any_frac = o.relax_any_frac;
  h->sopts.small_front_max = o.small_front_max;
  h->sopts.panel_nb = o.panel_nb;
  h->early_exit = o.early_exit != 0;
  if (!o.host_symbolic_only) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { delete h; return OKKT_ERR_NO_DEVICE; }
    int dev = o.device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= count || hipSetDevice(dev) != hipSuccess) { delete h; return OKKT_ERR_NO_DEVICE; }
    h->device = dev;
    // Look-ahead needs a CU that the trailing update never occupies (k_big_diag wants a whole CU's LDS): levels that
    // use it run on a twin of the handle's stream whose CU mask leaves out the first `reserved` CUs (mask bit b =
    // CU b / 8 of XCD b % 8 on gfx950, probed with scripts/cumask_probe.hip); the panel streams are unmasked and high
    // priority.  Everything else (small fronts, levels without look-ahead, the solves) keeps all CUs.
    const char* ela = getenv("OKKT_LOOKAHEAD");
    const char* ercu = getenv("OKKT_RESERVED_CUS");
    const int la = ela ? atoi(ela) : 1;
    // 32 = one CU of every shader engine of every XCD (mask bit b = CU index b / 8 of XCD b % 8, CU index c in shader engine c % 4:
    // scripts/cumask_map.hip).  The hardware deals workgroups to the shader engines round-robin and IN ORDER: with an uneven mask
    // (round 4: 8 = one CU per XCD) the engine that lost a CU fills up first and the dispatch stalls behind it -- 460 of 496 workgroups
    // resident in scripts/occ_probe.hip, as few as 393 in situ -- so reserving one CU per engine costs the masked stream nothing more
    int reserved = ercu ? atoi(ercu) : 32;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { delete h; return OKKT_ERR_HIP; }
    const int ncu = prop.multiProcessorCount;
    if (reserved < 1) reserved = 1;
    if (reserved > ncu / 2) reserved = ncu / 2;
    StreamSet set;
    if (take_stream_set(dev, la ? 1 : 0, reserved, &set)) {
      h->stream = set.stream; h->stream_masked = set.masked; h->stream_panel = set.panel; h->stream_aux = set.aux;
      h->stream_seq = set.seq;
    } else if (la) {
      std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
      for (int b = reserved; b < ncu; ++b) mask[(size_t)b >> 5] |= 1u << (b & 31);
      int lo = 0, hi = 0;
      if (hipExtStreamCreateWithCUMask(&h->stream_masked, (uint32_t)mask.size(), mask.data()) != hipSuccess ||
          hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
          hipStreamCreateWithPriority(&h->stream_panel, hipStreamNonBlocking, hi) != hipSuccess ||
          hipStreamCreateWithPriority(&h->stream_aux, hipStreamNonBlocking, hi) != hipSuccess) {
        (void)hipGetLastError();
        if (h->stream_masked) { (void)hipStreamDestroy(h->stream_masked); h->stream_masked = nullptr; }
        if (h->stream_panel) { (void)hipStreamDestroy(h->stream_panel); }
        h->stream_panel = nullptr;
        h->stream_aux = nullptr;
      }
    }
    if (!h->stream && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
      // nothing of this set is registered yet: destroy the look-ahead streams that were created above
      for (hipStream_t q : {h->stream_masked, h->stream_panel, h->stream_aux}) if (q) (void)hipStreamDestroy(q);
      delete h;
      return OKKT_ERR_HIP;
    }
    h->stream_la = la ? 1 : 0;
    h->stream_reserved = reserved;
    if (set.device < 0) {   // a new set: the pool owns its streams from now on
      set.device = dev; set.la = h->stream_la; set.reserved = reserved;
      set.stream = h->stream; set.masked = h->stream_masked; set.panel = h->stream_panel; set.aux = h->stream_aux;
      register_stream_set(set);
      h->stream_seq = pool_size();
    }
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
      if (h->ev0) (void)hipEventDestroy(h->ev0);
      give_stream_set(set);      // registered (new or reused): back to the free list for the next handle
      delete h;
      return OKKT_ERR_HIP;
    }
    h->device_ready = true;
  }
  *out = h;
  return OKKT_OK;
}

int okkt_destroy(okkt_handle h) {
  if (!h) return OKKT_ERR_INVALID;
  if (h->rccl_comm || h->dist_cb || h->dist_x) (void)okkt_dist_comm_destroy(h);
  bool closed;
  { std::lock_guard<std::mutex> lock(pool_mutex()); closed = g_pool_closed; }
  if (h->device_ready && closed) {
    // a finalizer that runs after the process-exit handler: every pooled stream has been synchronised and destroyed
    // there, so nothing is in flight; only memory and events are released, no stream is touched
    numeric_release(h->N);
    solver_refine_release(h);
    if (h->d_rhs_stage) (void)hipFree(h->d_rhs_stage);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
  } else if (h->device_ready) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    numeric_release(h->N);
    solver_refine_release(h);
    if (h->d_rhs_stage) (void)hipFree(h->d_rhs_stage);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    // the streams go back to the pool (idle: everything on them was synchronised above or joined into h->stream)
    for (hipStream_t q : {h->stream_masked, h->stream_panel, h->stream_aux})
      if (q) (void)hipStreamSynchronize(q);
    if (h->stream) {
      StreamSet set;
      set.device = h->device; set.la = h->stream_la; set.reserved = h->stream_reserved;
      set.stream = h->stream; set.masked = h->stream_masked; set.panel = h->stream_panel; set.aux = h->stream_aux;
      set.seq = h->stream_seq;
      give_stream_set(set);
    }
  }
  delete h;
  return OKKT_OK;
}

int okkt_set_early_exit(okkt_handle h, int enable) {
  if (!h) return OKKT_ERR_INVALID;
  h->early_exit = enable != 0;
  return OKKT_OK;
}

const char* okkt_last_error(okkt_handle h) { return h ? h->err.c_str() : "null handle"; }

int okkt_set_perm(okkt_handle h, const int64_t* perm, int64_t n) {
  if (!h || !perm || n < 0) return OKKT_ERR_INVALID;
  h->user_perm.assign(perm, perm + n);
  h->analyzed = false;  // force re-analysis with the new permutation
  return OKKT_OK;
}

int okkt_analyze(okkt_handle h, int64_t dim, const int64_t* colptr, const int64_t* rowval, int index_base) {
  if (!h || !colptr || (dim > 0 && !rowval && colptr[dim] != colptr[0])) return OKKT_ERR_INVALID;
  if (dim < 0) return solver_set_error(h, OKKT_ERR_INVALID, "dim < 0");
  try {
    if (h->analyzed && h->S.n == dim) {
      // same pattern as last time?  (the reference rebuilds Q every outer iteration with an
      // identical structure; ls_factor! may therefore call this unconditionally)
      // exact comparison with the analysed pattern (kept on the host): 26 MB of memcmp at S-metric = 2-3 ms per
      // ls_factor!, where the byte-wise hash of the same arrays took 21 ms
      const int64_t nnz = colptr[dim] - colptr[0];
      if (nnz == h->S.nnz_in && (int64_t)h->pat_colptr.size() == dim + 1 && (int64_t)h->pat_rowval.size() == nnz &&
          std::memcmp(h->pat_colptr.data(), colptr, (size_t)(dim + 1) * sizeof(int64_t)) == 0 &&
          (nnz == 0 || std::memcmp(h->pat_rowval.data(), rowval, (size_t)nnz * sizeof(int64_t)) == 0))
        return OKKT_OK;
    }
    if (h->opts.ordering == 2 && (int64_t)h->user_perm.size() != dim)
      return solver_set_error(h, OKKT_ERR_INVALID, "ordering=user: okkt_set_perm must supply dim entries first");
    auto t0 = std::chrono::steady_clock::now();
    if (h->device_ready && (h->rf.ready || h->rf_work || h->rf_om || h->cd.X || h->sl.planned || h->kr.V || h->dl.F || h->sc.ready || h->pv.planned)) {   // the refinement map (and Z) belong to the old pattern
      (void)hipSetDevice(h->device);
      (void)hipStreamSynchronize(h->stream);
      solver_refine_release(h);
    }
    if (h->numeric_ready) {
      (void)hipSetDevice(h->device);
      (void)hipStreamSynchronize(h->stream);
      numeric_release(h->N);
      h->numeric_ready = false;
    }
    h->analyzed = false;
    h->factored = false;
    std::string e = analyze_pattern(dim, colptr, rowval, index_base, h->sopts,
                                    h->opts.ordering == 2 ? h->user_perm.data() : nullptr, h->S, h->schur_idx.data(), (int64_t)h->schur_idx.size());
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_INVALID, e);
    h->analyze_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    h->analyzed = true;
    h->pat_colptr.assign(colptr, colptr + dim + 1);
    h->pat_rowval.assign(rowval, rowval + (colptr[dim] - colptr[0]));
    ++h->n_analyze_calls;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_analyze");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_analyze");
  }
}

int okkt_get_perm(okkt_handle h, int64_t* perm_out) {
  if (!h || !perm_out) return OKKT_ERR_INVALID;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  for (int64_t k = 0; k < h->S.n; ++k) perm_out[k] = h->S.perm[k];
  return OKKT_OK;
}

int okkt_get_etree(okkt_handle h, int64_t* parent_out, int64_t* colcount_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  for (int64_t k = 0; k < h->S.n; ++k) {
    if (parent_out) parent_out[k] = h->S.parent[k];
    if (colcount_out) colcount_out[k] = h->S.colcount[k];
  }
  return OKKT_OK;
}

int okkt_get_stats(okkt_handle h, okkt_stats* out) {
  if (!h || !out) return OKKT_ERR_INVALID;
  std::memset(out, 0, sizeof(*out));
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  const Symbolic& S = h->S;
  out->n = S.n;
  out->nnz_lower = S.nnz_lower;
  out->nnzL = S.nnzL;
  out->nnzL_stored = S.nnzL_stored;
  out->flops_exact = S.flops_exact;
  out->flops_stored = S.flops_stored;
  out->arena_bytes = (h->N.arena_doubles > 0 ? h->N.arena_doubles : S.arena_doubles) * 8;      // as allocated (panels + the shared contribution-block region) once the device plan exists
  out->nsuper = S.nsuper;
  out->nlevels = S.nlevels;
  out->max_front = S.max_front;
  int64_t nsmall = 0, nbig = 0;
  for (int s = 0; s < S.nsuper; ++s) {
    int64_t f = S.row_ptr[s + 1] - S.row_ptr[s];
    if (f <= std::max(32, std::min(h->sopts.small_front_max, 136))) ++nsmall; else ++nbig;
  }
  out->n_small_fronts = nsmall;
  out->n_big_fronts = nbig;
  out->sum_rowidx = (int64_t)S.rows.size();
  out->analyze_seconds = h->analyze_seconds;
  out->last_factor_ms = h->last_factor_ms;
  out->last_solve_ms = h->last_solve_ms;
  out->pattern_hash = S.pattern_hash;
  out->n_analyze_calls = h->n_analyze_calls;
  out->ordering_used = h->S.ordering_used;
  out->critical_pivots = h->S.critical_pivots;
  out->top_separator = h->S.top_separator;
  out->amd_skipped = h->S.amd_skipped ? 1 : 0;
  out->flops_other = h->S.flops_other;
  out->arena_dense_bytes = S.arena_doubles * 8;
  return OKKT_OK;
}

int okkt_factor_dev(okkt_handle h, const double* d_nzval, int64_t n, int64_t m, int sym_kind, okkt_inertia* out) {
  if (!h || (!d_nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  if (schur_mode(h)) return schur_refuse(h, "okkt_factor_dev");
  try {
    return solver_factor_device(h, d_nzval, n, m, sym_kind, out);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_factor_dev");
  }
}

int okkt_factor(okkt_handle h, const double* nzval, int64_t n, int64_t m, int sym_kind, okkt_inertia* out) {
  if (!h || (!nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  if (schur_mode(h)) return schur_refuse(h, "okkt_factor");
  try {
    int rc = solver_ensure_numeric(h);
    if (rc != OKKT_OK) return rc;
    if (h->S.nnz_in > 0) {
      hipError_t he = hipMemcpyAsync(h->N.vals_owned, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, h->stream);
      if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("nzval upload: ") + hipGetErrorString(he));
    }
    return solver_factor_device(h, h->N.vals_owned, n, m, sym_kind, out);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_factor");
  }
}

// h->d_rhs_stage holds at least len doubles
static int rhs_stage(okkt_solver_s* h, int64_t len) {
  if (h->rhs_stage_len >= len) return OKKT_OK;
  if (h->d_rhs_stage) (void)hipFree(h->d_rhs_stage);
  h->d_rhs_stage = nullptr;
  h->rhs_stage_len = 0;
  if (hipMalloc((void**)&h->d_rhs_stage, (size_t)len * sizeof(double)) != hipSuccess)
    return solver_set_error(h, OKKT_ERR_ALLOC, "rhs staging allocation failed");
  h->rhs_stage_len = len;
  return OKKT_OK;
}

int okkt_solve_dev(okkt_handle h, const double* d_rhs, double* d_sol, int64_t nrhs) {
  if (!h || !d_rhs || !d_sol) return OKKT_ERR_INVALID;
  if (schur_mode(h)) return schur_refuse(h, "okkt_solve_dev");
  try {
    return solver_solve_device(h, d_rhs, d_sol, nrhs);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_solve_dev");
  }
}

int okkt_solve(okkt_handle h, const double* rhs, double* sol, int64_t nrhs) {
  if (!h || !rhs || !sol) return OKKT_ERR_INVALID;
  if (schur_mode(h)) return schur_refuse(h, "okkt_solve");
  try {
    int rc = solver_ensure_numeric(h);
    if (rc != OKKT_OK) return rc;
    if (!h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "solve called before a factorisation");
    const int64_t len = h->S.n * std::max<int64_t>(nrhs, 0);
    if (len == 0) return OKKT_OK;
    if ((rc = rhs_stage(h, len)) != OKKT_OK) return rc;
    hipError_t he = hipMemcpyAsync(h->d_rhs_stage, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("rhs upload: ") + hipGetErrorString(he));
    rc = solver_solve_device(h, h->d_rhs_stage, h->d_rhs_stage, nrhs);
    if (rc != OKKT_OK) return rc;
    he = hipMemcpy(sol, h->d_rhs_stage, (size_t)len * sizeof(double), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("sol download: ") + hipGetErrorString(he));
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_solve");
  }
}

int okkt_get_diag(okkt_handle h, double* d_out) {
  if (!h || !d_out) return OKKT_ERR_INVALID;
  int rc = solver_ensure_numeric(h);
  if (rc != OKKT_OK) return rc;
  if (!h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "no factorisation");
  if (hipMemcpy(d_out, h->N.d.dvals, (size_t)h->S.n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return solver_set_error(h, OKKT_ERR_HIP, "download of D failed");
  return OKKT_OK;
}

int okkt_get_factor_csc(okkt_handle h, int64_t* colptr_out, int64_t* rowval_out, double* val_out, int64_t* nnz_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  const Symbolic& S = h->S;
  const int64_t nnz = S.nnzL_stored - S.n;
  if (nnz_out) *nnz_out = nnz;
  if (!colptr_out || !rowval_out || !val_out) return OKKT_OK;
  try {
    int rc = solver_ensure_numeric(h);
    if (rc != OKKT_OK) return rc;
    if (!h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "no factorisation");
    std::vector<double> front;
    int64_t q = 0;
    for (int s = 0; s < S.nsuper; ++s) {
      const int64_t f = S.row_ptr[s + 1] - S.row_ptr[s];
      const int64_t k = S.sn_col0[s + 1] - S.sn_col0[s];
      front.resize((size_t)(f * k));
      if (hipMemcpy(front.data(), h->N.d.arena + h->N.front_pos_host[s], (size_t)(f * k) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return solver_set_error(h, OKKT_ERR_HIP, "download of a front failed");
      for (int64_t lc = 0; lc < k; ++lc) {
        colptr_out[S.sn_col0[s] + lc] = q;
        for (int64_t i = lc + 1; i < f; ++i) {
          rowval_out[q] = S.rows[S.row_ptr[s] + i];
          val_out[q] = front[(size_t)(lc * f + i)];
          ++q;
        }
      }
    }
    colptr_out[S.n] = q;
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_factor_csc");
  }
}

int okkt_dev_alloc(okkt_handle h, int64_t bytes, void** out) {
  if (!h || !out || bytes < 0) return OKKT_ERR_INVALID;
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (hipMalloc(out, (size_t)std::max<int64_t>(bytes, 8)) != hipSuccess) return solver_set_error(h, OKKT_ERR_ALLOC, "hipMalloc failed");
  return OKKT_OK;
}
int okkt_dev_free(okkt_handle h, void* p) {
  if (!h) return OKKT_ERR_INVALID;
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  (void)hipStreamSynchronize(h->stream);
  return hipFree(p) == hipSuccess ? OKKT_OK : solver_set_error(h, OKKT_ERR_HIP, "hipFree failed");
}
int okkt_dev_upload(okkt_handle h, void* d_dst, const void* src, int64_t bytes) {
  if (!h || bytes < 0 || (bytes > 0 && (!d_dst || !src))) return OKKT_ERR_INVALID;
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (bytes == 0) return OKKT_OK;
  (void)hipStreamSynchronize(h->stream);
  return hipMemcpy(d_dst, src, (size_t)bytes, hipMemcpyHostToDevice) == hipSuccess ? OKKT_OK : solver_set_error(h, OKKT_ERR_HIP, "upload failed");
}
int okkt_dev_download(okkt_handle h, void* dst, const void* d_src, int64_t bytes) {
  if (!h || bytes < 0 || (bytes > 0 && (!dst || !d_src))) return OKKT_ERR_INVALID;
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (bytes == 0) return OKKT_OK;
  (void)hipStreamSynchronize(h->stream);
  return hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess ? OKKT_OK : solver_set_error(h, OKKT_ERR_HIP, "download failed");
}
void* okkt_get_stream(okkt_handle h) { return h ? (void*)h->stream : nullptr; }

int okkt_profile_dominant(okkt_handle h, int enable) {
  if (!h) return OKKT_ERR_INVALID;
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  (void)hipStreamSynchronize(h->stream);
  h->N.profile = enable != 0;
  h->N.prof_used = 0;
  h->N.prof_flops.clear();
  return OKKT_OK;
}

int okkt_get_profile(okkt_handle h, int64_t* n_launches, double* total_ms, double* total_flops) {
  if (!h || !n_launches || !total_ms || !total_flops) return OKKT_ERR_INVALID;
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, "stream sync failed");
  double ms = 0, fl = 0;
  const size_t n = h->N.prof_used / 2;
  for (size_t i = 0; i < n; ++i) {
    float t = 0;
    if (hipEventElapsedTime(&t, h->N.prof_events[2 * i], h->N.prof_events[2 * i + 1]) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "hipEventElapsedTime failed");
    ms += t;
    fl += h->N.prof_flops[i];
    if (getenv("OKKT_DEBUG_SYRK_LOG")) fprintf(stderr, "syrk launch %3zu: %9.1f us %8.3f GFLOP %6.1f TFLOP/s\n", i, t * 1e3, h->N.prof_flops[i] * 1e-9, h->N.prof_flops[i] / (t * 1e-3) * 1e-12);
  }
  if (getenv("OKKT_DEBUG_SYRK_LOG") && h->N.d.zero_page) {   // phase ticks of k_big_syrk<16, .> (OKKT_DEBUG_SYRK=96), 10 ns each
    unsigned long long T[8];
    if (hipMemcpy(T, h->N.d.zero_page + 256, sizeof(T), hipMemcpyDeviceToHost) == hipSuccess && T[0] > 0) {
      fprintf(stderr, "syrk workgroups %llu: per workgroup (us) start->first chunk ready %.2f, main loop %.2f (%.3f per 16-column chunk), store issue %.2f, store drain %.2f\n",
              T[0], T[1] * 0.01 / T[0], T[2] * 0.01 / T[0], T[2] * 0.01 / (double)T[5], T[3] * 0.01 / T[0], T[4] * 0.01 / T[0]);
      fprintf(stderr, "   of the start: scalar set-up %.2f us, C tile loaded (if waited for) %.2f us\n", T[6] * 0.01 / T[0], T[7] * 0.01 / T[0]);
      (void)hipMemset(h->N.d.zero_page + 256, 0, sizeof(T));
    }
  }
  *n_launches = (int64_t)n;
  *total_ms = ms;
  *total_flops = fl;
  return OKKT_OK;
}

int okkt_residual_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, double* d_r, int64_t nrhs,
                      double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  try {
    int rc = refine_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (nrhs == 0) return OKKT_OK;
    if ((!d_nzval && h->S.nnz_in > 0) || !d_rhs || !d_x || !d_r) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
    return residual_device(h, d_nzval, d_rhs, d_x, d_r, nrhs, omega_out);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_residual_dev");
  }
}

int okkt_residual(okkt_handle h, const double* nzval, const double* rhs, const double* x, double* r, int64_t nrhs, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  try {
    int rc = refine_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (nrhs == 0) return OKKT_OK;
    if ((!nzval && h->S.nnz_in > 0) || !rhs || !x || !r) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
    const int64_t len = nrhs * h->S.n;
    std::string e = refine_stage_alloc(h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "nzval staging: " + e);
    if ((rc = refine_work(h, 3 * len, 2 * nrhs)) != OKKT_OK) return rc;
    double* db = h->rf_work;
    double* dxv = db + len;
    double* dr = dxv + len;
    hipStream_t st = h->stream;
    hipError_t he = hipSuccess;
    if (h->S.nnz_in > 0) he = hipMemcpyAsync(h->rf.nz_stage, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && len > 0) he = hipMemcpyAsync(db, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && len > 0) he = hipMemcpyAsync(dxv, x, (size_t)len * sizeof(double), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("residual upload: ") + hipGetErrorString(he));
    if ((rc = residual_device(h, h->rf.nz_stage, db, dxv, dr, nrhs, omega_out)) != OKKT_OK) return rc;
    if (len > 0 && hipMemcpy(r, dr, (size_t)len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "residual download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_residual");
  }
}

int okkt_solve_refine_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                          double tol, okkt_refine_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs > 0 && (!d_rhs || !d_sol || (!d_nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    return solver_refine_device(h, d_nzval, d_rhs, d_sol, nrhs, max_steps, tol, info, omega_out);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_solve_refine_dev");
  }
}

int okkt_solve_refine(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t max_steps, double tol,
                      okkt_refine_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (max_steps < 0) return solver_set_error(h, OKKT_ERR_INVALID, "max_steps < 0");
  if (nrhs > 0 && (!rhs || !sol || (!nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = refine_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs;
    if (len == 0) return solver_refine_device(h, nullptr, nullptr, nullptr, nrhs, max_steps, tol, info, omega_out);
    std::string e = refine_stage_alloc(h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "nzval staging: " + e);
    if (h->rhs_stage_len < len) {
      (void)hipStreamSynchronize(h->stream);
      if (h->d_rhs_stage) (void)hipFree(h->d_rhs_stage);
      h->d_rhs_stage = nullptr;
      h->rhs_stage_len = 0;
      if (hipMalloc((void**)&h->d_rhs_stage, (size_t)len * sizeof(double)) != hipSuccess)
        return solver_set_error(h, OKKT_ERR_ALLOC, "rhs staging allocation failed");
      h->rhs_stage_len = len;
    }
    hipStream_t st = h->stream;
    hipError_t he = hipSuccess;
    if (h->S.nnz_in > 0) he = hipMemcpyAsync(h->rf.nz_stage, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(h->d_rhs_stage, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("refinement upload: ") + hipGetErrorString(he));
    rc = solver_refine_device(h, h->rf.nz_stage, h->d_rhs_stage, h->d_rhs_stage, nrhs, max_steps, tol, info, omega_out);
    if (rc != OKKT_OK) return rc;
    if (hipMemcpy(sol, h->d_rhs_stage, (size_t)len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "sol download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_solve_refine");
  }
}

// okkt_solve_gmres_dev / okkt_solve_gmres and their twins through the Schur route
static int gmres_dev_entry(okkt_handle h, bool schur_route, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                           int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs > 0 && (!d_rhs || !d_sol || (!d_nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    return solver_gmres_device(h, d_nzval, d_rhs, d_sol, nrhs, restart, max_iters, tol, info, omega_out, schur_route);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, schur_route ? "unexpected exception in okkt_schur_solve_gmres_dev" : "unexpected exception in okkt_solve_gmres_dev");
  }
}

int okkt_solve_gmres_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                         int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_dev_entry(h, false, d_nzval, d_rhs, d_sol, nrhs, restart, max_iters, tol, info, omega_out);
}

int okkt_schur_solve_gmres_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                               int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_dev_entry(h, true, d_nzval, d_rhs, d_sol, nrhs, restart, max_iters, tol, info, omega_out);
}

static int gmres_host_entry(okkt_handle h, bool schur_route, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t restart,
                            int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (max_iters < 0) return solver_set_error(h, OKKT_ERR_INVALID, "max_iters < 0");
  if (restart > kKryMaxRestart) return solver_set_error(h, OKKT_ERR_INVALID, "restart > 64");
  if (nrhs > 0 && (!rhs || !sol || (!nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = schur_route ? schur_route_ready(h) : refine_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs;
    if (len == 0) return solver_gmres_device(h, nullptr, nullptr, nullptr, nrhs, restart, max_iters, tol, info, omega_out, schur_route);
    std::string e = refine_stage_alloc(h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "nzval staging: " + e);
    if (h->rhs_stage_len < len) {
      (void)hipStreamSynchronize(h->stream);
      if (h->d_rhs_stage) (void)hipFree(h->d_rhs_stage);
      h->d_rhs_stage = nullptr;
      h->rhs_stage_len = 0;
      if (hipMalloc((void**)&h->d_rhs_stage, (size_t)len * sizeof(double)) != hipSuccess)
        return solver_set_error(h, OKKT_ERR_ALLOC, "rhs staging allocation failed");
      h->rhs_stage_len = len;
    }
    hipStream_t st = h->stream;
    hipError_t he = hipSuccess;
    if (h->S.nnz_in > 0) he = hipMemcpyAsync(h->rf.nz_stage, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(h->d_rhs_stage, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("GMRES upload: ") + hipGetErrorString(he));
    rc = solver_gmres_device(h, h->rf.nz_stage, h->d_rhs_stage, h->d_rhs_stage, nrhs, restart, max_iters, tol, info, omega_out, schur_route);
    if (rc != OKKT_OK) return rc;
    if (hipMemcpy(sol, h->d_rhs_stage, (size_t)len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "sol download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, schur_route ? "unexpected exception in okkt_schur_solve_gmres" : "unexpected exception in okkt_solve_gmres");
  }
}

int okkt_solve_gmres(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t restart, int32_t max_iters,
                     double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_host_entry(h, false, nzval, rhs, sol, nrhs, restart, max_iters, tol, info, omega_out);
}

int okkt_schur_solve_gmres(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t restart, int32_t max_iters,
                           double tol, okkt_gmres_info* info, double* omega_out) {
  return gmres_host_entry(h, true, nzval, rhs, sol, nrhs, restart, max_iters, tol, info, omega_out);
}

// okkt_condest_dev / okkt_condest and their twins through the Schur route
static int condest_dev_entry(okkt_handle h, bool schur_route, const double* d_nzval, int32_t t, okkt_condest_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  if (!d_nzval && h->S.nnz_in > 0) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    return solver_condest_device(h, d_nzval, t, info, schur_route);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in the condition estimate");
  }
}

int okkt_condest_dev(okkt_handle h, const double* d_nzval, int32_t t, okkt_condest_info* info) { return condest_dev_entry(h, false, d_nzval, t, info); }
int okkt_schur_condest_dev(okkt_handle h, const double* d_nzval, int32_t t, okkt_condest_info* info) { return condest_dev_entry(h, true, d_nzval, t, info); }

static int condest_host_entry(okkt_handle h, bool schur_route, const double* nzval, int32_t t, okkt_condest_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  if (!nzval && h->S.nnz_in > 0) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = condest_ready(h, schur_route);
    if (rc != OKKT_OK) return rc;
    std::string e = refine_stage_alloc(h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "nzval staging: " + e);
    if (h->S.nnz_in > 0) {
      hipError_t he = hipMemcpyAsync(h->rf.nz_stage, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, h->stream);
      if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("nzval upload: ") + hipGetErrorString(he));
    }
    return solver_condest_device(h, h->rf.nz_stage, t, info, schur_route);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in the condition estimate");
  }
}

int okkt_condest(okkt_handle h, const double* nzval, int32_t t, okkt_condest_info* info) { return condest_host_entry(h, false, nzval, t, info); }
int okkt_schur_condest(okkt_handle h, const double* nzval, int32_t t, okkt_condest_info* info) { return condest_host_entry(h, true, nzval, t, info); }

int64_t okkt_condest_indices(okkt_handle h, int64_t* ind_out, int64_t cap) {
  if (!h || (cap > 0 && !ind_out)) return OKKT_ERR_INVALID;
  const int64_t cnt = (int64_t)h->cd_hist.size();
  for (int64_t i = 0; i < std::min(cnt, cap); ++i) ind_out[i] = h->cd_hist[(size_t)i];
  return cnt;
}

// okkt_forward_error_dev / okkt_forward_error and their twins through the Schur route
static int ferr_dev_entry(okkt_handle h, bool schur_route, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs, double* ferr_out,
                          double* berr_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs > 0 && (!d_rhs || !d_x || !ferr_out || (!d_nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    return solver_forward_error_device(h, d_nzval, d_rhs, d_x, nrhs, ferr_out, berr_out, schur_route);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in the forward error bound");
  }
}

int okkt_forward_error_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs, double* ferr_out,
                           double* berr_out) {
  return ferr_dev_entry(h, false, d_nzval, d_rhs, d_x, nrhs, ferr_out, berr_out);
}

int okkt_schur_forward_error_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs, double* ferr_out,
                                 double* berr_out) {
  return ferr_dev_entry(h, true, d_nzval, d_rhs, d_x, nrhs, ferr_out, berr_out);
}

static int ferr_host_entry(okkt_handle h, bool schur_route, const double* nzval, const double* rhs, const double* x, int64_t nrhs, double* ferr_out,
                           double* berr_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!rhs || !x || !ferr_out || (!nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = condest_ready(h, schur_route);
    if (rc != OKKT_OK) return rc;
    const int64_t len = nrhs * h->S.n;
    std::string e = refine_stage_alloc(h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "nzval staging: " + e);
    if ((rc = refine_work(h, 2 * len, 2 * nrhs)) != OKKT_OK) return rc;
    double* db = h->rf_work;
    double* dxv = db + len;
    hipStream_t st = h->stream;
    hipError_t he = hipSuccess;
    if (h->S.nnz_in > 0) he = hipMemcpyAsync(h->rf.nz_stage, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && len > 0) he = hipMemcpyAsync(db, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && len > 0) he = hipMemcpyAsync(dxv, x, (size_t)len * sizeof(double), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("forward error upload: ") + hipGetErrorString(he));
    return solver_forward_error_device(h, h->rf.nz_stage, db, dxv, nrhs, ferr_out, berr_out, schur_route);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in the forward error bound");
  }
}

int okkt_forward_error(okkt_handle h, const double* nzval, const double* rhs, const double* x, int64_t nrhs, double* ferr_out,
                       double* berr_out) {
  return ferr_host_entry(h, false, nzval, rhs, x, nrhs, ferr_out, berr_out);
}

int okkt_schur_forward_error(okkt_handle h, const double* nzval, const double* rhs, const double* x, int64_t nrhs, double* ferr_out,
                             double* berr_out) {
  return ferr_host_entry(h, true, nzval, rhs, x, nrhs, ferr_out, berr_out);
}

// ---- symmetric equilibration (scaling.hip) ------------------------------------------------------------------

int okkt_set_scaling(okkt_handle h, int mode, int32_t sweeps, const double* s_user) {
  if (!h) return OKKT_ERR_INVALID;
  try {
    return solver_set_scaling(h, mode, sweeps, s_user);
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_set_scaling");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_set_scaling");
  }
}

// the scaling of the current factor: device, a complete factorisation that used one
static int scaling_current(okkt_solver_s* h) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (!h->analyzed || !h->factored || !h->sc.valid || !h->sc.ready)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_scaling: the handle holds no complete factorisation that used a scaling (okkt_set_scaling, then okkt_factor)");
  return OKKT_OK;
}

int okkt_get_scaling_dev(okkt_handle h, double* d_s_out) {
  if (!h) return OKKT_ERR_INVALID;
  int rc = scaling_current(h);
  if (rc != OKKT_OK) return rc;
  if (h->S.n == 0) return OKKT_OK;
  if (!d_s_out) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_scaling_dev: null pointer");
  hipError_t he = hipMemcpyAsync(d_s_out, h->sc.s_cur, (size_t)h->S.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("okkt_get_scaling_dev: ") + hipGetErrorString(he));
  return OKKT_OK;
}

int okkt_get_scaling(okkt_handle h, double* s_out, okkt_scaling_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  int rc = scaling_current(h);
  if (rc != OKKT_OK) return rc;
  if (h->S.n > 0 && !s_out) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_scaling: null pointer");
  if (h->S.n > 0) {
    hipError_t he = hipStreamSynchronize(h->stream);
    if (he == hipSuccess) he = hipMemcpy(s_out, h->sc.s_cur, (size_t)h->S.n * sizeof(double), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("okkt_get_scaling: ") + hipGetErrorString(he));
  }
  if (info) *info = h->sc.info;
  return OKKT_OK;
}

int64_t okkt_debug_dataflow_queue(int32_t nfronts, const int32_t* f, const int32_t* k, int32_t workers, int32_t group,
                                  int32_t* tasks, int64_t cap, double* model_us) {
  if (nfronts < 0 || !f || !k || (cap > 0 && !tasks)) return OKKT_ERR_INVALID;
  try {
    std::vector<okkt::DfFront> fronts;
    for (int a = 0; a < nfronts; ++a) {
      if (k[a] < 1 || f[a] < k[a]) return OKKT_ERR_INVALID;
      fronts.push_back({a, f[a], k[a]});
    }
    std::vector<okkt::DfTask> q;
    double model = 0;
    okkt::df_build_queue(fronts, workers, group & 255, std::max(1, (group >> 8) & 255), (group >> 16) & 1, (group >> 17) & 1, q, &model, (group >> 18) & 1);
    if (model_us) *model_us = model;
    for (int64_t t = 0; t < (int64_t)q.size() && t < cap; ++t) {
      tasks[4 * t] = q[t].front; tasks[4 * t + 1] = q[t].type_nq; tasks[4 * t + 2] = q[t].ij; tasks[4 * t + 3] = q[t].q0;
    }
    return (int64_t)q.size();
  } catch (...) { return OKKT_ERR_ALLOC; }
}

// ---- Schur mode ------------------------------------------------------------------------------

int okkt_set_schur(okkt_handle h, int64_t ns, const int64_t* idx) {
  if (!h) return OKKT_ERR_INVALID;
  if (ns < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: ns < 0");
  if (ns > 0 && !idx) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: null idx");
  try {
    std::vector<int64_t> v(idx, idx + ns);
    std::vector<int64_t> sorted(v);
    std::sort(sorted.begin(), sorted.end());
    if (ns > 0 && sorted[0] < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: negative index");
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: duplicate index");
    // the order of the analysed pattern is known: the range is checked now (okkt_analyze checks it against the pattern it is given)
    if (h->analyzed && ns > 0 && (ns >= h->S.n || sorted.back() >= h->S.n))
      return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: index out of range or ns >= dim of the analysed pattern");
    if (v == h->schur_idx) return OKKT_OK;
    if (ns > 0 && h->sc.mode != OKKT_SCALE_NONE)
      return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: a scaling is set on this handle and Schur mode does not factor a scaled matrix (okkt_set_scaling with OKKT_SCALE_NONE first)");
    h->schur_idx.swap(v);
    h->analyzed = false;      // the plan changes: okkt_analyze builds it again
    h->factored = false;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_set_schur");
  }
}

// Schur mode, analysed, device plan ready; need_factor: a complete okkt_factor_schur
static int schur_ready(okkt_solver_s* h, bool need_factor) {
  if (!schur_mode(h)) return solver_set_error(h, OKKT_ERR_INVALID, "the handle is not in Schur mode (okkt_set_schur before okkt_analyze)");
  int rc = solver_ensure_numeric(h);
  if (rc != OKKT_OK) return rc;
  if (h->S.nschur != (int64_t)h->schur_idx.size() || h->N.schur_sn < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called since okkt_set_schur");
  if (need_factor && !h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "no complete okkt_factor_schur");
  return OKKT_OK;
}

int okkt_factor_schur_dev(okkt_handle h, const double* d_nzval, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* out) {
  if (!h || (!d_nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  try {
    int rc = schur_ready(h, false);
    if (rc != OKKT_OK) return rc;
    return solver_factor_device(h, d_nzval, n1, m1, sym_kind, out);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_factor_schur_dev");
  }
}

int okkt_factor_schur(okkt_handle h, const double* nzval, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* out) {
  if (!h || (!nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  try {
    int rc = schur_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (h->S.nnz_in > 0) {
      hipError_t he = hipMemcpyAsync(h->N.vals_owned, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, h->stream);
      if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("nzval upload: ") + hipGetErrorString(he));
    }
    return solver_factor_device(h, h->N.vals_owned, n1, m1, sym_kind, out);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_factor_schur");
  }
}

// a device buffer for the length of one host-side call
namespace {
struct DevTemp {
  double* p = nullptr;
  ~DevTemp() { if (p) (void)hipFree(p); }
  bool alloc(int64_t n) { return n <= 0 || hipMalloc((void**)&p, (size_t)n * sizeof(double)) == hipSuccess; }
};
}  // namespace

static int schur_sync(okkt_solver_s* h, const char* what) {
  hipError_t he = hipGetLastError();
  if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string(what) + " failed: " + hipGetErrorString(he));
  return OKKT_OK;
}

int okkt_get_schur_dev(okkt_handle h, double* d_S, int64_t ld) {
  if (!h || !d_S) return OKKT_ERR_INVALID;
  try {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    if (ld < h->S.nschur) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_schur: ld < ns");
    schur_export_enqueue(h->N, d_S, ld);
    return schur_sync(h, "Schur complement export");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_schur_dev");
  }
}

int okkt_get_schur(okkt_handle h, double* S, int64_t ld) {
  if (!h || !S) return OKKT_ERR_INVALID;
  try {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t ns = h->S.nschur;
    if (ld < ns) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_schur: ld < ns");
    DevTemp t;
    if (!t.alloc(ns * ns)) return solver_set_error(h, OKKT_ERR_ALLOC, "Schur complement staging allocation failed");
    schur_export_enqueue(h->N, t.p, ns);
    if ((rc = schur_sync(h, "Schur complement export")) != OKKT_OK) return rc;
    if (hipMemcpy2D(S, (size_t)ld * sizeof(double), t.p, (size_t)ns * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "Schur complement download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_schur");
  }
}

// batches of up to kMaxRhs right-hand sides, as solver_solve_enqueue; d_x2 == nullptr: condense into d_r2, else expand into d_x
static int schur_sweeps(okkt_solver_s* h, const double* d_rhs, double* d_r2, const double* d_x2, double* d_x, int64_t nrhs) {
  const int64_t n = h->S.n, ns = h->S.nschur;
  for (int64_t r = 0; r < nrhs;) {
    const int nr = (int)std::min<int64_t>(nrhs - r, kMaxRhs);
    const int R = nr >= 3 ? 4 : nr;
    solve_permute_in(h->N, d_rhs + r * n, n, nr, R);
    std::string e = d_x2 ? schur_expand_enqueue(h->N, d_x2 + r * ns, nr, R) : schur_condense_enqueue(h->N, d_r2 + r * ns, nr, R);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    if (d_x2) solve_permute_out(h->N, d_x + r * n, n, nr, R, false);
    r += nr;
  }
  return schur_sync(h, d_x2 ? "Schur expand" : "Schur condense");
}

int okkt_schur_condense_dev(okkt_handle h, const double* d_rhs, double* d_r2, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!d_rhs || !d_r2)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    return schur_sweeps(h, d_rhs, d_r2, nullptr, nullptr, nrhs);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_condense_dev");
  }
}

int okkt_schur_condense(okkt_handle h, const double* rhs, double* r2, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!rhs || !r2)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs, len2 = h->S.nschur * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc = rhs_stage(h, len)) != OKKT_OK) return rc;
    DevTemp t;
    if (!t.alloc(len2)) return solver_set_error(h, OKKT_ERR_ALLOC, "Schur condense staging allocation failed");
    if (hipMemcpyAsync(h->d_rhs_stage, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "rhs upload failed");
    if ((rc = schur_sweeps(h, h->d_rhs_stage, t.p, nullptr, nullptr, nrhs)) != OKKT_OK) return rc;
    if (hipMemcpy(r2, t.p, (size_t)len2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, "r2 download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_condense");
  }
}

int okkt_schur_expand_dev(okkt_handle h, const double* d_rhs, const double* d_x2, double* d_x, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!d_rhs || !d_x2 || !d_x)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    return schur_sweeps(h, d_rhs, nullptr, d_x2, d_x, nrhs);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_expand_dev");
  }
}

int okkt_schur_expand(okkt_handle h, const double* rhs, const double* x2, double* x, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!rhs || !x2 || !x)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs, len2 = h->S.nschur * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc = rhs_stage(h, len)) != OKKT_OK) return rc;
    DevTemp t;
    if (!t.alloc(len2)) return solver_set_error(h, OKKT_ERR_ALLOC, "Schur expand staging allocation failed");
    hipError_t he = hipMemcpyAsync(h->d_rhs_stage, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(t.p, x2, (size_t)len2 * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, "Schur expand upload failed");
    if ((rc = schur_sweeps(h, h->d_rhs_stage, nullptr, t.p, h->d_rhs_stage, nrhs)) != OKKT_OK) return rc;
    if (hipMemcpy(x, h->d_rhs_stage, (size_t)len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, "x download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_expand");
  }
}

// ---- the dense factor of the Schur complement (dense_ldlt.hip) -------------------------------------------

// a factor to solve with: made by okkt_schur_factor and, when it is of the handle's own S, not older than the last okkt_factor_schur
static int schur_dense_ready(okkt_solver_s* h) {
  if (!h->dl.valid) return solver_set_error(h, OKKT_ERR_INVALID, "no okkt_schur_factor has succeeded on this handle");
  if (h->dl.own && h->dl.factor_seq != h->factor_seq)
    return solver_set_error(h, OKKT_ERR_INVALID, "S has been assembled again since okkt_schur_factor: call okkt_schur_factor again");
  return OKKT_OK;
}

// S (host or device memory, NULL: the handle's own) into the factor's buffer, the factorisation, the two inertias
static int schur_factor_impl(okkt_solver_s* h, const double* S, int64_t ld, bool on_device, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  int rc = schur_ready(h, S == nullptr);
  if (rc != OKKT_OK) return rc;
  const int64_t ns = h->S.nschur;
  if (S && ld < ns) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_factor: ld < ns");
  h->dl.valid = false;
  std::string e = dense_ldlt_alloc(h->dl, ns);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "dense Schur factor allocation failed: " + e);
  h->dl.seq = ++h->dense_seq;      // a selected inverse seeded from the previous dense factor is stale from here on
  if (!S) {
    schur_export_enqueue(h->N, h->dl.F, ns);
  } else if (hipMemcpy2DAsync(h->dl.F, (size_t)ns * sizeof(double), S, (size_t)ld * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns,
                              on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream) != hipSuccess) {
    return solver_set_error(h, OKKT_ERR_HIP, "okkt_schur_factor: the copy of S failed");
  }
  if (!(e = dense_ldlt_factor(h->dl, h->stream)).empty()) return solver_set_error(h, OKKT_ERR_HIP, "dense Schur factorisation failed: " + e);
  h->dl.own = S == nullptr;
  h->dl.factor_seq = h->factor_seq;
  okkt_inertia in;
  in.pos = h->dl.cnt[0]; in.neg = h->dl.cnt[1]; in.zero = h->dl.cnt[2]; in.nonfinite = h->dl.cnt[3];
  if (in.pos + in.neg + in.zero + in.nonfinite != ns) {
    h->dl.valid = false;
    return solver_set_error(h, OKKT_ERR_INTERNAL, "pivot counts of the dense factor do not add up to ns");
  }
  if (inertia_S) *inertia_S = in;
  if (inertia_total) {
    const okkt_inertia a = h->factored ? h->a11_inertia : okkt_inertia{0, 0, 0, 0};
    inertia_total->pos = a.pos + in.pos; inertia_total->neg = a.neg + in.neg;
    inertia_total->zero = a.zero + in.zero; inertia_total->nonfinite = a.nonfinite + in.nonfinite;
  }
  return (in.zero == 0 && in.nonfinite == 0) ? 1 : 0;
}

int okkt_schur_factor(okkt_handle h, const double* S, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  if (!h) return OKKT_ERR_INVALID;
  try {
    return schur_factor_impl(h, S, ld, false, inertia_S, inertia_total);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_factor");
  }
}

int okkt_schur_factor_dev(okkt_handle h, const double* d_S, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  if (!h) return OKKT_ERR_INVALID;
  try {
    return schur_factor_impl(h, d_S, ld, true, inertia_S, inertia_total);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_factor_dev");
  }
}

int okkt_schur_get_factor(okkt_handle h, double* LD, int64_t ld, int32_t* ipiv) {
  if (!h || !LD || !ipiv) return OKKT_ERR_INVALID;
  try {
    int rc = schur_ready(h, false);
    if (rc == OKKT_OK) rc = schur_dense_ready(h);
    if (rc != OKKT_OK) return rc;
    const int64_t ns = h->S.nschur;
    if (ld < ns) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_get_factor: ld < ns");
    std::vector<int> piv((size_t)ns);
    (void)hipStreamSynchronize(h->stream);
    if (hipMemcpy2D(LD, (size_t)ld * sizeof(double), h->dl.F, (size_t)ns * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(piv.data(), h->dl.ipiv, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "dense Schur factor download failed");
    for (int64_t j = 0; j < ns; ++j) {
      ipiv[j] = piv[j];
      for (int64_t i = 0; i < j; ++i) LD[j * ld + i] = 0.0;
    }
    // the device keeps every interchange applied to every column of L; dsytrf applies to a column only the interchanges made before
    // it was eliminated: undo the later ones, last first (the end of dlasyf does the same for its panel)
    for (int64_t j = ns - 1; j > 0;) {
      const int64_t jj = j;                    // row interchanged with jp by the pivot block that ends at column j
      int64_t jp = piv[j];
      if (jp < 0) { jp = -jp; --j; }           // a 2 x 2 block: j is its first column now
      --jp;
      if (jp != jj) for (int64_t c = 0; c < j; ++c) std::swap(LD[c * ld + jj], LD[c * ld + jp]);
      --j;
    }
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_get_factor");
  }
}

// batches of up to kMaxRhs right-hand sides; whole: the fused whole-system solve (rhs and sol of order dim), else x2 = S^-1 r2
static int schur_dense_sweeps(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs, bool whole, bool sync) {
  const int64_t n = h->S.n, ns = h->S.nschur;
  double* t2 = h->dl.X + 8 * ns;      // r2 / x2 of the fused solve
  for (int64_t r = 0; r < nrhs;) {
    const int nr = (int)std::min<int64_t>(nrhs - r, kMaxRhs);
    const int R = nr >= 3 ? 4 : nr;
    std::string e;
    if (whole) {
      solve_permute_in(h->N, d_rhs + r * n, n, nr, R);
      e = solve_fwd_enqueue(h->N, 0, R);
      if (e.empty()) e = schur_gather_enqueue(h->N, t2, nr, R);
      if (e.empty()) e = dense_ldlt_solve_enqueue(h->dl, t2, t2, nr, R, h->stream);
      if (e.empty()) e = schur_put_enqueue(h->N, t2, nr, R);
      if (e.empty()) e = solve_bwd_enqueue(h->N, 0, R);
      if (e.empty()) solve_permute_out(h->N, d_sol + r * n, n, nr, R, false);
    } else {
      e = dense_ldlt_solve_enqueue(h->dl, d_rhs + r * ns, d_sol + r * ns, nr, R, h->stream);
    }
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    r += nr;
  }
  if (!sync) return OKKT_OK;      // the refinement loop of okkt_schur_solve_refine: its own read of omega synchronises
  return schur_sync(h, whole ? "Schur solve" : "dense Schur solve");
}

static int schur_dense_solve_impl(okkt_solver_s* h, const double* rhs, double* sol, int64_t nrhs, bool whole, bool on_device) {
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!rhs || !sol)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  int rc = schur_ready(h, whole);
  if (rc == OKKT_OK) rc = schur_dense_ready(h);
  if (rc != OKKT_OK) return rc;
  if (on_device) return schur_dense_sweeps(h, rhs, sol, nrhs, whole);
  const int64_t len = (whole ? h->S.n : h->S.nschur) * nrhs;
  if (len == 0) return OKKT_OK;
  if ((rc = rhs_stage(h, len)) != OKKT_OK) return rc;
  if (hipMemcpyAsync(h->d_rhs_stage, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess)
    return solver_set_error(h, OKKT_ERR_HIP, "rhs upload failed");
  if ((rc = schur_dense_sweeps(h, h->d_rhs_stage, h->d_rhs_stage, nrhs, whole)) != OKKT_OK) return rc;
  if (hipMemcpy(sol, h->d_rhs_stage, (size_t)len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, "solution download failed");
  return OKKT_OK;
}

#define OKKT_SCHUR_SOLVE_ENTRY(name, whole, on_device)                                            \
  int name(okkt_handle h, const double* rhs, double* sol, int64_t nrhs) {                         \
    if (!h) return OKKT_ERR_INVALID;                                                              \
    try {                                                                                         \
      return schur_dense_solve_impl(h, rhs, sol, nrhs, whole, on_device);                         \
    } catch (...) {                                                                               \
      return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in " #name);            \
    }                                                                                             \
  }
OKKT_SCHUR_SOLVE_ENTRY(okkt_schur_dense_solve, false, false)
OKKT_SCHUR_SOLVE_ENTRY(okkt_schur_dense_solve_dev, false, true)
OKKT_SCHUR_SOLVE_ENTRY(okkt_schur_solve, true, false)
OKKT_SCHUR_SOLVE_ENTRY(okkt_schur_solve_dev, true, true)
#undef OKKT_SCHUR_SOLVE_ENTRY

// ---- refinement through the Schur route ------------------------------------------------------------------

// Schur mode, a complete okkt_factor_schur, a current dense factor of the handle's own S; the row map of the pattern (it does not
// depend on the mode: pat_colptr / pat_rowval hold the whole pattern as okkt_analyze was given it)
static int schur_refine_ready(okkt_solver_s* h) {
  int rc = schur_ready(h, true);
  if (rc == OKKT_OK) rc = schur_dense_ready(h);
  if (rc != OKKT_OK) return rc;
  if (!h->dl.own)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_solve_refine: the dense factor is of a caller's S, so the factored matrix is not this handle's A (okkt_schur_factor with S = NULL first)");
  if (h->S.nparts > 1)
    return solver_set_error(h, OKKT_ERR_INVALID, "residuals and refinement are not available on a partitioned handle (okkt_dist_set_partition with nparts > 1)");
  if (!h->rf.ready) {
    std::string e = refine_map_build(h->S.n, h->pat_colptr.data(), h->pat_rowval.data(), h->pat_colptr[0], h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, "refinement map: " + e);
  }
  return OKKT_OK;
}

int okkt_schur_solve_refine_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                                double tol, okkt_refine_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs > 0 && (!d_rhs || !d_sol || (!d_nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    return refine_loop(h, true, d_nzval, d_rhs, d_sol, nrhs, max_steps, tol, info, omega_out, nullptr, nullptr, nullptr);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_solve_refine_dev");
  }
}

int okkt_schur_solve_refine(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t max_steps, double tol,
                            okkt_refine_info* info, double* omega_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (max_steps < 0) return solver_set_error(h, OKKT_ERR_INVALID, "max_steps < 0");
  if (nrhs > 0 && (!rhs || !sol || (!nzval && h->S.nnz_in > 0))) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  try {
    int rc = schur_refine_ready(h);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs;
    if (len == 0) return refine_loop(h, true, nullptr, nullptr, nullptr, nrhs, max_steps, tol, info, omega_out, nullptr, nullptr, nullptr);
    std::string e = refine_stage_alloc(h->rf);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "nzval staging: " + e);
    if (h->rhs_stage_len < len) (void)hipStreamSynchronize(h->stream);
    if ((rc = rhs_stage(h, len)) != OKKT_OK) return rc;
    hipStream_t st = h->stream;
    hipError_t he = hipSuccess;
    if (h->S.nnz_in > 0) he = hipMemcpyAsync(h->rf.nz_stage, nzval, (size_t)h->S.nnz_in * sizeof(double), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(h->d_rhs_stage, rhs, (size_t)len * sizeof(double), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("refinement upload: ") + hipGetErrorString(he));
    rc = refine_loop(h, true, h->rf.nz_stage, h->d_rhs_stage, h->d_rhs_stage, nrhs, max_steps, tol, info, omega_out, nullptr, nullptr, nullptr);
    if (rc != OKKT_OK) return rc;
    if (hipMemcpy(sol, h->d_rhs_stage, (size_t)len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "sol download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_solve_refine");
  }
}

// ---- selected inversion (selinv.hip) --------------------------------------------------------------------

// device, analysis, no partition, not Schur mode, a complete factorisation; need_z: a Z computed from that factorisation
static int selinv_ready(okkt_solver_s* h, bool need_z) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (schur_mode(h) && need_z) {
    // the exports serve the Z of okkt_schur_selinv: current against both factors it was made from
    if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
    const SelinvWork& W = h->sl;
    if (!h->numeric_ready || !h->factored || !h->dl.valid || !W.planned || W.skip_sn < 0 || W.skip_sn != h->N.schur_sn || W.factor_seq != h->factor_seq ||
        W.dense_seq != h->dl.seq)
      return solver_set_error(h, OKKT_ERR_INVALID, "no selected inverse of the current factorisation: call okkt_schur_selinv after okkt_factor_schur and okkt_schur_factor");
    return OKKT_OK;
  }
  if (schur_mode(h)) return schur_refuse(h, "selected inversion");
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  if (h->S.nparts > 1)
    return solver_set_error(h, OKKT_ERR_INVALID, "selected inversion is not available on a partitioned handle (okkt_dist_set_partition with nparts > 1)");
  if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
  if (!h->factored)
    return solver_set_error(h, OKKT_ERR_INVALID, "selected inversion needs a complete factorisation (none yet, or an early exit stopped it)");
  if (need_z && (!h->sl.planned || h->sl.factor_seq != h->factor_seq))
    return solver_set_error(h, OKKT_ERR_INVALID, "no selected inverse of the current factorisation: call okkt_selinv after okkt_factor");
  return OKKT_OK;
}

static int selinv_sync(okkt_solver_s* h, const char* what) {
  hipError_t he = hipGetLastError();
  if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string(what) + " failed: " + hipGetErrorString(he));
  return OKKT_OK;
}

int okkt_selinv(okkt_handle h, okkt_selinv_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  try {
    int rc = selinv_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (h->sc.valid)
      return solver_set_error(h, OKKT_ERR_INVALID, "selected inversion of a scaled factor is not available: the current factor is that of S F S (okkt_set_scaling with OKKT_SCALE_NONE, then factor again)");
    SelinvWork& W = h->sl;
    if (!W.planned || W.analysis != h->n_analyze_calls || W.arena != h->N.d.arena) {
      (void)hipStreamSynchronize(h->stream);
      std::string e = selinv_setup(h->S, h->N, h->pat_colptr.data(), h->pat_rowval.data(), W);
      if (!e.empty()) { selinv_release(W); return solver_set_error(h, OKKT_ERR_ALLOC, "selected inversion set-up: " + e); }
      W.analysis = h->n_analyze_calls;
      W.arena = h->N.d.arena;
    }
    W.factor_seq = -1;
    (void)hipEventRecord(h->ev0, h->stream);
    std::string e = selinv_enqueue(h->N, W);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    (void)hipEventRecord(h->ev1, h->stream);
    unsigned long long nf = 0;
    hipError_t he = hipMemcpyAsync(&nf, W.count, sizeof(nf), hipMemcpyDeviceToHost, h->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("selected inversion failed: ") + hipGetErrorString(he));
    W.factor_seq = h->factor_seq;
    if (info) {
      float ms = 0;
      info->seconds_device = hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess ? ms * 1e-3 : 0.0;
      info->arena_bytes = W.bytes;
      info->nonfinite = (int64_t)nf;
      info->status = nf ? 1 : 0;
      info->flops = W.flops;
    }
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_selinv");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_selinv");
  }
}

int okkt_get_inverse_diag_dev(okkt_handle h, double* d_out) {
  if (!h || !d_out) return OKKT_ERR_INVALID;
  try {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    selinv_diag_enqueue(h->N, h->sl, h->S.n, d_out, h->stream);
    return selinv_sync(h, "inverse diagonal export");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_inverse_diag_dev");
  }
}

int okkt_get_inverse_diag(okkt_handle h, double* d_out) {
  if (!h || !d_out) return OKKT_ERR_INVALID;
  try {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t n = h->S.n;
    if (n == 0) return OKKT_OK;
    if ((rc = rhs_stage(h, n)) != OKKT_OK) return rc;
    selinv_diag_enqueue(h->N, h->sl, n, h->d_rhs_stage, h->stream);
    if ((rc = selinv_sync(h, "inverse diagonal export")) != OKKT_OK) return rc;
    if (hipMemcpy(d_out, h->d_rhs_stage, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "inverse diagonal download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_inverse_diag");
  }
}

int okkt_get_inverse_on_pattern_dev(okkt_handle h, double* d_zval) {
  if (!h || (!d_zval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  try {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    selinv_pattern_enqueue(h->sl, h->S.nnz_in, d_zval, h->stream);
    return selinv_sync(h, "inverse export on the input pattern");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_inverse_on_pattern_dev");
  }
}

int okkt_get_inverse_on_pattern(okkt_handle h, double* zval, int64_t* nnz_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  if (nnz_out) *nnz_out = h->S.nnz_in;
  if (!zval) return nnz_out ? OKKT_OK : OKKT_ERR_INVALID;
  try {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t nnz = h->S.nnz_in;
    if (nnz == 0) return OKKT_OK;
    DevTemp t;
    if (!t.alloc(nnz)) return solver_set_error(h, OKKT_ERR_ALLOC, "inverse export staging allocation failed");
    selinv_pattern_enqueue(h->sl, nnz, t.p, h->stream);
    if ((rc = selinv_sync(h, "inverse export on the input pattern")) != OKKT_OK) return rc;
    if (hipMemcpy(zval, t.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "inverse export download failed");
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_inverse_on_pattern");
  }
}

int okkt_get_inverse_csc(okkt_handle h, int64_t* colptr_out, int64_t* rowval_out, double* val_out, int64_t* nnz_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  const Symbolic& S = h->S;
  if (nnz_out) *nnz_out = S.nnzL_stored;
  if (!colptr_out || !rowval_out || !val_out) return OKKT_OK;
  try {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const SelinvWork& W = h->sl;
    std::vector<double> z((size_t)W.z_doubles);
    if ((rc = selinv_sync(h, "inverse export")) != OKKT_OK) return rc;
    if (W.z_doubles > 0 && hipMemcpy(z.data(), W.Z, (size_t)W.z_doubles * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "download of Z failed");
    int64_t q = 0;
    for (int s = 0; s < S.nsuper; ++s) {
      const int64_t f = S.row_ptr[s + 1] - S.row_ptr[s];
      const int64_t k = S.sn_col0[s + 1] - S.sn_col0[s];
      const double* zf = z.data() + W.zpos_host[s];
      for (int64_t lc = 0; lc < k; ++lc) {
        colptr_out[S.sn_col0[s] + lc] = q;
        for (int64_t i = lc; i < f; ++i) {
          rowval_out[q] = S.rows[S.row_ptr[s] + i];
          val_out[q] = zf[i + lc * f];
          ++q;
        }
      }
    }
    colptr_out[S.n] = q;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_get_inverse_csc");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_inverse_csc");
  }
}

int okkt_logdet(okkt_handle h, double* logabsdet, int32_t* sign) {
  if (!h || !logabsdet || !sign) return OKKT_ERR_INVALID;
  try {
    int rc = selinv_ready(h, false);
    if (rc != OKKT_OK) return rc;
    const int64_t n = h->S.n;
    std::vector<double> d((size_t)n);
    if ((rc = selinv_sync(h, "logdet")) != OKKT_OK) return rc;
    if (n > 0 && hipMemcpy(d.data(), h->N.d.dvals, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "download of D failed");
    double acc = 0.0;
    int32_t sg = 1;
    for (int64_t i = 0; i < n; ++i) {
      const double v = d[(size_t)i];
      if (v < 0) sg = -sg;
      else if (!(v > 0)) sg = 0;   // zero or NaN
      acc += std::log(std::fabs(v));
    }
    if (h->sc.valid && n > 0) {
      // log |det F| = log |det F~| - 2 sum_i log s_i: for powers of two 2 ln 2 times the integer sum of the exponents
      int64_t esum = 0;
      double lsum = 0.0;
      if (h->sc.info.mode == OKKT_SCALE_RUIZ) {
        std::vector<int> ex((size_t)n);
        if (hipMemcpy(ex.data(), h->sc.expo, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
          return solver_set_error(h, OKKT_ERR_HIP, "download of the scaling exponents failed");
        for (int64_t i = 0; i < n; ++i) esum += ex[(size_t)i];
      } else {
        std::vector<double> sv((size_t)n);
        if (hipMemcpy(sv.data(), h->sc.s_cur, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
          return solver_set_error(h, OKKT_ERR_HIP, "download of the scaling failed");
        for (int64_t i = 0; i < n; ++i) {
          int ex = 0;
          if (std::frexp(sv[(size_t)i], &ex) == 0.5) esum += ex - 1;
          else lsum += std::log(sv[(size_t)i]);
        }
      }
      acc -= 2.0 * 0.69314718055994530942 * (double)esum + 2.0 * lsum;
    }
    *logabsdet = acc;
    *sign = sg;
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_logdet");
  }
}

// ---- the Schur route made whole: S^-1, selected inversion and the log-determinant through it ------------------

static int schur_inverse_impl(okkt_solver_s* h, double* Z, int64_t ld, bool on_device) {
  int rc = ensure_device(h);
  if (rc == OKKT_OK) rc = schur_ready(h, false);
  if (rc == OKKT_OK) rc = schur_dense_ready(h);
  if (rc != OKKT_OK) return rc;
  const int64_t ns = h->S.nschur;
  if (ld < ns) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_get_inverse: ld < ns");
  DevTemp t;
  if (!on_device && !t.alloc(ns * ns)) return solver_set_error(h, OKKT_ERR_ALLOC, "inverse staging allocation failed");
  (void)hipEventRecord(h->ev0, h->stream);
  std::string e = dense_ldlt_inverse_enqueue(h->dl, on_device ? Z : t.p, on_device ? ld : ns, h->stream);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, "dense Schur inverse: " + e);
  (void)hipEventRecord(h->ev1, h->stream);
  unsigned long long nf = 0;
  hipError_t he = hipMemcpyAsync(&nf, h->dl.nonfinite, sizeof(nf), hipMemcpyDeviceToHost, h->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("dense Schur inverse failed: ") + hipGetErrorString(he));
  h->dl.inv_nonfinite = (long long)nf;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_solve_ms = ms;
  if (!on_device && hipMemcpy2D(Z, (size_t)ld * sizeof(double), t.p, (size_t)ns * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess)
    return solver_set_error(h, OKKT_ERR_HIP, "inverse download failed");
  return OKKT_OK;
}

int okkt_schur_get_inverse(okkt_handle h, double* Z, int64_t ld) {
  if (!h || !Z) return OKKT_ERR_INVALID;
  try {
    return schur_inverse_impl(h, Z, ld, false);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_get_inverse");
  }
}

int okkt_schur_get_inverse_dev(okkt_handle h, double* d_Z, int64_t ld) {
  if (!h || !d_Z) return OKKT_ERR_INVALID;
  try {
    return schur_inverse_impl(h, d_Z, ld, true);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_get_inverse_dev");
  }
}

int64_t okkt_schur_inverse_nonfinite(okkt_handle h) {
  if (!h) return OKKT_ERR_INVALID;
  return (int64_t)h->dl.inv_nonfinite;
}

int okkt_schur_selinv(okkt_handle h, okkt_selinv_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  try {
    int rc = schur_route_ready(h);
    if (rc != OKKT_OK) return rc;
    SelinvWork& W = h->sl;
    const int ssn = h->N.schur_sn;
    const int64_t ns = h->S.nschur;
    if (!W.planned || W.analysis != h->n_analyze_calls || W.arena != h->N.d.arena || W.skip_sn != ssn) {
      (void)hipStreamSynchronize(h->stream);
      std::string e = selinv_setup(h->S, h->N, h->pat_colptr.data(), h->pat_rowval.data(), W, ssn);
      if (!e.empty()) { selinv_release(W); return solver_set_error(h, OKKT_ERR_ALLOC, "selected inversion set-up: " + e); }
      W.analysis = h->n_analyze_calls;
      W.arena = h->N.d.arena;
    }
    W.factor_seq = -1;
    (void)hipEventRecord(h->ev0, h->stream);
    // the Schur front's panel is S^-1 in the set's order, which is the front's column order (k_schur_gather / k_schur_put); the
    // schedule of the plain route then runs on everything below it
    std::string e = dense_ldlt_inverse_enqueue(h->dl, W.Z + W.zpos_host[(size_t)ssn], ns, h->stream);
    if (e.empty()) e = selinv_enqueue(h->N, W);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    (void)hipEventRecord(h->ev1, h->stream);
    unsigned long long nf = 0;
    hipError_t he = hipMemcpyAsync(&nf, W.count, sizeof(nf), hipMemcpyDeviceToHost, h->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("selected inversion failed: ") + hipGetErrorString(he));
    W.factor_seq = h->factor_seq;
    W.dense_seq = h->dl.seq;
    if (info) {
      float ms = 0;
      info->seconds_device = hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess ? ms * 1e-3 : 0.0;
      info->arena_bytes = W.bytes;
      info->nonfinite = (int64_t)nf;
      info->status = nf ? 1 : 0;
      info->flops = W.flops + (double)ns * (double)ns * (double)ns;
    }
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_schur_selinv");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_selinv");
  }
}

int okkt_schur_logdet(okkt_handle h, double* logabsdet, int32_t* sign) {
  if (!h || !logabsdet || !sign) return OKKT_ERR_INVALID;
  try {
    int rc = schur_route_ready(h);
    if (rc != OKKT_OK) return rc;
    const int64_t ns = h->S.nschur, n1 = h->S.n - ns;
    std::vector<double> d((size_t)n1), dg((size_t)ns), sub((size_t)ns, 0.0);
    std::vector<int> ptype((size_t)ns);
    if ((rc = schur_sync(h, "logdet")) != OKKT_OK) return rc;
    const size_t pitch = (size_t)(ns + 1) * sizeof(double);      // down the diagonal of the dense factor, and the entries below it
    if ((n1 > 0 && hipMemcpy(d.data(), h->N.d.dvals, (size_t)n1 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy2D(dg.data(), sizeof(double), h->dl.F, pitch, sizeof(double), (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess ||
        (ns > 1 && hipMemcpy2D(sub.data(), sizeof(double), h->dl.F + 1, pitch, sizeof(double), (size_t)(ns - 1), hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy(ptype.data(), h->dl.ptype, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "download of D failed");
    double acc = 0.0;
    int32_t sg = 1;
    auto take = [&](double v) {
      if (v < 0) sg = -sg;
      else if (!(v > 0)) sg = 0;   // zero or NaN
      acc += std::log(std::fabs(v));
    };
    for (int64_t i = 0; i < n1; ++i) take(d[(size_t)i]);
    for (int64_t k = 0; k < ns; ++k) {
      if (ptype[(size_t)k] == 0) { take(dg[(size_t)k]); continue; }
      // a 2 x 2 block [a b; b c]: det = b^2 ((a / |b|)(c / |b|) - 1), the scaled form of the solves
      const double b = sub[(size_t)k], t = std::fabs(b);
      take(t);
      take(t);
      take((dg[(size_t)k] / t) * (dg[(size_t)k + 1] / t) - 1.0);
      ++k;
    }
    *logabsdet = acc;
    *sign = sg;
    return OKKT_OK;
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_schur_logdet");
  }
}

// ---- threshold pivot report (pivots.hip) ------------------------------------------------------------------

// device, analysis, no partition, a complete factorisation (Schur mode: a complete okkt_factor_schur); need_report: a report of it
static int pivots_ready(okkt_solver_s* h, bool need_report) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  if (h->S.nparts > 1)
    return solver_set_error(h, OKKT_ERR_INVALID, "the pivot report is not available on a partitioned handle (okkt_dist_set_partition with nparts > 1)");
  if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
  if (!h->factored)
    return solver_set_error(h, OKKT_ERR_INVALID, "the pivot report needs a complete factorisation (none yet, or an early exit stopped it)");
  if (need_report && (!h->pv.planned || h->pv.factor_seq != h->factor_seq))
    return solver_set_error(h, OKKT_ERR_INVALID, "no pivot report of the current factorisation: call okkt_pivot_report after okkt_factor");
  return OKKT_OK;
}

int okkt_pivot_report(okkt_handle h, double u, okkt_pivot_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  try {
    int rc = pivots_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (!std::isfinite(u) || u > 1.0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_pivot_report: u must be finite and at most 1");
    if (u <= 0.0) u = 1e-8;      // parameters.jl:25 (ma97_u)
    PivotWork& W = h->pv;
    hipStream_t st = h->stream;
    if (!W.planned || W.analysis != h->n_analyze_calls || W.arena != h->N.d.arena) {
      (void)hipStreamSynchronize(st);
      std::string e = pivots_setup(h->S, h->N, W);
      if (!e.empty()) { pivots_release(W); return solver_set_error(h, OKKT_ERR_ALLOC, "pivot report set-up: " + e); }
      W.analysis = h->n_analyze_calls;
      W.arena = h->N.d.arena;
    }
    const bool scan = W.factor_seq != h->factor_seq;
    if (scan) {
      W.factor_seq = -1;
      (void)hipEventRecord(h->ev0, st);
      std::string e = pivots_scan_enqueue(h->N, W, st);
      if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
      (void)hipEventRecord(h->ev1, st);
    }
    pivots_count_enqueue(W, 1.0 / u, st);
    PvCount part[kPvCountBlocks];
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(part, W.count, sizeof(part), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("pivot report failed: ") + hipGetErrorString(he));
    if (scan) {
      float ms = 0;
      W.seconds_device = hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess ? ms * 1e-3 : 0.0;
      W.factor_seq = h->factor_seq;
    }
    W.u = u;
    W.rejected = 0; W.nonfinite_cols = 0; W.max_col = -1; W.max_multiplier = 0.0;
    for (int b = 0; b < kPvCountBlocks; ++b) {
      W.rejected += part[b].rejected;
      W.nonfinite_cols += part[b].nonfinite;
      if (part[b].max_idx < 0) continue;
      if (W.max_col < 0 || part[b].max_g > W.max_multiplier || (part[b].max_g == W.max_multiplier && part[b].max_idx < W.max_col)) {
        W.max_multiplier = part[b].max_g;
        W.max_col = part[b].max_idx;
      }
    }
    if (info) {
      info->u = W.u; info->rejected = W.rejected; info->nonfinite_cols = W.nonfinite_cols;
      info->max_multiplier = W.max_multiplier; info->max_col = W.max_col; info->seconds_device = W.seconds_device;
    }
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_pivot_report");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_pivot_report");
  }
}

static int pivots_copy_out(okkt_solver_s* h, double* g_out, int64_t* partner_out, hipMemcpyKind kind) {
  const size_t n = (size_t)h->S.n;
  hipError_t he = hipSuccess;
  if (n > 0) he = hipMemcpyAsync(g_out, h->pv.g, n * sizeof(double), kind, h->stream);
  if (he == hipSuccess && n > 0 && partner_out) he = hipMemcpyAsync(partner_out, h->pv.partner, n * sizeof(int64_t), kind, h->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
  if (he != hipSuccess) return solver_set_error(h, OKKT_ERR_HIP, std::string("multiplier export failed: ") + hipGetErrorString(he));
  return OKKT_OK;
}

int okkt_get_multipliers(okkt_handle h, double* g_out, int64_t* partner_out) {
  if (!h || !g_out) return OKKT_ERR_INVALID;
  try {
    int rc = pivots_ready(h, true);
    if (rc != OKKT_OK) return rc;
    return pivots_copy_out(h, g_out, partner_out, hipMemcpyDeviceToHost);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_multipliers");
  }
}

int okkt_get_multipliers_dev(okkt_handle h, double* d_g_out, int64_t* d_partner_out) {
  if (!h || !d_g_out) return OKKT_ERR_INVALID;
  try {
    int rc = pivots_ready(h, true);
    if (rc != OKKT_OK) return rc;
    return pivots_copy_out(h, d_g_out, d_partner_out, hipMemcpyDeviceToDevice);
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_multipliers_dev");
  }
}

int64_t okkt_get_rejected_pivots(okkt_handle h, int64_t* idx_out, int64_t* partner_out, int64_t cap) {
  if (!h) return OKKT_ERR_INVALID;
  try {
    int rc = pivots_ready(h, true);
    if (rc != OKKT_OK) return rc;
    PivotWork& W = h->pv;
    const int64_t n = h->S.n;
    if (W.host_seq != W.factor_seq || (int64_t)W.g_host.size() != n) {
      W.host_seq = -1;
      W.g_host.resize((size_t)n);
      W.partner_host.resize((size_t)n);
      if ((rc = pivots_copy_out(h, W.g_host.data(), W.partner_host.data(), hipMemcpyDeviceToHost)) != OKKT_OK) return rc;
      W.host_seq = W.factor_seq;
    }
    const double inv_u = 1.0 / W.u;
    std::vector<int64_t> rej;
    for (int64_t c = 0; c < n; ++c)
      if (W.g_host[(size_t)c] > inv_u) rej.push_back(c);
    std::sort(rej.begin(), rej.end(), [&](int64_t a, int64_t b) {
      const double ga = W.g_host[(size_t)a], gb = W.g_host[(size_t)b];
      return ga > gb || (ga == gb && a < b);
    });
    for (int64_t t = 0; t < (int64_t)rej.size() && t < cap; ++t) {
      if (idx_out) idx_out[t] = rej[(size_t)t];
      if (partner_out) partner_out[t] = W.partner_host[(size_t)rej[(size_t)t]];
    }
    return (int64_t)rej.size();
  } catch (const std::bad_alloc&) {
    return solver_set_error(h, OKKT_ERR_ALLOC, "out of host memory in okkt_get_rejected_pivots");
  } catch (...) {
    return solver_set_error(h, OKKT_ERR_INTERNAL, "unexpected exception in okkt_get_rejected_pivots");
  }
}

}  // extern "C"

