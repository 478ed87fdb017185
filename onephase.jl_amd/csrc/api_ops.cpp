// C ABI, linear-solver level: the factor as an operator (factor_ops.hip) -- the two halves of a solve, the
// quadratic form b' F^-1 b from one sweep, products with L, L^T, L D L^T and |L||D||L^T|, the growth factor and a sampled backward
// error of the factor.
#include <algorithm>
#include <cmath>

#include "api_internal.h"

using namespace okkt;

// device, analysis, not Schur mode, no partition, a complete factorisation; plan: the work-item lists and vectors of the products
static int ops_ready(okkt_solver_s* h, const char* what, bool plan) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  if (schur_mode(h)) return schur_refuse(h, what);
  if (h->S.nparts > 1)
    return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + " is not available on a partitioned handle (okkt_dist_set_partition with nparts > 1)");
  if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
  if (!h->factored)
    return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + " needs a complete factorisation (none yet, or an early exit stopped it)");
  FactorOpsWork& W = h->fo;
  if (plan && (!W.planned || W.analysis != h->n_analyze_calls || W.arena != h->N.d.arena)) {
    (void)hipStreamSynchronize(h->stream);
    std::string e = factor_ops_setup(h->S, h->N, W);
    if (!e.empty()) { factor_ops_release(W); return solver_set_error(h, OKKT_ERR_ALLOC, "factor products set-up: " + e); }
    W.analysis = h->n_analyze_calls;
    W.arena = h->N.d.arena;
  }
  return OKKT_OK;
}

static inline const double* ops_scale(const okkt_solver_s* h) { return h->sc.valid ? h->sc.s_cur : nullptr; }

// the span of an entry on the stream, timed into last_solve_ms, and the wait for it
template <class F>
static int ops_timed(okkt_solver_s* h, const char* what, F&& body) {
  (void)hipEventRecord(h->ev0, h->stream);
  int rc = body();
  if (rc != OKKT_OK) return rc;
  (void)hipEventRecord(h->ev1, h->stream);
  if ((rc = stream_sync(h, what)) != OKKT_OK) return rc;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_solve_ms = ms;
  return OKKT_OK;
}

// okkt_solve's batches, stopped behind the forward sweep: z out
static int forward_enqueue(okkt_solver_s* h, const double* d_rhs, double* d_z, int64_t nrhs) {
  const int64_t n = h->S.n;
  return for_rhs_batches(h, nrhs, [&](int64_t r, int nr, int R) {
    solve_permute_in(h->N, d_rhs + r * n, n, nr, R, ops_scale(h));
    std::string e = solve_fwd_enqueue(h->N, 0, R);
    if (e.empty()) factor_ops_z_out(h->N, d_z + r * n, n, nr);
    return e;
  });
}

// ... and started in front of the backward sweep: z in
static int backward_enqueue(okkt_solver_s* h, const double* d_z, double* d_sol, int64_t nrhs) {
  const int64_t n = h->S.n;
  return for_rhs_batches(h, nrhs, [&](int64_t r, int nr, int R) {
    factor_ops_z_in(h->N, d_z + r * n, n, nr, R);
    std::string e = solve_bwd_enqueue(h->N, 0, R);
    if (e.empty()) solve_permute_out(h->N, d_sol + r * n, n, nr, R, false, ops_scale(h));
    return e;
  });
}

// one forward sweep and the reduction per batch; the results are read batch by batch (a few doubles)
static int quadform_device(okkt_solver_s* h, const double* d_rhs, int64_t nrhs, double* q_pos, double* q_neg) {
  const int64_t n = h->S.n;
  FactorOpsWork& W = h->fo;
  for (int64_t r = 0; r < nrhs;) {
    const int nr = (int)std::min<int64_t>(nrhs - r, kMaxRhs);
    const int R = nr >= 3 ? 4 : nr;
    solve_permute_in(h->N, d_rhs + r * n, n, nr, R, ops_scale(h));
    std::string e = solve_fwd_enqueue(h->N, 0, R);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    factor_ops_quadform(h->N, W, nr);
    FoQuad res;
    int rc = hip_check(h, hipGetLastError(), "quadratic form failed");
    if (rc == OKKT_OK) rc = stream_read(h, &res, W.quad + kFoRedBlocks, sizeof(res), "quadratic form failed");
    if (rc != OKKT_OK) return rc;
    for (int q = 0; q < nr; ++q) { q_pos[r + q] = res.pos_h[q]; q_neg[r + q] = res.neg_h[q]; }
    r += nr;
  }
  return OKKT_OK;
}

// y = op x for the columns of one batch, x and y device pointers with columns n apart
static std::string multiply_batch(okkt_solver_s* h, int op, const double* d_x, double* d_y, int nr, int R) {
  const int64_t n = h->S.n;
  FactorOpsWork& W = h->fo;
  const bool abs = op == OKKT_OP_ABS_LDLT;
  std::string e;
  if (op == OKKT_OP_L) {
    factor_ops_load(h->N, W, W.wb, d_x, n, nr, R, false, nullptr, false);
    if (!(e = factor_ops_l(h->N, W, R, false)).empty()) return e;
    factor_ops_store(h->N, W, W.wa, d_y, n, nr, false, nullptr);
    return e;
  }
  if (op == OKKT_OP_LT) {
    factor_ops_load(h->N, W, W.wa, d_x, n, nr, R, false, nullptr, false);
    if (!(e = factor_ops_lt(h->N, W, R, false)).empty()) return e;
    factor_ops_store(h->N, W, W.wb, d_y, n, nr, false, nullptr);
    return e;
  }
  // S^-1 P^T L D L^T P S^-1: the permutation and the scaling in the load and the store, D between the two products
  factor_ops_load(h->N, W, W.wa, d_x, n, nr, R, true, ops_scale(h), abs);
  if (!(e = factor_ops_lt(h->N, W, R, abs)).empty()) return e;
  factor_ops_d(h->N, W, R, abs);
  if (!(e = factor_ops_l(h->N, W, R, abs)).empty()) return e;
  factor_ops_store(h->N, W, W.wa, d_y, n, nr, true, ops_scale(h));
  return e;
}

static int multiply_enqueue(okkt_solver_s* h, int op, const double* d_x, double* d_y, int64_t nrhs) {
  const int64_t n = h->S.n;
  return for_rhs_batches(h, nrhs, [&](int64_t r, int nr, int R) { return multiply_batch(h, op, d_x + r * n, d_y + r * n, nr, R); });
}

static int factor_error_device(okkt_solver_s* h, const double* d_nzval, int32_t probes, okkt_factor_error_info* info) {
  int rc = ensure_row_map(h, "factor error: row map");
  if (rc != OKKT_OK) return rc;
  FactorOpsWork& W = h->fo;
  const int64_t n = h->S.n;
  std::string e = factor_ops_error_alloc(W);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "factor error workspace: " + e);
  if (probes <= 0) probes = 2;
  hipStream_t st = h->stream;
  double* const ones = W.ev, * const zeros = W.ev + n, * const fe = W.ev + 2 * n, * const ae = W.ev + 3 * n, * const scratch = W.ev + 4 * n;
  double* const V = W.ev + 5 * n, * const P = W.ev + (5 + kMaxRhs) * n, * const D = W.ev + (5 + 2 * kMaxRhs) * n;
  info->rho = 0; info->norm_abs_ldlt = 0; info->norm_f = 0; info->eta = 0; info->eta_row = -1; info->probes = probes;
  refine_gather_enqueue(h->rf, d_nzval, st);
  for (int p0 = 0; p0 < probes; p0 += kMaxRhs) {
    const int np = std::min(kMaxRhs, probes - p0);
    const int R = np >= 3 ? 4 : np;
    factor_ops_error_init(W, p0, np, st);
    if (p0 == 0) {
      // |F0| e: the denominators of okkt_residual's pass for x = e, b = 0; |L||D||L^T| e
      ResidSet S;
      DenSet Dn;
      for (int s = 0; s < 4; ++s) { S.b[s] = zeros; S.x[s] = ones; S.r[s] = scratch; S.om[s] = W.eom; Dn.d[s] = fe; }
      refine_residual_den_enqueue(h->rf, S, Dn, 1, st);
      if (!(e = multiply_batch(h, OKKT_OP_ABS_LDLT, ones, ae, 1, 1)).empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    }
    if (!(e = multiply_batch(h, OKKT_OP_LDLT, V, P, np, R)).empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    ResidSet S;
    for (int s = 0; s < 4; ++s) {
      const int64_t q = std::min(s, np - 1);
      S.b[s] = P + q * n; S.x[s] = V + q * n; S.r[s] = D + q * n; S.om[s] = W.eom + 2 * q;
    }
    refine_residual_enqueue(h->rf, S, np, st);
    factor_ops_error_reduce(h->N, W, np, st);
    FoErr part[kFoRedBlocks];
    if ((rc = hip_check(h, hipGetLastError(), "factor error failed")) != OKKT_OK) return rc;
    if ((rc = stream_read(h, part, W.err, sizeof(part), "factor error failed")) != OKKT_OK) return rc;
    for (int b = 0; b < kFoRedBlocks; ++b) {
      info->norm_f = std::max(info->norm_f, part[b].norm_f);
      info->norm_abs_ldlt = std::max(info->norm_abs_ldlt, part[b].norm_a);
      if (part[b].row < 0) continue;
      if (info->eta_row < 0 || part[b].eta > info->eta || (part[b].eta == info->eta && part[b].row < info->eta_row)) {
        info->eta = part[b].eta;
        info->eta_row = part[b].row;
      }
    }
  }
  info->rho = info->norm_f > 0 ? info->norm_abs_ldlt / info->norm_f : (info->norm_abs_ldlt > 0 ? INFINITY : 0.0);
  return OKKT_OK;
}

extern "C" {

int okkt_solve_forward_dev(okkt_handle h, const double* d_rhs, double* d_z, int64_t nrhs) {
  if (!h || !d_rhs || !d_z) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_solve_forward_dev", [&]() -> int {
    int rc = ops_ready(h, "okkt_solve_forward", false);
    if (rc != OKKT_OK) return rc;
    return ops_timed(h, "forward sweep", [&] { return forward_enqueue(h, d_rhs, d_z, nrhs); });
  });
}

int okkt_solve_forward(okkt_handle h, const double* rhs, double* z, int64_t nrhs) {
  if (!h || !rhs || !z) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_solve_forward", [&]() -> int {
    int rc = ops_ready(h, "okkt_solve_forward", false);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc = stage_reserve(h, len)) != OKKT_OK) return rc;
    if ((rc = stage_upload(h, h->d_rhs_stage, rhs, len, "rhs upload")) != OKKT_OK) return rc;
    if ((rc = ops_timed(h, "forward sweep", [&] { return forward_enqueue(h, h->d_rhs_stage, h->d_rhs_stage, nrhs); })) != OKKT_OK) return rc;
    return stage_download(h, z, h->d_rhs_stage, len, "z download");
  });
}

int okkt_solve_backward_dev(okkt_handle h, const double* d_z, double* d_sol, int64_t nrhs) {
  if (!h || !d_z || !d_sol) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_solve_backward_dev", [&]() -> int {
    int rc = ops_ready(h, "okkt_solve_backward", false);
    if (rc != OKKT_OK) return rc;
    return ops_timed(h, "backward sweep", [&] { return backward_enqueue(h, d_z, d_sol, nrhs); });
  });
}

int okkt_solve_backward(okkt_handle h, const double* z, double* sol, int64_t nrhs) {
  if (!h || !z || !sol) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_solve_backward", [&]() -> int {
    int rc = ops_ready(h, "okkt_solve_backward", false);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc = stage_reserve(h, len)) != OKKT_OK) return rc;
    if ((rc = stage_upload(h, h->d_rhs_stage, z, len, "z upload")) != OKKT_OK) return rc;
    if ((rc = ops_timed(h, "backward sweep", [&] { return backward_enqueue(h, h->d_rhs_stage, h->d_rhs_stage, nrhs); })) != OKKT_OK) return rc;
    return stage_download(h, sol, h->d_rhs_stage, len, "sol download");
  });
}

int okkt_quadform_dev(okkt_handle h, const double* d_rhs, int64_t nrhs, double* q_pos, double* q_neg) {
  if (!h || !d_rhs || !q_pos || !q_neg) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_quadform_dev", [&]() -> int {
    int rc = ops_ready(h, "okkt_quadform", true);
    return rc != OKKT_OK ? rc : quadform_device(h, d_rhs, nrhs, q_pos, q_neg);
  }, true);
}

int okkt_quadform(okkt_handle h, const double* rhs, int64_t nrhs, double* q_pos, double* q_neg) {
  if (!h || !rhs || !q_pos || !q_neg) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  return fence(h, "okkt_quadform", [&]() -> int {
    int rc = ops_ready(h, "okkt_quadform", true);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs;
    if (nrhs == 0) return OKKT_OK;
    if ((rc = stage_reserve(h, std::max<int64_t>(len, 1))) != OKKT_OK) return rc;
    if ((rc = stage_upload(h, h->d_rhs_stage, rhs, len, "rhs upload")) != OKKT_OK) return rc;
    return quadform_device(h, h->d_rhs_stage, nrhs, q_pos, q_neg);
  }, true);
}

static int multiply_check(okkt_solver_s* h, int op, int64_t nrhs) {
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (op != OKKT_OP_L && op != OKKT_OP_LT && op != OKKT_OP_LDLT && op != OKKT_OP_ABS_LDLT)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_multiply: unknown op (OKKT_OP_L, OKKT_OP_LT, OKKT_OP_LDLT, OKKT_OP_ABS_LDLT)");
  return OKKT_OK;
}

int okkt_factor_multiply_dev(okkt_handle h, int op, const double* d_x, double* d_y, int64_t nrhs) {
  if (!h || !d_x || !d_y) return OKKT_ERR_INVALID;
  int rc = multiply_check(h, op, nrhs);
  if (rc != OKKT_OK) return rc;
  return fence(h, "okkt_factor_multiply_dev", [&]() -> int {
    int rc2 = ops_ready(h, "okkt_factor_multiply", true);
    if (rc2 != OKKT_OK) return rc2;
    return ops_timed(h, "factor product", [&] { return multiply_enqueue(h, op, d_x, d_y, nrhs); });
  }, true);
}

int okkt_factor_multiply(okkt_handle h, int op, const double* x, double* y, int64_t nrhs) {
  if (!h || !x || !y) return OKKT_ERR_INVALID;
  int rc = multiply_check(h, op, nrhs);
  if (rc != OKKT_OK) return rc;
  return fence(h, "okkt_factor_multiply", [&]() -> int {
    int rc2 = ops_ready(h, "okkt_factor_multiply", true);
    if (rc2 != OKKT_OK) return rc2;
    const int64_t len = h->S.n * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc2 = stage_reserve(h, len)) != OKKT_OK) return rc2;
    if ((rc2 = stage_upload(h, h->d_rhs_stage, x, len, "x upload")) != OKKT_OK) return rc2;
    if ((rc2 = ops_timed(h, "factor product", [&] { return multiply_enqueue(h, op, h->d_rhs_stage, h->d_rhs_stage, nrhs); })) != OKKT_OK) return rc2;
    return stage_download(h, y, h->d_rhs_stage, len, "y download");
  }, true);
}

int okkt_factor_error_dev(okkt_handle h, const double* d_nzval, int32_t probes, okkt_factor_error_info* info) {
  if (!h || !info || (!d_nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  if (probes > kFoMaxProbes) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_error: probes > 8");
  return fence(h, "okkt_factor_error_dev", [&]() -> int {
    int rc = ops_ready(h, "okkt_factor_error", true);
    return rc != OKKT_OK ? rc : factor_error_device(h, d_nzval, probes, info);
  }, true);
}

int okkt_factor_error(okkt_handle h, const double* nzval, int32_t probes, okkt_factor_error_info* info) {
  if (!h || !info || (!nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  if (probes > kFoMaxProbes) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_error: probes > 8");
  return fence(h, "okkt_factor_error", [&]() -> int {
    int rc = ops_ready(h, "okkt_factor_error", true);
    if (rc == OKKT_OK) rc = ensure_row_map(h, "factor error: row map");
    if (rc == OKKT_OK) rc = stage_nzval(h, nzval, "nzval upload");
    return rc != OKKT_OK ? rc : factor_error_device(h, h->rf.nz_stage, probes, info);
  }, true);
}

}  // extern "C"
