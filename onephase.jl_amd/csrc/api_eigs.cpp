// C ABI, linear-solver level: the eigenpairs of the factored matrix nearest zero by block shift-invert Krylov-Schur (eigs.hip,
// sym_eig.h): the driver, its entry points and the test hook of the dense eigen-solver.
#include <cmath>
#include <cstring>

#include "api_internal.h"
#include "sym_eig.h"

using namespace okkt;

namespace okkt {

namespace {

// the options behind their checks: the operator's order n, the basis and the tolerance in effect
struct EigsPlan {
  int nev = 0, block = 0, mb = 0, max_restarts = 0;
  double tol = 0.0;
  int64_t n = 0;        // order of the operator: nlead in pencil mode, else dim
  bool pencil = false;
  uint64_t seed = 0;
};

// the checks that need no device; the analysis must exist (n comes from it)
int eigs_plan(okkt_solver_s* h, const okkt_eigs_opts* o, EigsPlan& P) {
  if (o->nev < 1 || o->nev > kEigMaxNev) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs: nev must be 1..32");
  if (o->block < 1 || o->block > kEigMaxBlock) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs: block must be 1..4");
  if (o->max_restarts < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs: max_restarts < 0");
  if (!(o->tol >= 0.0)) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs: tol must be >= 0 (0: 2^-26)");
  const int floor_mb = 2 * o->nev + 3 * o->block;
  if (o->max_basis != 0 && (o->max_basis < floor_mb || o->max_basis > kEigMaxBasis))
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs: max_basis must be 0 or in 2 nev + 3 block .. 128");
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  const int64_t dim = h->S.n;
  if (o->nlead < 0 || o->nlead > dim) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs: nlead must be 0..dim");
  P.pencil = o->nlead > 0 && o->nlead < dim;
  P.n = P.pencil ? o->nlead : dim;
  if ((int64_t)o->nev > P.n) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs: nev exceeds the order of the problem (nlead in pencil mode, else dim)");
  P.nev = o->nev;
  P.block = o->block;
  P.max_restarts = o->max_restarts;
  P.tol = o->tol > 0.0 ? o->tol : std::ldexp(1.0, -26);
  P.seed = o->seed;
  if (o->max_basis != 0) P.mb = o->max_basis;
  else P.mb = (int)std::max<int64_t>(floor_mb, std::min<int64_t>(std::min(std::max(48, floor_mb), kEigMaxBasis), P.n));
  return OKKT_OK;
}

// as okkt_condest: a device, an analysis, no partition, no Schur mode, a complete factorisation; the row map of the residual pass
int eigs_ready(okkt_solver_s* h) {
  if (schur_mode(h)) return schur_refuse(h, "okkt_eigs");
  int rc = refine_ready(h, false);
  if (rc != OKKT_OK) return rc;
  if (!h->numeric_ready || !h->factored)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_eigs called before a complete factorisation (none yet, or an early exit stopped it)");
  return OKKT_OK;
}

}  // namespace

int solver_eigs_device(okkt_solver_s* h, const okkt_eigs_opts* o, const double* d_nzval, double* lambda, double* d_vecs, double* resid,
                       okkt_eigs_info* info) {
  EigsPlan P;
  int rc = eigs_plan(h, o, P);
  if (rc != OKKT_OK) return rc;
  if ((rc = eigs_ready(h)) != OKKT_OK) return rc;
  const int64_t dim = h->S.n, n = P.n;
  const int nev = P.nev, mb = P.mb;
  if (h->eg.base && (h->eg.dim != dim || h->eg.mb < mb)) (void)hipStreamSynchronize(h->stream);   // before the smaller workspace is freed
  std::string e = eigs_alloc(dim, mb, h->eg);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_ALLOC, "okkt_eigs workspace: " + e);
  if ((rc = refine_work(h, 0, 8)) != OKKT_OK) return rc;
  EigsWork& W = h->eg;
  W.nb = eigs_workgroups(n);
  hipStream_t st = h->stream;
  okkt_eigs_info I;
  std::memset(&I, 0, sizeof(I));
  I.basis = mb;
  I.bytes = W.bytes;
  I.status = 1;

  int cur = 0;                     // the buffers that hold V and OV
  int m = 0;                       // columns of V
  uint64_t next_col = 0;           // hashed columns drawn so far
  std::vector<double> G((size_t)mb * mb, 0.0), S((size_t)mb * mb), work((size_t)mb * mb), Gm((size_t)mb * mb);
  std::vector<double> theta((size_t)mb, 0.0), Sh((size_t)kEigMaxBasis * kEigMaxKeep, 0.0), c1((size_t)mb * 4), rel((size_t)nev, NAN);
  double out[kEigOut];
  const double kDrop = std::ldexp(1.0, -33);
  constexpr int kOffRitz = 0, kOffN0 = 32, kOffN1 = 36, kOffCol = 40, kOffRes = 64;

  auto col = [&](double* base, int j) { return base + (int64_t)j * dim; };
  auto read_out = [&]() { return stream_read(h, out, W.out, sizeof(out), "okkt_eigs"); };
  // the first cnt columns of S (m rows) on the device, theta behind them
  auto upload_s = [&](int cnt) -> int {
    for (int v = 0; v < m; ++v)
      for (int j = 0; j < cnt; ++j) Sh[(size_t)v * kEigMaxKeep + j] = S[(size_t)v * m + j];
    int r = stage_upload(h, W.sd, Sh.data(), (int64_t)m * kEigMaxKeep, "okkt_eigs: upload of the Ritz coefficients");
    if (r == OKKT_OK) r = stage_upload(h, W.sd + (size_t)kEigMaxBasis * kEigMaxKeep, theta.data(), std::min(m, kEigMaxNev), "okkt_eigs: upload of the Ritz values");
    return r;
  };
  // Q's p columns orthonormalised against the m columns of V and among themselves (two classical Gram-Schmidt passes each); the
  // columns that survive the drop rule are packed to the front of Q.  have_c1: W.c1 already holds V' Q
  auto orth_block = [&](int p, bool have_c1, int* kept) -> int {
    double* V = W.V[cur];
    eigs_orth_norm_enqueue(W, n, nullptr, 0, W.Q, p, kOffN0, st);
    if (m > 0) {
      if (!have_c1) eigs_project_enqueue(W, n, V, m, W.Q, p, st);
      eigs_orth_project_enqueue(W, n, V, m, W.Q, p, st);
      eigs_orth_norm_enqueue(W, n, V, m, W.Q, p, kOffN1, st);
    }
    int a = 0;
    for (int j = 0; j < p; ++j) {
      double* w = col(W.Q, j);
      if (a > 0) {
        eigs_project_enqueue(W, n, W.Q, a, w, 1, st);
        eigs_orth_project_enqueue(W, n, W.Q, a, w, 1, st);
      }
      eigs_orth_norm_enqueue(W, n, W.Q, a, w, 1, kOffCol + j, st);
      int r = read_out();
      if (r != OKKT_OK) return r;
      const double n0 = out[kOffN0 + j], n1 = out[kOffCol + j];
      if (n1 > 0.0 && n1 >= kDrop * n0 && std::isfinite(n1)) {
        eigs_scale_enqueue(W, n, w, col(W.Q, a), kOffCol + j, st);
        ++a;
      } else {
        ++I.dropped_columns;
      }
    }
    *kept = a;
    return OKKT_OK;
  };
  auto fresh_block = [&](int* kept) -> int {
    eigs_fill_enqueue(W, n, W.Q, P.block, P.seed, next_col, st);
    next_col += (uint64_t)P.block;
    return orth_block(P.block, false, kept);
  };
  // W = Op(x) for p columns at x, into dst (both with leading dimension dim): one solve pass
  auto apply_op = [&](const double* x, double* dst, int p) -> int {
    I.solves += p;
    if (!P.pencil) return solver_solve_enqueue(h, x, dst, p, false);
    eigs_pad_enqueue(W, n, x, p, st);
    int r = solver_solve_enqueue(h, W.P, W.Y, p, false);
    if (r == OKKT_OK && dst != W.Y) eigs_restrict_enqueue(W, n, dst, p, st);
    return r;
  };

  int q = 0;
  if ((rc = fresh_block(&q)) != OKKT_OK) return rc;
  int nconv = 0;
  bool nonfinite = false;
  while (q > 0) {
    double *V = W.V[cur], *OV = W.OV[cur];
    if ((rc = hip_check(h, hipMemcpyAsync(col(V, m), W.Q, (size_t)((int64_t)q * dim) * sizeof(double), hipMemcpyDeviceToDevice, st), "okkt_eigs: block copy")) != OKKT_OK)
      return rc;
    if ((rc = apply_op(col(V, m), col(OV, m), q)) != OKKT_OK) return rc;
    ++I.sweeps;
    // the new block column of G = V' Op V, formed in full and mirrored
    const int mq = m + q;
    eigs_project_enqueue(W, n, V, mq, col(OV, m), q, st);
    if ((rc = stream_read(h, c1.data(), W.c1, (size_t)mq * 4 * sizeof(double), "okkt_eigs")) != OKKT_OK) return rc;
    for (int v = 0; v < mq && !nonfinite; ++v)
      for (int c = 0; c < q; ++c) nonfinite = nonfinite || !std::isfinite(c1[(size_t)v * 4 + c]);
    if (nonfinite) break;
    for (int c = 0; c < q; ++c) {
      const int j = m + c;
      for (int v = 0; v <= j; ++v) G[(size_t)v * mb + j] = G[(size_t)j * mb + v] = c1[(size_t)v * 4 + c];
    }
    m = mq;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) Gm[(size_t)i * m + j] = G[(size_t)i * mb + j];
    if (sym_eig(m, Gm.data(), m, theta.data(), S.data(), work.data()) == 1) { nonfinite = true; break; }
    // the residual norms of the leading Ritz pairs
    const int k = std::min(nev, m);
    if ((rc = upload_s(k)) != OKKT_OK) return rc;
    eigs_ritz_enqueue(W, n, m, k, V, OV, st);
    if ((rc = read_out()) != OKKT_OK) return rc;
    nconv = 0;
    bool lead = true;
    for (int j = 0; j < k; ++j) {
      rel[(size_t)j] = out[kOffRitz + j] / std::fabs(theta[(size_t)j]);
      lead = lead && rel[(size_t)j] <= P.tol;
      if (lead) ++nconv;
    }
    if ((int64_t)m == n) { I.status = 2; break; }
    if (k == nev && nconv == nev) { I.status = 0; break; }
    // the next block: Op(Q) against the whole of the current V (its first projection is the block column of G just read)
    if ((rc = hip_check(h, hipMemcpyAsync(W.Q, col(OV, m - q), (size_t)((int64_t)q * dim) * sizeof(double), hipMemcpyDeviceToDevice, st), "okkt_eigs: block copy")) != OKKT_OK)
      return rc;
    int qn = 0;
    if ((rc = orth_block(q, true, &qn)) != OKKT_OK) return rc;
    for (int tries = 0; qn == 0 && tries < 4; ++tries) {   // an invariant subspace: a fresh hashed block
      ++I.fresh_blocks;
      if ((rc = fresh_block(&qn)) != OKKT_OK) return rc;
    }
    q = qn;
    if (q == 0) break;
    if (m + q > mb) {
      // restart: the next block was taken against the whole basis; V and OV are compressed out of place, never a block truncated
      if (I.restarts >= P.max_restarts) break;
      const int keep = std::min(m, nev + P.block);
      if ((rc = upload_s(keep)) != OKKT_OK) return rc;
      eigs_compress_enqueue(W, n, m, keep, V, W.V[cur ^ 1], OV, W.OV[cur ^ 1], 2, st);
      cur ^= 1;
      std::fill(G.begin(), G.end(), 0.0);
      for (int j = 0; j < keep; ++j) G[(size_t)j * mb + j] = theta[(size_t)j];
      m = keep;
      ++I.restarts;
    }
  }
  if (nonfinite) {
    (void)hipStreamSynchronize(st);
    I.status = 3;
    for (int j = 0; j < nev; ++j) { lambda[j] = NAN; resid[j] = NAN; }
    if (info) *info = I;
    return OKKT_OK;
  }
  I.nconv = nconv;
  // the returned pairs: lambda = 1 / theta, v = F^-1 E' (V s) scaled -- in standard mode that is OV s, which the basis already holds
  const int k = std::min(nev, m);
  for (int j = 0; j < nev; ++j) { lambda[j] = j < k ? 1.0 / theta[(size_t)j] : NAN; resid[j] = j < k ? rel[(size_t)j] : NAN; }
  if ((rc = upload_s(k)) != OKKT_OK) return rc;
  if (!P.pencil) {
    eigs_compress_enqueue(W, n, m, k, W.OV[cur], W.X, nullptr, nullptr, 1, st);
  } else {
    double* xs = W.V[cur ^ 1];
    eigs_compress_enqueue(W, n, m, k, W.V[cur], xs, nullptr, nullptr, 1, st);
    for (int j0 = 0; j0 < k; j0 += kEigMaxBlock) {
      const int nr = std::min(kEigMaxBlock, k - j0);
      if ((rc = apply_op(col(xs, j0), W.Y, nr)) != OKKT_OK) return rc;
      if ((rc = hip_check(h, hipMemcpyAsync(col(W.X, j0), W.Y, (size_t)((int64_t)nr * dim) * sizeof(double), hipMemcpyDeviceToDevice, st), "okkt_eigs: vector copy")) != OKKT_OK)
        return rc;
    }
  }
  eigs_finish_enqueue(W, n, W.X, k, st);
  if (d_nzval) {
    // the true residuals lambda B v - F v of the returned vectors: the double-double pass of okkt_residual
    I.true_residuals = 1;
    refine_gather_enqueue(h->rf, d_nzval, st);
    for (int j0 = 0; j0 < k; j0 += 4) {
      const int nr = std::min(4, k - j0);
      EigsLam L;
      for (int c = 0; c < 4; ++c) L.lam[c] = lambda[j0 + std::min(c, nr - 1)];
      eigs_lambda_b_enqueue(W, n, col(W.X, j0), nr, L, st);
      ResidSet R;
      for (int s = 0; s < 4; ++s) {
        const int c = std::min(s, nr - 1);
        R.b[s] = col(W.P, c); R.x[s] = col(W.X, j0 + c); R.r[s] = col(W.Y, c); R.om[s] = h->rf_om + 2 * c;
      }
      refine_residual_enqueue(h->rf, R, nr, st);
      eigs_orth_norm_enqueue(W, dim, nullptr, 0, W.Y, nr, kOffRes + j0, st);
    }
    if ((rc = read_out()) != OKKT_OK) return rc;
    for (int j = 0; j < k; ++j) resid[j] = out[kOffRes + j];
  }
  if (d_vecs && (rc = hip_check(h, hipMemcpyAsync(d_vecs, W.X, (size_t)((int64_t)k * dim) * sizeof(double), hipMemcpyDeviceToDevice, st), "okkt_eigs: vector copy")) != OKKT_OK)
    return rc;
  if ((rc = stream_sync(h, "okkt_eigs")) != OKKT_OK) return rc;
  if (info) *info = I;
  return OKKT_OK;
}

}  // namespace okkt

extern "C" {

int okkt_eigs_dev(okkt_handle h, const okkt_eigs_opts* opts, const double* d_nzval, double* lambda, double* d_vecs, double* resid,
                  okkt_eigs_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  if (!opts || !lambda || !resid) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "okkt_eigs", [&] { return solver_eigs_device(h, opts, d_nzval, lambda, d_vecs, resid, info); }, true);
}

int okkt_eigs(okkt_handle h, const okkt_eigs_opts* opts, const double* nzval, double* lambda, double* vecs, double* resid, okkt_eigs_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  if (!opts || !lambda || !resid) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "okkt_eigs", [&]() -> int {
    EigsPlan P;
    int rc = eigs_plan(h, opts, P);
    if (rc == OKKT_OK) rc = eigs_ready(h);
    if (rc == OKKT_OK && nzval) rc = stage_nzval(h, nzval, "nzval upload");
    if (rc != OKKT_OK) return rc;
    okkt_eigs_info I;
    std::memset(&I, 0, sizeof(I));
    rc = solver_eigs_device(h, opts, nzval ? h->rf.nz_stage : nullptr, lambda, nullptr, resid, &I);
    if (rc != OKKT_OK) return rc;
    if (info) *info = I;
    if (vecs) {
      const int64_t len = (int64_t)opts->nev * h->S.n;
      if (I.status == 3) { for (int64_t i = 0; i < len; ++i) vecs[i] = NAN; }
      else if ((rc = stage_download(h, vecs, h->eg.X, len, "okkt_eigs: vector download failed")) != OKKT_OK) return rc;
    }
    return OKKT_OK;
  }, true);
}

int okkt_debug_sym_eig(int32_t m, const double* a, double* theta, double* s) {
  if (m < 1 || m > kSymEigMax || !a || !theta || !s) return OKKT_ERR_INVALID;
  double* work = new (std::nothrow) double[(size_t)m * m];
  if (!work) return OKKT_ERR_ALLOC;
  const int rc = sym_eig(m, a, m, theta, s, work);
  delete[] work;
  return rc == 1 ? OKKT_ERR_INVALID : rc;
}

}  // extern "C"
