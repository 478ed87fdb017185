// C ABI, linear-solver level: sparse right-hand sides (solve_sparse_host.cpp / .hip) -- solves that visit only the
// supernodes between the non-zeros of b, the wanted entries of x and the roots of the elimination forest; columns of the inverse.
#include <algorithm>
#include <cstring>

#include "api_internal.h"

using namespace okkt;

namespace {

// the arguments of one call as the checks leave them: the columns' rows and the wanted rows in factor order
struct SparseArgs {
  int64_t nrhs = 0, nx = 0;      // nx: entries per column of the result
  bool x_all = true;
  std::vector<int> b_pos;        // [nnz] permuted rows, column after column
  std::vector<int64_t> b_ptr;    // [nrhs + 1] into b_pos
  std::vector<int> x_pos;        // [nx] (x_all: empty)
};

// analysis, no Schur mode, no partition; the host tables of the reach
int sparse_host_ready(okkt_solver_s* h, const char* what) {
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called");
  if (schur_mode(h)) return schur_refuse(h, what);
  if (h->S.nparts > 1)
    return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + " is not available on a partitioned handle (okkt_dist_set_partition with nparts > 1)");
  if (h->sp.analysis != h->n_analyze_calls) {
    sparse_host_setup(h->S, h->sopts, h->sp);
    h->sp.analysis = h->n_analyze_calls;
  }
  return OKKT_OK;
}

// the indices of a call against the analysed dimension: range, a row twice in one column
int sparse_indices(okkt_solver_s* h, const char* what, int64_t nrhs, const int64_t* colptr, const int64_t* rowidx, bool x_all, int64_t nx, const int64_t* x_idx,
                   SparseArgs& a) {
  const Symbolic& S = h->S;
  SparseWork& W = h->sp;
  a.nrhs = nrhs;
  a.x_all = x_all;
  a.nx = x_all ? S.n : nx;
  a.b_ptr.assign((size_t)nrhs + 1, 0);
  const int64_t base = nrhs > 0 ? colptr[0] : 0;
  const int64_t nnz = nrhs > 0 ? colptr[nrhs] - base : 0;
  a.b_pos.resize((size_t)nnz);
  for (int64_t q = 0; q < nrhs; ++q) {
    ++W.col_epoch;
    a.b_ptr[q + 1] = colptr[q + 1] - base;
    for (int64_t e = colptr[q]; e < colptr[q + 1]; ++e) {
      const int64_t i = rowidx[e];
      if (i < 0 || i >= S.n) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": index " + std::to_string(i) + " is out of range");
      if (W.colmark[i] == W.col_epoch)
        return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": index " + std::to_string(i) + " is given twice in one column of b");
      W.colmark[i] = W.col_epoch;
      a.b_pos[e - base] = S.iperm[i];
    }
  }
  if (W.col_epoch >= 0x7ffffff0) { std::fill(W.colmark.begin(), W.colmark.end(), 0); W.col_epoch = 0; }
  if (!x_all) {
    a.x_pos.resize((size_t)nx);
    for (int64_t t = 0; t < nx; ++t) {
      const int64_t i = x_idx[t];
      if (i < 0 || i >= S.n) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": requested index " + std::to_string(i) + " is out of range");
      a.x_pos[t] = S.iperm[i];
    }
  }
  return OKKT_OK;
}

// what okkt_solve_forward asks for, and the units' places in the device plan
int sparse_device_ready(okkt_solver_s* h, const char* what) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
  if (!h->factored)
    return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + " needs a complete factorisation (none yet, or an early exit stopped it)");
  SparseWork& W = h->sp;
  if (W.plan_analysis != h->n_analyze_calls || W.plan_arena != h->N.d.arena) {
    (void)hipStreamSynchronize(h->stream);
    std::string e = sparse_plan_setup(h->S, h->N, W);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_INTERNAL, "sparse solve set-up: " + e);
    W.plan_analysis = h->n_analyze_calls;
    W.plan_arena = h->N.d.arena;
  }
  return OKKT_OK;
}

void fill_info(const okkt_solver_s* h, const SparseSets& A, okkt_sparse_info* info) {
  info->nsuper = h->S.nsuper;
  info->fwd_reach = A.fwd_reach; info->bwd_reach = A.bwd_reach;
  info->fwd_run = A.fwd_run; info->bwd_run = A.bwd_run;
  info->fringe = A.fringe; info->fringe_entries = A.fringe_entries;
  info->fwd_panel_bytes = A.fwd_panel_bytes; info->bwd_panel_bytes = A.bwd_panel_bytes;
  info->factor_panel_bytes = h->sp.factor_panel_bytes;
  info->batches = 0;
  info->pruned = (A.fwd_full && A.bwd_full) ? 0 : 1;
  info->seconds_device = 0.0;
}

// the batches of a checked call on the stream, timed into last_solve_ms and info, and the wait for them.  d_val: the values in the
// order of a.b_pos; d_out: nrhs x a.nx
int sparse_solve_device(okkt_solver_s* h, const SparseArgs& a, const double* d_val, double* d_out, okkt_sparse_info* info) {
  SparseWork& W = h->sp;
  const Symbolic& S = h->S;
  const double* scale = h->sc.valid ? h->sc.s_cur : nullptr;
  int rc;
  if (!a.x_all && a.nx > 0) {
    if (W.xsel_cap < a.nx) {
      if (W.d_xsel) (void)hipFree(W.d_xsel);
      W.d_xsel = nullptr; W.xsel_cap = 0;
      if (hipMalloc((void**)&W.d_xsel, (size_t)a.nx * sizeof(int)) != hipSuccess) return solver_set_error(h, OKKT_ERR_ALLOC, "sparse solve: allocation of the requested rows failed");
      W.xsel_cap = a.nx;
    }
    if ((rc = hip_check(h, hipMemcpy(W.d_xsel, a.x_pos.data(), (size_t)a.nx * sizeof(int), hipMemcpyHostToDevice), "sparse solve: upload of the requested rows")) != OKKT_OK) return rc;
  }
  SparseSets A;
  if (info) {      // the sets of the whole call
    sparse_reach(S, W, a.b_pos.data(), (int64_t)a.b_pos.size(), a.x_pos.data(), (int64_t)a.x_pos.size(), a.x_all, A);
    fill_info(h, A, info);
    info->pruned = 0;
  }
  (void)hipEventRecord(h->ev0, h->stream);
  rc = for_rhs_batches(h, a.nrhs, [&](int64_t r, int nr, int R) {
    SparseScatter sc;
    sc.pos = a.b_pos.data() + a.b_ptr[r];
    sc.count = (int)(a.b_ptr[r + nr] - a.b_ptr[r]);
    for (int q = 0; q <= kMaxRhs; ++q) sc.col[q] = (int)(a.b_ptr[r + std::min(q, nr)] - a.b_ptr[r]);
    if (!info || a.nrhs > kMaxRhs) sparse_reach(S, W, sc.pos, sc.count, a.x_pos.data(), (int64_t)a.x_pos.size(), a.x_all, A);
    if (info) { ++info->batches; if (!(A.fwd_full && A.bwd_full)) info->pruned = 1; }
    std::string e = sparse_batch_enqueue(S, h->N, W, A, sc, d_val + a.b_ptr[r], scale, R);
    if (!e.empty()) return e;
    if (a.x_all) solve_permute_out(h->N, d_out + r * S.n, S.n, nr, R, false, scale);
    else sparse_gather_enqueue(h->N, W.d_xsel, a.nx, d_out + r * a.nx, a.nx, nr, scale);
    return e;
  });
  if (rc != OKKT_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
  (void)hipEventRecord(h->ev1, h->stream);
  if ((rc = stream_sync(h, "sparse solve")) != OKKT_OK) return rc;
  h->sp.copy_pending = false;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) { h->last_solve_ms = ms; if (info) info->seconds_device = ms * 1e-3; }
  return OKKT_OK;
}

// the checks every form shares, in the order the header states: arguments, analysis and modes, indices
int sparse_check(okkt_solver_s* h, const char* what, int64_t nrhs, const int64_t* colptr, const int64_t* rowidx, const void* val, int64_t nx, const int64_t* x_idx,
                 const void* out, SparseArgs& a) {
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": a negative number of columns");
  if (x_idx && nx < 0) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": a negative number of requested rows");
  if (nrhs > 0 && !colptr) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": null pointer");
  if (nrhs > 0) {
    if (colptr[0] < 0) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": colptr[0] < 0");
    for (int64_t q = 0; q < nrhs; ++q)
      if (colptr[q + 1] < colptr[q]) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": colptr decreases");
    if (colptr[nrhs] > colptr[0] && (!rowidx || !val)) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": null pointer");
  }
  int rc = sparse_host_ready(h, what);
  if (rc != OKKT_OK) return rc;
  const bool x_all = x_idx == nullptr;
  if (nrhs > 0 && !out && (x_all ? h->S.n : nx) > 0) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": null pointer");
  for (int64_t q = 0; q < nrhs; ++q)      // (before anything is sized by the entries)
    if (colptr[q + 1] - colptr[q] > h->S.n) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": a column of b has more entries than rows");
  return sparse_indices(h, what, nrhs, colptr, rowidx, x_all, nx, x_idx, a);
}

int inverse_columns_check(okkt_solver_s* h, int64_t ncols, const int64_t* cols, std::vector<int64_t>& colptr) {
  if (ncols < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_inverse_columns: a negative number of columns");
  if (ncols > 0 && !cols) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_inverse_columns: null pointer");
  colptr.resize((size_t)ncols + 1);
  for (int64_t j = 0; j <= ncols; ++j) colptr[j] = j;
  return OKKT_OK;
}

}  // namespace

extern "C" {

int okkt_solve_sparse_dev(okkt_handle h, int64_t nrhs, const int64_t* b_colptr, const int64_t* b_rowidx, const double* d_b_val, int64_t nx, const int64_t* x_idx,
                          double* d_x_out, okkt_sparse_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_solve_sparse_dev", [&]() -> int {
    SparseArgs a;
    int rc = sparse_check(h, "okkt_solve_sparse", nrhs, b_colptr, b_rowidx, d_b_val, nx, x_idx, d_x_out, a);
    if (rc == OKKT_OK) rc = sparse_device_ready(h, "okkt_solve_sparse");
    if (rc != OKKT_OK) return rc;
    if (info) { SparseSets none; fill_info(h, none, info); info->pruned = 0; }
    if (a.nrhs == 0 || a.nx == 0) return OKKT_OK;
    return sparse_solve_device(h, a, d_b_val + (nrhs > 0 ? b_colptr[0] : 0), d_x_out, info);
  }, true);
}

int okkt_solve_sparse(okkt_handle h, int64_t nrhs, const int64_t* b_colptr, const int64_t* b_rowidx, const double* b_val, int64_t nx, const int64_t* x_idx, double* x_out,
                      okkt_sparse_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_solve_sparse", [&]() -> int {
    SparseArgs a;
    int rc = sparse_check(h, "okkt_solve_sparse", nrhs, b_colptr, b_rowidx, b_val, nx, x_idx, x_out, a);
    if (rc == OKKT_OK) rc = sparse_device_ready(h, "okkt_solve_sparse");
    if (rc != OKKT_OK) return rc;
    if (info) { SparseSets none; fill_info(h, none, info); info->pruned = 0; }
    if (a.nrhs == 0 || a.nx == 0) return OKKT_OK;
    const int64_t nnz = (int64_t)a.b_pos.size(), nout = a.nrhs * a.nx;
    if ((rc = stage_reserve(h, nnz + nout)) != OKKT_OK) return rc;
    double* const d_val = h->d_rhs_stage, * const d_out = h->d_rhs_stage + nnz;
    if ((rc = stage_upload(h, d_val, b_val + b_colptr[0], nnz, "values upload")) != OKKT_OK) return rc;
    if ((rc = sparse_solve_device(h, a, d_val, d_out, info)) != OKKT_OK) return rc;
    return stage_download(h, x_out, d_out, nout, "x download");
  }, true);
}

int okkt_get_inverse_columns_dev(okkt_handle h, int64_t ncols, const int64_t* cols, int64_t nrows, const int64_t* rows, double* d_out, okkt_sparse_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_inverse_columns_dev", [&]() -> int {
    std::vector<int64_t> colptr;
    int rc = inverse_columns_check(h, ncols, cols, colptr);
    if (rc != OKKT_OK) return rc;
    SparseArgs a;
    rc = sparse_check(h, "okkt_get_inverse_columns", ncols, colptr.data(), cols, cols, nrows, rows, d_out, a);
    if (rc == OKKT_OK) rc = sparse_device_ready(h, "okkt_get_inverse_columns");
    if (rc != OKKT_OK) return rc;
    if (info) { SparseSets none; fill_info(h, none, info); info->pruned = 0; }
    if (a.nrhs == 0 || a.nx == 0) return OKKT_OK;
    SparseWork& W = h->sp;
    if (W.ones_cap < ncols) {
      (void)hipStreamSynchronize(h->stream);
      if (W.d_ones) (void)hipFree(W.d_ones);
      W.d_ones = nullptr; W.ones_cap = 0;
      const int64_t cap = std::max<int64_t>(ncols, 256);
      if (hipMalloc((void**)&W.d_ones, (size_t)cap * sizeof(double)) != hipSuccess) return solver_set_error(h, OKKT_ERR_ALLOC, "okkt_get_inverse_columns: allocation of the unit values failed");
      const std::vector<double> ones((size_t)cap, 1.0);
      if ((rc = hip_check(h, hipMemcpy(W.d_ones, ones.data(), (size_t)cap * sizeof(double), hipMemcpyHostToDevice), "okkt_get_inverse_columns: upload of the unit values")) != OKKT_OK) return rc;
      W.ones_cap = cap;
    }
    return sparse_solve_device(h, a, W.d_ones, d_out, info);
  }, true);
}

int okkt_get_inverse_columns(okkt_handle h, int64_t ncols, const int64_t* cols, int64_t nrows, const int64_t* rows, double* out, okkt_sparse_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_inverse_columns", [&]() -> int {
    std::vector<int64_t> colptr;
    int rc = inverse_columns_check(h, ncols, cols, colptr);
    if (rc != OKKT_OK) return rc;
    SparseArgs a;
    rc = sparse_check(h, "okkt_get_inverse_columns", ncols, colptr.data(), cols, cols, nrows, rows, out, a);
    if (rc == OKKT_OK) rc = sparse_device_ready(h, "okkt_get_inverse_columns");
    if (rc != OKKT_OK) return rc;
    if (info) { SparseSets none; fill_info(h, none, info); info->pruned = 0; }
    if (a.nrhs == 0 || a.nx == 0) return OKKT_OK;
    const int64_t nout = a.nrhs * a.nx;
    if ((rc = stage_reserve(h, ncols + nout)) != OKKT_OK) return rc;
    double* const d_val = h->d_rhs_stage, * const d_out = h->d_rhs_stage + ncols;
    const std::vector<double> ones((size_t)ncols, 1.0);
    if ((rc = hip_check(h, hipMemcpy(d_val, ones.data(), (size_t)ncols * sizeof(double), hipMemcpyHostToDevice), "unit values upload")) != OKKT_OK) return rc;
    if ((rc = sparse_solve_device(h, a, d_val, d_out, info)) != OKKT_OK) return rc;
    return stage_download(h, out, d_out, nout, "inverse columns download");
  }, true);
}

int okkt_sparse_reach(okkt_handle h, int64_t nb, const int64_t* b_rows, int64_t nx, const int64_t* x_idx, okkt_sparse_info* info, uint8_t* active_out) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_sparse_reach", [&]() -> int {
    if (!info) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_sparse_reach: null pointer");
    if (nb < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_sparse_reach: a negative number of rows");
    if (x_idx && nx < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_sparse_reach: a negative number of requested rows");
    if (nb > 0 && !b_rows) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_sparse_reach: null pointer");
    int rc = sparse_host_ready(h, "okkt_sparse_reach");
    if (rc != OKKT_OK) return rc;
    const Symbolic& S = h->S;
    SparseWork& W = h->sp;
    std::vector<int> bp((size_t)nb), xp((size_t)(x_idx ? nx : 0));
    for (int64_t t = 0; t < nb; ++t) {
      if (b_rows[t] < 0 || b_rows[t] >= S.n) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_sparse_reach: index " + std::to_string(b_rows[t]) + " is out of range");
      bp[t] = S.iperm[b_rows[t]];
    }
    for (int64_t t = 0; t < (int64_t)xp.size(); ++t) {
      if (x_idx[t] < 0 || x_idx[t] >= S.n) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_sparse_reach: requested index " + std::to_string(x_idx[t]) + " is out of range");
      xp[t] = S.iperm[x_idx[t]];
    }
    SparseSets A;
    sparse_reach(S, W, bp.data(), nb, xp.data(), (int64_t)xp.size(), x_idx == nullptr, A);
    fill_info(h, A, info);
    info->batches = 1;
    if (active_out) {
      std::memset(active_out, 0, (size_t)S.n);
      auto set = [&](int s, uint8_t bit) { for (int j = S.sn_col0[s]; j < S.sn_col0[s + 1]; ++j) active_out[j] |= bit; };
      for (int s : A.fwd_fronts) set(s, 1);
      if (A.bwd_full) { for (int64_t j = 0; j < S.n; ++j) active_out[j] |= 2; }
      else for (int s = 0; s < S.nsuper; ++s) if (W.brun[s] == W.epoch) set(s, 2);
      for (int s : A.fringe_fronts) set(s, 4);
    }
    return OKKT_OK;
  }, true);
}

}  // extern "C"
