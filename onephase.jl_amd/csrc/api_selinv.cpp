// C ABI, linear-solver level: what is read off a finished factor.  Selected inversion (selinv.hip) and the
// log-determinant, each also through the Schur route (section 8.10), and the threshold pivot report (pivots.hip, section 8.9).
#include <algorithm>
#include <cmath>

#include "api_internal.h"

using namespace okkt;

// ---- selected inversion --------------------------------------------------------------------------------------------------------

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

// okkt_selinv and, schur_route, okkt_schur_selinv.  What schur_route changes, and nothing else:
//   the gate           schur_route_ready instead of selinv_ready, and no refusal of a scaled factor (Schur mode has none)
//   the plan           leaves the Schur front out of its block steps (skip_sn = the front; the plain route plans with -1, so
//                      a plan of the other route is planned again)
//   before the sweep   the Schur front's panel of Z is filled with S^-1 from the dense factor
//   afterwards         Z is stamped with the dense factor's sequence number too, and the flops count the ns^3 of that inverse
static int selinv_entry(okkt_handle h, bool schur_route, okkt_selinv_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, schur_route ? "okkt_schur_selinv" : "okkt_selinv", [&]() -> int {
    int rc = schur_route ? schur_route_ready(h) : selinv_ready(h, false);
    if (rc != OKKT_OK) return rc;
    if (!schur_route && h->sc.valid)
      return solver_set_error(h, OKKT_ERR_INVALID, "selected inversion of a scaled factor is not available: the current factor is that of S F S (okkt_set_scaling with OKKT_SCALE_NONE, then factor again)");
    SelinvWork& W = h->sl;
    const int ssn = schur_route ? h->N.schur_sn : -1;
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
    std::string e;
    if (schur_route) e = dense_ldlt_inverse_enqueue(h->dl, W.Z + W.zpos_host[(size_t)ssn], ns, h->stream);
    if (e.empty()) e = selinv_enqueue(h->N, W);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    (void)hipEventRecord(h->ev1, h->stream);
    unsigned long long nf = 0;
    if ((rc = stream_read(h, &nf, W.count, sizeof(nf), "selected inversion failed")) != OKKT_OK) return rc;
    W.factor_seq = h->factor_seq;
    if (schur_route) W.dense_seq = h->dl.seq;
    if (info) {
      float ms = 0;
      info->seconds_device = hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess ? ms * 1e-3 : 0.0;
      info->arena_bytes = W.bytes;
      info->nonfinite = (int64_t)nf;
      info->status = nf ? 1 : 0;
      info->flops = schur_route ? W.flops + (double)ns * (double)ns * (double)ns : W.flops;
    }
    return OKKT_OK;
  }, true);
}

// sign and log |.| of a product, factor by factor
namespace {
struct LogDet {
  double acc = 0.0;
  int32_t sg = 1;
  void take(double v) {
    if (v < 0) sg = -sg;
    else if (!(v > 0)) sg = 0;   // zero or NaN
    acc += std::log(std::fabs(v));
  }
};
}  // namespace

// ---- threshold pivot report ------------------------------------------------------------------------------------------------------

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

// g and the partners (int64: not the staging helpers' doubles) to host or device memory
static int pivots_copy_out(okkt_solver_s* h, double* g_out, int64_t* partner_out, hipMemcpyKind kind) {
  const size_t n = (size_t)h->S.n;
  hipError_t he = hipSuccess;
  if (n > 0) he = hipMemcpyAsync(g_out, h->pv.g, n * sizeof(double), kind, h->stream);
  if (he == hipSuccess && n > 0 && partner_out) he = hipMemcpyAsync(partner_out, h->pv.partner, n * sizeof(int64_t), kind, h->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
  return hip_check(h, he, "multiplier export failed");
}

extern "C" {

int okkt_selinv(okkt_handle h, okkt_selinv_info* info) { return selinv_entry(h, false, info); }
int okkt_schur_selinv(okkt_handle h, okkt_selinv_info* info) { return selinv_entry(h, true, info); }

int okkt_get_inverse_diag_dev(okkt_handle h, double* d_out) {
  if (!h || !d_out) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_inverse_diag_dev", [&]() -> int {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    selinv_diag_enqueue(h->N, h->sl, h->S.n, d_out, h->stream);
    return stream_sync(h, "inverse diagonal export");
  });
}

int okkt_get_inverse_diag(okkt_handle h, double* d_out) {
  if (!h || !d_out) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_inverse_diag", [&]() -> int {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t n = h->S.n;
    if (n == 0) return OKKT_OK;
    if ((rc = stage_reserve(h, n)) != OKKT_OK) return rc;
    selinv_diag_enqueue(h->N, h->sl, n, h->d_rhs_stage, h->stream);
    if ((rc = stream_sync(h, "inverse diagonal export")) != OKKT_OK) return rc;
    return stage_download(h, d_out, h->d_rhs_stage, n, "inverse diagonal download failed");
  });
}

int okkt_get_inverse_on_pattern_dev(okkt_handle h, double* d_zval) {
  if (!h || (!d_zval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_inverse_on_pattern_dev", [&]() -> int {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    selinv_pattern_enqueue(h->sl, h->S.nnz_in, d_zval, h->stream);
    return stream_sync(h, "inverse export on the input pattern");
  });
}

int okkt_get_inverse_on_pattern(okkt_handle h, double* zval, int64_t* nnz_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  if (nnz_out) *nnz_out = h->S.nnz_in;
  if (!zval) return nnz_out ? OKKT_OK : OKKT_ERR_INVALID;
  return fence(h, "okkt_get_inverse_on_pattern", [&]() -> int {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t nnz = h->S.nnz_in;
    if (nnz == 0) return OKKT_OK;
    DevTemp t;
    if (!t.alloc(nnz)) return solver_set_error(h, OKKT_ERR_ALLOC, "inverse export staging allocation failed");
    selinv_pattern_enqueue(h->sl, nnz, t.p, h->stream);
    if ((rc = stream_sync(h, "inverse export on the input pattern")) != OKKT_OK) return rc;
    return stage_download(h, zval, t.p, nnz, "inverse export download failed");
  });
}

int okkt_get_inverse_csc(okkt_handle h, int64_t* colptr_out, int64_t* rowval_out, double* val_out, int64_t* nnz_out) {
  if (!h) return OKKT_ERR_INVALID;
  if (!h->analyzed) return solver_set_error(h, OKKT_ERR_INVALID, "not analysed");
  const Symbolic& S = h->S;
  if (nnz_out) *nnz_out = S.nnzL_stored;
  if (!colptr_out || !rowval_out || !val_out) return OKKT_OK;
  return fence(h, "okkt_get_inverse_csc", [&]() -> int {
    int rc = selinv_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const SelinvWork& W = h->sl;
    std::vector<double> z((size_t)W.z_doubles);
    if ((rc = stream_sync(h, "inverse export")) != OKKT_OK) return rc;
    if ((rc = stage_download(h, z.data(), W.Z, W.z_doubles, "download of Z failed")) != OKKT_OK) return rc;
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
  }, true);
}

int okkt_logdet(okkt_handle h, double* logabsdet, int32_t* sign) {
  if (!h || !logabsdet || !sign) return OKKT_ERR_INVALID;
  return fence(h, "okkt_logdet", [&]() -> int {
    int rc = selinv_ready(h, false);
    if (rc != OKKT_OK) return rc;
    const int64_t n = h->S.n;
    std::vector<double> d((size_t)n);
    if ((rc = stream_sync(h, "logdet")) != OKKT_OK) return rc;
    if ((rc = stage_download(h, d.data(), h->N.d.dvals, n, "download of D failed")) != OKKT_OK) return rc;
    LogDet L;
    for (int64_t i = 0; i < n; ++i) L.take(d[(size_t)i]);
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
        if ((rc = stage_download(h, sv.data(), h->sc.s_cur, n, "download of the scaling failed")) != OKKT_OK) return rc;
        for (int64_t i = 0; i < n; ++i) {
          int ex = 0;
          if (std::frexp(sv[(size_t)i], &ex) == 0.5) esum += ex - 1;
          else lsum += std::log(sv[(size_t)i]);
        }
      }
      L.acc -= 2.0 * 0.69314718055994530942 * (double)esum + 2.0 * lsum;
    }
    *logabsdet = L.acc;
    *sign = L.sg;
    return OKKT_OK;
  });
}

int okkt_schur_logdet(okkt_handle h, double* logabsdet, int32_t* sign) {
  if (!h || !logabsdet || !sign) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_logdet", [&]() -> int {
    int rc = schur_route_ready(h);
    if (rc != OKKT_OK) return rc;
    const int64_t ns = h->S.nschur, n1 = h->S.n - ns;
    std::vector<double> d((size_t)n1), dg((size_t)ns), sub((size_t)ns, 0.0);
    std::vector<int> ptype((size_t)ns);
    if ((rc = stream_sync(h, "logdet")) != OKKT_OK) return rc;
    const size_t pitch = (size_t)(ns + 1) * sizeof(double);      // down the diagonal of the dense factor, and the entries below it
    if ((n1 > 0 && hipMemcpy(d.data(), h->N.d.dvals, (size_t)n1 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy2D(dg.data(), sizeof(double), h->dl.F, pitch, sizeof(double), (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess ||
        (ns > 1 && hipMemcpy2D(sub.data(), sizeof(double), h->dl.F + 1, pitch, sizeof(double), (size_t)(ns - 1), hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy(ptype.data(), h->dl.ptype, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "download of D failed");
    LogDet L;
    for (int64_t i = 0; i < n1; ++i) L.take(d[(size_t)i]);
    for (int64_t k = 0; k < ns; ++k) {
      if (ptype[(size_t)k] == 0) { L.take(dg[(size_t)k]); continue; }
      // a 2 x 2 block [a b; b c]: det = b^2 ((a / |b|)(c / |b|) - 1), the scaled form of the solves
      const double b = sub[(size_t)k], t = std::fabs(b);
      L.take(t);
      L.take(t);
      L.take((dg[(size_t)k] / t) * (dg[(size_t)k + 1] / t) - 1.0);
      ++k;
    }
    *logabsdet = L.acc;
    *sign = L.sg;
    return OKKT_OK;
  });
}

int okkt_pivot_report(okkt_handle h, double u, okkt_pivot_info* info) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_pivot_report", [&]() -> int {
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
    if ((rc = hip_check(h, hipGetLastError(), "pivot report failed")) != OKKT_OK) return rc;
    if ((rc = stream_read(h, part, W.count, sizeof(part), "pivot report failed")) != OKKT_OK) return rc;
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
  }, true);
}

int okkt_get_multipliers(okkt_handle h, double* g_out, int64_t* partner_out) {
  if (!h || !g_out) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_multipliers", [&]() -> int {
    int rc = pivots_ready(h, true);
    return rc != OKKT_OK ? rc : pivots_copy_out(h, g_out, partner_out, hipMemcpyDeviceToHost);
  });
}

int okkt_get_multipliers_dev(okkt_handle h, double* d_g_out, int64_t* d_partner_out) {
  if (!h || !d_g_out) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_multipliers_dev", [&]() -> int {
    int rc = pivots_ready(h, true);
    return rc != OKKT_OK ? rc : pivots_copy_out(h, d_g_out, d_partner_out, hipMemcpyDeviceToDevice);
  });
}

int64_t okkt_get_rejected_pivots(okkt_handle h, int64_t* idx_out, int64_t* partner_out, int64_t cap) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_rejected_pivots", [&]() -> int64_t {
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
  }, true);
}

}  // extern "C"
