// C ABI, linear-solver level: Schur mode, the dense factor of the Schur complement (dense_ldlt.hip, section 8.7)
// and the solves and the inverse through it (sections 8.9, 8.10).  The refinement, the estimates and the selected inversion through the
// Schur route are beside their plain twins (api_refine.cpp, api_condest.cpp, api_selinv.cpp).
#include <algorithm>

#include "api_internal.h"

using namespace okkt;

namespace okkt {

int schur_ready(okkt_solver_s* h, bool need_factor) {
  if (!schur_mode(h)) return solver_set_error(h, OKKT_ERR_INVALID, "the handle is not in Schur mode (okkt_set_schur before okkt_analyze)");
  int rc = solver_ensure_numeric(h);
  if (rc != OKKT_OK) return rc;
  if (h->S.nschur != (int64_t)h->schur_idx.size() || h->N.schur_sn < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_analyze has not been called since okkt_set_schur");
  if (need_factor && !h->factored) return solver_set_error(h, OKKT_ERR_INVALID, "no complete okkt_factor_schur");
  return OKKT_OK;
}

int schur_dense_ready(okkt_solver_s* h) {
  if (!h->dl.valid) return solver_set_error(h, OKKT_ERR_INVALID, "no okkt_schur_factor has succeeded on this handle");
  if (h->dl.own && h->dl.factor_seq != h->factor_seq)
    return solver_set_error(h, OKKT_ERR_INVALID, "S has been assembled again since okkt_schur_factor: call okkt_schur_factor again");
  return OKKT_OK;
}

// (the row map does not depend on the mode: pat_colptr / pat_rowval hold the whole pattern as okkt_analyze was given it)
int schur_refine_ready(okkt_solver_s* h) {
  int rc = schur_ready(h, true);
  if (rc == OKKT_OK) rc = schur_dense_ready(h);
  if (rc != OKKT_OK) return rc;
  if (!h->dl.own)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_solve_refine: the dense factor is of a caller's S, so the factored matrix is not this handle's A (okkt_schur_factor with S = NULL first)");
  if (h->S.nparts > 1) return refuse_partitioned(h);
  return ensure_row_map(h, "refinement map");
}

int schur_route_ready(okkt_solver_s* h) {
  int rc = ensure_device(h);
  return rc != OKKT_OK ? rc : schur_refine_ready(h);
}

int schur_dense_sweeps(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs, bool whole, bool sync) {
  const int64_t n = h->S.n, ns = h->S.nschur;
  double* t2 = h->dl.X + 8 * ns;      // r2 / x2 of the fused solve
  int rc = for_rhs_batches(h, nrhs, [&](int64_t r, int nr, int R) {
    if (!whole) return dense_ldlt_solve_enqueue(h->dl, d_rhs + r * ns, d_sol + r * ns, nr, R, h->stream);
    solve_permute_in(h->N, d_rhs + r * n, n, nr, R);
    std::string e = solve_fwd_enqueue(h->N, 0, R);
    if (e.empty()) e = schur_gather_enqueue(h->N, t2, nr, R);
    if (e.empty()) e = dense_ldlt_solve_enqueue(h->dl, t2, t2, nr, R, h->stream);
    if (e.empty()) e = schur_put_enqueue(h->N, t2, nr, R);
    if (e.empty()) e = solve_bwd_enqueue(h->N, 0, R);
    if (e.empty()) solve_permute_out(h->N, d_sol + r * n, n, nr, R, false);
    return e;
  });
  if (rc != OKKT_OK || !sync) return rc;      // (not sync: the refinement loop of okkt_schur_solve_refine, whose own read of omega synchronises)
  return stream_sync(h, whole ? "Schur solve" : "dense Schur solve");
}

}  // namespace okkt

// batches of right-hand sides, as solver_solve_enqueue; d_x2 == nullptr: condense into d_r2, else expand into d_x
static int schur_sweeps(okkt_solver_s* h, const double* d_rhs, double* d_r2, const double* d_x2, double* d_x, int64_t nrhs) {
  const int64_t n = h->S.n, ns = h->S.nschur;
  int rc = for_rhs_batches(h, nrhs, [&](int64_t r, int nr, int R) {
    solve_permute_in(h->N, d_rhs + r * n, n, nr, R);
    std::string e = d_x2 ? schur_expand_enqueue(h->N, d_x2 + r * ns, nr, R) : schur_condense_enqueue(h->N, d_r2 + r * ns, nr, R);
    if (e.empty() && d_x2) solve_permute_out(h->N, d_x + r * n, n, nr, R, false);
    return e;
  });
  return rc != OKKT_OK ? rc : stream_sync(h, d_x2 ? "Schur expand" : "Schur condense");
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

// okkt_schur_dense_solve (x2 = S^-1 r2) and okkt_schur_solve (whole: the fused whole-system solve), host or device pointers
static int schur_solve_entry(okkt_handle h, const char* name, const double* rhs, double* sol, int64_t nrhs, bool whole, bool on_device) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, name, [&]() -> int {
    if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
    if (nrhs > 0 && (!rhs || !sol)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
    int rc = schur_ready(h, whole);
    if (rc == OKKT_OK) rc = schur_dense_ready(h);
    if (rc != OKKT_OK) return rc;
    if (on_device) return schur_dense_sweeps(h, rhs, sol, nrhs, whole);
    const int64_t len = (whole ? h->S.n : h->S.nschur) * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc = stage_reserve(h, len)) != OKKT_OK) return rc;
    if ((rc = stage_upload(h, h->d_rhs_stage, rhs, len, "rhs upload failed")) != OKKT_OK) return rc;
    if ((rc = schur_dense_sweeps(h, h->d_rhs_stage, h->d_rhs_stage, nrhs, whole)) != OKKT_OK) return rc;
    return stage_download(h, sol, h->d_rhs_stage, len, "solution download failed");
  });
}

// S^-1 into Z, host or device memory with leading dimension ld
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
  if ((rc = stream_read(h, &nf, h->dl.nonfinite, sizeof(nf), "dense Schur inverse failed")) != OKKT_OK) return rc;
  h->dl.inv_nonfinite = (long long)nf;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_solve_ms = ms;
  if (!on_device && hipMemcpy2D(Z, (size_t)ld * sizeof(double), t.p, (size_t)ns * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess)
    return solver_set_error(h, OKKT_ERR_HIP, "inverse download failed");
  return OKKT_OK;
}

extern "C" {

int okkt_set_schur(okkt_handle h, int64_t ns, const int64_t* idx) {
  if (!h) return OKKT_ERR_INVALID;
  if (ns < 0) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: ns < 0");
  if (ns > 0 && !idx) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_set_schur: null idx");
  return fence(h, "okkt_set_schur", [&]() -> int {
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
  }, true);
}

int okkt_factor_schur_dev(okkt_handle h, const double* d_nzval, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* out) {
  if (!h || (!d_nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  return fence(h, "okkt_factor_schur_dev", [&]() -> int {
    int rc = schur_ready(h, false);
    return rc != OKKT_OK ? rc : solver_factor_device(h, d_nzval, n1, m1, sym_kind, out);
  });
}

int okkt_factor_schur(okkt_handle h, const double* nzval, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* out) {
  if (!h || (!nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  return fence(h, "okkt_factor_schur", [&]() -> int {
    int rc = schur_ready(h, false);
    if (rc == OKKT_OK) rc = stage_upload(h, h->N.vals_owned, nzval, h->S.nnz_in, "nzval upload");
    return rc != OKKT_OK ? rc : solver_factor_device(h, h->N.vals_owned, n1, m1, sym_kind, out);
  });
}

int okkt_get_schur_dev(okkt_handle h, double* d_S, int64_t ld) {
  if (!h || !d_S) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_schur_dev", [&]() -> int {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    if (ld < h->S.nschur) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_schur: ld < ns");
    schur_export_enqueue(h->N, d_S, ld);
    return stream_sync(h, "Schur complement export");
  });
}

int okkt_get_schur(okkt_handle h, double* S, int64_t ld) {
  if (!h || !S) return OKKT_ERR_INVALID;
  return fence(h, "okkt_get_schur", [&]() -> int {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t ns = h->S.nschur;
    if (ld < ns) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_get_schur: ld < ns");
    DevTemp t;
    if (!t.alloc(ns * ns)) return solver_set_error(h, OKKT_ERR_ALLOC, "Schur complement staging allocation failed");
    schur_export_enqueue(h->N, t.p, ns);
    if ((rc = stream_sync(h, "Schur complement export")) != OKKT_OK) return rc;
    if (hipMemcpy2D(S, (size_t)ld * sizeof(double), t.p, (size_t)ns * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "Schur complement download failed");
    return OKKT_OK;
  });
}

int okkt_schur_condense_dev(okkt_handle h, const double* d_rhs, double* d_r2, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!d_rhs || !d_r2)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "okkt_schur_condense_dev", [&]() -> int {
    int rc = schur_ready(h, true);
    return rc != OKKT_OK ? rc : schur_sweeps(h, d_rhs, d_r2, nullptr, nullptr, nrhs);
  });
}

int okkt_schur_condense(okkt_handle h, const double* rhs, double* r2, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!rhs || !r2)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "okkt_schur_condense", [&]() -> int {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs, len2 = h->S.nschur * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc = stage_reserve(h, len)) != OKKT_OK) return rc;
    DevTemp t;
    if (!t.alloc(len2)) return solver_set_error(h, OKKT_ERR_ALLOC, "Schur condense staging allocation failed");
    if ((rc = stage_upload(h, h->d_rhs_stage, rhs, len, "rhs upload failed")) != OKKT_OK) return rc;
    if ((rc = schur_sweeps(h, h->d_rhs_stage, t.p, nullptr, nullptr, nrhs)) != OKKT_OK) return rc;
    return stage_download(h, r2, t.p, len2, "r2 download failed");
  });
}

int okkt_schur_expand_dev(okkt_handle h, const double* d_rhs, const double* d_x2, double* d_x, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!d_rhs || !d_x2 || !d_x)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "okkt_schur_expand_dev", [&]() -> int {
    int rc = schur_ready(h, true);
    return rc != OKKT_OK ? rc : schur_sweeps(h, d_rhs, nullptr, d_x2, d_x, nrhs);
  });
}

int okkt_schur_expand(okkt_handle h, const double* rhs, const double* x2, double* x, int64_t nrhs) {
  if (!h) return OKKT_ERR_INVALID;
  if (nrhs < 0) return solver_set_error(h, OKKT_ERR_INVALID, "nrhs < 0");
  if (nrhs > 0 && (!rhs || !x2 || !x)) return solver_set_error(h, OKKT_ERR_INVALID, "null pointer");
  return fence(h, "okkt_schur_expand", [&]() -> int {
    int rc = schur_ready(h, true);
    if (rc != OKKT_OK) return rc;
    const int64_t len = h->S.n * nrhs, len2 = h->S.nschur * nrhs;
    if (len == 0) return OKKT_OK;
    if ((rc = stage_reserve(h, len)) != OKKT_OK) return rc;
    DevTemp t;
    if (!t.alloc(len2)) return solver_set_error(h, OKKT_ERR_ALLOC, "Schur expand staging allocation failed");
    if ((rc = stage_upload(h, h->d_rhs_stage, rhs, len, "Schur expand upload failed")) != OKKT_OK) return rc;
    if ((rc = stage_upload(h, t.p, x2, len2, "Schur expand upload failed")) != OKKT_OK) return rc;
    if ((rc = schur_sweeps(h, h->d_rhs_stage, nullptr, t.p, h->d_rhs_stage, nrhs)) != OKKT_OK) return rc;
    return stage_download(h, x, h->d_rhs_stage, len, "x download failed");
  });
}

int okkt_schur_factor(okkt_handle h, const double* S, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_factor", [&] { return schur_factor_impl(h, S, ld, false, inertia_S, inertia_total); });
}

int okkt_schur_factor_dev(okkt_handle h, const double* d_S, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_factor_dev", [&] { return schur_factor_impl(h, d_S, ld, true, inertia_S, inertia_total); });
}

int okkt_schur_get_factor(okkt_handle h, double* LD, int64_t ld, int32_t* ipiv) {
  if (!h || !LD || !ipiv) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_get_factor", [&]() -> int {
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
  });
}

int okkt_schur_dense_solve(okkt_handle h, const double* rhs, double* sol, int64_t nrhs) {
  return schur_solve_entry(h, "okkt_schur_dense_solve", rhs, sol, nrhs, false, false);
}
int okkt_schur_dense_solve_dev(okkt_handle h, const double* rhs, double* sol, int64_t nrhs) {
  return schur_solve_entry(h, "okkt_schur_dense_solve_dev", rhs, sol, nrhs, false, true);
}
int okkt_schur_solve(okkt_handle h, const double* rhs, double* sol, int64_t nrhs) {
  return schur_solve_entry(h, "okkt_schur_solve", rhs, sol, nrhs, true, false);
}
int okkt_schur_solve_dev(okkt_handle h, const double* rhs, double* sol, int64_t nrhs) {
  return schur_solve_entry(h, "okkt_schur_solve_dev", rhs, sol, nrhs, true, true);
}

int okkt_schur_get_inverse(okkt_handle h, double* Z, int64_t ld) {
  if (!h || !Z) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_get_inverse", [&] { return schur_inverse_impl(h, Z, ld, false); });
}

int okkt_schur_get_inverse_dev(okkt_handle h, double* d_Z, int64_t ld) {
  if (!h || !d_Z) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_get_inverse_dev", [&] { return schur_inverse_impl(h, d_Z, ld, true); });
}

int64_t okkt_schur_inverse_nonfinite(okkt_handle h) {
  if (!h) return OKKT_ERR_INVALID;
  return (int64_t)h->dl.inv_nonfinite;
}

}  // extern "C"
