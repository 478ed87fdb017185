// C ABI of the scenario batches (include/okkt.h): B items in Schur mode on the analysed pattern of one handle,
// their Schur complements summed on the device, one dense factor of the sum.  The interior's launches are batch.hip's in level mode,
// the Schur front's and the sums' batch_schur.hip's, the dense factor dense_ldlt.hip's on a work area of the batch; this file is the
// checks, the staging of host-side arguments and the per-item flags.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "api_internal.h"

using namespace okkt;

namespace {

// the first reason that applies, in the order of the codes; shape filled when the plan is eligible
int sbatch_reason(okkt_solver_s* h, SchurBatchShape& shape, std::string* why) {
  shape = SchurBatchShape();
  if (!h->analyzed) { *why = "okkt_analyze has not been called (since the last okkt_set_schur)"; return OKKT_SBATCH_NOT_ANALYZED; }
  if (h->S.nparts > 1) { *why = "the handle is partitioned (okkt_dist_set_partition with nparts > 1)"; return OKKT_SBATCH_PARTITIONED; }
  if (!schur_mode(h) || h->S.nschur <= 0) { *why = "the handle is not in Schur mode (okkt_set_schur before okkt_analyze)"; return OKKT_SBATCH_NO_SET; }
  SchurBatchWork& W = h->sb;
  if (W.shape_analysis != h->n_analyze_calls || W.shape_small_max != small_max_of(h)) {
    schur_batch_shape(h->S, small_max_of(h), W.shape);
    W.shape_analysis = h->n_analyze_calls;
    W.shape_small_max = small_max_of(h);
  }
  shape = W.shape;
  if (shape.reason == OKKT_SBATCH_BIG_FRONTS)
    *why = "the interior has fronts of more than " + std::to_string(small_max_of(h)) + " rows (the largest has " + std::to_string(shape.max_front) +
           "): a scenario batch takes interiors of small fronts only";
  if (shape.reason == OKKT_SBATCH_SET_TOO_LARGE)
    *why = "the Schur set has " + std::to_string(shape.ns) + " variables: a scenario batch assembles sets of at most " + std::to_string(kSchurBatchMaxSet);
  return shape.reason;
}

int sbatch_ready(okkt_solver_s* h, const char* what, int64_t B) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  SchurBatchWork& W = h->sb;
  if (!W.w.s.arena) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": no slots are reserved (okkt_schur_batch_reserve)");
  // the slots and the place of the Schur front in them were laid out for the device plan of the reservation: a changed or cleared set
  // (the handle is then not analysed), a partition, a plan rebuilt on another footing make the reservation stale
  if (!h->analyzed || !h->numeric_ready || h->S.nparts > 1 || !schur_mode(h) || h->S.nschur != W.ns || h->N.schur_sn != W.schur_sn || h->N.n_big != 0 ||
      h->N.arena_doubles != W.w.plan_arena_doubles || (int)h->N.levels.size() != W.w.plan_levels || h->N.n_tasks != W.w.plan_tasks || !h->N.levels_top.empty() ||
      h->N.front_pos_host[(size_t)h->N.schur_sn] != W.front_pos || h->N.schur_gcb != W.gcb) {
    (void)hipStreamSynchronize(h->stream);
    schur_batch_free(W);
    return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": the plan has changed since okkt_schur_batch_reserve (another Schur set, a partition, a new analysis): "
                                                 "the slots are released");
  }
  if (h->sc.mode != OKKT_SCALE_NONE) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": a scaling is set (okkt_set_scaling with OKKT_SCALE_NONE first)");
  if (B < 1 || B > W.w.B) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": B must be in 1 .. the reserved " + std::to_string(W.w.B));
  return OKKT_OK;
}

int factor_device(okkt_solver_s* h, int64_t B, const double* d_vals, int64_t val_stride, const double* shift, int64_t nshift, int64_t n1, int64_t m1, int sym_kind,
                  okkt_inertia* inertia_out, int32_t* flag_out) {
  const char* what = "okkt_factor_schur_batch";
  int rc = sbatch_ready(h, what, B);
  if (rc != OKKT_OK) return rc;
  SchurBatchWork& W = h->sb;
  const int64_t order = h->S.n - h->S.nschur;
  if (val_stride != 0 && val_stride < h->S.nnz_in) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": val_stride must be 0 or at least the number of entries");
  if (n1 < 0 || m1 < 0 || n1 + m1 != order) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": n1 + m1 does not match dim - ns");
  if (sym_kind != OKKT_SYM_DEFINITE && sym_kind != OKKT_SYM_SYMMETRIC) return solver_set_error(h, OKKT_ERR_INVALID, "unknown sym_kind");
  if (sym_kind == OKKT_SYM_DEFINITE && m1 != 0) return solver_set_error(h, OKKT_ERR_INVALID, ":definite requires m == 0 (julia.jl:30)");
  if (nshift < 0 || nshift > h->S.n) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": nshift outside 0 .. dim");
  const double tol = sym_kind == OKKT_SYM_DEFINITE ? 0.0 : h->opts.inertia_tol;
  W.w.factored_B = 0;
  W.dense_ok = false;
  if (shift && (rc = stage_upload(h, W.w.shift, shift, B, "okkt_factor_schur_batch: shift upload")) != OKKT_OK) return rc;
  (void)hipEventRecord(h->ev0, h->stream);
  std::string e = batch_factor_enqueue(h->N, W.w, OKKT_BATCH_LEVEL, B, d_vals, val_stride, shift != nullptr, nshift, tol);
  if (e.empty()) e = schur_batch_assemble_enqueue(h->N, W, B, d_vals, val_stride);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
  (void)hipEventRecord(h->ev1, h->stream);
  W.w.raw.resize((size_t)B * kCountStride);
  if ((rc = stream_read(h, W.w.raw.data(), W.w.s.counters, W.w.raw.size() * sizeof(unsigned long long), "okkt_factor_schur_batch failed")) != OKKT_OK) return rc;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_factor_ms = ms;
  W.w.mode_used = OKKT_BATCH_LEVEL;
  W.w.inertia.assign((size_t)B * 4, 0);
  W.w.flags.assign((size_t)B, 0);
  if ((rc = batch_counts_to_flags(h, W.w, what, "dim - ns", B, nullptr, order, n1, m1, sym_kind, inertia_out, flag_out)) != OKKT_OK) return rc;
  W.w.factored_B = B;
  return OKKT_OK;
}

// b in -1 .. factored_B - 1 into S (host or device memory)
int get_impl(okkt_solver_s* h, int64_t b, double* S, int64_t ld, bool on_device) {
  int rc = sbatch_ready(h, "okkt_schur_batch_get", 1);
  if (rc != OKKT_OK) return rc;
  SchurBatchWork& W = h->sb;
  const int64_t ns = W.ns;
  if (W.w.factored_B < 1) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_get: no factored batch (okkt_factor_schur_batch)");
  if (b < -1 || b >= W.w.factored_B) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_get: b outside -1 .. the items of the last okkt_factor_schur_batch");
  if (ld < ns) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_get: ld < ns");
  // through W.sum: full and symmetric with leading dimension ns, then one strided copy
  std::string e = b < 0 ? schur_batch_sum_enqueue(h->N, W, W.w.factored_B, nullptr, 0, W.sum) : schur_batch_export_enqueue(h->N, W, b, W.sum, ns);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
  if (hipMemcpy2DAsync(S, (size_t)ld * sizeof(double), W.sum, (size_t)ns * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns,
                       on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream) != hipSuccess)
    return solver_set_error(h, OKKT_ERR_HIP, "okkt_schur_batch_get: the copy of S failed");
  return stream_sync(h, "okkt_schur_batch_get");
}

int dense_factor_impl(okkt_solver_s* h, const double* S_add, int64_t ld, bool on_device, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  int rc = sbatch_ready(h, "okkt_schur_batch_factor", 1);
  if (rc != OKKT_OK) return rc;
  SchurBatchWork& W = h->sb;
  const int64_t ns = W.ns, B = W.w.factored_B;
  if (B < 1) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_factor: no factored batch (okkt_factor_schur_batch)");
  if (S_add && ld < ns) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_factor: ld < ns");
  W.dense_ok = false;
  DevTemp t;
  const double* d_add = S_add;
  int64_t d_ld = ld;
  if (S_add && !on_device) {
    if (!t.alloc(ns * ns)) return solver_set_error(h, OKKT_ERR_ALLOC, "okkt_schur_batch_factor: the device copy of S_add does not fit");
    if (hipMemcpy2DAsync(t.p, (size_t)ns * sizeof(double), S_add, (size_t)ld * sizeof(double), (size_t)ns * sizeof(double), (size_t)ns, hipMemcpyHostToDevice, h->stream) != hipSuccess)
      return solver_set_error(h, OKKT_ERR_HIP, "okkt_schur_batch_factor: the upload of S_add failed");
    d_add = t.p;
    d_ld = ns;
  }
  std::string e = schur_batch_sum_enqueue(h->N, W, B, d_add, d_ld, W.dl.F);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
  if (!(e = dense_ldlt_factor(W.dl, h->stream)).empty()) {      // (synchronises: the copy of S_add is free behind it)
    (void)hipStreamSynchronize(h->stream);
    return solver_set_error(h, OKKT_ERR_HIP, "okkt_schur_batch_factor: dense factorisation failed: " + e);
  }
  okkt_inertia in;
  in.pos = W.dl.cnt[0]; in.neg = W.dl.cnt[1]; in.zero = W.dl.cnt[2]; in.nonfinite = W.dl.cnt[3];
  if (in.pos + in.neg + in.zero + in.nonfinite != ns) return solver_set_error(h, OKKT_ERR_INTERNAL, "okkt_schur_batch_factor: the pivot counts of the dense factor do not add up to ns");
  if (inertia_S) *inertia_S = in;
  if (inertia_total) {
    okkt_inertia tt = in;
    for (int64_t b = 0; b < B; ++b) {
      const int64_t* a = W.w.inertia.data() + (size_t)b * 4;
      tt.pos += a[0]; tt.neg += a[1]; tt.zero += a[2]; tt.nonfinite += a[3];
    }
    *inertia_total = tt;
  }
  W.dense_ok = true;
  return (in.zero == 0 && in.nonfinite == 0) ? 1 : 0;
}

enum Sweep { kCondense, kExpand, kSolve };

// all pointers on the device.  condense: a = r2_sum, c = r2_items or NULL; expand: a = x2; solve: a = rhs0 or NULL
int sweeps_device(okkt_solver_s* h, const char* what, Sweep kind, int64_t B, const double* d_rhs, const double* d_in, double* d_r2_sum, double* d_r2_items, double* d_sol,
                  int64_t nrhs) {
  int rc = sbatch_ready(h, what, B);
  if (rc != OKKT_OK) return rc;
  SchurBatchWork& W = h->sb;
  const int64_t ns = W.ns;
  if (B > W.w.factored_B) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": no factored batch of at least B items (okkt_factor_schur_batch)");
  if (kind == kSolve && !W.dense_ok) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": no okkt_schur_batch_factor since the last okkt_factor_schur_batch");
  if (kind == kSolve && B != W.w.factored_B) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": B is not that of the last okkt_factor_schur_batch, whose sum the dense factor is of");
  if (nrhs < 0 || nrhs > W.w.nrhs_max) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": nrhs outside 0 .. the reserved nrhs_max");
  (void)hipEventRecord(h->ev0, h->stream);
  rc = for_rhs_batches(h, nrhs, [&](int64_t r, int nr, int R) {
    std::string e = batch_permute_in_enqueue(h->N, W.w, B, d_rhs, nrhs, r, nr, R);
    if (e.empty()) e = batch_fwd_enqueue(h->N, W.w, B, R);
    if (kind == kCondense) {
      if (e.empty()) e = schur_batch_gather_enqueue(h->N, W, B, d_r2_items, nrhs, r, nr, R);
      if (e.empty()) e = schur_batch_r2sum_enqueue(h->N, W, B, nullptr, d_r2_sum + r * ns, nr, R);
      return e;
    }
    if (kind == kSolve) {
      if (e.empty()) e = schur_batch_gather_enqueue(h->N, W, B, nullptr, nrhs, r, nr, R);
      if (e.empty()) e = schur_batch_r2sum_enqueue(h->N, W, B, d_in ? d_in + r * ns : nullptr, W.r2, nr, R);
      if (e.empty()) e = dense_ldlt_solve_enqueue(W.dl, W.r2, W.r2, nr, R, h->stream);
      if (e.empty()) e = schur_batch_put_enqueue(h->N, W, B, W.r2, nr, R);
    } else {
      if (e.empty()) e = schur_batch_put_enqueue(h->N, W, B, d_in + r * ns, nr, R);
    }
    if (e.empty()) e = batch_bwd_enqueue(h->N, W.w, B, R);
    if (e.empty()) e = batch_permute_out_enqueue(h->N, W.w, B, d_sol, nrhs, r, nr, R);
    return e;
  });
  if (rc != OKKT_OK) return rc;
  (void)hipEventRecord(h->ev1, h->stream);
  if ((rc = stream_sync(h, what)) != OKKT_OK) return rc;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_solve_ms = ms;
  return OKKT_OK;
}

// host pointers: the device copies for the length of the call
int sweeps_host(okkt_solver_s* h, const char* what, Sweep kind, int64_t B, const double* rhs, const double* in, double* r2_sum, double* r2_items, double* sol, int64_t nrhs) {
  int rc = sbatch_ready(h, what, B);
  if (rc != OKKT_OK) return rc;
  const int64_t ns = h->sb.ns;
  if (nrhs < 0 || nrhs > h->sb.w.nrhs_max) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": nrhs outside 0 .. the reserved nrhs_max");
  const int64_t len = B * nrhs * h->S.n, len2 = nrhs * ns, leni = B * nrhs * ns;
  DevTemp x, a, items;
  if (!x.alloc(std::max<int64_t>(len, 1)) || !a.alloc(std::max<int64_t>(len2, 1)) || (r2_items && !items.alloc(std::max<int64_t>(leni, 1))))
    return solver_set_error(h, OKKT_ERR_ALLOC, std::string(what) + ": the device copy of the right-hand sides does not fit");
  if ((rc = stage_upload(h, x.p, rhs, len, "okkt_schur_batch: rhs upload")) != OKKT_OK) return rc;
  if (in && (rc = stage_upload(h, a.p, in, len2, "okkt_schur_batch: x2 / rhs0 upload")) != OKKT_OK) return rc;
  rc = sweeps_device(h, what, kind, B, x.p, in ? a.p : nullptr, a.p, r2_items ? items.p : nullptr, x.p, nrhs);
  (void)hipStreamSynchronize(h->stream);      // the copies are freed behind everything that reads them
  if (rc != OKKT_OK) return rc;
  if (kind != kCondense) return stage_download(h, sol, x.p, len, "okkt_schur_batch: sol download");
  if ((rc = stage_download(h, r2_sum, a.p, len2, "okkt_schur_batch: r2 download")) != OKKT_OK) return rc;
  return r2_items ? stage_download(h, r2_items, items.p, leni, "okkt_schur_batch: r2 download") : OKKT_OK;
}

}  // namespace

extern "C" {

int okkt_schur_batch_query(okkt_handle h, int64_t nrhs_max, okkt_schur_batch_info* out) {
  if (!h || !out) return OKKT_ERR_INVALID;
  std::memset(out, 0, sizeof(*out));
  if (nrhs_max < 1) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_query: nrhs_max < 1");
  return fence(h, "okkt_schur_batch_query", [&]() -> int {
    SchurBatchShape shape;
    std::string why;
    out->reason = sbatch_reason(h, shape, &why);
    out->eligible = out->reason == OKKT_SBATCH_OK ? 1 : 0;
    if (!h->analyzed) return OKKT_OK;
    out->ns = h->S.nschur;
    out->max_front = shape.max_front;
    if (!out->eligible) return OKKT_OK;
    const int R = batch_work_columns(nrhs_max);
    const int64_t arena = h->numeric_ready && h->N.arena_doubles > 0 ? h->N.arena_doubles : h->S.arena_doubles;
    out->bytes_per_item = (batch_slot_doubles(h->S, arena, R) + schur_batch_item_doubles(shape.ns, 4)) * 8;
    out->bytes_shared = schur_batch_shared_doubles(shape.ns) * 8;
    out->tasks_per_item = shape.tasks;
    out->levels = shape.levels;
    out->launches_factor = shape.levels + 2;        // the shifts and counters, one launch per level, the Schur fronts
    out->launches_solve = 2 * shape.levels + 6;     // gather, upwards, the items' r2, two stages of their sum, the put, downwards, scatter
    return OKKT_OK;
  }, true);
}

int okkt_schur_batch_reserve(okkt_handle h, int64_t B, int64_t nrhs_max) {
  if (!h) return OKKT_ERR_INVALID;
  if (B < 1 || B > 65535) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_reserve: B outside 1 .. 65535");
  if (nrhs_max < 1) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_reserve: nrhs_max < 1");
  return fence(h, "okkt_schur_batch_reserve", [&]() -> int {
    int rc = ensure_device(h);
    if (rc != OKKT_OK) return rc;
    SchurBatchShape shape;
    std::string why;
    if (sbatch_reason(h, shape, &why) != OKKT_SBATCH_OK) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_reserve: " + why);
    if (h->sc.mode != OKKT_SCALE_NONE) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_reserve: a scaling is set (okkt_set_scaling with OKKT_SCALE_NONE first)");
    if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
    if ((int)h->N.levels.size() != shape.levels || h->N.n_tasks != shape.tasks || h->N.n_big != 0 || h->N.schur_sn < 0 || !h->N.levels_top.empty())
      return solver_set_error(h, OKKT_ERR_INTERNAL, "okkt_schur_batch_reserve: the device schedule is not the one the batch grids were counted from");
    (void)hipStreamSynchronize(h->stream);
    bool oom = false;
    std::string e = schur_batch_alloc(h->sb, h->S, h->N, B, nrhs_max, &oom);
    if (!e.empty()) return solver_set_error(h, oom ? OKKT_ERR_ALLOC : OKKT_ERR_HIP, e);
    h->sb.w.plan_arena_doubles = h->N.arena_doubles;
    h->sb.w.plan_levels = (int)h->N.levels.size();
    h->sb.w.plan_tasks = h->N.n_tasks;
    return OKKT_OK;
  }, true);
}

int okkt_schur_batch_release(okkt_handle h) {
  if (!h) return OKKT_ERR_INVALID;
  if (h->sb.w.s.arena) {
    int rc = ensure_device(h);
    if (rc != OKKT_OK) return rc;
    (void)hipStreamSynchronize(h->stream);
  }
  schur_batch_free(h->sb);
  return OKKT_OK;
}

int okkt_factor_schur_batch_dev(okkt_handle h, int64_t B, const double* d_nzval, int64_t val_stride, const double* shift, int64_t nshift, int64_t n1, int64_t m1, int sym_kind,
                                okkt_inertia* inertia_items, int32_t* flag_items) {
  if (!h || (!d_nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  return fence(h, "okkt_factor_schur_batch_dev", [&] { return factor_device(h, B, d_nzval, val_stride, shift, nshift, n1, m1, sym_kind, inertia_items, flag_items); }, true);
}

int okkt_factor_schur_batch(okkt_handle h, int64_t B, const double* nzval, int64_t val_stride, const double* shift, int64_t nshift, int64_t n1, int64_t m1, int sym_kind,
                            okkt_inertia* inertia_items, int32_t* flag_items) {
  if (!h || (!nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  return fence(h, "okkt_factor_schur_batch", [&]() -> int {
    int rc = sbatch_ready(h, "okkt_factor_schur_batch", B);
    if (rc != OKKT_OK) return rc;
    return batch_factor_host_values(h, "okkt_factor_schur_batch", B, nzval, val_stride, [&](const double* d_vals, int64_t stride) {
      return factor_device(h, B, d_vals, stride, shift, nshift, n1, m1, sym_kind, inertia_items, flag_items);
    });
  }, true);
}

int okkt_schur_batch_get(okkt_handle h, int64_t b, double* S, int64_t ld) {
  if (!h || !S) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_get", [&] { return get_impl(h, b, S, ld, false); });
}
int okkt_schur_batch_get_dev(okkt_handle h, int64_t b, double* d_S, int64_t ld) {
  if (!h || !d_S) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_get_dev", [&] { return get_impl(h, b, d_S, ld, true); });
}

int okkt_schur_batch_factor(okkt_handle h, const double* S_add, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_factor", [&] { return dense_factor_impl(h, S_add, ld, false, inertia_S, inertia_total); });
}
int okkt_schur_batch_factor_dev(okkt_handle h, const double* d_S_add, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_factor_dev", [&] { return dense_factor_impl(h, d_S_add, ld, true, inertia_S, inertia_total); });
}

int okkt_schur_batch_condense(okkt_handle h, int64_t B, const double* rhs, double* r2_sum, double* r2_items, int64_t nrhs) {
  if (!h || !rhs || !r2_sum) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_condense", [&] { return sweeps_host(h, "okkt_schur_batch_condense", kCondense, B, rhs, nullptr, r2_sum, r2_items, nullptr, nrhs); });
}
int okkt_schur_batch_condense_dev(okkt_handle h, int64_t B, const double* d_rhs, double* d_r2_sum, double* d_r2_items, int64_t nrhs) {
  if (!h || !d_rhs || !d_r2_sum) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_condense_dev", [&] { return sweeps_device(h, "okkt_schur_batch_condense", kCondense, B, d_rhs, nullptr, d_r2_sum, d_r2_items, nullptr, nrhs); });
}

int okkt_schur_batch_expand(okkt_handle h, int64_t B, const double* rhs, const double* x2, double* sol, int64_t nrhs) {
  if (!h || !rhs || !x2 || !sol) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_expand", [&] { return sweeps_host(h, "okkt_schur_batch_expand", kExpand, B, rhs, x2, nullptr, nullptr, sol, nrhs); });
}
int okkt_schur_batch_expand_dev(okkt_handle h, int64_t B, const double* d_rhs, const double* d_x2, double* d_sol, int64_t nrhs) {
  if (!h || !d_rhs || !d_x2 || !d_sol) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_expand_dev", [&] { return sweeps_device(h, "okkt_schur_batch_expand", kExpand, B, d_rhs, d_x2, nullptr, nullptr, d_sol, nrhs); });
}

int okkt_schur_batch_solve(okkt_handle h, int64_t B, const double* rhs, const double* rhs0, double* sol, int64_t nrhs) {
  if (!h || !rhs || !sol) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_solve", [&] { return sweeps_host(h, "okkt_schur_batch_solve", kSolve, B, rhs, rhs0, nullptr, nullptr, sol, nrhs); });
}
int okkt_schur_batch_solve_dev(okkt_handle h, int64_t B, const double* d_rhs, const double* d_rhs0, double* d_sol, int64_t nrhs) {
  if (!h || !d_rhs || !d_sol) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_solve_dev", [&] { return sweeps_device(h, "okkt_schur_batch_solve", kSolve, B, d_rhs, d_rhs0, nullptr, nullptr, d_sol, nrhs); });
}

int okkt_schur_batch_select(okkt_handle h, int64_t b) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_schur_batch_select", [&]() -> int {
    int rc = sbatch_ready(h, "okkt_schur_batch_select", 1);
    if (rc != OKKT_OK) return rc;
    SchurBatchWork& W = h->sb;
    if (b < 0 || b >= W.w.factored_B) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_schur_batch_select: b outside the items of the last okkt_factor_schur_batch");
    return batch_select_slot(h, W.w, "okkt_schur_batch_select", b);
  });
}

}  // extern "C"
