// C ABI of the uniform batches (include/okkt.h): B systems on the analysed pattern of one handle.  The
// kernels and their launches are batch.hip's, the grids' description batch_host.cpp's; this file is the checks, the staging of
// host-side arguments, the per-item flags and the copy of a slot into the handle's own state.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "api_internal.h"

using namespace okkt;

namespace {

// the first reason that applies, in the order of the codes; shape filled when the plan is eligible
int batch_reason(okkt_solver_s* h, BatchShape& shape, std::string* why) {
  shape = BatchShape();
  if (!h->analyzed) { *why = "okkt_analyze has not been called"; return OKKT_BATCH_NOT_ANALYZED; }
  if (h->S.nparts > 1) { *why = "the handle is partitioned (okkt_dist_set_partition with nparts > 1)"; return OKKT_BATCH_PARTITIONED; }
  if (schur_mode(h) || h->S.nschur > 0) { *why = "the handle is in Schur mode (okkt_set_schur)"; return OKKT_BATCH_SCHUR; }
  if (h->sc.mode != OKKT_SCALE_NONE) { *why = "a scaling is set (okkt_set_scaling with OKKT_SCALE_NONE first)"; return OKKT_BATCH_SCALING; }
  BatchWork& W = h->bt;
  if (W.shape_analysis != h->n_analyze_calls || W.shape_small_max != small_max_of(h)) {      // fixed per analysis: the delta loop asks every time
    batch_shape(h->S, small_max_of(h), W.shape);
    W.shape_analysis = h->n_analyze_calls;
    W.shape_small_max = small_max_of(h);
  }
  shape = W.shape;
  if (shape.reason == OKKT_BATCH_BIG_FRONTS)
    *why = "the plan has fronts of more than " + std::to_string(small_max_of(h)) + " rows (the largest has " + std::to_string(h->S.max_front) +
           "): a batch takes plans of small fronts only";
  return shape.reason;
}

int batch_ready(okkt_solver_s* h, const char* what, int64_t B) {
  int rc = ensure_device(h);
  if (rc != OKKT_OK) return rc;
  if (!h->analyzed || !h->numeric_ready || !h->bt.s.arena) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": no slots are reserved (okkt_batch_reserve)");
  // The slots were laid out for the device plan of the reservation.  A plan rebuilt since on another footing -- okkt_dist_set_partition on
  // the analysed handle, then any call that sets the plan up again: dense f x f fronts at other offsets, this part's tasks only -- would
  // send an item's fronts into its neighbour's slot: the reservation is stale, it is released and the call refused
  BatchWork& W = h->bt;
  if (h->S.nparts > 1 || schur_mode(h) || h->S.nschur > 0 || h->N.n_big != 0 || h->N.arena_doubles != W.plan_arena_doubles ||
      (int)h->N.levels.size() != W.plan_levels || h->N.n_tasks != W.plan_tasks || !h->N.levels_top.empty()) {
    (void)hipStreamSynchronize(h->stream);
    batch_free(W);
    return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": the device plan has changed since okkt_batch_reserve (a partition or a Schur set on the handle): "
                                                 "the slots are released; a batch takes unpartitioned plans of small fronts only");
  }
  if (B < 1 || B > h->bt.B) return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + ": B must be in 1 .. the reserved " + std::to_string(h->bt.B));
  return OKKT_OK;
}

int solve_batch_device(okkt_solver_s* h, int64_t B, const double* d_rhs, double* d_sol, int64_t nrhs) {
  int rc = batch_ready(h, "okkt_solve_batch", B);
  if (rc != OKKT_OK) return rc;
  BatchWork& W = h->bt;
  if (B > W.factored_B) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_solve_batch: no factored batch of at least B items (okkt_factor_batch)");
  if (nrhs < 0 || nrhs > W.nrhs_max) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_solve_batch: nrhs outside 0 .. the reserved nrhs_max");
  (void)hipEventRecord(h->ev0, h->stream);
  rc = for_rhs_batches(h, nrhs, [&](int64_t r, int nr, int R) { return batch_solve_enqueue(h->N, W, W.mode_used, B, d_rhs, d_sol, nrhs, r, nr, R); });
  if (rc != OKKT_OK) return rc;
  (void)hipEventRecord(h->ev1, h->stream);
  if ((rc = stream_sync(h, "okkt_solve_batch")) != OKKT_OK) return rc;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_solve_ms = ms;
  return OKKT_OK;
}

}  // namespace

namespace okkt {

int batch_counts_to_flags(okkt_solver_s* h, BatchWork& W, const char* name, const char* order_words, int64_t B, const int32_t* items, int64_t order, int64_t n, int64_t m,
                          int sym_kind, okkt_inertia* inertia_out, int32_t* flag_out) {
  for (int64_t j = 0; j < B; ++j) {
    const int64_t b = items ? items[j] : j;
    const unsigned long long* c = W.raw.data() + (size_t)b * kCountStride;
    int64_t* in = W.inertia.data() + (size_t)b * 4;
    for (int q = 0; q < 4; ++q) in[q] = (int64_t)c[q];
    if (in[0] + in[1] + in[2] + in[3] != order)
      return solver_set_error(h, OKKT_ERR_INTERNAL, std::string(name) + ": the pivot counts of item " + std::to_string(b) + " do not add up to " + order_words);
    int flag = 0;
    if (in[3] == 0) flag = sym_kind == OKKT_SYM_DEFINITE ? (in[0] == n ? 1 : 0) : ((in[0] == n && in[1] == m) ? 1 : 0);
    W.flags[(size_t)b] = flag;
    if (inertia_out) { inertia_out[b].pos = in[0]; inertia_out[b].neg = in[1]; inertia_out[b].zero = in[2]; inertia_out[b].nonfinite = in[3]; }
    if (flag_out) flag_out[b] = flag;
  }
  return OKKT_OK;
}

int batch_select_slot(okkt_solver_s* h, BatchWork& W, const char* name, int64_t b) {
  h->factored = false;
  ++h->factor_seq;      // the handle's own dense factor, a selected inverse, a pivot report of the previous factor are stale from here on
  h->sc.valid = false;
  std::string e = batch_select_enqueue(h->N, W, b);      // (a scenario batch: the arena holds the item's Schur front where the handle's own plan has it)
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
  int rc = stream_sync(h, name);
  if (rc != OKKT_OK) return rc;
  const int64_t* in = W.inertia.data() + (size_t)b * 4;
  h->a11_inertia.pos = in[0]; h->a11_inertia.neg = in[1]; h->a11_inertia.zero = in[2]; h->a11_inertia.nonfinite = in[3];
  h->N.early_exited = false;
  h->last_failed = W.flags[(size_t)b] == 0;
  h->factored = true;
  return OKKT_OK;
}

int solver_factor_batch_device(okkt_solver_s* h, int64_t B, const double* d_vals, int64_t val_stride, const double* shift, int64_t nshift, int64_t n, int64_t m,
                               int sym_kind, okkt_inertia* inertia_out, int32_t* flag_out, bool zero_tol, const int32_t* items, int64_t nslots) {
  int rc = batch_ready(h, "okkt_factor_batch", items ? std::max<int64_t>(nslots, 1) : B);
  if (rc != OKKT_OK) return rc;
  BatchWork& W = h->bt;
  if (items) {
    // an item list: B distinct slots below nslots; values, shift and the outputs are indexed by slot, the other slots are not touched
    if (B < 1 || B > nslots) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_batch: the item list must hold 1 .. nslots slots");
    std::vector<char> seen((size_t)nslots, 0);
    for (int64_t j = 0; j < B; ++j) {
      if (items[j] < 0 || items[j] >= nslots || seen[(size_t)items[j]]) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_batch: the item list names a slot twice or one outside the batch");
      seen[(size_t)items[j]] = 1;
    }
  }
  const int64_t nout = items ? nslots : B;      // entries of shift and of the outputs
  if (h->sc.mode != OKKT_SCALE_NONE) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_batch: a scaling is set (okkt_set_scaling with OKKT_SCALE_NONE first)");
  if (val_stride != 0 && val_stride < h->S.nnz_in) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_batch: val_stride must be 0 or at least the number of entries");
  if (n < 0 || m < 0 || n + m != h->S.n) return solver_set_error(h, OKKT_ERR_INVALID, "n + m does not match the analysed dimension");
  if (sym_kind != OKKT_SYM_DEFINITE && sym_kind != OKKT_SYM_SYMMETRIC) return solver_set_error(h, OKKT_ERR_INVALID, "unknown sym_kind");
  if (sym_kind == OKKT_SYM_DEFINITE && m != 0) return solver_set_error(h, OKKT_ERR_INVALID, ":definite requires m == 0 (julia.jl:30)");
  if (nshift < 0 || nshift > h->S.n) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_batch: nshift outside 0 .. dim");
  const double tol = (sym_kind == OKKT_SYM_DEFINITE || zero_tol) ? 0.0 : h->opts.inertia_tol;
  // an item list is a level-mode launch (the grid's second coordinate is looked up); a list after a factorisation in item mode would mix
  // the two, so the list's first use must cover a batch factored in level mode or none
  const int mode = items ? OKKT_BATCH_LEVEL : batch_pick_mode(W, h->N, B);
  const int64_t kept_B = items && W.mode_used == OKKT_BATCH_LEVEL && (int64_t)W.flags.size() >= nslots ? W.factored_B : 0;
  if (items && B < nslots && kept_B < nslots)
    return solver_set_error(h, OKKT_ERR_INVALID, "okkt_factor_batch: an item list that leaves slots out needs a level-mode factorisation of all of them before it "
                                                 "(the slots it does not name would hold no factor)");
  W.factored_B = 0;
  if (shift && (rc = stage_upload(h, W.shift, shift, nout, "okkt_factor_batch: shift upload")) != OKKT_OK) return rc;
  if (items) {
    static_assert(sizeof(int) == sizeof(int32_t), "the device list holds int");
    if ((rc = hip_check(h, hipMemcpyAsync(W.items, items, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream), "okkt_factor_batch: item list upload")) != OKKT_OK) return rc;
  }
  (void)hipEventRecord(h->ev0, h->stream);
  std::string e = batch_factor_enqueue(h->N, W, mode, B, d_vals, val_stride, shift != nullptr, nshift, tol, items ? W.items : nullptr);
  if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
  (void)hipEventRecord(h->ev1, h->stream);
  W.raw.resize((size_t)nout * kCountStride);
  if ((rc = stream_read(h, W.raw.data(), W.s.counters, W.raw.size() * sizeof(unsigned long long), "okkt_factor_batch failed")) != OKKT_OK) return rc;
  float ms = 0;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_factor_ms = ms;
  W.mode_used = mode;
  if (!items || kept_B == 0) {
    W.inertia.assign((size_t)nout * 4, 0);
    W.flags.assign((size_t)nout, 0);
  }
  if ((rc = batch_counts_to_flags(h, W, "okkt_factor_batch", "the matrix order", B, items, h->S.n, n, m, sym_kind, inertia_out, flag_out)) != OKKT_OK) return rc;
  // with a list: the slots it does not name keep the factor, the counts and the flag an earlier factorisation left them
  // (a list that leaves slots out is accepted only behind a factorisation of all nslots, above: every slot below factored_B holds a factor)
  W.factored_B = items ? std::max(kept_B, nslots) : B;
  return OKKT_OK;
}

}  // namespace okkt

extern "C" {

int okkt_batch_query(okkt_handle h, int64_t nrhs_max, okkt_batch_info* out) {
  if (!h || !out) return OKKT_ERR_INVALID;
  std::memset(out, 0, sizeof(*out));
  if (nrhs_max < 1) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_batch_query: nrhs_max < 1");
  return fence(h, "okkt_batch_query", [&]() -> int {
    BatchShape shape;
    std::string why;
    out->reason = batch_reason(h, shape, &why);
    out->eligible = out->reason == OKKT_BATCH_OK ? 1 : 0;
    if (!h->analyzed) return OKKT_OK;
    out->max_front = (int32_t)h->S.max_front;
    if (!out->eligible) return OKKT_OK;
    const int64_t arena = h->numeric_ready && h->N.arena_doubles > 0 ? h->N.arena_doubles : h->S.arena_doubles;
    out->bytes_per_item = batch_slot_doubles(h->S, arena, batch_work_columns(nrhs_max)) * 8;
    out->tasks_per_item = shape.tasks;
    out->levels = shape.levels;
    out->launches_factor_level = shape.levels + 1;          // the shifts and counters, then one launch per level
    out->launches_solve_level = 2 * shape.levels + 2;       // gather, the levels upwards, the levels downwards, scatter
    out->launches_factor_item = 1;
    out->launches_solve_item = 1;
    return OKKT_OK;
  }, true);
}

int okkt_batch_reserve(okkt_handle h, int64_t B, int64_t nrhs_max) {
  if (!h) return OKKT_ERR_INVALID;
  if (B < 1 || B > 65535) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_batch_reserve: B outside 1 .. 65535");
  if (nrhs_max < 1) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_batch_reserve: nrhs_max < 1");
  return fence(h, "okkt_batch_reserve", [&]() -> int {
    int rc = ensure_device(h);
    if (rc != OKKT_OK) return rc;
    BatchShape shape;
    std::string why;
    if (batch_reason(h, shape, &why) != OKKT_BATCH_OK) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_batch_reserve: " + why);
    if ((rc = solver_ensure_numeric(h)) != OKKT_OK) return rc;
    if ((int)h->N.levels.size() != shape.levels || h->N.n_tasks != shape.tasks || h->N.n_big != 0)
      return solver_set_error(h, OKKT_ERR_INTERNAL, "okkt_batch_reserve: the device schedule is not the one the batch grids were counted from");
    (void)hipStreamSynchronize(h->stream);
    bool oom = false;
    std::string e = batch_alloc(h->bt, h->S, h->N.arena_doubles, B, nrhs_max, &oom);
    if (!e.empty()) return solver_set_error(h, oom ? OKKT_ERR_ALLOC : OKKT_ERR_HIP, e);
    h->bt.plan_arena_doubles = h->N.arena_doubles;
    h->bt.plan_levels = (int)h->N.levels.size();
    h->bt.plan_tasks = h->N.n_tasks;
    // the environment decides only where okkt_batch_set_mode has not: a mode forced on the handle stays
    h->bt.env_mode = OKKT_BATCH_AUTO;
    if (const char* em = getenv("OKKT_BATCH_MODE")) { const int v = atoi(em); if (v == OKKT_BATCH_LEVEL || v == OKKT_BATCH_ITEM) h->bt.env_mode = v; }
    return OKKT_OK;
  }, true);
}

int okkt_batch_release(okkt_handle h) {
  if (!h) return OKKT_ERR_INVALID;
  if (h->bt.s.arena) {
    int rc = ensure_device(h);
    if (rc != OKKT_OK) return rc;
    (void)hipStreamSynchronize(h->stream);
  }
  batch_free(h->bt);      // (the forced mode is the handle's, not the reservation's: it stays)
  return OKKT_OK;
}

int okkt_batch_set_mode(okkt_handle h, int mode) {
  if (!h) return OKKT_ERR_INVALID;
  if (mode < OKKT_BATCH_AUTO || mode > OKKT_BATCH_ITEM) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_batch_set_mode: unknown mode");
  h->bt.mode = mode;
  return OKKT_OK;
}

int okkt_batch_mode_used(okkt_handle h) { return h ? h->bt.mode_used : OKKT_ERR_INVALID; }

int okkt_factor_batch_dev(okkt_handle h, int64_t B, const double* d_nzval, int64_t val_stride, const double* shift, int64_t nshift, int64_t n, int64_t m,
                          int sym_kind, okkt_inertia* inertia_out, int32_t* flag_out) {
  if (!h || (!d_nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  return fence(h, "okkt_factor_batch_dev", [&] { return solver_factor_batch_device(h, B, d_nzval, val_stride, shift, nshift, n, m, sym_kind, inertia_out, flag_out); }, true);
}

int okkt_factor_batch(okkt_handle h, int64_t B, const double* nzval, int64_t val_stride, const double* shift, int64_t nshift, int64_t n, int64_t m, int sym_kind,
                      okkt_inertia* inertia_out, int32_t* flag_out) {
  if (!h || (!nzval && h->S.nnz_in > 0)) return OKKT_ERR_INVALID;
  return fence(h, "okkt_factor_batch", [&]() -> int {
    int rc = batch_ready(h, "okkt_factor_batch", B);
    if (rc != OKKT_OK) return rc;
    return batch_factor_host_values(h, "okkt_factor_batch", B, nzval, val_stride, [&](const double* d_vals, int64_t stride) {
      return solver_factor_batch_device(h, B, d_vals, stride, shift, nshift, n, m, sym_kind, inertia_out, flag_out);
    });
  }, true);
}

int okkt_solve_batch_dev(okkt_handle h, int64_t B, const double* d_rhs, double* d_sol, int64_t nrhs) {
  if (!h || !d_rhs || !d_sol) return OKKT_ERR_INVALID;
  return fence(h, "okkt_solve_batch_dev", [&] { return solve_batch_device(h, B, d_rhs, d_sol, nrhs); });
}

int okkt_solve_batch(okkt_handle h, int64_t B, const double* rhs, double* sol, int64_t nrhs) {
  if (!h || !rhs || !sol) return OKKT_ERR_INVALID;
  return fence(h, "okkt_solve_batch", [&]() -> int {
    int rc = batch_ready(h, "okkt_solve_batch", B);
    if (rc != OKKT_OK) return rc;
    const int64_t len = B * std::max<int64_t>(nrhs, 0) * h->S.n;
    DevTemp x;
    if (!x.alloc(std::max<int64_t>(len, 1))) return solver_set_error(h, OKKT_ERR_ALLOC, "okkt_solve_batch: the device copy of the right-hand sides does not fit");
    if ((rc = stage_upload(h, x.p, rhs, len, "okkt_solve_batch: rhs upload")) != OKKT_OK) return rc;
    rc = solve_batch_device(h, B, x.p, x.p, nrhs);
    (void)hipStreamSynchronize(h->stream);
    return rc != OKKT_OK ? rc : stage_download(h, sol, x.p, len, "okkt_solve_batch: sol download");
  });
}

int okkt_batch_select(okkt_handle h, int64_t b) {
  if (!h) return OKKT_ERR_INVALID;
  return fence(h, "okkt_batch_select", [&]() -> int {
    int rc = batch_ready(h, "okkt_batch_select", 1);
    if (rc != OKKT_OK) return rc;
    BatchWork& W = h->bt;
    if (b < 0 || b >= W.factored_B) return solver_set_error(h, OKKT_ERR_INVALID, "okkt_batch_select: b outside the items of the last okkt_factor_batch");
    return batch_select_slot(h, W, "okkt_batch_select", b);
  });
}

}  // extern "C"
