// What the files of the C ABI layer (api.cpp, api_refine.cpp, api_condest.cpp, api_schur.cpp, api_selinv.cpp, api_batch.cpp,
// api_batch_schur.cpp) share: the exception fence, the staging of host-side arguments, the gates, the batching of right-hand sides, the
// host side of a batched factorisation.  Defined in api.cpp unless noted.
#pragma once
#include <algorithm>
#include <new>

#include "solver.h"

namespace okkt {

// No exception leaves the layer: body() behind the one catch of it.  where: the entry's name, or the words its message has had.
// oom: std::bad_alloc is OKKT_ERR_ALLOC "out of host memory in <where>" (the entries that size host vectors by the problem)
template <class F>
inline auto fence(okkt_solver_s* h, const char* where, F&& body, bool oom = false) -> decltype(body()) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    if (oom) return solver_set_error(h, OKKT_ERR_ALLOC, std::string("out of host memory in ") + where);
  } catch (...) {
  }
  return solver_set_error(h, OKKT_ERR_INTERNAL, std::string("unexpected exception in ") + where);
}

// a device buffer for the length of one host-side call
struct DevTemp {
  double* p = nullptr;
  ~DevTemp() { if (p) (void)hipFree(p); }
  bool alloc(int64_t n) { return n <= 0 || hipMalloc((void**)&p, (size_t)n * sizeof(double)) == hipSuccess; }
};

int ensure_device(okkt_solver_s* h);
// OKKT_OK, or OKKT_ERR_HIP "<what>: <HIP's error string>"
int hip_check(okkt_solver_s* h, hipError_t he, const char* what);
// the launches before it and the handle's stream: OKKT_OK, or OKKT_ERR_HIP "<what> failed: <HIP's error string>"
int stream_sync(okkt_solver_s* h, const char* what);
// a small result of what the stream holds, to the host and waited for: OKKT_OK, or hip_check's error
int stream_read(okkt_solver_s* h, void* dst, const void* d_src, size_t bytes, const char* what);

// ---- host-side arguments: an entry that takes host pointers is its checks, these, and the body of its _dev twin ---------------------
// h->d_rhs_stage holds at least len doubles (the stream is synchronised before a smaller one is freed)
int stage_reserve(okkt_solver_s* h, int64_t len);
// len doubles to the device on the handle's stream (asynchronous) / back (blocking; the body has synchronised the stream).
// what: the words the entry's message has always had ("rhs upload", "r2 download failed"); hip_check adds HIP's error string
int stage_upload(okkt_solver_s* h, double* d_dst, const double* src, int64_t len, const char* what);
int stage_download(okkt_solver_s* h, double* dst, const double* d_src, int64_t len, const char* what);
// the caller's nzval in the stage of the row map (h->rf.nz_stage, allocated on the first call)
int stage_nzval(okkt_solver_s* h, const double* nzval, const char* what);

// the row map of the analysed pattern (refine.hip), built on the first call after an analysis; what: the prefix of its error
int ensure_row_map(okkt_solver_s* h, const char* what);
inline int refuse_partitioned(okkt_solver_s* h) {
  return solver_set_error(h, OKKT_ERR_INVALID, "residuals and refinement are not available on a partitioned handle (okkt_dist_set_partition with nparts > 1)");
}

// batches of up to kMaxRhs right-hand sides: one pass over L per batch (R = 1, 2 or 4 kernels; three are padded to four).
// body(r, nr, R) enqueues right-hand sides r .. r + nr and returns the error text of its launches
template <class F>
inline int for_rhs_batches(okkt_solver_s* h, int64_t nrhs, F&& body) {
  for (int64_t r = 0; r < nrhs;) {
    const int nr = (int)std::min<int64_t>(nrhs - r, kMaxRhs);
    std::string e = body(r, nr, nr >= 3 ? 4 : nr);
    if (!e.empty()) return solver_set_error(h, OKKT_ERR_HIP, e);
    r += nr;
  }
  return OKKT_OK;
}

// ---- what the uniform and the scenario batches share (api_batch.cpp defines, api_batch_schur.cpp uses) -------------------------------
// small_front_max as numeric_setup clamps it
inline int small_max_of(const okkt_solver_s* h) { return std::max(32, std::min(h->sopts.small_front_max, 136)); }
// The host-values form of a batched factorisation, behind the entry's own ready check: the val_stride check, B (or with val_stride 0 one)
// sets of values to the device, device_factor(d_vals, device stride), and the wait that keeps the copy alive for everything that reads it.
// name: the entry's, the prefix of every message
template <class F>
inline int batch_factor_host_values(okkt_solver_s* h, const char* name, int64_t B, const double* nzval, int64_t val_stride, F&& device_factor) {
  const std::string what = name;
  const int64_t nnz = h->S.nnz_in;
  if (val_stride != 0 && val_stride < nnz) return solver_set_error(h, OKKT_ERR_INVALID, what + ": val_stride must be 0 or at least the number of entries");
  const int64_t copies = val_stride == 0 ? 1 : B;
  DevTemp vals;
  if (!vals.alloc(std::max<int64_t>(copies * nnz, 1))) return solver_set_error(h, OKKT_ERR_ALLOC, what + ": the device copy of the values does not fit");
  int rc;
  if (nnz > 0) {
    const hipError_t he = hipMemcpy2DAsync(vals.p, (size_t)nnz * sizeof(double), nzval, (size_t)std::max(val_stride, nnz) * sizeof(double), (size_t)nnz * sizeof(double),
                                           (size_t)copies, hipMemcpyHostToDevice, h->stream);
    if ((rc = hip_check(h, he, (what + ": nzval upload").c_str())) != OKKT_OK) return rc;
  }
  rc = device_factor(vals.p, val_stride == 0 ? 0 : nnz);
  (void)hipStreamSynchronize(h->stream);      // the copy of the values is freed behind everything that reads it
  return rc;
}
// W.raw (the counters of the slots) -> W.inertia and W.flags of the B items (items: the slots of an item list, NULL: 0 .. B - 1), and
// the caller's outputs where given.  The flag is okkt_factor's (solver_factor_device): no non-finite pivot, then the inertia (n, m).
// OKKT_ERR_INTERNAL "<name>: the pivot counts of item <b> do not add up to <order_words>" when the counts do not sum to order
int batch_counts_to_flags(okkt_solver_s* h, BatchWork& W, const char* name, const char* order_words, int64_t B, const int32_t* items, int64_t order, int64_t n, int64_t m,
                          int sym_kind, okkt_inertia* inertia_out, int32_t* flag_out);
// slot b of a factored batch into the handle's own arena, D and shift: the handle is then factored with the item's inertia and flag
int batch_select_slot(okkt_solver_s* h, BatchWork& W, const char* name, int64_t b);

// ---- residuals and refinement (api_refine.cpp) ----------------------------------------------------------------------------------
// device, analysis, no partition (need_factor: not Schur mode, a complete factorisation); the row map
int refine_ready(okkt_solver_s* h, bool need_factor);
// work vectors of the handle: len doubles and nom (omega, |r|) pairs' doubles (grown, never shrunk until the next analysis)
int refine_work(okkt_solver_s* h, int64_t len, int64_t nom);
// A^-1 for the drivers that run on either route: the factor of the whole matrix, or, schur_route, the fused
// whole-system sweeps of okkt_schur_solve.  No synchronisation
int route_solve_enqueue(okkt_solver_s* h, bool schur_route, const double* d_rhs, double* d_sol, int64_t nrhs);

// ---- Schur mode (api_schur.cpp) -----------------------------------------------------------------------------------------------
// Schur mode, analysed, device plan ready; need_factor: a complete okkt_factor_schur
int schur_ready(okkt_solver_s* h, bool need_factor);
// a dense factor to solve with: made by okkt_schur_factor and, when it is of the handle's own S, not older than the last okkt_factor_schur
int schur_dense_ready(okkt_solver_s* h);
// the Schur route's gate: a device, then the rules of okkt_schur_solve_refine (a complete okkt_factor_schur, a
// current dense factor of the handle's own S, no partition, the row map)
int schur_refine_ready(okkt_solver_s* h);
int schur_route_ready(okkt_solver_s* h);
// batches of right-hand sides; whole: the fused whole-system solve (rhs and sol of order dim), else x2 = S^-1 r2.  sync false: enqueue only
int schur_dense_sweeps(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs, bool whole, bool sync = true);

}  // namespace okkt
