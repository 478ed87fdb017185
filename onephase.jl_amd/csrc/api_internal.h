// What the files of the C ABI layer (api.cpp, api_refine.cpp, api_condest.cpp, api_schur.cpp, api_selinv.cpp) share: the exception
// fence, the staging of host-side arguments, the gates, the batching of right-hand sides.  Defined in api.cpp unless noted.
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
