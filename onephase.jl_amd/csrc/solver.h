// Internal C++ object behind okkt_handle.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/okkt.h"
#include "batch.h"
#include "batch_schur.h"
#include "condest.h"
#include "dense_ldlt.h"
#include "eigs.h"
#include "factor_ops.h"
#include "krylov.h"
#include "numeric.h"
#include "pivots.h"
#include "refine.h"
#include "scaling.h"
#include "selinv.h"
#include "solve_sparse.h"
#include "symbolic.h"

struct okkt_solver_s {
  okkt_opts opts;
  okkt::SymbolicOptions sopts;
  okkt::Symbolic S;
  okkt::Numeric N;
  bool analyzed = false;
  bool factored = false;
  bool device_ready = false;  // HIP device selected and stream created
  bool numeric_ready = false; // device plan uploaded for the current pattern
  bool last_failed = false;   // the last factorisation did not give the wanted inertia (the next one is a retry of the delta loop)
  bool early_exit = false;    // stop a factorisation whose inertia is already wrong (set by the KKT level for factor! / the delta loop)
  int device = 0;
  hipStream_t stream = nullptr;        // the handle's stream (all CUs)
  hipStream_t stream_masked = nullptr; // look-ahead main stream: CU mask without the reserved CUs (segments that use the look-ahead run here)
  int stream_la = 0, stream_reserved = 0;   // key of the pooled stream set (api.cpp)
  int stream_seq = 0;                       // its order of creation in the process
  hipStream_t stream_panel = nullptr;  // look-ahead panel stream (high priority, all CUs)
  hipStream_t stream_aux = nullptr;    // second panel stream: the part of the in-group updates that k_big_diag does not wait for
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<int64_t> user_perm;
  std::vector<int64_t> schur_idx;   // Schur set (okkt_set_schur); empty: not in Schur mode
  std::vector<int64_t> pat_colptr, pat_rowval;   // the analysed pattern as the caller passed it (exact re-use test in okkt_analyze)
  std::string err;
  double analyze_seconds = 0, last_factor_ms = 0, last_solve_ms = 0;
  int64_t n_analyze_calls = 0;
  int part_id = 0;                 // multi-GPU part of this handle (okkt_dist_set_partition)
  const double* dist_vals = nullptr;
  int64_t dist_n = 0, dist_m = 0;
  int dist_kind = 0;
  double dist_tol = 0;
  // RCCL transport of the sharded path (dist.cpp): communicator and the three exchange buffers
  void* rccl_comm = nullptr;
  int rccl_nranks = 0, rccl_rank = 0;
  double *dist_cb = nullptr, *dist_cv = nullptr, *dist_x = nullptr;
  size_t dist_cb_cap = 0, dist_cv_cap = 0, dist_x_cap = 0;   // doubles the exchange buffers were allocated for (okkt_dist_comm_init)
  long long* dist_counts = nullptr;  // 4 summed pivot counts on the device
  double* d_rhs_stage = nullptr;  // staging for host-side rhs/sol
  int64_t rhs_stage_len = 0;
  // refinement (refine.hip): the row-wise map of the analysed input pattern, built on the first residual / refine call after an
  // analysis and released with it; per-call work vectors of nrhs x n (b, r, d, the previous iterate, host-side x) and (omega, |r|) pairs
  okkt::RefineMap rf;
  double* rf_work = nullptr;
  int64_t rf_work_len = 0;
  double* rf_om = nullptr;
  int64_t rf_om_len = 0;
  // condition estimation (condest.hip): the estimator's blocks, allocated on the first estimate after an analysis and released with
  // the refinement map; the unit vectors the last estimate used
  okkt::CondestWork cd;
  std::vector<int64_t> cd_hist;
  // selected inversion (selinv.hip): its plan and Z, allocated on the first okkt_selinv after an analysis and released with it;
  // factor_seq counts the factorisations started, so that Z is known stale after the next one
  okkt::SelinvWork sl;
  int64_t factor_seq = 0;
  // GMRES-based refinement (krylov.hip): the basis and the vectors of one group of right-hand sides, allocated on the first
  // okkt_solve_gmres after an analysis (grown for a larger restart) and released with the refinement map
  okkt::KrylovWork kr;
  // dense factor of the Schur complement (dense_ldlt.hip): allocated by the first okkt_schur_factor after an
  // analysis and released with the refinement map; the pivot counts of the last okkt_factor_schur (A11's) for the whole-matrix inertia
  okkt::DenseLdltWork dl;
  int64_t dense_seq = 0;        // okkt_schur_factor calls started: a selected inverse through the Schur route is stale after the next
  okkt_inertia a11_inertia = {0, 0, 0, 0};
  // symmetric equilibration (scaling.hip): the configuration of okkt_set_scaling (kept across analyses) and the
  // device state of the current analysis, allocated by the first scaled factorisation and released with the refinement map
  okkt::ScalingWork sc;
  // threshold pivot report (pivots.hip): the work-item lists, g and the partners, allocated by the first
  // okkt_pivot_report after an analysis and released with the refinement map; stale after the next factorisation (factor_seq)
  okkt::PivotWork pv;
  // the factor as an operator (factor_ops.hip): the work-item lists of the products and their vectors, allocated
  // by the first product after an analysis and released with the refinement map
  okkt::FactorOpsWork fo;
  // sparse right-hand sides (solve_sparse_host.cpp / .hip): the units and marks of the reach (host, built by the first
  // call after an analysis), the units' places in the schedules and the list buffers (device, released with the refinement map)
  okkt::SparseWork sp;
  // eigenpairs nearest zero (eigs.hip): the basis V, Op V and the block vectors of the Krylov-Schur method, allocated
  // by the first okkt_eigs after an analysis (grown for a larger basis) and released with the refinement map
  okkt::EigsWork eg;
  // uniform batches (batch.hip): the items' slots, allocated by okkt_batch_reserve and released by okkt_batch_release
  // and with the refinement map
  okkt::BatchWork bt;
  // scenario batches (batch_schur.hip): B items in Schur mode on one pattern -- their slots, the sum buffers and a
  // dense factor of their own; allocated by okkt_schur_batch_reserve, released by okkt_schur_batch_release and with the refinement map
  okkt::SchurBatchWork sb;
};

namespace okkt {
// shared by the linear-solver level and the KKT level
// zero_tol: count a pivot as zero only when it is exactly 0 (|d| <= 0), the rule of OKKT_SYM_DEFINITE, also for OKKT_SYM_SYMMETRIC
// (the bordered Schur system decides its flag the way the Cholesky rule of the plain one does)
int solver_factor_device(okkt_solver_s* h, const double* d_vals, int64_t n, int64_t m, int sym_kind,
                         okkt_inertia* out, bool zero_tol = false);
int solver_solve_device(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs);
// the same without synchronisation or timing (the KKT level strings solves and vector kernels together on the stream);
// accumulate: d_sol += F \ d_rhs
int solver_solve_enqueue(okkt_solver_s* h, const double* d_rhs, double* d_sol, int64_t nrhs, bool accumulate);
int solver_set_error(okkt_solver_s* h, int code, const std::string& msg);
// Schur mode (okkt_set_schur): the calls that need a factor of the whole of A refuse with OKKT_ERR_INVALID
inline bool schur_mode(const okkt_solver_s* h) { return !h->schur_idx.empty(); }
inline int schur_refuse(okkt_solver_s* h, const char* what) {
  return solver_set_error(h, OKKT_ERR_INVALID, std::string(what) + " needs a factor of the whole matrix: the handle is in Schur mode (okkt_set_schur; "
                                                   "use okkt_factor_schur / okkt_schur_condense / okkt_schur_expand, or clear the set with ns = 0)");
}
int solver_ensure_numeric(okkt_solver_s* h);
// okkt_factor_batch_dev behind its pointer checks (api_batch.cpp); zero_tol as solver_factor_device's.
// items (host, or NULL: slots 0 .. B-1): B distinct slots below nslots, factored in level mode; d_vals, shift, inertia_out and flag_out
// are then indexed by slot (nslots entries), and the slots not named keep their factor, counts and flag
int solver_factor_batch_device(okkt_solver_s* h, int64_t B, const double* d_vals, int64_t val_stride, const double* shift, int64_t nshift, int64_t n, int64_t m,
                               int sym_kind, okkt_inertia* inertia_out, int32_t* flag_out, bool zero_tol = false, const int32_t* items = nullptr,
                               int64_t nslots = 0);
// okkt_set_scaling behind its argument checks (api.cpp): also what okkt_kkt_set_ls_scaling forwards to
int solver_set_scaling(okkt_solver_s* h, int mode, int32_t sweeps, const double* s_user);
// refinement driver (api_refine.cpp): x = F \ b, then corrections from the double-double residual against d_nzval until omega <= tol,
// stagnation, a non-finite value or max_steps.  d_rhs, d_sol: nrhs x n on the device (they may alias).  lap(tag), if given, is called at
// the phase boundaries (tag 0: a solve ended, 1: residual / vector work ended); n_solves_out: right-hand sides solved
int solver_refine_device(okkt_solver_s* h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                         double tol, okkt_refine_info* info, double* omega_out, void (*lap)(void*, int) = nullptr, void* lap_ctx = nullptr,
                         int* n_solves_out = nullptr);
void solver_refine_release(okkt_solver_s* h);
// GMRES-based refinement driver (api_refine.cpp): x = F \ b, then outer steps of one double-double residual and one
// right-preconditioned GMRES(restart) cycle on A d = r each, right-hand sides in lockstep groups of up to four.  Pointers as
// solver_refine_device's.  schur_route (here and in the two estimates below): F^-1 is the Schur route's whole-system solve (section 8.10)
int solver_gmres_device(okkt_solver_s* h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                        int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out, bool schur_route = false);
// condition estimate of the factored F (the values d_nzval plus the factorisation's diagonal shift) and forward error bounds (api_condest.cpp)
int solver_condest_device(okkt_solver_s* h, const double* d_nzval, int32_t t, okkt_condest_info* info, bool schur_route = false);
int solver_forward_error_device(okkt_solver_s* h, const double* d_nzval, const double* d_b, const double* d_x, int64_t nrhs, double* ferr_out,
                                double* berr_out, bool schur_route = false);
// the eigenpairs of the factored F nearest zero (api_eigs.cpp): okkt_eigs_dev behind its pointer checks.  The vectors
// stay in h->eg.X (dim x nev) as well; d_vecs may be NULL
int solver_eigs_device(okkt_solver_s* h, const okkt_eigs_opts* o, const double* d_nzval, double* lambda, double* d_vecs, double* resid,
                       okkt_eigs_info* info);
}  // namespace okkt
