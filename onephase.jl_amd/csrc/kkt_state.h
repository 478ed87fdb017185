// State of a KKT-system handle (include/okkt.h, level 2), shared by kkt.hip (system, factor, direction) and
// linesearch.hip (step-side vector kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "solver.h"

namespace okkt { struct LanczosWork; struct KktItems; }

struct okkt_kkt_s {
  okkt_handle ls = nullptr;
  int kind = OKKT_KKT_SCHUR;
  int64_t n = 0, m = 0, nnzH = 0, nnzJ = 0, nnzA = 0, dimA = 0;
  bool structured = false, formed = false, factored = false;
  bool have_dxnorm = false;   // dxnorm = norm(dir.x, Inf) of the resident direction is known (step-side functions)
  double dxnorm = 0.0;
  bool have_dir = false;   // dx, dy, ds hold the direction of the last okkt_kkt_compute_direction for the current (s, y)
  double delta = 0.0;
  std::string err;
  std::vector<void*> allocs;
  // assembled matrix pattern (host copy, 0-based CSC lower)
  std::vector<int64_t> Ap, Ai;
  // device: H (CSC lower + CSR view), J (CSC + CSR view), point
  int64_t *Hp = nullptr, *Hrp = nullptr, *Hrmap = nullptr, *Jp = nullptr, *Jrp = nullptr, *Jrmap = nullptr;
  int *Hi = nullptr, *Hrj = nullptr, *Ji = nullptr, *Jrj = nullptr;
  double *Hx = nullptr, *Jx = nullptr, *s = nullptr, *y = nullptr, *sig = nullptr;
  double* Avals = nullptr;
  int64_t *mapH = nullptr, *mapJ = nullptr, *diagA = nullptr;   // symmetric: value slots in A
  int64_t *qptr = nullptr, *qh = nullptr;                        // schur: contributions per Q entry
  int *qa = nullptr, *qb = nullptr, *qi = nullptr;
  // schur, LDS-staged assembly: per CSC entry (row i, column b) of J the start of row i's CSR segment with columns >= b and
  // its first term; per term the slot of its Q entry inside column b (16 bits); groups of 16 lanes own one column of Q
  int64_t *seg_q = nullptr, *seg_t = nullptr, *dAp64 = nullptr;
  uint16_t* tslot = nullptr;
  int schur_groups = 0, schur_maxcol = 0;
  double* schur_diag = nullptr;
  // schur, dense rows of J (okkt_opts.schur_dense_rows): the kd rows left out of J' Sigma J border the factorised matrix,
  // A = [[Q_s + delta I, J_d'], [J_d, -diag(s_d / y_d)]] of order n + kd.  Host: the rows (ascending); device: per row of J its index
  // among the dense rows or -1, the rows, and the slots of the border (the CSC entries of J_d and the k diagonal entries)
  int64_t kd = 0;
  std::vector<int64_t> h_drows;
  int *dflag = nullptr;
  int64_t *drows = nullptr, *bsrc = nullptr, *bslot = nullptr, *bdiag = nullptr;
  int64_t nnzJd = 0, dchunks = 0;   // entries of J_d, workgroups per dense row of k_dense_dot
  double *ddot = nullptr, *dpart = nullptr;   // dense-row dots (k_dense_dot): results [pair][kd], per-workgroup partials
  double *pad_res = nullptr;                  // residual of the refinement, n + kd (tail stays 0)
  // work vectors
  double *rD = nullptr, *rP = nullptr, *rC = nullptr, *dx = nullptr, *dy = nullptr, *ds = nullptr;
  double *vn1 = nullptr, *vn2 = nullptr, *vn3 = nullptr, *vm1 = nullptr, *vm2 = nullptr, *big1 = nullptr, *big2 = nullptr;
  double* red = nullptr;  // reduction outputs
  // batched directions (okkt_kkt_compute_directions): gradient and constraint values of the last okkt_kkt_system_rhs kept resident,
  // per-rhs slots of the rhs triples, the linear-system rhs / solution, the directions and the error reductions
  double *cur_grad = nullptr, *cur_cons = nullptr;
  double cur_mu = 0.0, cur_pen = 0.0;
  int batch_cap = 0;
  double *b_rD = nullptr, *b_rP = nullptr, *b_rC = nullptr, *b_rhs = nullptr, *b_sol = nullptr, *b_res = nullptr, *b_dx = nullptr, *b_dy = nullptr, *b_ds = nullptr, *b_red = nullptr;
  double* ones = nullptr; // max(n, m) ones (row / column sums of the diagonal-dominance scan), allocated on first use
  int diag_dom_warnings = 0;   // failed attempts of the last ipopt_strategy! whose x-block was diagonally dominant (delta_strategy.jl:95)
  // step-side kernels (linesearch.hip): staged host vectors and reduction partials, allocated on first use
  double *ls_m[4] = {nullptr, nullptr, nullptr, nullptr}, *ls_n[2] = {nullptr, nullptr}, *ls_part = nullptr, *ls_out = nullptr;
  double* Jcur = nullptr; // Jacobian values of a current iterate that differs from the factorised one
  // CSR-ordered copies of the values (refreshed by form_system): the row-wise products read values and column indices
  // contiguously instead of gathering through the CSC -> CSR map
  double *Jcsr = nullptr, *Hcsr = nullptr, *Hdiag = nullptr, *Jcur_csr = nullptr;
  int lprJr = 16, lprJc = 16, lprH = 8;      // lanes per row / column of the segmented products (from the average lengths)
  // current iterate of the last okkt_kkt_system_rhs (kkt_associate_rhs!, schur.jl:34-45): Schur_KKT_solver_direct reads it
  double *cur_s = nullptr, *cur_y = nullptr, *cur_sig = nullptr;
  const double* cur_Jx = nullptr;            // CSC values of the current iterate's Jacobian (Jx or Jcur)
  const double* cur_Jcsr = nullptr;          // the same in CSR order
  bool have_cur = false, have_rhs = false;
  double* part = nullptr;                    // per-workgroup partial maxima of the N-err kernels
  // symmetric kind, okkt_kkt_set_ls_refine: refinement steps of the direction's solve (0 = the plain solve), its tolerance, the
  // values it refines against (K with delta on the first n diagonal entries: the matrix the factor sees) and the last outcome
  int32_t ls_refine_steps = 0;
  double ls_refine_tol = 0.0;
  double* rf_vals = nullptr;
  okkt_refine_info last_refine = {0, 0, 0.0, 0.0, 0.0};
  // symmetric kind, okkt_kkt_direction_error_bound: rD, rP, rC, y, dx and dy still hold the rhs and the solution of the last
  // okkt_kkt_compute_direction's solve (cleared by every call that writes one of them); the rhs and the solution reassembled
  bool sym_dir_ok = false;
  // clever-symmetric kind, okkt_kkt_get_clever_vectors: vm1, crhs and big4 still hold symmetric_primal_rhs, the combined rhs and v of
  // the last okkt_kkt_compute_direction (cleared where sym_dir_ok is)
  bool clever_vecs_ok = false;
  double *eb_rhs = nullptr, *eb_sol = nullptr;
  int64_t part_blocks = 0;
  // device timers: (tag, start, stop) event segments of the last call of each kind, summed per tag on request
  struct Timer {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    struct Seg { int tag; size_t a, b; };
    std::vector<Seg> segs;
    void reset() { used = 0; segs.clear(); }
    size_t mark(hipStream_t st) {
      if (used == ev.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return used; ev.push_back(e); }
      (void)hipEventRecord(ev[used], st);
      return used++;
    }
    void seg(int tag, size_t a, size_t b) { if (a < used && b < used) segs.push_back(Seg{tag, a, b}); }
    double sum(int tag) const {
      double tot = 0.0;
      for (const Seg& g : segs) { float ms = 0; if (g.tag == tag && hipEventElapsedTime(&ms, ev[g.a], ev[g.b]) == hipSuccess) tot += ms; }
      return tot;
    }
    void destroy() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); ev.clear(); reset(); }
  };
  Timer tm_form, tm_factor, tm_rhs, tm_dir;
  double t_factor_ms = 0.0;
  int n_solves = 0;
  // ---- clever symmetric (clever_symmetric.jl): parallel-row groups and the reduced system
  bool indexed = false;
  int64_t m_new = 0;
  int rescale_mode = OKKT_RESCALE_NONE;
  double rescale_mu = 0.0, rescale_xinf = 0.0;
  std::vector<int64_t> h_Jrp, h_Jrmap;           // host CSR view of J (kept for compute_indicies)
  std::vector<int> h_Jrj;
  std::vector<int64_t> h_Hp, h_Jp;               // host copies of the column pointers / row indices
  std::vector<int> h_Hi, h_Ji;
  std::vector<int64_t> h_first, h_gptr, h_mind;  // groups: first row, member ranges, member rows (ls order)
  std::vector<double> h_mratio;
  int64_t *gptr = nullptr, *mapJc = nullptr, *Arp = nullptr, *Armap = nullptr, *dAp = nullptr;
  int *mind = nullptr, *row_grp = nullptr, *dAi = nullptr, *Arj = nullptr, *Hcol = nullptr, *Jcol = nullptr;
  double *mratio = nullptr, *row_ratio = nullptr, *gU = nullptr, *rowg = nullptr, *Dres = nullptr, *true_x_diag = nullptr;
  double *crhs = nullptr, *big3 = nullptr, *big4 = nullptr;
  // okkt_kkt_min_eig (lanczos.hip): its workspace (allocated on first use, released with the handle) and the longest of the sums its
  // operator nests (rows and columns of J, rows of the symmetric H), from okkt_kkt_set_structure
  okkt::LanczosWork* lz = nullptr;
  int64_t eig_maxlen = 0;
  // KKT batches (kkt_batch.hip): the slots of okkt_kkt_items_reserve, released by okkt_kkt_items_release and with the handle
  okkt::KktItems* items = nullptr;
};

#define KK_TRY(k, expr)                                                                      \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) { (k)->err = std::string(#expr) + ": " + hipGetErrorString(e__); return OKKT_ERR_HIP; } \
  } while (0)

// a refusal: the message the caller reads through okkt_kkt_last_error, and the code to return
inline int kk_fail(okkt_kkt_s* k, int code, const std::string& msg) { k->err = msg; return code; }
// a return code of the level-1 handle passed on: a negative one takes that handle's message along
inline int kk_check_ls(okkt_kkt_s* k, int rc, const char* what) {
  if (rc < 0) { k->err = std::string(what) + ": " + okkt_last_error(k->ls); }
  return rc;
}
// update_kkt_error! (kkt_system_solver.jl:67-96) from the six maxima the N-err kernels reduce: (error_D, |dual_r|, error_P, error_mu,
// |primal_r|, |comp_r|); max as Julia's, a NaN wins
inline okkt_kkt_error kkt_error_from(const double* red) {
  auto mx = [](double a, double b) { return (a != a || b != b) ? NAN : std::max(a, b); };
  okkt_kkt_error E;
  E.error_D = red[0]; E.error_P = red[2]; E.error_mu = red[3];
  E.overall = mx(mx(red[0], red[2]), red[3]);
  E.rhs_norm = mx(mx(red[1], red[4]), red[5]);
  E.ratio = E.overall / E.rhs_norm;
  return E;
}

namespace okkt {
// OKKT_DIAG_DOM_SCAN=0 in the environment: the delta loops skip the diagonal-dominance scan after a failed attempt (read once)
inline bool kk_diag_dom_scan_on() {
  static const bool on = !(getenv("OKKT_DIAG_DOM_SCAN") && atoi(getenv("OKKT_DIAG_DOM_SCAN")) == 0);
  return on;
}
// y = J x (m), y = J' v with the Jacobian values Jx (n), y = H x with the lower-stored H (n): on the handle's stream
void kk_spmv_J(okkt_kkt_s* k, const double* x, double* y);
void kk_spmv_JT(okkt_kkt_s* k, const double* Jx, const double* v, double* y);
void kk_spmv_H(okkt_kkt_s* k, const double* x, double* y);
inline hipStream_t kk_stream(okkt_kkt_s* k) { return k->ls->stream; }
// the grid of a segmented row kernel: lpr lanes per row, workgroups of 256
inline dim3 seg_grid(int64_t rows, int lpr) { return dim3((unsigned)std::max<int64_t>(1, (rows * lpr + 255) / 256)); }
// the slots of the KKT batch and the synchronisation before them (kkt_batch.hip); okkt_kkt_destroy calls it
void kkt_items_free(okkt_kkt_s* k);
// what ls_batch.hip shares with kkt_batch.hip: the gate of the family (eligible handle, a standing reservation of at least B), and the
// batched products on the items' values -- y_b = A_b x_b over the rows of (ptr, idx) with lpr lanes per row, and y_b = hess_product(x_b)
// with the item's H -- for the nl listed slots (d_list NULL: slots 0 .. nl-1), enqueued on the handle's stream
int kkt_items_gate(okkt_kkt_s* k, const char* what, int64_t B);
void kkt_items_spmv(okkt_kkt_s* k, int lpr, int64_t rows, int64_t nl, const int64_t* ptr, const int* idx, const double* vals, int64_t vals_stride,
                    const double* x, int64_t x_stride, double* y, int64_t y_stride, const int* d_list);
void kkt_items_hess(okkt_kkt_s* k, int64_t nl, const double* x, int64_t x_stride, double* y, int64_t y_stride, const int* d_list);
}  // namespace okkt
