// KKT batches: B iterates on the structure of one KKT handle.  The per-item slots (kkt_batch.hip allocates
// them at okkt_kkt_items_reserve and launches on them) and the host-side state of the okkt_kkt_items_* family.
#pragma once
#include <cstdint>
#include <vector>

namespace okkt {

// Per-item state in HBM, one allocation per array; item b of an array starts at base + b * stride, strides in doubles.  Index arrays, the
// maps and the `ones` vector are the handle's and never duplicated.
struct KktItemSlots {
  int64_t n = 0, m = 0, nnzH = 0, nnzJ = 0, nnzA = 0;
  // the iterate: values of H and J (stride 0: one array shared by every item), the point, Sigma, the CSR-ordered copies, diag(H)
  double *Hx = nullptr, *Jx = nullptr;
  int64_t Hx_stride = 0, Jx_stride = 0;
  double *s = nullptr, *y = nullptr, *sig = nullptr;                                  // stride m
  double *Jcsr = nullptr, *Hcsr = nullptr;                                            // stride nnzJ, nnzH
  double *Hdiag = nullptr, *schur_diag = nullptr;                                     // stride n
  double* Avals = nullptr;                                                            // stride nnzA
  // the resident rhs, the current iterate of okkt_kkt_items_system_rhs, the direction
  double *rD = nullptr, *rP = nullptr, *rC = nullptr;                                 // n, m, m
  double *cur_grad = nullptr, *cur_cons = nullptr, *cur_s = nullptr, *cur_y = nullptr, *cur_sig = nullptr;
  double *dx = nullptr, *dy = nullptr, *ds = nullptr;                                 // n, m, m
  // work vectors of the two kinds' directions and of the diagonal-dominance scan
  double *vn1 = nullptr, *vn2 = nullptr, *vn3 = nullptr, *vm1 = nullptr, *vm2 = nullptr;   // n, n, n, m, m
  double *big1 = nullptr, *big2 = nullptr;                                            // n + m
  double *part = nullptr, *red = nullptr;                                             // part_stride, 8
  int64_t part_stride = 0;
  // per-item scalars, [B] each: delta, (mu * eta_mu) * pen and mu * eta_mu of the last rhs call (computed on the host in the
  // expression order of okkt_kkt_system_rhs), the outputs of the one-workgroup-per-item reductions
  double *delta = nullptr, *mu_pen = nullptr, *mu_target = nullptr, *rmin = nullptr;
};

// Line-search slots (ls_batch.hip): what the batched step-side calls stage and reduce through, allocated at
// the first of them after a reservation and freed with it (they sit in KktItems::allocs)
struct KktLsSlots {
  bool ready = false;
  double *sm[4] = {nullptr, nullptr, nullptr, nullptr};   // [B][m] staging: frac, s_cand / s_new / J dx, y_cand / w, y - mu pen
  double *sn[2] = {nullptr, nullptr};                     // [B][n] staging: grad, J'w
  double *part = nullptr, *out = nullptr;                 // partials [B][256 * 8], results [B][8]
  double* scal = nullptr;                                 // the per-item scalars the maps read: [kLsScalars][B]
  int* list = nullptr;                                    // [B] the item list of a launch
  double* Jcand = nullptr;                                // [B or 1][nnzJ] Jacobian values of the candidates (okkt_kkt_items_dual_step)
  int64_t Jcand_cap = 0;                                  // arrays Jcand has room for
};
// rows of KktLsSlots::scal
enum { kLsThr = 0, kLsNxMin, kLsMu, kLsMuNew, kLsStep, kLsScaleD, kLsScaleMu, kLsAfter, kLsUbInit, kLsAxA, kLsAxB, kLsScalars };

struct KktItems {
  KktItemSlots S;
  KktLsSlots LS;
  // items whose direction is the solve's of the last okkt_kkt_items_compute_direction (okkt_kkt_items_set_direction leaves it: dir_B
  // counts the items that hold a direction of either origin), and the cached norm(dx, Inf) of the items 0 .. dir_B-1
  int64_t solved_B = 0;
  bool dxnorm_ok = false;
  std::vector<double> dxnorm;
  int64_t B = 0;                 // reserved slots
  std::vector<void*> allocs;
  int64_t Hx_cap = 0, Jx_cap = 0;   // arrays S.Hx / S.Jx have room for (0: not allocated yet; 1: a shared array; else B)
  int* d_list = nullptr;        // [B] item list of the scan over the failed items
  int64_t formed_B = 0, factored_B = 0, rhs_B = 0, dir_B = 0;   // items the last call of each step covered (0: none)
  std::vector<double> delta, mu, pen, mu_pen, mu_target;          // host copies of the per-item scalars
  std::vector<int32_t> warnings;
  int64_t ls_generation = -1;         // the linear solver's reservation these slots go with (another okkt_batch_reserve replaces it)
  int64_t bytes_per_item = 0;
};

}  // namespace okkt
