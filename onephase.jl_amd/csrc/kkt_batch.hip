// C ABI, KKT batches (include/okkt.h: okkt_kkt_items_*): B iterates on the structure of one KKT handle --
// form_system!, the delta loop of ipopt_strategy! with every item's own inertia, System_rhs and compute_direction! with its N err.
//
// Every kernel here is the body of its single-iterate twin in kkt.hip (kkt_device.h) on a grid with one more coordinate: blockIdx.y is
// the item (or, with an item list, the position in the list), whose arrays are reached as base + b * stride.  The thread-to-entry map,
// the lanes per row (from the structure: equal for all items) and the order of every sum are the twin's, so item b is bit for bit what
// the single-iterate calls compute for that iterate on a handle of its own.  Reductions run as one workgroup per item; there are no
// atomics and no workgroup waits for another inside a launch.  The factorisations and the solves are the uniform batches' (batch.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "kkt_batch.h"
#include "kkt_device.h"
#include "kkt_items_seq.h"
#include "kkt_state.h"

using namespace okkt;

namespace {

// the slot of a workgroup: blockIdx.y, or through the item list
__device__ __forceinline__ int64_t item_of(const int* __restrict__ items) { return items ? items[blockIdx.y] : (int)blockIdx.y; }

// ---- form_system! -------------------------------------------------------------------------------------------------------
__global__ void kb_form_prep(KktItemSlots S, const int64_t* __restrict__ Jrmap, const int64_t* __restrict__ Hrmap, const int64_t* __restrict__ Hp,
                             const int* __restrict__ Hi) {
  const int64_t b = blockIdx.y;
  kd_form_prep(S.nnzJ, S.nnzH, S.n, S.m, S.Jx + b * S.Jx_stride, Jrmap, S.Hx + b * S.Hx_stride, Hrmap, Hp, Hi, S.s + b * S.m, S.y + b * S.m,
               S.Jcsr + b * S.nnzJ, S.Hcsr + b * S.nnzH, S.Hdiag + b * S.n, S.sig + b * S.m);
}
__global__ void kb_assemble_aug(KktItemSlots S, const int64_t* __restrict__ mapH, const int64_t* __restrict__ mapJ, const int64_t* __restrict__ diagA) {
  const int64_t b = blockIdx.y;
  kd_assemble_aug(S.nnzH, S.nnzJ, S.n, S.m, S.Hx + b * S.Hx_stride, S.Jx + b * S.Jx_stride, S.s + b * S.m, S.y + b * S.m, mapH, mapJ, diagA,
                  S.Avals + b * S.nnzA);
}
__global__ void kb_assemble_schur(KktItemSlots S, const int64_t* __restrict__ qptr, const int* __restrict__ qa, const int* __restrict__ qb,
                                  const int* __restrict__ qi, const int64_t* __restrict__ qh) {
  const int64_t b = blockIdx.y;
  kd_assemble_schur(S.nnzA, qptr, qa, qb, qi, qh, S.Jx + b * S.Jx_stride, S.sig + b * S.m, S.Hx + b * S.Hx_stride, S.Avals + b * S.nnzA);
}
// the dynamic LDS of a workgroup is that of k_assemble_schur_lds: G columns of maxcol doubles
__global__ __launch_bounds__(256) void kb_assemble_schur_lds(KktItemSlots S, int G, int maxcol, const int64_t* __restrict__ Ap, const int64_t* __restrict__ Jp,
                                                             const int* __restrict__ Ji, const int64_t* __restrict__ Jrp, const int64_t* __restrict__ seg_q,
                                                             const int64_t* __restrict__ seg_t, const uint16_t* __restrict__ tslot, const int64_t* __restrict__ qh) {
  extern __shared__ __attribute__((aligned(16))) double sacc[];
  const int64_t b = blockIdx.y;
  kd_assemble_schur_lds(sacc, S.n, G, maxcol, Ap, Jp, Ji, S.Jx + b * S.Jx_stride, Jrp, S.Jcsr + b * S.nnzJ, seg_q, seg_t, tslot, S.sig + b * S.m, qh,
                        S.Hx + b * S.Hx_stride, S.Avals + b * S.nnzA);
}
__global__ void kb_gather_diag(KktItemSlots S, const int64_t* __restrict__ diagA) {      // schur_diag = diag(Q), schur.jl:56
  const int64_t b = blockIdx.y;
  kd_gather(S.n, diagA, S.Avals + b * S.nnzA, S.schur_diag + b * S.n);
}
template <int LPR>
__global__ __launch_bounds__(256) void kb_schur_diag_seg(KktItemSlots S, const int64_t* __restrict__ Jp, const int* __restrict__ Ji) {
  const int64_t b = blockIdx.y;
  kd_schur_diag_seg<LPR>(S.n, Jp, Ji, S.Jx + b * S.Jx_stride, S.sig + b * S.m, S.Hdiag + b * S.n, S.schur_diag + b * S.n);
}

// ---- reductions and the diagonal-dominance scan ------------------------------------------------------------------------------
// one workgroup per item, the tree of k_reduce: out[slot]
__global__ __launch_bounds__(1024) void kb_reduce(int64_t n, const double* __restrict__ v, int64_t vstride, int mode, double* __restrict__ out,
                                                  const int* __restrict__ items) {
  const int64_t b = item_of(items);
  kd_reduce(n, v + b * vstride, mode, out + b);
}
// k_seg_spmv with a stride per operand (0: shared by the items, as `ones` and the index arrays are)
template <int LPR>
__global__ __launch_bounds__(256) void kb_seg_spmv(int64_t nrows, const int64_t* __restrict__ ptr, const int* __restrict__ idx, const double* __restrict__ vals,
                                                   int64_t vals_stride, const double* __restrict__ x, int64_t x_stride, const double* __restrict__ scale,
                                                   int64_t scale_stride, const double* __restrict__ addv, int64_t addv_stride, double beta,
                                                   double* __restrict__ y, int64_t y_stride, const int* __restrict__ items) {
  const int64_t b = item_of(items);
  kd_seg_spmv<LPR, false>(nrows, ptr, idx, vals + b * vals_stride, x + b * x_stride, scale ? scale + b * scale_stride : nullptr,
                          addv ? addv + b * addv_stride : nullptr, beta, y + b * y_stride, nullptr, nullptr);
}
// k_seg_hess with the item's H: y_b = hess_product(x_b)
template <int LPR>
__global__ __launch_bounds__(256) void kb_seg_hess(KktItemSlots S, const int64_t* __restrict__ Hrp, const int* __restrict__ Hrj, const int64_t* __restrict__ Hp,
                                                   const int* __restrict__ Hi, const double* __restrict__ x, int64_t x_stride, double* __restrict__ y,
                                                   int64_t y_stride, const int* __restrict__ items) {
  const int64_t b = item_of(items);
  kd_seg_hess<LPR>(S.n, Hrp, Hrj, S.Hcsr + b * S.nnzH, Hp, Hi, S.Hx + b * S.Hx_stride, S.Hdiag + b * S.n, x + b * x_stride, y + b * y_stride);
}
// hcol = vn1, hrow = vn2, jsj = vn3 (schur) of the item, its delta from the array; margins into big1
__global__ void kb_diag_dom_margin(KktItemSlots S, int with_jsj, const double* __restrict__ qdiag, const int* __restrict__ items) {
  const int64_t b = item_of(items);
  kd_diag_dom_margin(S.n, S.vn1 + b * S.n, S.vn2 + b * S.n, with_jsj ? S.vn3 + b * S.n : nullptr, qdiag + b * S.n, S.delta[b], S.big1 + b * (S.n + S.m));
}

// ---- System_rhs -------------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void kb_rhs_dual_seg(KktItemSlots S, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, double one_minus_D) {
  const int64_t b = blockIdx.y;
  kd_rhs_dual_seg<LPR>(S.n, Jp, Ji, S.Jx + b * S.Jx_stride, S.cur_y + b * S.m, S.cur_grad + b * S.n, S.mu_pen[b], one_minus_D, S.rD + b * S.n);
}
__global__ void kb_rhs_pc(KktItemSlots S, double one_minus_P) {
  const int64_t b = blockIdx.y;
  kd_rhs_pc(S.m, S.cur_cons + b * S.m, S.cur_s + b * S.m, S.cur_y + b * S.m, one_minus_P, S.mu_target[b], S.rP + b * S.m, S.rC + b * S.m);
}
__global__ void kb_cur_sig(KktItemSlots S) {      // Sigma of the current iterate (schur_direct.jl:47)
  const int64_t b = blockIdx.y;
  kd_div(S.m, S.cur_y + b * S.m, S.cur_s + b * S.m, S.cur_sig + b * S.m);
}

// ---- compute_direction! -------------------------------------------------------------------------------------------------
__global__ void kb_schur_t1(KktItemSlots S) {
  const int64_t b = blockIdx.y;
  kd_schur_t1(S.m, S.rP + b * S.m, S.rC + b * S.m, S.sig + b * S.m, S.s + b * S.m, S.vm1 + b * S.m);
}
__global__ void kb_sym_rhs(KktItemSlots S) {
  const int64_t b = blockIdx.y;
  kd_sym_rhs(S.n, S.m, S.rD + b * S.n, S.rP + b * S.m, S.rC + b * S.m, S.y + b * S.m, S.big1 + b * (S.n + S.m));
}
__global__ void kb_sym_split(KktItemSlots S) {
  const int64_t b = blockIdx.y;
  kd_sym_split(S.n, S.m, S.big2 + b * (S.n + S.m), S.dx + b * S.n, S.dy + b * S.m);
}
// dir_x .+= ls_solve(res_old): the addition of k_permute_out_r with accumulate (solve.hip), *d = *d + v, one add per entry
__global__ void kb_accumulate(int64_t n, const double* __restrict__ sol, double* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (i < n) { double* d = dx + b * n + i; const double v = sol[b * n + i]; *d = *d + v; }
}
// rhs = vn2, v = vm2, the residual into vn1
template <int LPR>
__global__ __launch_bounds__(256) void kb_schur_resid(KktItemSlots S, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, const int64_t* __restrict__ Hrp,
                                                      const int* __restrict__ Hrj, const int64_t* __restrict__ Hp, const int* __restrict__ Hi) {
  const int64_t b = blockIdx.y;
  kd_schur_resid<LPR>(S.n, Jp, Ji, S.Jx + b * S.Jx_stride, S.vm2 + b * S.m, Hrp, Hrj, S.Hcsr + b * S.nnzH, Hp, Hi, S.Hx + b * S.Hx_stride, S.Hdiag + b * S.n,
                      S.dx + b * S.n, S.vn2 + b * S.n, S.delta[b], S.vn1 + b * S.n);
}
template <int LPR>
__global__ __launch_bounds__(256) void kb_schur_dyds(KktItemSlots S, const int64_t* __restrict__ Jrp, const int* __restrict__ Jrj) {
  const int64_t b = blockIdx.y;
  kd_schur_dyds<LPR, false>(S.m, Jrp, Jrj, S.Jcsr + b * S.nnzJ, S.dx + b * S.n, S.rP + b * S.m, S.rC + b * S.m, S.y + b * S.m, S.s + b * S.m, S.sig + b * S.m, 0,
                            S.dy + b * S.m, S.ds + b * S.m, nullptr, nullptr);
}
template <int LPR>
__global__ __launch_bounds__(256) void kb_err_dual(KktItemSlots S, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, const int64_t* __restrict__ Hrp,
                                                   const int* __restrict__ Hrj, const int64_t* __restrict__ Hp, const int* __restrict__ Hi) {
  const int64_t b = blockIdx.y;
  kd_err_dual<LPR>(S.n, Jp, Ji, S.Jx + b * S.Jx_stride, S.dy + b * S.m, Hrp, Hrj, S.Hcsr + b * S.nnzH, Hp, Hi, S.Hx + b * S.Hx_stride, S.Hdiag + b * S.n,
                   S.dx + b * S.n, S.rD + b * S.n, S.delta[b], S.part + b * S.part_stride);
}
template <int LPR>
__global__ __launch_bounds__(256) void kb_err_pc(KktItemSlots S, const int64_t* __restrict__ Jrp, const int* __restrict__ Jrj, int64_t nbD) {
  const int64_t b = blockIdx.y;
  kd_err_pc<LPR, false>(S.m, Jrp, Jrj, S.Jcsr + b * S.nnzJ, S.dx + b * S.n, S.ds + b * S.m, S.dy + b * S.m, S.s + b * S.m, S.y + b * S.m, S.rP + b * S.m,
                        S.rC + b * S.m, S.part + b * S.part_stride + nbD * 8, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void kb_err_final(KktItemSlots S, int64_t nbD, int64_t nbM) {
  const int64_t b = blockIdx.y;
  kd_err_final(nbD, nbM, S.part + b * S.part_stride, S.red + b * 8);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline dim3 grid1b(int64_t n, int64_t B) { return dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256), (unsigned)B); }
inline dim3 seg_grid_b(int64_t rows, int lpr, int64_t B) { return dim3(seg_grid(rows, lpr).x, (unsigned)B); }
// a row kernel for the structure's lanes per row on the grid (rows x lpr / 256, B)
#define SEGB_LAUNCH(KERN, lpr, rows, B, st, ...)                                                                     \
  do {                                                                                                               \
    const int64_t rows__ = (rows);                                                                                   \
    if (rows__ > 0) switch (lpr) {                                                                                   \
        case 4: hipLaunchKernelGGL((KERN<4>), seg_grid_b(rows__, 4, B), dim3(256), 0, st, __VA_ARGS__); break;       \
        case 8: hipLaunchKernelGGL((KERN<8>), seg_grid_b(rows__, 8, B), dim3(256), 0, st, __VA_ARGS__); break;       \
        case 16: hipLaunchKernelGGL((KERN<16>), seg_grid_b(rows__, 16, B), dim3(256), 0, st, __VA_ARGS__); break;    \
        case 32: hipLaunchKernelGGL((KERN<32>), seg_grid_b(rows__, 32, B), dim3(256), 0, st, __VA_ARGS__); break;    \
        default: hipLaunchKernelGGL((KERN<64>), seg_grid_b(rows__, 64, B), dim3(256), 0, st, __VA_ARGS__); break;    \
      }                                                                                                              \
  } while (0)

const double* const kNoVec = nullptr;

// why the family does not apply to the handle: the first reason in the order of the codes (okkt.h), 0 when it does
// plan_known: a reservation stands, so the plan took a batch when it was made (the structure is set once; what changes the linear
// solver's plan afterwards is caught by its own batch calls): the plan is not asked again
int items_reason(okkt_kkt_s* k, std::string* why, okkt_batch_info* q_out, bool plan_known = false) {
  if (q_out) std::memset(q_out, 0, sizeof(*q_out));
  if (!k->structured) { *why = "okkt_kkt_set_structure has not been called"; return OKKT_KKT_ITEMS_NO_STRUCTURE; }
  if (k->kind == OKKT_KKT_CLEVER_SYMMETRIC) { *why = "not for the clever-symmetric kind (its shift rewrites the values)"; return OKKT_KKT_ITEMS_CLEVER; }
  if (k->kind == OKKT_KKT_SCHUR_DIRECT) { *why = "not for the Schur-direct kind (its direction reads a second iterate)"; return OKKT_KKT_ITEMS_SCHUR_DIRECT; }
  if (k->kd > 0) { *why = "schur_dense_rows is active (" + std::to_string(k->kd) + " dense rows border the system)"; return OKKT_KKT_ITEMS_DENSE_ROWS; }
  if (k->ls->sc.mode != OKKT_SCALE_NONE) { *why = "the linear solver's scaling is on (okkt_kkt_set_ls_scaling with OKKT_SCALE_NONE first)"; return OKKT_KKT_ITEMS_SCALING; }
  if (k->ls_refine_steps > 0) { *why = "okkt_kkt_set_ls_refine is on (steps > 0)"; return OKKT_KKT_ITEMS_LS_REFINE; }
  if (plan_known) return OKKT_KKT_ITEMS_OK;
  okkt_batch_info q;
  if (okkt_batch_query(k->ls, 1, &q) != OKKT_OK) { *why = std::string("batch query: ") + okkt_last_error(k->ls); return OKKT_KKT_ITEMS_PLAN + OKKT_BATCH_NOT_ANALYZED; }
  if (q_out) *q_out = q;
  if (!q.eligible) {
    *why = "the plan takes no uniform batch (okkt_batch_query reason " + std::to_string(q.reason) + "; plans of small fronts only)";
    return OKKT_KKT_ITEMS_PLAN + q.reason;
  }
  return OKKT_KKT_ITEMS_OK;
}

// doubles of one item's slot (Hx and Jx counted: a shared array saves them)
int64_t slot_doubles(const okkt_kkt_s* k) {
  const int64_t n = k->n, m = k->m;
  return k->nnzH * 2 + k->nnzJ * 2 + k->nnzA + /* s y sig rP rC cur_cons cur_s cur_y cur_sig dy ds vm1 vm2 */ 13 * m +
         /* Hdiag schur_diag rD cur_grad dx vn1 vn2 vn3 */ 8 * n + 2 * (n + m) + k->part_blocks * 8 + 8 + /* scalars */ 4;
}

// no device -> NO_DEVICE; not eligible -> INVALID with the reason; with need_B: a reservation of at least B
int items_gate(okkt_kkt_s* k, const char* what, int64_t B, bool need_slots) {
  if (!k->ls || k->ls->opts.host_symbolic_only || !k->ls->device_ready) return kk_fail(k, OKKT_ERR_NO_DEVICE, "no HIP device (host_symbolic_only handle)");
  std::string why;
  KktItems* I = k->items;
  const bool plan_known = need_slots && I && I->B && k->ls->bt.s.arena && k->ls->bt.generation == I->ls_generation;
  if (items_reason(k, &why, nullptr, plan_known) != OKKT_KKT_ITEMS_OK) return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": " + why);
  if (!need_slots) return OKKT_OK;
  if (!I || !I->B) return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": no slots are reserved (okkt_kkt_items_reserve)");
  if (!k->ls->bt.s.arena || k->ls->bt.generation != I->ls_generation || k->ls->bt.B < I->B)
    return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": the linear solver's slots have been replaced since okkt_kkt_items_reserve (okkt_batch_reserve, "
                                            "okkt_kkt_ipopt_strategy_batch): reserve again");
  if (B < 1 || B > I->B) return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": B must be in 1 .. the reserved " + std::to_string(I->B));
  KK_TRY(k, hipSetDevice(k->ls->device));
  return OKKT_OK;
}

template <typename T>
bool slot_alloc(KktItems* I, T** p, size_t count) {
  void* q = nullptr;
  if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (hipMemset(q, 0, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { (void)hipFree(q); return false; }
  I->allocs.push_back(q);
  *p = (T*)q;
  return true;
}

// the items' values of H or J: room for `count` arrays of nnz entries (1: one array shared by every item, else the reserved B), made by
// the first okkt_kkt_items_form_system that needs it and grown when a later one passes per-item arrays
int ensure_vals(okkt_kkt_s* k, double** p, int64_t* cap, int64_t count, int64_t nnz) {
  if (*cap >= count) return OKKT_OK;
  KktItems* I = k->items;
  KK_TRY(k, hipStreamSynchronize(kk_stream(k)));
  if (*p) {
    I->allocs.erase(std::remove(I->allocs.begin(), I->allocs.end(), (void*)*p), I->allocs.end());
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
  }
  if (!slot_alloc(I, p, (size_t)count * (size_t)nnz))
    return kk_fail(k, OKKT_ERR_ALLOC, "okkt_kkt_items_form_system: " + std::to_string(count) + " value arrays of " + std::to_string(nnz * 8) + " bytes do not fit the device memory");
  KK_TRY(k, hipDeviceSynchronize());      // the fill ran on the null stream
  *cap = count;
  return OKKT_OK;
}

int ensure_ones(okkt_kkt_s* k) {     // as okkt_kkt_is_diag_dom allocates it: max(n, m) ones, shared by the items
  if (k->ones) return OKKT_OK;
  const int64_t len = std::max<int64_t>(std::max(k->n, k->m), 1);
  void* p = nullptr;
  KK_TRY(k, hipMalloc(&p, (size_t)len * 8));
  k->allocs.push_back(p);
  std::vector<double> one((size_t)len, 1.0);
  KK_TRY(k, hipMemcpy(p, one.data(), (size_t)len * 8, hipMemcpyHostToDevice));
  k->ones = (double*)p;
  return OKKT_OK;
}

// is_diag_dom of the listed items (nl of them, slots d_list[0 .. nl), or all of 0 .. nl with d_list = NULL) at S.delta: rmin[slot] = the
// smallest margin.  The launches of okkt_kkt_is_diag_dom, enqueued only
void scan_enqueue(okkt_kkt_s* k, int64_t nl, const int* d_list) {
  KktItemSlots& S = k->items->S;
  hipStream_t st = kk_stream(k);
  const int64_t n = k->n, m = k->m;
  const bool schur = k->kind == OKKT_KKT_SCHUR;
  SEGB_LAUNCH(kb_seg_spmv, k->lprH, n, nl, st, n, k->Hp, k->Hi, S.Hx, S.Hx_stride, k->ones, (int64_t)0, kNoVec, (int64_t)0, kNoVec, (int64_t)0, 0.0, S.vn1, n, d_list);
  SEGB_LAUNCH(kb_seg_spmv, k->lprH, n, nl, st, n, k->Hrp, k->Hrj, S.Hcsr, S.nnzH, k->ones, (int64_t)0, kNoVec, (int64_t)0, kNoVec, (int64_t)0, 0.0, S.vn2, n, d_list);
  if (schur && m) {
    SEGB_LAUNCH(kb_seg_spmv, k->lprJr, m, nl, st, m, k->Jrp, k->Jrj, S.Jcsr, S.nnzJ, k->ones, (int64_t)0, S.sig, m, kNoVec, (int64_t)0, 0.0, S.vm2, m, d_list);
    SEGB_LAUNCH(kb_seg_spmv, k->lprJc, n, nl, st, n, k->Jp, k->Ji, S.Jx, S.Jx_stride, S.vm2, m, kNoVec, (int64_t)0, kNoVec, (int64_t)0, 0.0, S.vn3, n, d_list);
  }
  hipLaunchKernelGGL(kb_diag_dom_margin, grid1b(n, nl), dim3(256), 0, st, S, (schur && m) ? 1 : 0, schur ? S.schur_diag : S.Hdiag, d_list);
  hipLaunchKernelGGL(kb_reduce, dim3(1, (unsigned)nl), dim3(1024), 0, st, n, S.big1, n + m, 0, S.rmin, d_list);
}

// one batched factorisation over the listed slots with the shifts delta[slot]; flags / inertia by slot
int factor_round(okkt_kkt_s* k, int64_t B, const std::vector<int32_t>& list, const double* delta, okkt_inertia* inertia, int32_t* flags) {
  KktItems* I = k->items;
  const int64_t mm = k->kind == OKKT_KKT_SYMMETRIC ? k->m : 0;
  const int sym = k->kind == OKKT_KKT_SYMMETRIC ? OKKT_SYM_SYMMETRIC : OKKT_SYM_DEFINITE;
  const int rc = solver_factor_batch_device(k->ls, (int64_t)list.size(), I->S.Avals, k->nnzA, delta, k->n, k->n, mm, sym, inertia, flags, false, list.data(), B);
  if (rc < 0) return kk_check_ls(k, rc, "batched factor");
  k->t_factor_ms += k->ls->last_factor_ms;
  return OKKT_OK;
}

void items_state_reset(KktItems* I) { I->formed_B = I->factored_B = I->rhs_B = I->dir_B = I->solved_B = 0; I->dxnorm_ok = false; }

}  // namespace

namespace okkt {
void kkt_items_free(okkt_kkt_s* k) {
  KktItems* I = k->items;
  if (!I) return;
  if (k->ls && k->ls->device_ready) { (void)hipSetDevice(k->ls->device); (void)hipStreamSynchronize(k->ls->stream); }
  for (void* p : I->allocs) (void)hipFree(p);
  delete I;
  k->items = nullptr;
}
int kkt_items_gate(okkt_kkt_s* k, const char* what, int64_t B) { return items_gate(k, what, B, true); }
void kkt_items_spmv(okkt_kkt_s* k, int lpr, int64_t rows, int64_t nl, const int64_t* ptr, const int* idx, const double* vals, int64_t vals_stride,
                    const double* x, int64_t x_stride, double* y, int64_t y_stride, const int* d_list) {
  SEGB_LAUNCH(kb_seg_spmv, lpr, rows, nl, kk_stream(k), rows, ptr, idx, vals, vals_stride, x, x_stride, kNoVec, (int64_t)0, kNoVec, (int64_t)0, 0.0, y, y_stride, d_list);
}
void kkt_items_hess(okkt_kkt_s* k, int64_t nl, const double* x, int64_t x_stride, double* y, int64_t y_stride, const int* d_list) {
  SEGB_LAUNCH(kb_seg_hess, k->lprH, k->n, nl, kk_stream(k), k->items->S, k->Hrp, k->Hrj, k->Hp, k->Hi, x, x_stride, y, y_stride, d_list);
}
}  // namespace okkt

extern "C" {

int okkt_kkt_items_query(okkt_kkt_handle k, okkt_kkt_items_info* out) {
  if (!k || !out) return OKKT_ERR_INVALID;
  std::memset(out, 0, sizeof(*out));
  try {
    std::string why;
    okkt_batch_info q;
    out->reason = items_reason(k, &why, &q);
    out->eligible = out->reason == OKKT_KKT_ITEMS_OK ? 1 : 0;
    if (!out->eligible) return OKKT_OK;
    out->bytes_per_item = slot_doubles(k) * 8 + q.bytes_per_item;
    const int solve = q.launches_solve_level;
    if (k->kind == OKKT_KKT_SYMMETRIC) {
      out->launches_form = 3;                                 // the CSR copies, the assembly, schur_diag
      out->launches_direction = 1 + solve + 2 + 3;           // the rhs, the solve, the split, ds, the three N-err kernels
    } else {
      okkt_kkt_pars P;
      okkt_kkt_default_pars(&P);
      const int R = P.ItRefine_Num;                           // counted for the default number of refinement rounds
      out->launches_form = 3;                                 // the CSR copies, the assembly, schur_diag
      out->launches_direction = 2 + R * (solve + 1) + (R - 1) * 2 + 1 + 3;
    }
    return OKKT_OK;
  } catch (...) {
    return kk_fail(k, OKKT_ERR_INTERNAL, "unexpected exception in okkt_kkt_items_query");
  }
}

int okkt_kkt_items_release(okkt_kkt_handle k) {
  if (!k) return OKKT_ERR_INVALID;
  // the linear solver's slots too, while they are still the ones this reservation made (another reservation there is its owner's)
  const bool ls_slots = k->items && k->ls && k->ls->bt.s.arena && k->ls->bt.generation == k->items->ls_generation;
  kkt_items_free(k);
  if (ls_slots) {
    const int rc = okkt_batch_release(k->ls);
    if (rc != OKKT_OK) return kk_check_ls(k, rc, "okkt_kkt_items_release");
  }
  return OKKT_OK;
}

int okkt_kkt_items_reserve(okkt_kkt_handle k, int64_t B) {
  if (!k) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_kkt_items_reserve", B, false);
  if (rc != OKKT_OK) return rc;
  if (B < 1 || B > 65535) return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_items_reserve: B outside 1 .. 65535");
  try {
    kkt_items_free(k);
    KK_TRY(k, hipSetDevice(k->ls->device));
    rc = okkt_batch_reserve(k->ls, B, 1);
    if (rc != OKKT_OK) return kk_check_ls(k, rc, "okkt_kkt_items_reserve");
    KktItems* I = new KktItems();
    k->items = I;
    KktItemSlots& S = I->S;
    const size_t b = (size_t)B, n = (size_t)k->n, m = (size_t)k->m, nm = n + m;
    S.n = k->n; S.m = k->m; S.nnzH = k->nnzH; S.nnzJ = k->nnzJ; S.nnzA = k->nnzA;
    S.part_stride = k->part_blocks * 8;
    S.Hx_stride = k->nnzH; S.Jx_stride = k->nnzJ;
    const bool ok =
        /* Hx, Jx: okkt_kkt_items_form_system, one array when shared */ slot_alloc(I, &S.s, b * m) && slot_alloc(I, &S.y, b * m) &&
        slot_alloc(I, &S.sig, b * m) && slot_alloc(I, &S.Jcsr, b * k->nnzJ) && slot_alloc(I, &S.Hcsr, b * k->nnzH) && slot_alloc(I, &S.Hdiag, b * n) &&
        slot_alloc(I, &S.schur_diag, b * n) && slot_alloc(I, &S.Avals, b * k->nnzA) && slot_alloc(I, &S.rD, b * n) && slot_alloc(I, &S.rP, b * m) &&
        slot_alloc(I, &S.rC, b * m) && slot_alloc(I, &S.cur_grad, b * n) && slot_alloc(I, &S.cur_cons, b * m) && slot_alloc(I, &S.cur_s, b * m) &&
        slot_alloc(I, &S.cur_y, b * m) && slot_alloc(I, &S.cur_sig, b * m) && slot_alloc(I, &S.dx, b * n) && slot_alloc(I, &S.dy, b * m) &&
        slot_alloc(I, &S.ds, b * m) && slot_alloc(I, &S.vn1, b * n) && slot_alloc(I, &S.vn2, b * n) && slot_alloc(I, &S.vn3, b * n) &&
        slot_alloc(I, &S.vm1, b * m) && slot_alloc(I, &S.vm2, b * m) && slot_alloc(I, &S.big1, b * nm) && slot_alloc(I, &S.big2, b * nm) &&
        slot_alloc(I, &S.part, b * (size_t)S.part_stride) && slot_alloc(I, &S.red, b * 8) && slot_alloc(I, &S.delta, b) && slot_alloc(I, &S.mu_pen, b) &&
        slot_alloc(I, &S.mu_target, b) && slot_alloc(I, &S.rmin, b) && slot_alloc(I, &I->d_list, b);
    if (!ok) {
      const int64_t bytes = slot_doubles(k) * 8;
      kkt_items_free(k);
      (void)okkt_batch_release(k->ls);
      return kk_fail(k, OKKT_ERR_ALLOC, "okkt_kkt_items_reserve: " + std::to_string(B) + " slots of " + std::to_string(bytes) + " bytes do not fit the device memory");
    }
    KK_TRY(k, hipDeviceSynchronize());      // the fills ran on the null stream
    // the LDS-staged Schur assembly asks for more dynamic LDS than the default limit allows only beyond 64 KiB: G * maxcol * 8 <= 64 KiB by construction
    I->B = B;
    I->delta.assign(b, 0.0); I->mu.assign(b, 0.0); I->pen.assign(b, 0.0); I->mu_pen.assign(b, 0.0); I->mu_target.assign(b, 0.0);
    I->warnings.assign(b, 0);
    I->ls_generation = k->ls->bt.generation;
    I->bytes_per_item = slot_doubles(k) * 8;
    if ((rc = ensure_ones(k)) != OKKT_OK) return rc;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, "out of host memory in okkt_kkt_items_reserve");
  } catch (...) {
    return kk_fail(k, OKKT_ERR_INTERNAL, "unexpected exception in okkt_kkt_items_reserve");
  }
}

int okkt_kkt_items_form_system(okkt_kkt_handle k, int64_t B, const double* H_nzval, int64_t H_stride, const double* J_nzval, int64_t J_stride,
                               const double* s, const double* y) {
  if (!k || !s || !y) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_kkt_items_form_system", B, true);
  if (rc != OKKT_OK) return rc;
  if ((k->nnzH > 0 && !H_nzval) || (k->nnzJ > 0 && !J_nzval)) return OKKT_ERR_INVALID;
  if ((H_stride != 0 && H_stride < k->nnzH) || (J_stride != 0 && J_stride < k->nnzJ))
    return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_items_form_system: a stride must be 0 (one array for every item) or at least the number of entries");
  KktItems* I = k->items;
  KktItemSlots& S = I->S;
  items_state_reset(I);
  if ((rc = ensure_vals(k, &S.Hx, &I->Hx_cap, H_stride ? I->B : 1, k->nnzH)) != OKKT_OK) return rc;
  if ((rc = ensure_vals(k, &S.Jx, &I->Jx_cap, J_stride ? I->B : 1, k->nnzJ)) != OKKT_OK) return rc;
  hipStream_t st = kk_stream(k);
  const int64_t n = k->n, m = k->m;
  k->tm_form.reset();
  const size_t e0 = k->tm_form.mark(st);
  S.Hx_stride = H_stride == 0 ? 0 : k->nnzH;
  S.Jx_stride = J_stride == 0 ? 0 : k->nnzJ;
  // the items' values: one copy where they are contiguous (stride = entries, or one shared array), else row by row
  auto upload_vals = [&](double* dst, const double* src, int64_t stride, int64_t nnz) -> hipError_t {
    if (!nnz) return hipSuccess;
    if (stride == 0 || stride == nnz) return hipMemcpyAsync(dst, src, (size_t)(stride ? B : 1) * nnz * 8, hipMemcpyHostToDevice, st);
    return hipMemcpy2DAsync(dst, (size_t)nnz * 8, src, (size_t)stride * 8, (size_t)nnz * 8, (size_t)B, hipMemcpyHostToDevice, st);
  };
  KK_TRY(k, upload_vals(S.Hx, H_nzval, H_stride, k->nnzH));
  KK_TRY(k, upload_vals(S.Jx, J_nzval, J_stride, k->nnzJ));
  if (m) {
    KK_TRY(k, hipMemcpyAsync(S.s, s, (size_t)(B * m) * 8, hipMemcpyHostToDevice, st));
    KK_TRY(k, hipMemcpyAsync(S.y, y, (size_t)(B * m) * 8, hipMemcpyHostToDevice, st));
  }
  const size_t e1 = k->tm_form.mark(st);
  {
    const int64_t tot = std::max(std::max(k->nnzJ, k->nnzH), std::max(n, m));
    if (tot) hipLaunchKernelGGL(kb_form_prep, grid1b(tot, B), dim3(256), 0, st, S, k->Jrmap, k->Hrmap, k->Hp, k->Hi);
  }
  if (k->kind == OKKT_KKT_SYMMETRIC) {
    KK_TRY(k, hipMemsetAsync(S.Avals, 0, (size_t)std::max<int64_t>(B * k->nnzA, 1) * 8, st));
    const int64_t tot = k->nnzH + k->nnzJ + m;
    if (tot) hipLaunchKernelGGL(kb_assemble_aug, grid1b(tot, B), dim3(256), 0, st, S, k->mapH, k->mapJ, k->diagA);
    SEGB_LAUNCH(kb_schur_diag_seg, k->lprJc, n, B, st, S, k->Jp, k->Ji);
  } else {
    if (k->nnzA && k->schur_groups > 0) {
      const int G = k->schur_groups;
      hipLaunchKernelGGL(kb_assemble_schur_lds, dim3((unsigned)((n + G - 1) / G), (unsigned)B), dim3(16 * G), (size_t)G * k->schur_maxcol * sizeof(double), st, S, G,
                         k->schur_maxcol, k->dAp64, k->Jp, k->Ji, k->Jrp, k->seg_q, k->seg_t, k->tslot, k->qh);
    } else if (k->nnzA) {
      hipLaunchKernelGGL(kb_assemble_schur, grid1b(k->nnzA, B), dim3(256), 0, st, S, k->qptr, k->qa, k->qb, k->qi, k->qh);
    }
    if (n) hipLaunchKernelGGL(kb_gather_diag, grid1b(n, B), dim3(256), 0, st, S, k->diagA);
  }
  const size_t e2 = k->tm_form.mark(st);
  k->tm_form.seg(0, e0, e1);
  k->tm_form.seg(1, e1, e2);
  KK_TRY(k, hipStreamSynchronize(st));
  KK_TRY(k, hipGetLastError());
  I->formed_B = B;
  return OKKT_OK;
}

int okkt_kkt_items_diag_min(okkt_kkt_handle k, int64_t B, double* out) {
  if (!k || !out) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_kkt_items_diag_min", B, true);
  if (rc != OKKT_OK) return rc;
  KktItems* I = k->items;
  if (I->formed_B < B) return kk_fail(k, OKKT_ERR_INVALID, "form_system has not been called");
  hipStream_t st = kk_stream(k);
  hipLaunchKernelGGL(kb_reduce, dim3(1, (unsigned)B), dim3(1024), 0, st, k->n, I->S.schur_diag, k->n, 0, I->S.rmin, (const int*)nullptr);
  KK_TRY(k, hipMemcpyAsync(out, I->S.rmin, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  KK_TRY(k, hipStreamSynchronize(st));
  KK_TRY(k, hipGetLastError());
  return OKKT_OK;
}

int okkt_kkt_items_factor(okkt_kkt_handle k, int64_t B, const double* delta, okkt_inertia* inertia_out, int32_t* flag_out) {
  if (!k || !delta) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_kkt_items_factor", B, true);
  if (rc != OKKT_OK) return rc;
  KktItems* I = k->items;
  if (I->formed_B < B) return kk_fail(k, OKKT_ERR_INVALID, "kkt solver not ready to factor: form_system has not been called");
  try {
    I->factored_B = I->dir_B = I->solved_B = 0;
    k->t_factor_ms = 0.0;
    k->tm_factor.reset();
    ItemsLoop L;
    L.start(B);
    for (int64_t b = 0; b < B; ++b) I->delta[(size_t)b] = delta[b];
    if ((rc = factor_round(k, B, L.active, I->delta.data(), inertia_out, flag_out)) != OKKT_OK) return rc;
    KK_TRY(k, hipMemcpyAsync(I->S.delta, I->delta.data(), (size_t)B * 8, hipMemcpyHostToDevice, kk_stream(k)));
    KK_TRY(k, hipStreamSynchronize(kk_stream(k)));
    I->factored_B = B;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, "out of host memory in okkt_kkt_items_factor");
  }
}

int okkt_kkt_items_ipopt_strategy(okkt_kkt_handle k, int64_t B, const double* delta_prev, const okkt_kkt_pars* pars, int32_t* status_out, int32_t* num_fac_out,
                                  double* delta_out, int32_t* diag_dom_warnings_out, int32_t* launches_out) {
  if (!k || !delta_prev || !status_out || !num_fac_out || !delta_out || !launches_out) return OKKT_ERR_INVALID;
  *launches_out = 0;
  int rc = items_gate(k, "okkt_kkt_items_ipopt_strategy", B, true);
  if (rc != OKKT_OK) return rc;
  KktItems* I = k->items;
  if (I->formed_B < B) return kk_fail(k, OKKT_ERR_INVALID, "kkt solver not ready to factor: form_system has not been called");
  try {
    okkt_kkt_pars P;
    okkt_kkt_default_pars(&P);
    if (pars) P = *pars;
    const bool scan = kk_diag_dom_scan_on();
    hipStream_t st = kk_stream(k);
    I->factored_B = I->dir_B = I->solved_B = 0;
    k->t_factor_ms = 0.0;
    k->tm_factor.reset();
    const size_t nb = (size_t)B;
    std::vector<double> dmin(nb), cand(nb, 0.0), rmin(nb, 0.0);
    std::vector<char> in_loop(nb, 0);
    std::vector<int32_t> flags(nb, 0);
    if ((rc = okkt_kkt_items_diag_min(k, B, dmin.data())) != OKKT_OK) return rc;
    std::vector<DeltaSeq> seq(nb);
    for (size_t b = 0; b < nb; ++b) {
      seq[b].start(dmin[b], delta_prev[b], P);
      status_out[b] = 0; num_fac_out[b] = 0; delta_out[b] = P.delta_zero;
      I->warnings[b] = 0;
    }
    ItemsLoop L;
    L.start(B);
    while (!L.active.empty()) {
      // every active item's next attempt, then ONE batched factorisation over the active items
      for (const int32_t b : L.active) {
        bool lp = false;
        if (!seq[(size_t)b].next(P, &cand[(size_t)b], &lp)) return kk_fail(k, OKKT_ERR_INTERNAL, "max it");      // error("max it"), delta_strategy.jl:113
        in_loop[(size_t)b] = lp ? 1 : 0;
      }
      if ((rc = factor_round(k, B, L.active, cand.data(), nullptr, flags.data())) != OKKT_OK) return rc;
      ++*launches_out;
      L.close_round(cand.data(), in_loop.data(), flags.data(), P.delta_max, status_out, num_fac_out, delta_out);
      if (scan && !L.failed.empty() && k->n > 0) {
        // is_diag_dom after a failed attempt (delta_strategy.jl:94-98): a function of the formed values and the attempt's delta only
        const int64_t nf = (int64_t)L.failed.size();
        KK_TRY(k, hipMemcpyAsync(I->S.delta, cand.data(), nb * 8, hipMemcpyHostToDevice, st));
        KK_TRY(k, hipMemcpyAsync(I->d_list, L.failed.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice, st));
        scan_enqueue(k, nf, I->d_list);
        KK_TRY(k, hipMemcpyAsync(rmin.data(), I->S.rmin, nb * 8, hipMemcpyDeviceToHost, st));
        KK_TRY(k, hipStreamSynchronize(st));
        KK_TRY(k, hipGetLastError());
        for (const int32_t b : L.failed)
          if (!(rmin[(size_t)b] < 0.0)) ++I->warnings[(size_t)b];
      } else if (scan && !L.failed.empty()) {
        for (const int32_t b : L.failed) ++I->warnings[(size_t)b];      // n = 0: dominant (okkt_kkt_is_diag_dom)
      }
    }
    for (size_t b = 0; b < nb; ++b) {
      I->delta[b] = delta_out[b];
      if (diag_dom_warnings_out) diag_dom_warnings_out[b] = I->warnings[b];
    }
    KK_TRY(k, hipMemcpyAsync(I->S.delta, I->delta.data(), nb * 8, hipMemcpyHostToDevice, st));
    KK_TRY(k, hipStreamSynchronize(st));
    I->factored_B = B;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, "out of host memory in okkt_kkt_items_ipopt_strategy");
  }
}

int okkt_debug_kkt_items_factor_list(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* delta, int32_t* flag_out) {
  if (!k || !items || !delta || !flag_out || nitems < 1) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_debug_kkt_items_factor_list", B, true);
  if (rc != OKKT_OK) return rc;
  if (k->items->formed_B < B) return kk_fail(k, OKKT_ERR_INVALID, "kkt solver not ready to factor: form_system has not been called");
  try {
    const std::vector<int32_t> list(items, items + nitems);
    return factor_round(k, B, list, delta, nullptr, flag_out);
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, "out of host memory in okkt_debug_kkt_items_factor_list");
  }
}

int okkt_debug_items_loop_model(int64_t B, const double* diag_min, const double* delta_prev, const double* need, const okkt_kkt_pars* pars,
                                int32_t* status_out, int32_t* num_fac_out, double* delta_out, int32_t* launches_out) {
  if (B < 1 || !diag_min || !delta_prev || !need || !status_out || !num_fac_out || !delta_out || !launches_out) return OKKT_ERR_INVALID;
  try {
    okkt_kkt_pars P;
    okkt_kkt_default_pars(&P);
    if (pars) P = *pars;
    const size_t nb = (size_t)B;
    std::vector<DeltaSeq> seq(nb);
    std::vector<double> cand(nb, 0.0);
    std::vector<char> in_loop(nb, 0);
    std::vector<int32_t> flags(nb, 0);
    for (size_t b = 0; b < nb; ++b) { seq[b].start(diag_min[b], delta_prev[b], P); status_out[b] = 0; num_fac_out[b] = 0; delta_out[b] = P.delta_zero; }
    ItemsLoop L;
    L.start(B);
    *launches_out = 0;
    while (!L.active.empty()) {
      for (const int32_t b : L.active) {
        bool lp = false;
        if (!seq[(size_t)b].next(P, &cand[(size_t)b], &lp)) return OKKT_ERR_INTERNAL;
        in_loop[(size_t)b] = lp ? 1 : 0;
        flags[(size_t)b] = cand[(size_t)b] >= need[b] ? 1 : 0;
      }
      ++*launches_out;
      L.close_round(cand.data(), in_loop.data(), flags.data(), P.delta_max, status_out, num_fac_out, delta_out);
    }
    return OKKT_OK;
  } catch (...) {
    return OKKT_ERR_ALLOC;
  }
}

int okkt_kkt_items_system_rhs(okkt_kkt_handle k, int64_t B, const double* grad, const double* cons, const double* s, const double* y, const double* mu,
                              const double* a_norm_penalty, double eta_P, double eta_D, double eta_mu, double* dual_r, double* primal_r, double* comp_r) {
  if (!k || !grad || !cons || !s || !y || !mu || !a_norm_penalty) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_kkt_items_system_rhs", B, true);
  if (rc != OKKT_OK) return rc;
  KktItems* I = k->items;
  if (I->formed_B < B) return kk_fail(k, OKKT_ERR_INVALID, "form_system has not been called");
  KktItemSlots& S = I->S;
  hipStream_t st = kk_stream(k);
  const int64_t n = k->n, m = k->m;
  I->rhs_B = I->dir_B = I->solved_B = 0;
  for (int64_t b = 0; b < B; ++b) {
    I->mu[(size_t)b] = mu[b];
    I->pen[(size_t)b] = a_norm_penalty[b];
    I->mu_pen[(size_t)b] = (mu[b] * eta_mu) * a_norm_penalty[b];      // the expressions of okkt_kkt_system_rhs, in its order
    I->mu_target[(size_t)b] = mu[b] * eta_mu;
  }
  KK_TRY(k, hipMemcpyAsync(S.mu_pen, I->mu_pen.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
  KK_TRY(k, hipMemcpyAsync(S.mu_target, I->mu_target.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
  if (n) KK_TRY(k, hipMemcpyAsync(S.cur_grad, grad, (size_t)(B * n) * 8, hipMemcpyHostToDevice, st));
  if (m) {
    KK_TRY(k, hipMemcpyAsync(S.cur_cons, cons, (size_t)(B * m) * 8, hipMemcpyHostToDevice, st));
    KK_TRY(k, hipMemcpyAsync(S.cur_s, s, (size_t)(B * m) * 8, hipMemcpyHostToDevice, st));
    KK_TRY(k, hipMemcpyAsync(S.cur_y, y, (size_t)(B * m) * 8, hipMemcpyHostToDevice, st));
  }
  k->tm_rhs.reset();
  const size_t e0 = k->tm_rhs.mark(st);
  SEGB_LAUNCH(kb_rhs_dual_seg, k->lprJc, n, B, st, S, k->Jp, k->Ji, 1.0 - eta_D);
  if (m) {
    hipLaunchKernelGGL(kb_rhs_pc, grid1b(m, B), dim3(256), 0, st, S, 1.0 - eta_P);
    hipLaunchKernelGGL(kb_cur_sig, grid1b(m, B), dim3(256), 0, st, S);
  }
  const size_t e1 = k->tm_rhs.mark(st);
  k->tm_rhs.seg(0, e0, e1);
  if (n && dual_r) KK_TRY(k, hipMemcpyAsync(dual_r, S.rD, (size_t)(B * n) * 8, hipMemcpyDeviceToHost, st));
  if (m && primal_r) KK_TRY(k, hipMemcpyAsync(primal_r, S.rP, (size_t)(B * m) * 8, hipMemcpyDeviceToHost, st));
  if (m && comp_r) KK_TRY(k, hipMemcpyAsync(comp_r, S.rC, (size_t)(B * m) * 8, hipMemcpyDeviceToHost, st));
  KK_TRY(k, hipStreamSynchronize(st));
  KK_TRY(k, hipGetLastError());
  I->rhs_B = B;
  return OKKT_OK;
}

int okkt_kkt_items_compute_direction(okkt_kkt_handle k, int64_t B, int32_t ItRefine_Num, double* dx, double* dy, double* ds, okkt_kkt_error* err_out) {
  if (!k) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_kkt_items_compute_direction", B, true);
  if (rc != OKKT_OK) return rc;
  const bool host_dir = dx || dy || ds;
  if (host_dir && (!dx || !dy || !ds)) return kk_fail(k, OKKT_ERR_INVALID, "dx, dy, ds: three host vectors or three NULLs");
  KktItems* I = k->items;
  if (I->factored_B < B) return kk_fail(k, OKKT_ERR_INVALID, "kkt solver not ready to compute direction!");  // kkt_system_solver.jl:181-183
  if (I->rhs_B < B) return kk_fail(k, OKKT_ERR_INVALID, "no resident rhs: okkt_kkt_system_rhs has not been called");
  if (k->ls->bt.factored_B < B) return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_items_compute_direction: the linear solver holds no factored batch of B items");
  try {
    KktItemSlots& S = I->S;
    okkt_solver_s* ls = k->ls;
    hipStream_t st = kk_stream(k);
    const int64_t n = k->n, m = k->m;
    I->dir_B = I->solved_B = 0;
    I->dxnorm_ok = false;
    okkt_kkt_s::Timer& T = k->tm_dir;
    T.reset();
    k->n_solves = 0;
    const size_t t_begin = T.mark(st);
    // one solve of every item, one right-hand side each: the level-mode sweeps of the uniform batch (rhs, sol: [B][dim])
    auto solve = [&](const double* rhs, double* sol) -> int {
      const std::string e = batch_solve_enqueue(ls->N, ls->bt, OKKT_BATCH_LEVEL, B, rhs, sol, 1, 0, 1, 1);
      if (!e.empty()) return kk_fail(k, OKKT_ERR_HIP, "ls_solve: " + e);
      k->n_solves += (int)B;
      return OKKT_OK;
    };
    if (k->kind == OKKT_KKT_SCHUR) {
      // schur.jl:89-128 + solver_schur_rhs, schur.jl:131-182: vn2 = schur_rhs, dx accumulates the rounds, vn1 the residual, vn3 a round's solution
      if (m) hipLaunchKernelGGL(kb_schur_t1, grid1b(m, B), dim3(256), 0, st, S);
      SEGB_LAUNCH(kb_seg_spmv, k->lprJc, n, B, st, n, k->Jp, k->Ji, S.Jx, S.Jx_stride, S.vm1, m, kNoVec, (int64_t)0, S.rD, n, 1.0, S.vn2, n, (const int*)nullptr);
      if (n) KK_TRY(k, hipMemsetAsync(S.dx, 0, (size_t)(B * n) * 8, st));
      for (int it = 0; it < ItRefine_Num; ++it) {
        if ((rc = solve(it == 0 ? S.vn2 : S.vn1, S.vn3)) != OKKT_OK) return rc;
        if (n) hipLaunchKernelGGL(kb_accumulate, grid1b(n, B), dim3(256), 0, st, n, S.vn3, S.dx);      // dir_x .+= ls_solve(res_old)
        if (it + 1 < ItRefine_Num && n) {
          SEGB_LAUNCH(kb_seg_spmv, k->lprJr, m, B, st, m, k->Jrp, k->Jrj, S.Jcsr, S.nnzJ, S.dx, n, S.sig, m, kNoVec, (int64_t)0, 0.0, S.vm2, m, (const int*)nullptr);
          SEGB_LAUNCH(kb_schur_resid, k->lprJc, n, B, st, S, k->Jp, k->Ji, k->Hrp, k->Hrj, k->Hp, k->Hi);
        }
      }
      SEGB_LAUNCH(kb_schur_dyds, k->lprJr, m, B, st, S, k->Jrp, k->Jrj);
    } else {
      // symmetric.jl:59-83
      if (n + m) hipLaunchKernelGGL(kb_sym_rhs, grid1b(n + m, B), dim3(256), 0, st, S);
      if ((rc = solve(S.big1, S.big2)) != OKKT_OK) return rc;
      if (n + m) hipLaunchKernelGGL(kb_sym_split, grid1b(n + m, B), dim3(256), 0, st, S);
      SEGB_LAUNCH(kb_seg_spmv, k->lprJr, m, B, st, m, k->Jrp, k->Jrj, S.Jcsr, S.nnzJ, S.dx, n, kNoVec, (int64_t)0, S.rP, m, -1.0, S.ds, m, (const int*)nullptr);   // J dx - primal_r
    }
    const size_t t_dir = T.mark(st);
    // update_kkt_error! (p = Inf), kkt_system_solver.jl:67-96
    const int64_t nbD = n ? (int64_t)seg_grid(n, k->lprJc).x : 0, nbM = m ? (int64_t)seg_grid(m, k->lprJr).x : 0;
    SEGB_LAUNCH(kb_err_dual, k->lprJc, n, B, st, S, k->Jp, k->Ji, k->Hrp, k->Hrj, k->Hp, k->Hi);
    SEGB_LAUNCH(kb_err_pc, k->lprJr, m, B, st, S, k->Jrp, k->Jrj, nbD);
    hipLaunchKernelGGL(kb_err_final, dim3(1, (unsigned)B), dim3(256), 0, st, S, nbD, nbM);
    const size_t t_end = T.mark(st);
    T.seg(1, t_begin, t_dir);
    T.seg(2, t_dir, t_end);
    T.seg(3, t_begin, t_end);
    std::vector<double> red((size_t)B * 8, 0.0);
    KK_TRY(k, hipMemcpyAsync(red.data(), S.red, red.size() * 8, hipMemcpyDeviceToHost, st));
    if (host_dir) {
      if (n) KK_TRY(k, hipMemcpyAsync(dx, S.dx, (size_t)(B * n) * 8, hipMemcpyDeviceToHost, st));
      if (m) {
        KK_TRY(k, hipMemcpyAsync(dy, S.dy, (size_t)(B * m) * 8, hipMemcpyDeviceToHost, st));
        KK_TRY(k, hipMemcpyAsync(ds, S.ds, (size_t)(B * m) * 8, hipMemcpyDeviceToHost, st));
      }
    }
    KK_TRY(k, hipStreamSynchronize(st));       // the only synchronisation of the call
    KK_TRY(k, hipGetLastError());
    for (int64_t b = 0; b < B && err_out; ++b) err_out[b] = kkt_error_from(red.data() + (size_t)b * 8);
    I->dir_B = I->solved_B = B;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, "out of host memory in okkt_kkt_items_compute_direction");
  }
}

int okkt_kkt_items_select(okkt_kkt_handle k, int64_t b) {
  if (!k) return OKKT_ERR_INVALID;
  int rc = items_gate(k, "okkt_kkt_items_select", 1, true);
  if (rc != OKKT_OK) return rc;
  KktItems* I = k->items;
  if (b < 0 || b >= I->formed_B) return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_items_select: b outside the items of the last okkt_kkt_items_form_system");
  const KktItemSlots& S = I->S;
  hipStream_t st = kk_stream(k);
  const int64_t n = k->n, m = k->m;
  if (!k->cur_grad || !k->cur_cons) {      // as okkt_kkt_system_rhs allocates them on its first call
    void *pg = nullptr, *pc = nullptr;
    KK_TRY(k, hipMalloc(&pg, (size_t)std::max<int64_t>(n, 1) * 8));
    k->allocs.push_back(pg);
    KK_TRY(k, hipMalloc(&pc, (size_t)std::max<int64_t>(m, 1) * 8));
    k->allocs.push_back(pc);
    k->cur_grad = (double*)pg; k->cur_cons = (double*)pc;
  }
  auto cp = [&](double* dst, const double* src, int64_t stride, int64_t len) -> hipError_t {
    return len ? hipMemcpyAsync(dst, src + b * stride, (size_t)len * 8, hipMemcpyDeviceToDevice, st) : hipSuccess;
  };
  KK_TRY(k, cp(k->Hx, S.Hx, S.Hx_stride, k->nnzH)); KK_TRY(k, cp(k->Jx, S.Jx, S.Jx_stride, k->nnzJ));
  KK_TRY(k, cp(k->s, S.s, m, m)); KK_TRY(k, cp(k->y, S.y, m, m)); KK_TRY(k, cp(k->sig, S.sig, m, m));
  KK_TRY(k, cp(k->Jcsr, S.Jcsr, k->nnzJ, k->nnzJ)); KK_TRY(k, cp(k->Hcsr, S.Hcsr, k->nnzH, k->nnzH));
  KK_TRY(k, cp(k->Hdiag, S.Hdiag, n, n)); KK_TRY(k, cp(k->schur_diag, S.schur_diag, n, n));
  KK_TRY(k, cp(k->Avals, S.Avals, k->nnzA, k->nnzA));
  const bool has_rhs = b < I->rhs_B, has_dir = b < I->dir_B, has_fac = b < I->factored_B;
  if (has_rhs) {
    KK_TRY(k, cp(k->rD, S.rD, n, n)); KK_TRY(k, cp(k->rP, S.rP, m, m)); KK_TRY(k, cp(k->rC, S.rC, m, m));
    KK_TRY(k, cp(k->cur_grad, S.cur_grad, n, n)); KK_TRY(k, cp(k->cur_cons, S.cur_cons, m, m));
    KK_TRY(k, cp(k->cur_s, S.cur_s, m, m)); KK_TRY(k, cp(k->cur_y, S.cur_y, m, m)); KK_TRY(k, cp(k->cur_sig, S.cur_sig, m, m));
  }
  if (has_dir) { KK_TRY(k, cp(k->dx, S.dx, n, n)); KK_TRY(k, cp(k->dy, S.dy, m, m)); KK_TRY(k, cp(k->ds, S.ds, m, m)); }
  KK_TRY(k, hipStreamSynchronize(st));
  k->formed = true;
  k->factored = false;
  k->have_dir = has_dir;
  k->have_dxnorm = false;
  k->sym_dir_ok = b < I->solved_B && has_rhs && k->kind == OKKT_KKT_SYMMETRIC;      // a direction of okkt_kkt_items_set_direction is no solve
  k->clever_vecs_ok = false;
  k->have_rhs = k->have_cur = has_rhs;
  k->cur_Jx = k->Jx;
  k->cur_Jcsr = k->Jcsr;
  if (has_rhs) { k->cur_mu = I->mu[(size_t)b]; k->cur_pen = I->pen[(size_t)b]; }
  if (has_fac) {
    k->delta = I->delta[(size_t)b];
    k->diag_dom_warnings = I->warnings[(size_t)b];
    if ((rc = okkt_batch_select(k->ls, b)) != OKKT_OK) return kk_check_ls(k, rc, "okkt_kkt_items_select");
    k->factored = true;
  }
  return OKKT_OK;
}

}  // extern "C"
