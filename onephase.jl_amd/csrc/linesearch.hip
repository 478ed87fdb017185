// C ABI, step-side vector kernels (include/okkt.h): what simple_ls computes either side of a
// primal-dual step from the cached J, H, the point and the direction -- on the device, against the state the KKT
// handle already holds.
//
//   lb_s_thres / lb_s_predict / lb_y / lb_s / simple_max_step   /root/reference/src/line_search/frac_boundary.jl:3-35
//   the s-bound test of move_primal, dual_bounds, move_dual      src/line_search/move.jl:15-17,28-80,82-118
//   how simple_ls combines them                                   src/line_search/line_search.jl:40-41,84-86
//   comp, eval_grad_phi, phi_predicted_reduction_primal_dual,
//   comp_predicted, merit_function_predicted_reduction            src/utils/eval.jl:11-13,117-120,236-273
//
// All of it is HBM-bound streaming: one pass over a few length-m (or length-n) vectors, a map per entry and a
// reduction.  A launch is (up to) 256 workgroups of 256 threads, grid-stride over the entries, one partial per
// channel and workgroup, then a one-workgroup final pass: fixed partition, so sums are reproducible; max / min
// propagate NaN the way Julia's maximum / max / min do.  This file is compiled with -ffp-contract=off: the maps
// are written operation by operation as the reference evaluates them, and the max / min results are bit-exact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "kkt_state.h"
#include "ls_device.h"
#include "ls_finish.h"

using namespace okkt;

namespace {

constexpr int kMaxBlocks = kLsMaxBlocks;

// the bodies, the maps and the reduction: ls_device.h (shared with the batched kernels of ls_batch.hip)
// partials: part[block * NCH + c]
template <int NCH, typename F>
__global__ __launch_bounds__(256) void k_map_reduce(int64_t n, F f, Channels<NCH> ch, double* __restrict__ part) {
  ld_map_reduce<NCH>(n, f, ch, part);
}
template <int NCH>
__global__ __launch_bounds__(256) void k_reduce_final(int nb, Channels<NCH> ch, const double* __restrict__ part, double* __restrict__ out) {
  ld_reduce_final<NCH>(nb, ch, part, out);
}
__global__ void k_axpb(int64_t n, double a, const double* __restrict__ x, double b, double* __restrict__ o, int recip) {
  ld_axpb(n, a, x, b, o, recip);
}


int ls_ready(okkt_kkt_s* k, bool need_dir) {
  if (!k) return OKKT_ERR_INVALID;
  if (!k->formed) return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_form_system has not been called");
  if (need_dir && !k->have_dir) return kk_fail(k, OKKT_ERR_INVALID, "no direction: call okkt_kkt_compute_direction for this system first");
  KK_TRY(k, hipSetDevice(k->ls->device));
  if (!k->ls_part) {
    auto grab = [&](size_t count, double** out) -> int {
      void* p = nullptr;
      KK_TRY(k, hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(double)));
      k->allocs.push_back(p);
      *out = (double*)p;
      return OKKT_OK;
    };
    int rc;
    for (int q = 0; q < 4; ++q) if ((rc = grab((size_t)k->m, &k->ls_m[q])) != OKKT_OK) return rc;
    for (int q = 0; q < 2; ++q) if ((rc = grab((size_t)k->n, &k->ls_n[q])) != OKKT_OK) return rc;
    if ((rc = grab(8, &k->ls_out)) != OKKT_OK) return rc;
    if ((rc = grab((size_t)kMaxBlocks * 8, &k->ls_part)) != OKKT_OK) return rc;
  }
  return OKKT_OK;
}

int stage(okkt_kkt_s* k, double* dst, const double* host, int64_t count) {
  if (count > 0) KK_TRY(k, hipMemcpyAsync(dst, host, (size_t)count * 8, hipMemcpyHostToDevice, kk_stream(k)));
  return OKKT_OK;
}

// map + reduce over n entries into host_out[NCH]; n == 0 gives the identities
template <int NCH, typename F>
int map_reduce(okkt_kkt_s* k, int64_t n, const F& f, const Channels<NCH>& ch, double* host_out) {
  if (n <= 0) {
    for (int c = 0; c < NCH; ++c) host_out[c] = ch.op[c] == kSum ? 0.0 : ch.init[c];
    return OKKT_OK;
  }
  hipStream_t st = kk_stream(k);
  const int nb = (int)std::min<int64_t>(kMaxBlocks, (n + 1023) / 1024);
  hipLaunchKernelGGL((k_map_reduce<NCH, F>), dim3(nb), dim3(256), 0, st, n, f, ch, k->ls_part);
  hipLaunchKernelGGL((k_reduce_final<NCH>), dim3(1), dim3(256), 0, st, nb, ch, k->ls_part, k->ls_out);
  KK_TRY(k, hipMemcpyAsync(host_out, k->ls_out, NCH * sizeof(double), hipMemcpyDeviceToHost, st));
  KK_TRY(k, hipStreamSynchronize(st));
  KK_TRY(k, hipGetLastError());
  return OKKT_OK;
}

// norm(dir.x, Inf), once per direction (the scalar steps behind the reductions: ls_finish.h)
int dx_norm(okkt_kkt_s* k, double* nx) {
  if (k->have_dxnorm) { *nx = k->dxnorm; return OKKT_OK; }     // once per direction
  Channels<1> ch{{kNanMax}, {0.0}};
  const int rc = map_reduce<1>(k, k->n, MapAbs{k->dx}, ch, nx);
  if (rc == OKKT_OK) { k->dxnorm = *nx; k->have_dxnorm = true; }
  return rc;
}

}  // namespace

extern "C" {

int okkt_kkt_set_direction(okkt_kkt_handle k, const double* dx, const double* dy, const double* ds) {
  int rc = ls_ready(k, false);
  if (rc != OKKT_OK) return rc;
  if ((k->n > 0 && !dx) || (k->m > 0 && (!dy || !ds))) return OKKT_ERR_INVALID;
  if ((rc = stage(k, k->dx, dx, k->n)) != OKKT_OK || (rc = stage(k, k->dy, dy, k->m)) != OKKT_OK || (rc = stage(k, k->ds, ds, k->m)) != OKKT_OK) return rc;
  KK_TRY(k, hipStreamSynchronize(kk_stream(k)));
  k->have_dir = true;
  k->have_dxnorm = false;
  return OKKT_OK;
}

int okkt_kkt_max_step_primal(okkt_kkt_handle k, const double* frac_bd_predict, double ex, double* step_size_P, double* dx_norm_inf) {
  int rc = ls_ready(k, true);
  if (rc != OKKT_OK) return rc;
  if (!step_size_P || (k->m > 0 && !frac_bd_predict)) return OKKT_ERR_INVALID;
  double nx = 0.0;
  if ((rc = dx_norm(k, &nx)) != OKKT_OK) return rc;
  if ((rc = stage(k, k->ls_m[0], frac_bd_predict, k->m)) != OKKT_OK) return rc;
  double ratio = 1.0;
  Channels<1> ch{{kNanMax}, {1.0}};
  if ((rc = map_reduce<1>(k, k->m, MapRatioS{k->s, k->ds, k->ls_m[0], k->s, thres_scalar(nx, ex)}, ch, &ratio)) != OKKT_OK) return rc;
  *step_size_P = step_from_ratio(ratio);
  if (dx_norm_inf) *dx_norm_inf = nx;
  return OKKT_OK;
}

int okkt_kkt_s_bound_ok(okkt_kkt_handle k, const double* s_new, const double* frac_bd, double ex, int32_t* ok) {
  int rc = ls_ready(k, true);
  if (rc != OKKT_OK) return rc;
  if (!ok || (k->m > 0 && (!s_new || !frac_bd))) return OKKT_ERR_INVALID;
  double nx = 0.0;
  if ((rc = dx_norm(k, &nx)) != OKKT_OK) return rc;
  if ((rc = stage(k, k->ls_m[0], frac_bd, k->m)) != OKKT_OK || (rc = stage(k, k->ls_m[1], s_new, k->m)) != OKKT_OK) return rc;
  double all_ok = 1.0;
  Channels<1> ch{{kNanMin}, {1.0}};
  if ((rc = map_reduce<1>(k, k->m, MapSBound{k->ls_m[1], k->ls_m[0], k->s, thres_scalar(nx, ex)}, ch, &all_ok)) != OKKT_OK) return rc;
  *ok = all_ok == 1.0 ? 1 : 0;
  return OKKT_OK;
}

int okkt_kkt_dual_step_range(okkt_kkt_handle k, const double* s_cand, const double* y_cand, double mu_cand, double comp_feas,
                             const double* frac_bd, double* lb_out, double* ub_out) {
  int rc = ls_ready(k, true);
  if (rc != OKKT_OK) return rc;
  if (!lb_out || !ub_out || (k->m > 0 && (!s_cand || !y_cand || !frac_bd))) return OKKT_ERR_INVALID;
  double nx = 0.0;
  if ((rc = dx_norm(k, &nx)) != OKKT_OK) return rc;
  if ((rc = stage(k, k->ls_m[0], frac_bd, k->m)) != OKKT_OK || (rc = stage(k, k->ls_m[1], s_cand, k->m)) != OKKT_OK ||
      (rc = stage(k, k->ls_m[2], y_cand, k->m)) != OKKT_OK)
    return rc;
  // lb = max over the entries behind the last reset (start 0), ub = min (start 1, or -1 behind a reset), the last
  // reset index, and the ratio of simple_max_step(y_cand, dy, lb_y)
  MapDualBounds f{k->ls_m[1], k->ls_m[2], k->dy, k->ls_m[0], k->y, mu_cand, comp_feas, jl_min(1.0, nx), -1};
  Channels<4> ch{{kNanMax, kNanMin, kNanMax, kNanMax}, {0.0, 1.0, -1.0, 1.0}};
  double r[4];
  if ((rc = map_reduce<4>(k, k->m, f, ch, r)) != OKKT_OK) return rc;
  if (r[2] >= 0.0) {   // an entry with dy == 0 reset the interval to (0, -1): only what follows it counts
    f.after = (int64_t)r[2];
    ch.init[1] = -1.0;
    const double ratio_y = r[3];
    if ((rc = map_reduce<4>(k, k->m, f, ch, r)) != OKKT_OK) return rc;
    r[3] = ratio_y;
  }
  dual_range_finish(r, lb_out, ub_out);
  return OKKT_OK;
}

int okkt_kkt_predicted_reduction(okkt_kkt_handle k, const double* grad, double mu, double dmu, double a_norm_penalty,
                                 double step_size, double out[4]) {
  int rc = ls_ready(k, true);
  if (rc != OKKT_OK) return rc;
  if (!out || (k->n > 0 && !grad)) return OKKT_ERR_INVALID;
  hipStream_t st = kk_stream(k);
  const int64_t n = k->n, m = k->m;
  if ((rc = stage(k, k->ls_n[0], grad, n)) != OKKT_OK) return rc;
  double rm[3] = {0.0, 0.0, 0.0}, rn[2] = {0.0, 0.0};
  if (m) {
    kk_spmv_J(k, k->dx, k->ls_m[0]);                                                          // v = J dx
    // eval_grad_phi = grad - J'(mu ./ s) + mu * pen * J'1 = grad - J'(mu ./ s - mu * pen)
    hipLaunchKernelGGL(k_axpb, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, m, mu, k->s, -(mu * a_norm_penalty), k->ls_m[1], 1);
    Channels<3> ch{{kSum, kNanMax, kNanMax}, {0.0, 0.0, 0.0}};
    if ((rc = map_reduce<3>(k, m, MapPredM{k->ls_m[0], k->s, k->y, k->dy, k->ds, mu, mu + dmu * step_size, step_size}, ch, rm)) != OKKT_OK) return rc;
  }
  if (n) {
    if (m) kk_spmv_JT(k, k->Jx, k->ls_m[1], k->ls_n[1]);
    else KK_TRY(k, hipMemsetAsync(k->ls_n[1], 0, (size_t)n * 8, st));
    kk_spmv_H(k, k->dx, k->vn1);
    Channels<2> ch{{kSum, kSum}, {0.0, 0.0}};
    if ((rc = map_reduce<2>(k, n, MapPredN{k->dx, k->ls_n[0], k->ls_n[1], k->vn1}, ch, rn)) != OKKT_OK) return rc;
  }
  predicted_reduction_finish(m, rm, rn, mu, step_size, out);
  return OKKT_OK;
}

int okkt_kkt_dual_step(okkt_kkt_handle k, const double* J_nzval_cand, const double* grad_cand, const double* s_cand,
                       const double* y_cand, double mu_cand, double a_norm_penalty, double step_size_P, double lb, double ub,
                       int dual_ls, double scale_D, double scale_mu, double* step_size_D) {
  int rc = ls_ready(k, true);
  if (rc != OKKT_OK) return rc;
  if (!step_size_D) return OKKT_ERR_INVALID;
  const double small_step = dual_small_step(lb, ub, step_size_P);
  if (dual_ls != 1 && dual_ls != 3) { *step_size_D = ub; return OKKT_OK; }
  const int64_t n = k->n, m = k->m;
  if ((n > 0 && !grad_cand) || (m > 0 && (!s_cand || !y_cand))) return OKKT_ERR_INVALID;
  hipStream_t st = kk_stream(k);
  const double* Jx = k->Jx;
  if (J_nzval_cand && k->nnzJ) {
    if (!k->Jcur) {
      void* p = nullptr;
      KK_TRY(k, hipMalloc(&p, (size_t)k->nnzJ * 8));
      k->allocs.push_back(p);
      k->Jcur = (double*)p;
    }
    KK_TRY(k, hipMemcpyAsync(k->Jcur, J_nzval_cand, (size_t)k->nnzJ * 8, hipMemcpyHostToDevice, st));
    Jx = k->Jcur;
  }
  if ((rc = stage(k, k->ls_n[0], grad_cand, n)) != OKKT_OK || (rc = stage(k, k->ls_m[1], s_cand, m)) != OKKT_OK ||
      (rc = stage(k, k->ls_m[2], y_cand, m)) != OKKT_OK)
    return rc;
  double rn[2] = {0.0, 0.0}, rm[2] = {0.0, 0.0};
  Channels<2> ch{{kSum, kSum}, {0.0, 0.0}};
  if (n) {
    if (m) {
      // eval_grad_lag(new_it, mu) = grad - J'y + mu * pen * J'1 = grad - J'(y - mu * pen)
      hipLaunchKernelGGL(k_axpb, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, m, 1.0, k->ls_m[2], -(mu_cand * a_norm_penalty), k->ls_m[3], 0);
      kk_spmv_JT(k, Jx, k->ls_m[3], k->ls_n[1]);
      kk_spmv_JT(k, Jx, k->dy, k->vn1);
    } else {
      KK_TRY(k, hipMemsetAsync(k->ls_n[1], 0, (size_t)n * 8, st));
      KK_TRY(k, hipMemsetAsync(k->vn1, 0, (size_t)n * 8, st));
    }
    if ((rc = map_reduce<2>(k, n, MapDualStepN{k->ls_n[0], k->ls_n[1], k->vn1, scale_D}, ch, rn)) != OKKT_OK) return rc;
  }
  if (m && (rc = map_reduce<2>(k, m, MapDualStepM{k->ls_m[1], k->ls_m[2], k->dy, scale_mu, mu_cand}, ch, rm)) != OKKT_OK) return rc;
  *step_size_D = dual_step_finish(rn, rm, ub, small_step);
  return OKKT_OK;
}

}  // extern "C"
