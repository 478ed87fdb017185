// The host arithmetic behind the reductions of the step-side functions (DESIGN.md sections 8f / 8.18): what linesearch.hip (one
// iterate) and ls_batch.hip (the items of a KKT batch) do with the numbers a launch returns, written once so that both evaluate the same
// expressions in the same order.  Plain C++ with no device code: csrc/asan_driver.cpp steps it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace okkt {

// lb_s_thres's scalar  norm * norm^ex  (frac_boundary.jl:3-10); pow on the host (one libm for all)
inline double thres_scalar(double nx, double ex) { return nx * std::pow(nx, ex); }
// Julia's min / max: NaN propagates
inline double jl_min(double a, double b) { return (a != a || b != b) ? NAN : std::min(a, b); }
inline double jl_max(double a, double b) { return (a != a || b != b) ? NAN : std::max(a, b); }

// simple_max_step from the reduced ratio
inline double step_from_ratio(double ratio) { return 1.0 / ratio; }

// dual_bounds + lb_y: r = (lb, ub, last reset, ratio of simple_max_step(y_cand, dy, lb_y)) of the last pass, the ratio that of pass 1
inline void dual_range_finish(const double r[4], double* lb_out, double* ub_out) {
  double lb = r[0], ub = r[1];
  if (!std::isfinite(lb) || !std::isfinite(ub)) { lb = 0.0; ub = -1.0; }   // isbad(lb) || isbad(ub), move.jl:74-76
  ub = jl_min(ub, 1.0 / r[3]);
  *lb_out = lb; *ub_out = ub;
}

// rm = ((J dx).^2 . (y ./ s), |comp|_inf, |comp_predicted|_inf), rn = (dx . eval_grad_phi, dx . H dx) (eval.jl:236-273)
inline void predicted_reduction_finish(int64_t m, const double rm[3], const double rn[2], double mu, double step_size, double out[4]) {
  const double phi_red = step_size * rn[0] + step_size * step_size * 0.5 * (rn[1] + rm[0]);
  const double C_k = rm[1], P_k = rm[2];
  const double comp_penalty = m > 0 ? (P_k * P_k * P_k - C_k * C_k * C_k) / (mu * mu) : 0.0;
  out[0] = phi_red; out[1] = C_k; out[2] = P_k; out[3] = phi_red + comp_penalty;
}

// move_dual (move.jl:100-118): the smallest step it may return, and the clamp of the least-squares step
inline double dual_small_step(double lb, double ub, double step_size_P) { return std::max(lb, std::min(ub, step_size_P)); }
inline double dual_step_finish(const double rn[2], const double rm[2], double ub, double small_step) {
  double sd = (rn[0] + rm[0]) / (rn[1] + rm[1]);
  sd = jl_min(sd, ub);
  sd = jl_max(sd, small_step);
  return sd;
}

}  // namespace okkt
