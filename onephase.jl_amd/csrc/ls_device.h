// The device code of the step-side vector kernels (DESIGN.md sections 8f / 8.18): the per-entry maps, the channel-wise reduction and the
// bodies of the map-reduce, final and a*x+b kernels as __device__ functions.  linesearch.hip's __global__ kernels call them for one
// iterate, ls_batch.hip's for the item of blockIdx.y, so that an item is bit for bit what the single-iterate call computes -- the
// arrangement kkt_device.h has for the KKT-level kernels.  A body reads blockIdx.x / threadIdx.x only: the item is a matter of the
// pointers and scalars it is given.  Both files are compiled with -ffp-contract=off: the maps are written operation by operation as the
// reference evaluates them.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace okkt {

enum { kSum = 0, kNanMax = 1, kNanMin = 2 };
constexpr int kLsMaxBlocks = 256;      // workgroups of a map-reduce launch (per item): min(256, ceil(len / 1024)) of 256 threads

template <int NCH>
struct Channels { int op[NCH]; double init[NCH]; };

__device__ __forceinline__ double combine(int op, double a, double b) {
  if (op == kSum) return a + b;
  if (a != a || b != b) return NAN;
  return op == kNanMax ? fmax(a, b) : fmin(a, b);
}
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || b != b) ? NAN : fmin(a, b); }

template <int NCH>
__device__ __forceinline__ void block_reduce(double (&v)[NCH], const Channels<NCH>& ch, double* out) {
  __shared__ double sh[NCH][256];
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < NCH; ++c) sh[c][t] = v[c];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) sh[c][t] = combine(ch.op[c], sh[c][t], sh[c][t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) out[c] = sh[c][0];
  }
}

// grid-stride over the n entries with gridDim.x workgroups; partials: part[blockIdx.x * NCH + c]
template <int NCH, typename F>
__device__ __forceinline__ void ld_map_reduce(int64_t n, const F& f, const Channels<NCH>& ch, double* __restrict__ part) {
  double acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc[c] = ch.op[c] == kSum ? 0.0 : ch.init[c];
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    double v[NCH];
    f(i, v);
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = combine(ch.op[c], acc[c], v[c]);
  }
  block_reduce<NCH>(acc, ch, part + (size_t)blockIdx.x * NCH);
}
// one workgroup: the nb partial rows into out[NCH]
template <int NCH>
__device__ __forceinline__ void ld_reduce_final(int nb, const Channels<NCH>& ch, const double* __restrict__ part, double* __restrict__ out) {
  double acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc[c] = ch.op[c] == kSum ? 0.0 : ch.init[c];
  for (int b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = combine(ch.op[c], acc[c], part[(size_t)b * NCH + c]);
  }
  block_reduce<NCH>(acc, ch, out);
}
__device__ __forceinline__ void ld_axpb(int64_t n, double a, const double* __restrict__ x, double b, double* __restrict__ o, int recip) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = (recip ? a / x[i] : a * x[i]) + b;   // recip: a ./ x + b
}

// ---- the maps ------------------------------------------------------------------------------------------------
struct MapAbs {   // norm(v, Inf)
  const double* v;
  __device__ void operator()(int64_t i, double (&o)[1]) const { o[0] = fabs(v[i]); }
};
// -dir ./ (val - frac .* min.(s, thr)): simple_max_step with lb = frac .* lb_s_thres (frac_boundary.jl:3-15,31-35)
struct MapRatioS {
  const double *val, *dir, *frac, *s;
  double thr;
  __device__ void operator()(int64_t i, double (&o)[1]) const {
    const double lb = frac[i] * nan_min(s[i], thr);
    o[0] = -dir[i] / (val[i] - lb);
  }
};
// s_new .>= frac .* min.(s, thr) (move.jl:15; frac_boundary.jl:22-28): 1 / 0, reduced with min
struct MapSBound {
  const double *s_new, *frac, *s;
  double thr;
  __device__ void operator()(int64_t i, double (&o)[1]) const { o[0] = s_new[i] >= frac[i] * nan_min(s[i], thr) ? 1.0 : 0.0; }
};
// dual_bounds (move.jl:28-80) entry i as (candidate for lb, candidate for ub, index if it resets the interval),
// counted only behind the last reset `after`; and -dy ./ (y_cand - frac .* y * min(1, |dx|_inf)) (line_search.jl:85-86)
struct MapDualBounds {
  const double *s_c, *y_c, *dy, *frac, *y;
  double mu, comp_feas, nxmin;
  int64_t after;
  __device__ void operator()(int64_t i, double (&o)[4]) const {
    const double s = s_c[i], d = dy[i], yc = y_c[i];
    const double safety_factor = 1.001, safety_add = 0.0;
    const double ub_dyi = mu / (comp_feas * s * d) - yc / d;
    const double lb_dyi = mu * comp_feas / (s * d) - yc / d;
    double a = -INFINITY, b = INFINITY, r = -1.0;
    if (d > 0.0) { a = lb_dyi * safety_factor + safety_add; b = ub_dyi / safety_factor - safety_add; }
    else if (d < 0.0) { a = ub_dyi * safety_factor + safety_add; b = lb_dyi / safety_factor - safety_add; }
    else if (lb_dyi >= 0.0 || ub_dyi <= 0.0) r = (double)i;
    if (i <= after) { a = -INFINITY; b = INFINITY; }
    o[0] = a; o[1] = b; o[2] = r;
    o[3] = -d / (yc - frac[i] * y[i] * nxmin);
  }
};
// m-part of the predicted reductions (eval.jl:236-273): (J dx).^2 . (y ./ s), |comp|, |comp_predicted|
struct MapPredM {
  const double *v, *s, *y, *dy, *ds;
  double mu, mu_new, step;
  __device__ void operator()(int64_t i, double (&o)[3]) const {
    const double si = s[i], yi = y[i];
    o[0] = v[i] * v[i] * (yi / si);
    o[1] = fabs(si * yi - mu);
    o[2] = fabs(si * yi + dy[i] * si * step + ds[i] * yi * step - mu_new);
  }
};
// n-part: dx . (grad - J'w) and dx . (H dx)
struct MapPredN {
  const double *dx, *grad, *jtw, *h;
  __device__ void operator()(int64_t i, double (&o)[2]) const {
    o[0] = dx[i] * (grad[i] - jtw[i]);
    o[1] = dx[i] * h[i];
  }
};
// move_dual (move.jl:100-112): res . q and q . q, first n entries / last m entries
struct MapDualStepN {
  const double *grad, *jtw, *jtdy;
  double scale_D;
  __device__ void operator()(int64_t i, double (&o)[2]) const {
    const double q = scale_D * jtdy[i], res = scale_D * (grad[i] - jtw[i]);
    o[0] = res * q; o[1] = q * q;
  }
};
struct MapDualStepM {
  const double *s_c, *y_c, *dy;
  double scale_mu, mu;
  __device__ void operator()(int64_t i, double (&o)[2]) const {
    const double q = scale_mu * s_c[i] * dy[i], res = -scale_mu * (s_c[i] * y_c[i] - mu);
    o[0] = res * q; o[1] = q * q;
  }
};

}  // namespace okkt
