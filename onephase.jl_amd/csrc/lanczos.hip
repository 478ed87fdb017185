// Lanczos estimate of lambda_min(Q(0)), Q(0) = H + J' Sigma J, on the device, gfx950.
//
// okkt_kkt_min_eig runs at most 64 Lanczos steps on Q(0) of the iterate of the last okkt_kkt_form_system (or on D Q(0) D, D the Jacobi
// scaling from schur_diag) and returns a vector v with its Rayleigh quotient rho on the unscaled Q(0).  Every delta <= -rho - rho_margin
// leaves Q(0) + delta I with a non-positive eigenvalue: okkt_kkt_ipopt_strategy_eig (kkt.hip) does not factor such attempts.
//
// The operator is matrix-free, two launches per application, from what form_system left in HBM:
//   k_lz_rows  t = Sigma .* (J (d .* x))                        a group of LPR lanes per row of the CSR copy of J
//   k_lz_cols  y = d .* (H_sym (d .* x) + J' t)                 a group of LPR lanes per column: the CSC column of J, the row and the
//              and the workgroup's partials of x'y and x'x      column of the lower-stored H (hess_product, eval.jl:221-234)
// MODE selects d = 1 (plain), the scaled operator, or the absolute-value operator |H|, |J|, |x| (once, for rho_abs).
// The recurrence orthogonalises every new vector against the whole basis with the Gram-Schmidt passes of krylov.hip (CGS2); alpha_j
// and beta_j+1 are read from the column those passes return, one small copy per step; the host solves the tridiagonal problem
// (lanczos_tridiag.h) and decides.
//
// No floating-point atomics, fixed summation orders (the lane groups' xor trees, the workgroup sums, one final workgroup that adds the
// partials in a strided order fixed by their count): two calls give identical bits.  Compiled without contraction, so that the sums
// are the ones the rounding bound of rho_margin counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <type_traits>

#include "krylov.h"
#include "lanczos.h"
#include "lanczos_tridiag.h"

namespace okkt {

struct LanczosWork {
  int64_t n = 0, m = 0;
  int steps = 0;               // the step count V was allocated for
  double* base = nullptr;
  KrylovWork K;                // one system: V [steps + 1][n], W [n], part, h1, h2, col (views into base; never krylov_release'd)
  double *x = nullptr, *q = nullptr, *d = nullptr, *t = nullptr;   // v = D V s, Q v, the scaling, the row pass' output [m]
  double *part2 = nullptr, *out = nullptr;                         // (x'y, x'x) per workgroup of k_lz_cols; the final sums
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

enum { kPlain = 0, kScaled = 1, kAbs = 2 };

template <int MODE>
__device__ __forceinline__ double lz_x(const double* __restrict__ x, const double* __restrict__ d, int64_t i) {
  if (MODE == kScaled) return d[i] * x[i];
  if (MODE == kAbs) return fabs(x[i]);
  return x[i];
}
// the dot of row / column `row` with the vector; VABS: absolute values of the entries; XMODE: how the vector is read.  All lanes of
// the group run the shuffles (no early return), the order of the sum is fixed by LPR alone
template <int LPR, bool VABS, int XMODE>
__device__ __forceinline__ double lz_dot(const int64_t* __restrict__ ptr, const int* __restrict__ idx, const double* __restrict__ vals,
                                         const double* __restrict__ x, const double* __restrict__ d, int64_t row, int sub) {
  double a = 0.0;
  const int64_t p1 = ptr[row + 1];
  for (int64_t p = ptr[row] + sub; p < p1; p += LPR) {
    const double v = VABS ? fabs(vals[p]) : vals[p];
    a += v * lz_x<XMODE>(x, d, idx[p]);
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}

template <int LPR, int MODE>
__global__ __launch_bounds__(256) void k_lz_rows(int64_t m, const int64_t* __restrict__ Jrp, const int* __restrict__ Jrj,
                                                 const double* __restrict__ Jcsr, const double* __restrict__ x, const double* __restrict__ d,
                                                 const double* __restrict__ sig, double* __restrict__ t) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = tid / LPR;
  const int sub = (int)(tid % LPR);
  const int64_t rc = row < m ? row : m - 1;
  const double r = lz_dot<LPR, MODE == kAbs, MODE>(Jrp, Jrj, Jcsr, x, d, rc, sub);
  if (sub == 0 && row < m) t[row] = sig[row] * r;
}

template <int LPR, int MODE>
__global__ __launch_bounds__(256) void k_lz_cols(int64_t n, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, const double* __restrict__ Jx,
                                                 const double* __restrict__ t, const int64_t* __restrict__ Hrp, const int* __restrict__ Hrj,
                                                 const double* __restrict__ Hcsr, const int64_t* __restrict__ Hp, const int* __restrict__ Hi,
                                                 const double* __restrict__ Hx, const double* __restrict__ Hdiag, const double* __restrict__ x,
                                                 const double* __restrict__ d, double* __restrict__ y, double* __restrict__ part) {
  __shared__ double sm[4][2];
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = tid / LPR;
  const int sub = (int)(tid % LPR);
  const int64_t j = row < n ? row : n - 1;
  const double jt = lz_dot<LPR, MODE == kAbs, kPlain>(Jp, Ji, Jx, t, nullptr, j, sub);
  const double v1 = lz_dot<LPR, MODE == kAbs, MODE>(Hrp, Hrj, Hcsr, x, d, j, sub);
  const double v2 = lz_dot<LPR, MODE == kAbs, MODE>(Hp, Hi, Hx, x, d, j, sub);
  double a0 = 0.0, a1 = 0.0;
  if (sub == 0 && row < n) {
    const double xs = lz_x<MODE>(x, d, j);
    const double hd = MODE == kAbs ? fabs(Hdiag[j]) : Hdiag[j];
    double yj = ((v1 + v2) - hd * xs) + jt;
    if (MODE == kScaled) yj = d[j] * yj;
    y[j] = yj;
    const double xj = MODE == kAbs ? fabs(x[j]) : x[j];
    a0 = xj * yj;
    a1 = xj * xj;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a0 = a0 + __shfl_xor(a0, o, 64); a1 = a1 + __shfl_xor(a1, o, 64); }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { sm[wv][0] = a0; sm[wv][1] = a1; }
  __syncthreads();
  if (threadIdx.x < 2) part[(size_t)blockIdx.x * 2 + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// out[0..1] = the sums of the nblk pairs of part: thread t adds the pairs t, t + 256, ... in order, then the workgroup's tree
__global__ __launch_bounds__(256) void k_lz_final(int64_t nblk, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double sm[4][2];
  double a0 = 0.0, a1 = 0.0;
  for (int64_t b = threadIdx.x; b < nblk; b += 256) { a0 = a0 + part[2 * b]; a1 = a1 + part[2 * b + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a0 = a0 + __shfl_xor(a0, o, 64); a1 = a1 + __shfl_xor(a1, o, 64); }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { sm[wv][0] = a0; sm[wv][1] = a1; }
  __syncthreads();
  if (threadIdx.x < 2) out[threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// the start vector: a fixed generator (splitmix64 of the index), magnitudes in [0.5, 1) with either sign -- never the zero vector
__global__ void k_lz_start(int64_t n, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t z = (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const double mag = 0.5 + 0.5 * ((double)(z >> 12) * 0x1.0p-52);
  w[i] = (z & 1) ? -mag : mag;
}
// d_i = 1 / sqrt(|schur_diag_i|), 1 where the entry is zero or not finite (or where the quotient would not be a finite positive number)
__global__ void k_lz_dscale(int64_t n, const double* __restrict__ sd, double* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = fabs(sd[i]);
  double v = 1.0;
  if (a > 0.0 && a < INFINITY) {
    v = 1.0 / sqrt(a);
    if (!(v > 0.0 && v < INFINITY)) v = 1.0;
  }
  d[i] = v;
}
__global__ void k_lz_mul(int64_t n, const double* __restrict__ d, const double* __restrict__ u, double* __restrict__ o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = d[i] * u[i];
}
__global__ void k_lz_resid(int64_t n, const double* __restrict__ q, const double* __restrict__ x, double rho, double* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) r[i] = q[i] - rho * x[i];
}

inline dim3 grid1(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256)); }
inline int64_t seg_blocks(int64_t rows, int lpr) { return std::max<int64_t>(1, (rows * lpr + 255) / 256); }

template <typename F>
inline void lpr_switch(int lpr, F&& f) {
  switch (lpr) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

// y = Op_MODE(x) and the partials of x'y, x'x in W.part2; returns the number of partial pairs
template <int MODE>
int64_t apply_op(okkt_kkt_s* k, LanczosWork& W, const double* x, double* y) {
  hipStream_t st = kk_stream(k);
  const int64_t n = k->n, m = k->m;
  if (m > 0)
    lpr_switch(k->lprJr, [&](auto L) {
      constexpr int LPR = decltype(L)::value;
      hipLaunchKernelGGL((k_lz_rows<LPR, MODE>), dim3((unsigned)seg_blocks(m, LPR)), dim3(256), 0, st, m, k->Jrp, k->Jrj, k->Jcsr, x, W.d, k->sig, W.t);
    });
  const int lprc = std::max(k->lprJc, k->lprH);
  int64_t nblk = 0;
  lpr_switch(lprc, [&](auto L) {
    constexpr int LPR = decltype(L)::value;
    nblk = seg_blocks(n, LPR);
    hipLaunchKernelGGL((k_lz_cols<LPR, MODE>), dim3((unsigned)nblk), dim3(256), 0, st, n, k->Jp, k->Ji, k->Jx, W.t, k->Hrp, k->Hrj, k->Hcsr, k->Hp, k->Hi,
                       k->Hx, k->Hdiag, x, W.d, y, W.part2);
  });
  return nblk;
}


int lz_ensure(okkt_kkt_s* k, int steps) {
  LanczosWork* W = k->lz;
  if (W && W->base && W->n == k->n && W->m == k->m && W->steps >= steps) return OKKT_OK;
  if (!W) {
    W = new (std::nothrow) LanczosWork();
    if (!W) return kk_fail(k, OKKT_ERR_ALLOC, "out of host memory in okkt_kkt_min_eig");
    k->lz = W;
  }
  if (W->base) { (void)hipFree(W->base); W->base = nullptr; }
  const int64_t n = k->n, m = k->m;
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048, 64));   // as krylov_alloc: a function of n alone
  const int64_t nblk_max = seg_blocks(n, 64) + 1;
  const int64_t total = (int64_t)(steps + 1) * n + 4 * n + std::max<int64_t>(m, 1) + (int64_t)kKryCol * nb + 3 * kKryCol + 2 * nblk_max + 8;
  double* p = nullptr;
  KK_TRY(k, hipMalloc((void**)&p, (size_t)total * sizeof(double)));
  W->base = p;
  W->n = n; W->m = m; W->steps = steps;
  W->K = KrylovWork();
  W->K.n = n; W->K.restart = steps; W->K.nb = nb;
  W->K.V = p; p += (int64_t)(steps + 1) * n;
  W->K.W = p; p += n;
  W->x = p; p += n;
  W->q = p; p += n;
  W->d = p; p += n;
  W->t = p; p += std::max<int64_t>(m, 1);
  W->K.part = p; p += (int64_t)kKryCol * nb;
  W->K.h1 = p; p += kKryCol;
  W->K.h2 = p; p += kKryCol;
  W->K.col = p; p += kKryCol;
  W->part2 = p; p += 2 * nblk_max;
  W->out = p;
  if (!W->ev0) KK_TRY(k, hipEventCreate(&W->ev0));
  if (!W->ev1) KK_TRY(k, hipEventCreate(&W->ev1));
  return OKKT_OK;
}

}  // namespace

void lanczos_release(okkt_kkt_s* k) {
  LanczosWork* W = k->lz;
  if (!W) return;
  if (W->base) (void)hipFree(W->base);
  if (W->ev0) (void)hipEventDestroy(W->ev0);
  if (W->ev1) (void)hipEventDestroy(W->ev1);
  delete W;
  k->lz = nullptr;
}

int kk_min_eig(okkt_kkt_s* k, int32_t max_steps, double tol, int32_t scaled, okkt_kkt_eig_info* info, double* v_out) {
  if (!info) return OKKT_ERR_INVALID;
  std::memset(info, 0, sizeof(*info));
  if (!k->ls || k->ls->opts.host_symbolic_only || !k->ls->device_ready) return kk_fail(k, OKKT_ERR_NO_DEVICE, "no HIP device (host_symbolic_only handle)");
  if (k->kind == OKKT_KKT_CLEVER_SYMMETRIC)
    return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_min_eig: not for the clever-symmetric kind (its factored matrix is the merged and rescaled M, not K(delta))");
  if (!k->formed) return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_min_eig: okkt_kkt_form_system has not been called");
  if (max_steps > kTriMax) return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_min_eig: max_steps > 64");
  if (scaled != 0 && scaled != 1) return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_min_eig: scaled must be 0 or 1");
  const int64_t lim = (int64_t)1 << 24;
  if (k->n >= lim || k->eig_maxlen >= lim)
    return kk_fail(k, OKKT_ERR_INVALID, "okkt_kkt_min_eig: n, the longest row or column of J or the longest row of H reaches 2^24: rho_margin = 2^-26 rho_abs would not cover the rounding of rho");
  const int steps_req = max_steps <= 0 ? 32 : (int)max_steps;
  const double tolv = tol > 0.0 ? tol : 0.0625;
  const int64_t n = k->n;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (n == 0) { info->status = 2; return OKKT_OK; }   // the empty matrix: nothing to estimate
  KK_TRY(k, hipSetDevice(k->ls->device));
  int rc = lz_ensure(k, steps_req);
  if (rc != OKKT_OK) return rc;
  LanczosWork& W = *k->lz;
  const KrylovWork& K = W.K;
  hipStream_t st = kk_stream(k);
  KK_TRY(k, hipEventRecord(W.ev0, st));
  if (scaled) hipLaunchKernelGGL(k_lz_dscale, grid1(n), dim3(256), 0, st, n, k->schur_diag, W.d);
  KrySet S;
  std::memset(&S, 0, sizeof(S));
  S.v[0] = K.V; S.w[0] = K.W; S.vstride = n;
  // v_0 = start / ||start||
  hipLaunchKernelGGL(k_lz_start, grid1(n), dim3(256), 0, st, n, K.W);
  krylov_norm_enqueue(K, S, 1, st);
  {
    KryScale C;
    std::memset(&C, 0, sizeof(C));
    C.src[0] = K.W; C.dst[0] = K.V; C.div[0] = K.col;
    krylov_scale_enqueue(n, C, 1, st);
  }
  const int kmax = (int)std::min<int64_t>(steps_req, n);
  double alpha[kTriMax], beta[kTriMax], s[kTriMax], hc[kKryCol];
  double tmin = 0.0, tmax = 0.0, bound = 0.0;
  int status = 1, steps = 0;
  for (int j = 0; j < kmax; ++j) {
    const double* vj = K.V + (int64_t)j * n;
    if (scaled) apply_op<kScaled>(k, W, vj, K.W); else apply_op<kPlain>(k, W, vj, K.W);
    krylov_dots_enqueue(K, S, 1, j + 1, false, st);
    krylov_orth_dots_enqueue(K, S, 1, j + 1, false, st);
    krylov_orth_norm_enqueue(K, S, 1, j + 1, st);
    KK_TRY(k, hipMemcpyAsync(hc, K.col, (size_t)(j + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
    KK_TRY(k, hipStreamSynchronize(st));
    const double a = hc[j], bn = hc[j + 1];
    if (!std::isfinite(a) || !std::isfinite(bn)) { status = 3; steps = j + 1; break; }
    alpha[j] = a;
    steps = j + 1;
    const int trc = tridiag_extreme(j + 1, alpha, beta, &tmin, &tmax, s);
    if (trc != 0) { status = 3; break; }
    bound = std::fabs(bn * s[j]);
    const double tn = std::fmax(std::fabs(tmin), std::fabs(tmax));
    if (bn <= std::ldexp(tn, -44)) { status = 2; break; }       // the Krylov space is invariant to rounding: beta = 0
    if (bound <= tolv * std::fabs(tmin)) { status = 0; break; }
    if (j + 1 == kmax) { status = 1; break; }
    beta[j] = bn;
    KryScale C;
    std::memset(&C, 0, sizeof(C));
    C.src[0] = K.W; C.dst[0] = K.V + (int64_t)(j + 1) * n; C.div[0] = K.col + (j + 1);
    krylov_scale_enqueue(n, C, 1, st);
  }
  info->theta_min = tmin; info->theta_max = tmax; info->bound = bound; info->steps = steps; info->status = status;
  info->rho = info->rho_abs = info->rho_margin = info->resid = nan;
  if (status != 3) {
    // v = D V s; rho and the residual on the unscaled Q(0); rho_abs from the absolute-value operator
    KryCombine C;
    std::memset(&C, 0, sizeof(C));
    C.v[0] = K.V; C.u[0] = scaled ? W.q : W.x; C.vstride = n; C.m[0] = steps;
    for (int i = 0; i < steps; ++i) C.y[0][i] = s[i];
    krylov_combine_enqueue(n, C, 1, st);
    if (scaled) hipLaunchKernelGGL(k_lz_mul, grid1(n), dim3(256), 0, st, n, W.d, W.q, W.x);
    int64_t nblk = apply_op<kPlain>(k, W, W.x, W.q);
    hipLaunchKernelGGL(k_lz_final, dim3(1), dim3(256), 0, st, nblk, W.part2, W.out);
    nblk = apply_op<kAbs>(k, W, W.x, K.W);
    hipLaunchKernelGGL(k_lz_final, dim3(1), dim3(256), 0, st, nblk, W.part2, W.out + 2);
    double o[4];
    KK_TRY(k, hipMemcpyAsync(o, W.out, sizeof(o), hipMemcpyDeviceToHost, st));
    KK_TRY(k, hipStreamSynchronize(st));
    const double rho = o[0] / o[1], rho_abs = o[2] / o[1];
    if (!std::isfinite(rho) || !std::isfinite(rho_abs)) {
      info->status = status = 3;
    } else {
      hipLaunchKernelGGL(k_lz_resid, grid1(n), dim3(256), 0, st, n, W.q, W.x, rho, K.W);
      krylov_norm_enqueue(K, S, 1, st);
      double rn = 0.0;
      KK_TRY(k, hipMemcpyAsync(&rn, K.col, sizeof(double), hipMemcpyDeviceToHost, st));
      if (v_out) KK_TRY(k, hipMemcpyAsync(v_out, W.x, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
      KK_TRY(k, hipStreamSynchronize(st));
      info->rho = rho;
      info->rho_abs = rho_abs;
      info->rho_margin = std::ldexp(rho_abs, -26);
      info->resid = rn / std::sqrt(o[1]);
    }
  }
  if (status == 3 && v_out) std::memset(v_out, 0, (size_t)n * sizeof(double));
  KK_TRY(k, hipEventRecord(W.ev1, st));
  KK_TRY(k, hipStreamSynchronize(st));
  KK_TRY(k, hipGetLastError());
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, W.ev0, W.ev1) == hipSuccess) info->seconds_device = 1e-3 * (double)ms;
  return OKKT_OK;
}

}  // namespace okkt

extern "C" {

int okkt_kkt_min_eig(okkt_kkt_handle k, int32_t max_steps, double tol, int32_t scaled, okkt_kkt_eig_info* info, double* v_out) {
  if (!k) return OKKT_ERR_INVALID;
  return okkt::kk_min_eig(k, max_steps, tol, scaled, info, v_out);
}

int okkt_debug_tridiag_eig(int32_t k, const double* alpha, const double* beta, double* theta_min, double* theta_max, double* s_out, double* bound) {
  if (!alpha || !beta || !theta_min || !theta_max || !s_out || !bound) return OKKT_ERR_INVALID;
  const int rc = okkt::tridiag_extreme(k, alpha, beta, theta_min, theta_max, s_out);
  if (rc == 1) return OKKT_ERR_INVALID;
  if (rc != 0) return OKKT_ERR_INTERNAL;
  *bound = std::fabs(beta[k - 1] * s_out[k - 1]);
  return OKKT_OK;
}

}  // extern "C"
