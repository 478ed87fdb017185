// The bodies of the KKT-level kernels that the symmetric kind and the Schur kind without dense rows run, as __device__ functions:
// kkt.hip's __global__ kernels call them for one iterate, kkt_batch.hip's for item blockIdx.y of a batch, so
// that an item is bit for bit what the single-iterate call computes -- the arrangement front_device.h has for the fronts.  A body reads
// blockIdx.x / threadIdx.x only: the item is a matter of the pointers it is given.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace okkt {

// ---- assembly ---------------------------------------------------------------------------------
// K = [[H, J'],[J, -diag(s/y)]], lower triangle only: pure gather/scatter through precomputed slots
__device__ __forceinline__ void kd_assemble_aug(int64_t nnzH, int64_t nnzJ, int64_t n, int64_t m, const double* __restrict__ Hx,
                                                const double* __restrict__ Jx, const double* __restrict__ s, const double* __restrict__ y,
                                                const int64_t* __restrict__ mapH, const int64_t* __restrict__ mapJ,
                                                const int64_t* __restrict__ diagA, double* __restrict__ A) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nnzH) A[mapH[t]] = Hx[t];
  else if (t < nnzH + nnzJ) A[mapJ[t - nnzH]] = Jx[t - nnzH];
  else if (t < nnzH + nnzJ + m) { const int64_t i = t - nnzH - nnzJ; A[diagA[n + i]] = -s[i] / y[i]; }
}

// Q = J' diag(sig) J + H on the lower triangle: every entry sums its own contribution list
// (row i ascending, like Gustavson's product in eval.jl:85-87), then adds H
__device__ __forceinline__ void kd_assemble_schur(int64_t nnzQ, const int64_t* __restrict__ qptr, const int* __restrict__ qa,
                                                  const int* __restrict__ qb, const int* __restrict__ qi, const int64_t* __restrict__ qh,
                                                  const double* __restrict__ Jx, const double* __restrict__ sig,
                                                  const double* __restrict__ Hx, double* __restrict__ A) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnzQ) return;
  double v = 0.0;
  for (int64_t t = qptr[e]; t < qptr[e + 1]; ++t) v += (Jx[qa[t]] * sig[qi[t]]) * Jx[qb[t]];
  if (qh[e] >= 0) v += Hx[qh[e]];
  A[e] = v;
}

// The same sum with the column of Q resident in LDS (eval_J_T_J, eval.jl:85-87; form_system!, schur.jl:55).  A group of 16
// lanes owns column b of Q: for every row i of J that holds column b (ascending: the reference's summation order) the lanes
// stream the CSR segment of row i with columns a >= b -- values contiguous in the CSR-ordered copy -- and add
// (J_ia sig_i) J_ib into the column's accumulator at a precomputed 16-bit slot; the column leaves LDS once, with H added.
// 12 bytes per term (8 value + 2 slot + the per-row scalars) instead of 12 bytes of index lists plus three gathers, and
// the read-modify-write chain of an entry runs in LDS.  Bitwise the same result as kd_assemble_schur.  sacc: the workgroup's
// dynamic LDS, G * maxcol doubles.
__device__ __forceinline__ void kd_assemble_schur_lds(double* sacc, int64_t n, int G, int maxcol, const int64_t* __restrict__ Ap, const int64_t* __restrict__ Jp,
                                                      const int* __restrict__ Ji, const double* __restrict__ Jx, const int64_t* __restrict__ Jrp,
                                                      const double* __restrict__ Jcsr, const int64_t* __restrict__ seg_q,
                                                      const int64_t* __restrict__ seg_t, const uint16_t* __restrict__ tslot,
                                                      const double* __restrict__ sig, const int64_t* __restrict__ qh,
                                                      const double* __restrict__ Hx, double* __restrict__ A) {
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int64_t b = (int64_t)blockIdx.x * G + g;
  if (g >= G || b >= n) return;                  // no workgroup barrier below: a group only talks to itself (one wave)
  double* acc = sacc + (size_t)g * maxcol;
  const int64_t a0 = Ap[b];
  const int ncol = (int)(Ap[b + 1] - a0);
  for (int e = l; e < ncol; e += 16) acc[e] = 0.0;
  __threadfence_block();
  for (int64_t p = Jp[b]; p < Jp[b + 1]; ++p) {
    const int i = Ji[p];
    const double c = sig[i], jb = Jx[p];
    const int64_t q0 = seg_q[p], q1 = Jrp[i + 1], t0 = seg_t[p];
    for (int64_t q = q0 + l; q < q1; q += 16) acc[tslot[t0 + (q - q0)]] += (Jcsr[q] * c) * jb;
    __threadfence_block();                       // the next row may touch the same slots from other lanes of the group
  }
  for (int e = l; e < ncol; e += 16) {
    double v = acc[e];
    const int64_t h = qh[a0 + e];
    if (h >= 0) v += Hx[h];
    A[a0 + e] = v;
  }
}

__device__ __forceinline__ void kd_gather(int64_t n, const int64_t* __restrict__ idx, const double* __restrict__ src, double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}
__device__ __forceinline__ void kd_div(int64_t n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] / b[i];
}

// ---- vector kernels -----------------------------------------------------------------------------
__device__ __forceinline__ void kd_schur_t1(int64_t m, const double* rP, const double* rC, const double* sig, const double* s, double* o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) o[i] = rP[i] * sig[i] + rC[i] / s[i];                 // schur.jl:103
}
__device__ __forceinline__ void kd_sym_rhs(int64_t n, int64_t m, const double* rD, const double* rP, const double* rC, const double* y, double* o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = rD[i];
  else if (i < n + m) o[i] = rP[i - n] + rC[i - n] / y[i - n];       // symmetric.jl:65
}
__device__ __forceinline__ void kd_sym_split(int64_t n, int64_t m, const double* sol, double* dx, double* dy) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dx[i] = sol[i];
  else if (i < n + m) dy[i - n] = -sol[i];                           // symmetric.jl:72-73
}
// system_rhs.jl:57-73 + eval.jl:59-63,136-142
__device__ __forceinline__ void kd_rhs_pc(int64_t m, const double* cons, const double* s, const double* y, double one_minus_P, double mu_target, double* rP, double* rC) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) { rP[i] = -(cons[i] - s[i]) * one_minus_P; rC[i] = mu_target - s[i] * y[i]; }
}

// single-workgroup reduction of 1024 threads (inputs are O(n+m) vectors; deterministic)
__device__ __forceinline__ void kd_reduce(int64_t n, const double* __restrict__ v, int mode /*0 min, 1 max|.|*/, double* out) {
  __shared__ double sh[1024];
  double a = mode == 0 ? INFINITY : 0.0;
  bool nan = false;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const double x = v[i];
    if (x != x) nan = true;
    if (mode == 0) a = fmin(a, x); else a = fmax(a, fabs(x));
  }
  sh[threadIdx.x] = nan ? NAN : a;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double p = sh[threadIdx.x], q = sh[threadIdx.x + o];
      sh[threadIdx.x] = (p != p || q != q) ? NAN : (mode == 0 ? fmin(p, q) : fmax(p, q));
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = n > 0 ? sh[0] : (mode == 0 ? INFINITY : 0.0);
}

// ---- segmented sparse products -----------------------------------------------------------------------------------
// A row (CSR) or column (CSC) of J / H holds 10 - 40 entries at the BASELINE sizes: one thread per row reads its values
// with a stride of a whole row between neighbouring lanes (uncoalesced), one wave per row idles most lanes.  Here a group
// of LPR lanes (4 ... 64, chosen from the average length) owns a row: consecutive groups of a wave own consecutive rows,
// so a wave reads one contiguous run of values and indices; the partial sums meet by xor-shuffles inside the group.
// The summation order is fixed by LPR alone (bitwise reproducible run to run).  No early return before the shuffles:
// rows past the end are clamped and simply not stored.
// skip: the group runs the shuffles of an empty row (a dense row whose dot k_dense_dot has computed)
template <int LPR>
__device__ __forceinline__ double seg_dot(const int64_t* __restrict__ ptr, const int* __restrict__ idx, const double* __restrict__ vals,
                                          const double* __restrict__ x, int64_t row, int sub, bool skip = false) {
  double a = 0.0;
  const int64_t p1 = ptr[row + 1];
  for (int64_t p = skip ? p1 : ptr[row] + sub; p < p1; p += LPR) a += vals[p] * x[idx[p]];
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}
// the dot of row `row` of J: from the segment, or with DR for a row flagged dense (dflag[row] = its index among the dense rows)
// the value k_dense_dot left in dd.  Without DR this is seg_dot itself.
template <int LPR, bool DR>
__device__ __forceinline__ double seg_dot_dr(const int64_t* __restrict__ ptr, const int* __restrict__ idx, const double* __restrict__ vals,
                                             const double* __restrict__ x, int64_t row, int sub, const int* __restrict__ dflag,
                                             const double* __restrict__ dd) {
  if constexpr (!DR) {
    return seg_dot<LPR>(ptr, idx, vals, x, row, sub);
  } else {
    const int t = dflag[row];
    const double a = seg_dot<LPR>(ptr, idx, vals, x, row, sub, t >= 0);
    return t >= 0 ? dd[t] : a;
  }
}
// hess_product (eval.jl:221-234) of row i: (L x)_i + (L' x)_i - diag(L)_i x_i with the lower-stored H in CSR and CSC order
template <int LPR>
__device__ __forceinline__ double seg_hess(const int64_t* __restrict__ Hrp, const int* __restrict__ Hrj, const double* __restrict__ Hcsr,
                                           const int64_t* __restrict__ Hp, const int* __restrict__ Hi, const double* __restrict__ Hx,
                                           const double* __restrict__ Hdiag, const double* __restrict__ x, int64_t i, int sub) {
  const double v1 = seg_dot<LPR>(Hrp, Hrj, Hcsr, x, i, sub);
  const double v2 = seg_dot<LPR>(Hp, Hi, Hx, x, i, sub);
  return (v1 + v2) - Hdiag[i] * x[i];
}
// y = hess_product(x): one group of LPR lanes per row
template <int LPR>
__device__ __forceinline__ void kd_seg_hess(int64_t n, const int64_t* __restrict__ Hrp, const int* __restrict__ Hrj, const double* __restrict__ Hcsr,
                                            const int64_t* __restrict__ Hp, const int* __restrict__ Hi, const double* __restrict__ Hx,
                                            const double* __restrict__ Hdiag, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t i = row < n ? row : n - 1;
  const double h = seg_hess<LPR>(Hrp, Hrj, Hcsr, Hp, Hi, Hx, Hdiag, x, i, sub);
  if (sub == 0 && row < n) y[i] = h;
}
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? NAN : fmax(a, b); }
// per-workgroup maxima of NV values per thread (NaN propagates like Julia's norm(., Inf)); slot v of workgroup b -> part[b * 8 + v]
template <int NV>
__device__ __forceinline__ void block_max_store(double (&v)[NV], double* __restrict__ part) {
  __shared__ double sh[NV][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double a = v[q];
    for (int o = 32; o > 0; o >>= 1) a = nan_max(a, __shfl_xor(a, o, 64));
    if (lane == 0) sh[q][wv] = a;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int q = threadIdx.x;
    part[(size_t)blockIdx.x * 8 + q] = nan_max(nan_max(sh[q][0], sh[q][1]), nan_max(sh[q][2], sh[q][3]));
  }
}

// is_diag_dom (delta_strategy.jl:1-9): margin[i] = 3 Q[i,i] - (sum(Q[:,i]) + sum(Q[i,:])) over the STORED entries of the x-block
// (H lower-stored; the Schur matrix carries the full J' Sigma J on top).  hcol / hrow: column / row sums of the stored H,
// jsj: row sum (= column sum) of J' Sigma J or NULL, qdiag: the block's diagonal without delta.  NaN compares false in Julia.
__device__ __forceinline__ void kd_diag_dom_margin(int64_t n, const double* __restrict__ hcol, const double* __restrict__ hrow, const double* __restrict__ jsj,
                                                   const double* __restrict__ qdiag, double delta, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = qdiag[i] + delta;
  const double cs = hcol[i] + (jsj ? jsj[i] : 0.0) + delta, rs = hrow[i] + (jsj ? jsj[i] : 0.0) + delta;
  const double v = 3.0 * d - (cs + rs);
  out[i] = (v != v) ? 1.0e308 : v;
}

// y[i] = dot_i (* scale[i]) (+ beta * addv[i]): J x, J' v, Sigma .* (J x), rD + J' t, J dx - rP
// DR: rows of J flagged dense take their dot from dd (k_dense_dot) instead of their own segment
template <int LPR, bool DR>
__device__ __forceinline__ void kd_seg_spmv(int64_t nrows, const int64_t* __restrict__ ptr, const int* __restrict__ idx,
                                            const double* __restrict__ vals, const double* __restrict__ x, const double* __restrict__ scale,
                                            const double* __restrict__ addv, double beta, double* __restrict__ y,
                                            const int* __restrict__ dflag, const double* __restrict__ dd) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t rc = row < nrows ? row : nrows - 1;
  double r = seg_dot_dr<LPR, DR>(ptr, idx, vals, x, rc, sub, dflag, dd);
  if (sub == 0 && row < nrows) {
    if (scale) r *= scale[row];
    if (addv) r = r + beta * addv[row];
    y[row] = r;
  }
}
// res = rhs - (J' v + (H dx + delta dx)) with v = Sigma .* (J dx) (schur.jl:166-170): one pass instead of J' v, H dx and
// the vector kernel
template <int LPR>
__device__ __forceinline__ void kd_schur_resid(int64_t n, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, const double* __restrict__ Jx,
                                               const double* __restrict__ v, const int64_t* __restrict__ Hrp, const int* __restrict__ Hrj,
                                               const double* __restrict__ Hcsr, const int64_t* __restrict__ Hp, const int* __restrict__ Hi,
                                               const double* __restrict__ Hx, const double* __restrict__ Hdiag, const double* __restrict__ dx,
                                               const double* __restrict__ rhs, double delta, double* __restrict__ res) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t i = row < n ? row : n - 1;
  const double jac = seg_dot<LPR>(Jp, Ji, Jx, v, i, sub);
  const double hx = seg_hess<LPR>(Hrp, Hrj, Hcsr, Hp, Hi, Hx, Hdiag, dx, i, sub);
  if (sub == 0 && row < n) res[i] = rhs[i] - (jac + (hx + delta * dx[i]));
}
// dy, ds from J dx (schur.jl:113-116); direct = 1: ds = (comp_r - dy .* s) ./ y (schur_direct.jl:54-56), y, s, sig of the CURRENT iterate
template <int LPR, bool DR>
__device__ __forceinline__ void kd_schur_dyds(int64_t m, const int64_t* __restrict__ Jrp, const int* __restrict__ Jrj, const double* __restrict__ Jcsr,
                                              const double* __restrict__ dx, const double* __restrict__ rP, const double* __restrict__ rC,
                                              const double* __restrict__ y, const double* __restrict__ s, const double* __restrict__ sig, int direct,
                                              double* __restrict__ dy, double* __restrict__ ds, const int* __restrict__ dflag,
                                              const double* __restrict__ dd) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t i = row < m ? row : m - 1;
  const double Jdx = seg_dot_dr<LPR, DR>(Jrp, Jrj, Jcsr, dx, i, sub, dflag, dd);
  if (sub == 0 && row < m) {
    const double dyi = -(Jdx - (rP[i] + rC[i] / y[i])) * sig[i];
    dy[i] = dyi;
    ds[i] = direct ? (rC[i] - dyi * s[i]) / y[i] : Jdx - rP[i];
  }
}
// update_kkt_error! (kkt_system_solver.jl:27-47,67-96), dual block: |predicted_lag_change - dual_r| and |dual_r|, maxima per workgroup
template <int LPR>
__device__ __forceinline__ void kd_err_dual(int64_t n, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, const double* __restrict__ Jx,
                                            const double* __restrict__ dy, const int64_t* __restrict__ Hrp, const int* __restrict__ Hrj,
                                            const double* __restrict__ Hcsr, const int64_t* __restrict__ Hp, const int* __restrict__ Hi,
                                            const double* __restrict__ Hx, const double* __restrict__ Hdiag, const double* __restrict__ dx,
                                            const double* __restrict__ rD, double delta, double* __restrict__ part) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t i = row < n ? row : n - 1;
  const double jty = seg_dot<LPR>(Jp, Ji, Jx, dy, i, sub);
  const double hx = seg_hess<LPR>(Hrp, Hrj, Hcsr, Hp, Hi, Hx, Hdiag, dx, i, sub);
  double v[2] = {0.0, 0.0};
  if (sub == 0 && row < n) {
    v[0] = fabs(((delta * dx[i] + 0.0) + hx - jty) - rD[i]);
    v[1] = fabs(rD[i]);
  }
  block_max_store<2>(v, part);
}
// primal and complementarity blocks: |J dx - ds - primal_r|, |s dy + y ds - comp_r|, |primal_r|, |comp_r|
template <int LPR, bool DR>
__device__ __forceinline__ void kd_err_pc(int64_t m, const int64_t* __restrict__ Jrp, const int* __restrict__ Jrj, const double* __restrict__ Jcsr,
                                          const double* __restrict__ dx, const double* __restrict__ ds, const double* __restrict__ dy,
                                          const double* __restrict__ s, const double* __restrict__ y, const double* __restrict__ rP,
                                          const double* __restrict__ rC, double* __restrict__ part, const int* __restrict__ dflag,
                                          const double* __restrict__ dd) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t i = row < m ? row : m - 1;
  const double Jdx = seg_dot_dr<LPR, DR>(Jrp, Jrj, Jcsr, dx, i, sub, dflag, dd);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (sub == 0 && row < m) {
    v[0] = fabs(Jdx - ds[i] - rP[i]);
    v[1] = fabs(s[i] * dy[i] + y[i] * ds[i] - rC[i]);
    v[2] = fabs(rP[i]);
    v[3] = fabs(rC[i]);
  }
  block_max_store<4>(v, part);
}
// the six norms: out[0..1] from the nbD dual partial rows, out[2..5] from the nbM rows behind them (one workgroup of 256)
__device__ __forceinline__ void kd_err_final(int64_t nbD, int64_t nbM, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double sh[6][256];
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nbD; b += 256) { a[0] = nan_max(a[0], part[b * 8]); a[1] = nan_max(a[1], part[b * 8 + 1]); }
  for (int64_t b = threadIdx.x; b < nbM; b += 256)
    for (int q = 0; q < 4; ++q) a[2 + q] = nan_max(a[2 + q], part[(nbD + b) * 8 + q]);
  for (int q = 0; q < 6; ++q) sh[q][threadIdx.x] = a[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 6; ++q) sh[q][threadIdx.x] = nan_max(sh[q][threadIdx.x], sh[q][threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x < 6) out[threadIdx.x] = sh[threadIdx.x][0];
}
// System_rhs, dual block (system_rhs.jl:57-73 + eval.jl:59-63,136-142): J' y and J' 1 in one pass over the column
template <int LPR>
__device__ __forceinline__ void kd_rhs_dual_seg(int64_t n, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, const double* __restrict__ Jx,
                                                const double* __restrict__ y, const double* __restrict__ grad, double mu_pen, double one_minus_D,
                                                double* __restrict__ o) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t i = row < n ? row : n - 1;
  double jty = 0.0, jt1 = 0.0;
  const int64_t p1 = Jp[i + 1];
  for (int64_t p = Jp[i] + sub; p < p1; p += LPR) { const double a = Jx[p]; jty += a * y[Ji[p]]; jt1 += a; }
#pragma unroll
  for (int q = LPR / 2; q > 0; q >>= 1) { jty += __shfl_xor(jty, q, 64); jt1 += __shfl_xor(jt1, q, 64); }
  if (sub == 0 && row < n) o[i] = -((grad[i] - jty) + mu_pen * jt1) * one_minus_D;
}
// schur_diag = diag(H) + sum_i J_ij^2 sig_i (kkt_system_solver.jl:296-300, eval.jl:89-100)
template <int LPR>
__device__ __forceinline__ void kd_schur_diag_seg(int64_t n, const int64_t* __restrict__ Jp, const int* __restrict__ Ji, const double* __restrict__ Jx,
                                                  const double* __restrict__ sig, const double* __restrict__ Hdiag, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t j = row < n ? row : n - 1;
  double di = 0.0;
  const int64_t p1 = Jp[j + 1];
  for (int64_t p = Jp[j] + sub; p < p1; p += LPR) di += Jx[p] * Jx[p] * sig[Ji[p]];
#pragma unroll
  for (int q = LPR / 2; q > 0; q >>= 1) di += __shfl_xor(di, q, 64);
  if (sub == 0 && row < n) out[j] = Hdiag[j] + di;
}
// values of J and H in CSR order, Sigma = y ./ s and diag(H), in one launch behind the uploads of form_system
__device__ __forceinline__ void kd_form_prep(int64_t nnzJ, int64_t nnzH, int64_t n, int64_t m, const double* __restrict__ Jx, const int64_t* __restrict__ Jrmap,
                                             const double* __restrict__ Hx, const int64_t* __restrict__ Hrmap, const int64_t* __restrict__ Hp, const int* __restrict__ Hi,
                                             const double* __restrict__ s, const double* __restrict__ y, double* __restrict__ Jcsr, double* __restrict__ Hcsr,
                                             double* __restrict__ Hdiag, double* __restrict__ sig) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nnzJ) Jcsr[t] = Jx[Jrmap[t]];
  if (t < nnzH) Hcsr[t] = Hx[Hrmap[t]];
  if (t < m) sig[t] = y[t] / s[t];
  if (t < n) {
    double v = 0.0;
    for (int64_t p = Hp[t]; p < Hp[t + 1]; ++p) if (Hi[p] == t) v += Hx[p];
    Hdiag[t] = v;
  }
}

}  // namespace okkt
