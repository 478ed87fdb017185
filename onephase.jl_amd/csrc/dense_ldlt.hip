// Dense symmetric-indefinite factorisation of the Schur complement, blocked and right-looking, and the substitutions with its factor
// (DESIGN.md section 8.7).  P S P' = L D L', Bunch-Kaufman partial pivoting as in LAPACK's dsytrf / dlasyf, lower variant.
//
// Layout.  F is ns x ns column-major and holds, below the diagonal, the unit L with every interchange applied to every column (one
// global P: what a blocked substitution needs), D on the diagonal (a 2 x 2 block keeps its off-diagonal entry at (k + 1, k), where L is
// zero).  okkt_schur_get_factor undoes the later interchanges column by column to hand out dsytrf's own layout.
//
// One panel = one launch of k_dl_panel (ONE workgroup: the pivot search is a chain of dependent column steps) + one launch of
// k_dl_trail (FP64 MFMA on the lower-triangle tiles behind the panel).  How many columns a panel eliminated is decided on the device
// (a panel stops one column early rather than split a 2 x 2 pivot), so the launches read their column range from DenseLdltState and
// the host enqueues the largest number of panels there can be; launches past the end return at once.  No atomics, no grid barrier:
// the same input gives the same bits.
#include "dense_ldlt.h"

#include <algorithm>
#include <cassert>

namespace okkt {

#define OKKT_HIP_TRY(expr)                                                         \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess)                                                         \
      return std::string(#expr) + ": " + hipGetErrorString(e__);                   \
  } while (0)

namespace {

constexpr int kPanelThreads = 1024;
constexpr int kPanelWaves = kPanelThreads / 64;

// max of v over the workgroup and the smallest index that attains it (idamax's rule); every thread returns the same pair
__device__ __forceinline__ void wg_argmax(double& v, int& idx, double* s_v, int* s_i) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(idx, o);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();      // the previous use of s_v / s_i has been read
  if ((threadIdx.x & 63) == 0) { s_v[wave] = v; s_i[wave] = idx; }
  __syncthreads();
  v = s_v[0]; idx = s_i[0];
  for (int w = 1; w < kPanelWaves; ++w) {
    const double ov = s_v[w];
    const int oi = s_i[w];
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
}

// The panel in the dlasyf form.  Column k of the trailing matrix (up to date against the earlier panels) is brought up to date
// against this panel's earlier columns into W(:, kw); the largest off-diagonal entry decides between a 1 x 1 pivot in place, and --
// after the row / column of that entry has been brought up to date into W(:, kw + 1) -- a 1 x 1 pivot there or the 2 x 2 pivot of the
// two.  The row W(k, 0 : kw) that every row's update multiplies is staged in LDS; W itself (panel height x kDlNB) is in memory, where
// k_dl_trail reads it.
__global__ __launch_bounds__(kPanelThreads) void k_dl_panel(double* F, int n, double* W, int* ipiv, int* ptype, int* perm, DenseLdltState* st) {
  __shared__ double s_row[kDlNB];
  __shared__ double s_v[kPanelWaves];
  __shared__ int s_i[kPanelWaves];
  const int tid = threadIdx.x;
  const int j0 = st->next;
  if (j0 >= n) return;
  const size_t ld = (size_t)n;
  const bool last = n - j0 <= kDlNB;      // the rest fits one panel: every column is eliminated
  const double alpha = (1.0 + sqrt(17.0)) / 8.0;
  long long c_pos = 0, c_neg = 0, c_zero = 0, c_bad = 0;      // thread 0's
  int k = j0;
  while (last ? k < n : k < j0 + kDlNB - 1) {
    const int kw = k - j0;
    double* Wk = W + (size_t)kw * ld;
    double* Wk1 = Wk + ld;
    __syncthreads();
    if (tid < kw) s_row[tid] = W[(size_t)tid * ld + k];
    __syncthreads();
    double cv = -1.0;
    int ci = n;
    for (int i = k + tid; i < n; i += kPanelThreads) {
      double w = F[(size_t)k * ld + i];
      for (int j = 0; j < kw; ++j) w = fma(-F[(size_t)(j0 + j) * ld + i], s_row[j], w);
      Wk[i] = w;
      const double a = fabs(w);
      if (i > k && a > cv) { cv = a; ci = i; }
    }
    wg_argmax(cv, ci, s_v, s_i);      // (its barriers also publish Wk)
    const double colmax = cv < 0.0 ? 0.0 : cv;
    const int imax = ci;
    const double akk = Wk[k];
    const double absakk = fabs(akk);
    int kstep = 1, kp = k;
    bool zero = false;
    if (!(absakk == absakk) || !(absakk <= 1.79769313486231570815e308)) {
      kp = k;      // non-finite pivot: eliminated in place, counted as such
    } else if (fmax(absakk, colmax) == 0.0) {
      zero = true;      // the column is exactly zero: nothing to eliminate (dsytf2)
    } else if (absakk >= alpha * colmax) {
      kp = k;
    } else {
      __syncthreads();
      if (tid < kw) s_row[tid] = W[(size_t)tid * ld + imax];
      __syncthreads();
      double rv = -1.0;
      int ri = n;
      for (int i = k + tid; i < n; i += kPanelThreads) {
        double w = i < imax ? F[(size_t)i * ld + imax] : F[(size_t)imax * ld + i];
        for (int j = 0; j < kw; ++j) w = fma(-F[(size_t)(j0 + j) * ld + i], s_row[j], w);
        Wk1[i] = w;
        const double a = fabs(w);
        if (i != imax && a > rv) { rv = a; ri = i; }
      }
      wg_argmax(rv, ri, s_v, s_i);
      const double rowmax = rv < 0.0 ? 0.0 : rv;
      if (absakk >= alpha * colmax * (colmax / rowmax)) {
        kp = k;
      } else if (fabs(Wk1[imax]) >= alpha * rowmax) {
        kp = imax;
        __syncthreads();
        for (int i = k + tid; i < n; i += kPanelThreads) Wk[i] = Wk1[i];
      } else {
        kp = imax;
        kstep = 2;
      }
    }
    const int kk = k + kstep - 1;
    __syncthreads();
    if (kp != kk) {
      // the column kk that has not been brought up to date moves to position kp; rows kk and kp change places in every column of L
      // and in W
      if (tid == 0) F[(size_t)kp * ld + kp] = F[(size_t)kk * ld + kk];
      for (int i = kk + 1 + tid; i < kp; i += kPanelThreads) F[(size_t)i * ld + kp] = F[(size_t)kk * ld + i];
      for (int i = kp + 1 + tid; i < n; i += kPanelThreads) F[(size_t)kp * ld + i] = F[(size_t)kk * ld + i];
      for (int c = tid; c < k; c += kPanelThreads) {
        const double t = F[(size_t)c * ld + kk];
        F[(size_t)c * ld + kk] = F[(size_t)c * ld + kp];
        F[(size_t)c * ld + kp] = t;
      }
      if (tid <= kk - j0) {
        const double t = W[(size_t)tid * ld + kk];
        W[(size_t)tid * ld + kk] = W[(size_t)tid * ld + kp];
        W[(size_t)tid * ld + kp] = t;
      }
      if (tid == 0) { const int t = perm[kk]; perm[kk] = perm[kp]; perm[kp] = t; }
      __syncthreads();
    }
    if (kstep == 1) {
      const double d = Wk[k];
      const double r1 = 1.0 / d;
      for (int i = k + tid; i < n; i += kPanelThreads) {
        const double w = Wk[i];
        F[(size_t)k * ld + i] = (i == k || zero) ? w : w * r1;
      }
      if (tid == 0) {
        ipiv[k] = kp + 1;
        ptype[k] = 0;
        if (zero) ++c_zero;
        else if (!(fabs(d) <= 1.79769313486231570815e308)) ++c_bad;
        else if (d > 0.0) ++c_pos;
        else ++c_neg;
      }
    } else {
      const double w21 = Wk[k + 1], w11 = Wk[k], w22 = Wk1[k + 1];
      const double d11 = w22 / w21, d22 = w11 / w21;
      const double t = 1.0 / (d11 * d22 - 1.0);
      const double d21 = t / w21;
      for (int i = k + 2 + tid; i < n; i += kPanelThreads) {
        const double a = Wk[i], b = Wk1[i];
        F[(size_t)k * ld + i] = d21 * (d11 * a - b);
        F[(size_t)(k + 1) * ld + i] = d21 * (d22 * b - a);
      }
      if (tid == 0) {
        F[(size_t)k * ld + k] = w11;
        F[(size_t)k * ld + k + 1] = w21;
        F[(size_t)(k + 1) * ld + k + 1] = w22;
        ipiv[k] = ipiv[k + 1] = -(kp + 1);
        ptype[k] = 1;
        ptype[k + 1] = 2;
        const double det = w11 * w22 - w21 * w21;
        if (!(fabs(det) <= 1.79769313486231570815e308)) c_bad += 2;
        else {
#ifdef OKKT_DL_DEBUG
          assert(det < 0.0);      // |w11 w22| < alpha^2 w21^2 by the two tests that failed: one pivot of each sign
#endif
          ++c_pos;
          ++c_neg;
        }
      }
    }
    k += kstep;
  }
  __syncthreads();
  if (tid == 0) {
    st->j0 = j0;
    st->next = k;
    st->cnt[0] += c_pos;
    st->cnt[1] += c_neg;
    st->cnt[2] += c_zero;
    st->cnt[3] += c_bad;
  }
}

// Trailing update S22 <- S22 - L21 W21' behind the panel [j0, j1): one workgroup per 64 x 64 tile of the lower triangle, counted from
// j1; wave w owns the 16 rows 16 w .. 16 w + 15 of the tile and its (up to) four 16 x 16 blocks at or below the diagonal.
// v_mfma_f64_16x16x4: lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and the results [(l >> 4) + 4 r][l & 15], r = 0..3.  The k
// loop runs over the panel's columns in one fixed order.
__global__ __launch_bounds__(256) void k_dl_trail(double* F, int n, const double* __restrict__ W, const DenseLdltState* st) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  const int j0 = st->j0, j1 = st->next;
  if (j1 >= n) return;
  const int kb = j1 - j0;
  const size_t ld = (size_t)n;
  const int64_t b = blockIdx.x;
  int ti = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((int64_t)ti * (ti + 1) / 2 > b) --ti;
  while ((int64_t)(ti + 1) * (ti + 2) / 2 <= b) ++ti;
  const int tj = (int)(b - (int64_t)ti * (ti + 1) / 2);
  const int64_t i0 = (int64_t)j1 + (int64_t)ti * 64, c0 = (int64_t)j1 + (int64_t)tj * 64;
  if (i0 >= n) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int64_t arow = i0 + 16 * wave + l15;
  const int nsub = ti == tj ? wave + 1 : 4;      // blocks above the tile's diagonal are not stored
  v4d acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t col = c0 + 16 * s + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = i0 + 16 * wave + l4 + 4 * r;
      acc[s][r] = (s < nsub && row < n && col < n && row >= col) ? F[(size_t)col * ld + row] : 0.0;
    }
  }
  for (int kq = 0; kq < kb; kq += 4) {
    const int kx = kq + l4;
    const bool kin = kx < kb;
    const double a = (kin && arow < n) ? -F[(size_t)(j0 + kx) * ld + arow] : 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < nsub) {
        const int64_t col = c0 + 16 * s + l15;
        const double bv = (kin && col < n) ? W[(size_t)kx * ld + col] : 0.0;
        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[s], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t col = c0 + 16 * s + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = i0 + 16 * wave + l4 + 4 * r;
      if (s < nsub && row < n && col < n && row >= col) F[(size_t)col * ld + row] = acc[s][r];
    }
  }
}

__global__ __launch_bounds__(256) void k_dl_init(int n, int* perm, DenseLdltState* st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) perm[i] = i;
  if (i == 0) {
    st->next = 0;
    st->j0 = 0;
    st->cnt[0] = st->cnt[1] = st->cnt[2] = st->cnt[3] = 0;
  }
}

// ---- substitutions ---------------------------------------------------------------------------------------------------------------
// L(i, c) of the solves: the stored entry, except that (k + 1, k) inside a 2 x 2 pivot holds D's off-diagonal entry and L is zero there
__device__ __forceinline__ double l_entry(const double* __restrict__ F, const int* __restrict__ ptype, size_t ld, int i, int c) {
  const double v = F[(size_t)c * ld + i];
  return (i == c + 1 && ptype[c] == 1) ? 0.0 : v;
}

template <int R>
__global__ __launch_bounds__(256) void k_dl_perm_in(int n, int nr, const int* __restrict__ perm, const double* __restrict__ r2, double* __restrict__ X) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = perm[i];
#pragma unroll
  for (int q = 0; q < R; ++q) X[(size_t)q * n + i] = q < nr ? r2[(size_t)q * n + p] : 0.0;
}
template <int R>
__global__ __launch_bounds__(256) void k_dl_perm_out(int n, int nr, const int* __restrict__ perm, const double* __restrict__ Y, double* __restrict__ x2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = perm[i];
#pragma unroll
  for (int q = 0; q < R; ++q) if (q < nr) x2[(size_t)q * n + p] = Y[(size_t)q * n + i];
}

// Forward block step on the columns [b0, b0 + bw): every workgroup stages the diagonal block in LDS and solves it (wave 0, one row
// per lane, the solved entries passed by lane reads); workgroup 0 stores the block's y into Y, workgroup g >= 1 takes it off the 64
// rows b0 + bw + 64 (g - 1) .. of X -- four groups of 16 columns per row, summed in a fixed order.  X's entries of the block itself
// are only read, so the redundant solves see the same input.
template <int R>
__global__ __launch_bounds__(256) void k_dl_fwd(const double* __restrict__ F, int n, const int* __restrict__ ptype, int b0, double* X, double* Y) {
  __shared__ double Ls[kDlSB][kDlSB + 1];      // Ls[c][i] = L(b0 + i, b0 + c)
  __shared__ double ys[R][kDlSB];
  __shared__ double part[4][R][kDlSB];
  const size_t ld = (size_t)n;
  const int bw = min(kDlSB, n - b0), b1 = b0 + bw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = wave; c < kDlSB; c += 4) Ls[c][lane] = (c < bw && lane < bw && lane > c) ? l_entry(F, ptype, ld, b0 + lane, b0 + c) : 0.0;
  __syncthreads();
  if (wave == 0) {
    double x[R];
#pragma unroll
    for (int q = 0; q < R; ++q) x[q] = lane < bw ? X[(size_t)q * n + b0 + lane] : 0.0;
    for (int c = 0; c < bw; ++c) {
      const double l = Ls[c][lane];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const double yc = __shfl(x[q], c);
        x[q] = fma(-l, yc, x[q]);      // l = 0 for the rows at and above c
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      ys[q][lane] = x[q];
      if (blockIdx.x == 0 && lane < bw) Y[(size_t)q * n + b0 + lane] = x[q];
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) return;
  const int64_t row = (int64_t)b1 + (int64_t)(blockIdx.x - 1) * 64 + lane;
  double s[R];
#pragma unroll
  for (int q = 0; q < R; ++q) s[q] = 0.0;
  if (row < n) {
    for (int c = 16 * wave; c < min(16 * wave + 16, bw); ++c) {
      const double l = l_entry(F, ptype, ld, (int)row, b0 + c);
#pragma unroll
      for (int q = 0; q < R; ++q) s[q] = fma(l, ys[q][c], s[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < R; ++q) part[wave][q][lane] = s[q];
  __syncthreads();
  if (wave == 0 && row < n) {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      double x = X[(size_t)q * n + row];
      x -= part[0][q][lane];
      x -= part[1][q][lane];
      x -= part[2][q][lane];
      x -= part[3][q][lane];
      X[(size_t)q * n + row] = x;
    }
  }
}

// the block-diagonal solve, one thread per pivot block (dsytrs' formulas for the 2 x 2 blocks): X = D^-1 Y
template <int R>
__global__ __launch_bounds__(256) void k_dl_diag(const double* __restrict__ F, int n, const int* __restrict__ ptype, const double* __restrict__ Y, double* __restrict__ X) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const size_t ld = (size_t)n;
  const int t = ptype[k];
  if (t == 2) return;
  if (t == 0) {
    const double d = F[(size_t)k * ld + k];
#pragma unroll
    for (int q = 0; q < R; ++q) X[(size_t)q * n + k] = Y[(size_t)q * n + k] / d;
    return;
  }
  const double akm1k = F[(size_t)k * ld + k + 1];
  const double akm1 = F[(size_t)k * ld + k] / akm1k, ak = F[(size_t)(k + 1) * ld + k + 1] / akm1k;
  const double denom = akm1 * ak - 1.0;
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const double bkm1 = Y[(size_t)q * n + k] / akm1k, bk = Y[(size_t)q * n + k + 1] / akm1k;
    X[(size_t)q * n + k] = (ak * bkm1 - bk) / denom;
    X[(size_t)q * n + k + 1] = (akm1 * bk - bkm1) / denom;
  }
}

// Backward block step on the columns [b0, b0 + bw), whose entries of X already carry the later blocks' terms: every workgroup solves
// the block with L', workgroup 0 stores its x into Y, workgroup g >= 1 takes L(block rows, c)' x off the 64 columns c = 64 (g - 1) ..
// before the block -- one wave per column, lanes over the block's rows, summed by a fixed butterfly.
template <int R>
__global__ __launch_bounds__(256) void k_dl_bwd(const double* __restrict__ F, int n, const int* __restrict__ ptype, int b0, double* X, double* Y) {
  __shared__ double Ls[kDlSB][kDlSB + 1];      // Ls[c][i] = L(b0 + c, b0 + i)
  __shared__ double xs[R][kDlSB];
  const size_t ld = (size_t)n;
  const int bw = min(kDlSB, n - b0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = wave; i < kDlSB; i += 4) Ls[lane][i] = (i < bw && lane < bw && lane > i) ? l_entry(F, ptype, ld, b0 + lane, b0 + i) : 0.0;
  __syncthreads();
  if (wave == 0) {
    double x[R];
#pragma unroll
    for (int q = 0; q < R; ++q) x[q] = lane < bw ? X[(size_t)q * n + b0 + lane] : 0.0;
    for (int c = bw - 1; c >= 0; --c) {
      const double l = Ls[c][lane];      // L(b0 + c, b0 + lane): 0 for lane >= c
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const double xc = __shfl(x[q], c);
        x[q] = fma(-l, xc, x[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      xs[q][lane] = x[q];
      if (blockIdx.x == 0 && lane < bw) Y[(size_t)q * n + b0 + lane] = x[q];
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) return;
  double xv[R];
#pragma unroll
  for (int q = 0; q < R; ++q) xv[q] = xs[q][lane];      // 0 beyond bw
  for (int t = 0; t < 16; ++t) {
    const int col = (blockIdx.x - 1) * 64 + wave + 4 * t;      // wave-uniform
    if (col >= b0) break;
    const double l = lane < bw ? l_entry(F, ptype, ld, b0 + lane, col) : 0.0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      double s = l * xv[q];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) X[(size_t)q * n + col] -= s;
    }
  }
}

template <int R>
std::string solve_r(DenseLdltWork& D, const double* d_r2, double* d_x2, int nr, hipStream_t st) {
  const int n = (int)D.ns;
  double* X = D.X;
  double* Y = D.X + (size_t)4 * D.ns;
  const dim3 gv((n + 255) / 256), bv(256);
  hipLaunchKernelGGL(k_dl_perm_in<R>, gv, bv, 0, st, n, nr, D.perm, d_r2, X);
  const int nblk = (n + kDlSB - 1) / kDlSB;
  for (int b = 0; b < nblk; ++b) {
    const int b0 = b * kDlSB, b1 = std::min(n, b0 + kDlSB);
    hipLaunchKernelGGL(k_dl_fwd<R>, dim3(1 + (n - b1 + 63) / 64), dim3(256), 0, st, D.F, n, D.ptype, b0, X, Y);
  }
  hipLaunchKernelGGL(k_dl_diag<R>, gv, bv, 0, st, D.F, n, D.ptype, Y, X);
  for (int b = nblk - 1; b >= 0; --b) {
    const int b0 = b * kDlSB;
    hipLaunchKernelGGL(k_dl_bwd<R>, dim3(1 + (b0 + 63) / 64), dim3(256), 0, st, D.F, n, D.ptype, b0, X, Y);
  }
  hipLaunchKernelGGL(k_dl_perm_out<R>, gv, bv, 0, st, n, nr, D.perm, Y, d_x2);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

// ---- the inverse ------------------------------------------------------------------------------------------
// Zt = (P S P')^-1 = L^-T D^-1 L^-1 by the recurrence of selected inversion (selinv.hip) on the dense factor as one front: the blocks
// of kDlIB columns from the last to the first, for block j (columns c0 .. j1, the rows below it B = j1 .. n)
//   W_j = L_Bj L_jj^-1,   Z_Bj = - Z_BB W_j,   Z_jj = L_jj^-T D_j^-1 L_jj^-1 - W_j' Z_Bj.
// Every entry is computed once, in the lower triangle, and stored at both places, so the two triangles are the same bits.  Three
// launches per block step (k_dli_block, k_dli_cols, k_dli_diag); where the blocks begin depends on the 2 x 2 pivots, so a launch reads
// its block from the list k_dli_plan made and the host enqueues the largest number of steps there can be.  Fixed summation orders,
// no floating-point atomics: the same factor gives the same bits.

__global__ void k_dli_plan(int n, const int* __restrict__ ptype, int* __restrict__ blk, unsigned long long* __restrict__ nonfinite) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int nb = 0, c = 0;
  while (c < n) {
    blk[1 + nb++] = c;
    int e = min(n, c + kDlIB);
    if (e < n && ptype[e - 1] == 1) --e;      // the 2 x 2 pivot (e - 1, e) opens the next block
    c = e;
  }
  blk[1 + nb] = n;
  blk[0] = nb;
  *nonfinite = 0ull;
}

// Every workgroup inverts L_jj in LDS.  Workgroup 0 stores L_jj^-T D_j^-1 L_jj^-1 (lower triangle) into Zt; workgroup g >= 1 the 256
// rows j1 + 256 (g - 1) .. of W_j, one row per thread, into Wt (row-major, kDlIB entries per row, zeros beyond the block's width).
__global__ __launch_bounds__(256) void k_dli_block(const double* __restrict__ F, int n, const int* __restrict__ ptype, const int* __restrict__ blk, int j,
                                                   double* __restrict__ Zt, double* __restrict__ Wt) {
  __shared__ double Lb[kDlIB][kDlIB + 1];
  __shared__ double Li[kDlIB][kDlIB + 1];
  __shared__ double Ms[kDlIB][kDlIB + 1];
  __shared__ double dd[kDlIB], od[kDlIB];
  __shared__ int pt[kDlIB];
  if (j >= blk[0]) return;
  const int c0 = blk[1 + j], j1 = blk[2 + j], w = j1 - c0;
  const size_t ld = (size_t)n;
  const int tid = threadIdx.x;
  if (blockIdx.x > 0 && (int64_t)j1 + (int64_t)(blockIdx.x - 1) * 256 >= n) return;
  for (int e = tid; e < kDlIB * kDlIB; e += 256) {
    const int x = e % kDlIB, y = e / kDlIB;
    Lb[x][y] = (x < w && y < x) ? l_entry(F, ptype, ld, c0 + x, c0 + y) : 0.0;
    Li[x][y] = (x == y && x < w) ? 1.0 : 0.0;
  }
  __syncthreads();
  // unit lower inverse, row by row: Li[x][y] = - sum_{y <= t < x} Lb[x][t] Li[t][y]
  for (int x = 1; x < w; ++x) {
    if (tid < x) {
      double s = 0.0;
      for (int t = tid; t < x; ++t) s += Lb[x][t] * Li[t][tid];
      Li[x][tid] = -s;
    }
    __syncthreads();
  }
  if (blockIdx.x == 0) {
    // D_j^-1, row t: dd[t] on the diagonal, od[t] at the partner pt[t] of a 2 x 2 pivot (dsytri's scaled formulas)
    if (tid < w) {
      const int k = c0 + tid, ty = ptype[k];
      if (ty == 0) {
        dd[tid] = 1.0 / F[(size_t)k * ld + k];
        od[tid] = 0.0;
        pt[tid] = tid;
      } else {
        const int k0 = ty == 1 ? k : k - 1;
        const double b = F[(size_t)k0 * ld + k0 + 1];
        const double t = fabs(b);
        const double ak = F[(size_t)k0 * ld + k0] / t, akp1 = F[(size_t)(k0 + 1) * ld + k0 + 1] / t, akkp1 = b / t;
        const double d = t * (ak * akp1 - 1.0);
        dd[tid] = (ty == 1 ? akp1 : ak) / d;
        od[tid] = -akkp1 / d;
        pt[tid] = ty == 1 ? tid + 1 : tid - 1;
      }
    }
    __syncthreads();
    for (int e = tid; e < kDlIB * kDlIB; e += 256) {
      const int t = e % kDlIB, y = e / kDlIB;
      Ms[t][y] = t < w ? dd[t] * Li[t][y] + od[t] * Li[pt[t]][y] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < kDlIB * kDlIB; e += 256) {
      const int x = e % kDlIB, y = e / kDlIB;
      if (x >= w || y > x) continue;
      double s = 0.0;
      for (int t = x; t < w; ++t) s += Li[t][x] * Ms[t][y];
      Zt[(size_t)(c0 + y) * ld + c0 + x] = s;
    }
    return;
  }
  const int64_t x = (int64_t)j1 + (int64_t)(blockIdx.x - 1) * 256 + tid;
  if (x >= n) return;
  double acc[kDlIB];
#pragma unroll
  for (int c = 0; c < kDlIB; ++c) acc[c] = 0.0;
  for (int t = 0; t < w; ++t) {
    const double l = F[(size_t)(c0 + t) * ld + x];
#pragma unroll
    for (int c = 0; c < kDlIB; ++c) acc[c] += l * Li[t][c];
  }
  double* wr = Wt + (size_t)(x - j1) * kDlIB;
#pragma unroll
  for (int c = 0; c < kDlIB; ++c) wr[c] = acc[c];
}

// Z_Bj = - Z_BB W_j, one workgroup per 16 rows of B.  The kDliWaves waves share the sum over B's rows y (wave v takes the groups of
// four rows 4 q .., q = v mod kDliWaves) on v_mfma_f64_16x16x4 (operand and result layout: k_dl_trail); their partial sums are added in
// wave order.  The workgroup then leaves its rows' part of W_j' Z_Bj (kDlIB x kDlIB) in Pt for k_dli_diag.
constexpr int kDliWaves = 8;
__global__ __launch_bounds__(64 * kDliWaves) void k_dli_cols(int n, const int* __restrict__ blk, int j, double* Zt, const double* __restrict__ Wt,
                                                             double* __restrict__ Pt) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  __shared__ double part[kDliWaves][2][4][64];
  __shared__ double Zs[16][kDlIB + 1];
  __shared__ double Ws[16][kDlIB + 1];
  if (j >= blk[0]) return;
  const int c0 = blk[1 + j], j1 = blk[2 + j], w = j1 - c0;
  const int64_t x0 = (int64_t)j1 + (int64_t)blockIdx.x * 16;
  if (x0 >= n) return;
  const size_t ld = (size_t)n;
  const int m = n - j1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int64_t arow = x0 + l15;
  v4d acc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s][r] = 0.0;
  for (int q = wave; 4 * q < m; q += kDliWaves) {
    const int yl = 4 * q + l4;
    const bool yin = yl < m;
    const double a = (yin && arow < n) ? Zt[(size_t)(j1 + yl) * ld + arow] : 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double bv = yin ? Wt[(size_t)yl * kDlIB + 16 * s + l15] : 0.0;
      acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[s], 0, 0, 0);
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][s][r][lane] = acc[s][r];
  {
    const int xl = tid >> 5, c = tid & 31;      // 16 x kDlIB entries of W_j, one per thread
    Ws[xl][c] = x0 + xl < n ? Wt[(size_t)(x0 + xl - j1) * kDlIB + c] : 0.0;
  }
  __syncthreads();
  {
    const int ln = tid & 63, r = (tid >> 6) & 3, s = tid >> 8;
    double v = part[0][s][r][ln];
#pragma unroll
    for (int v2 = 1; v2 < kDliWaves; ++v2) v += part[v2][s][r][ln];
    const int xl = (ln >> 4) + 4 * r;
    const int64_t x = x0 + xl;
    const int cc = 16 * s + (ln & 15);
    const bool in = x < n && cc < w;
    Zs[xl][cc] = in ? -v : 0.0;
    if (in) {
      Zt[(size_t)(c0 + cc) * ld + x] = -v;
      Zt[(size_t)x * ld + c0 + cc] = -v;
    }
  }
  __syncthreads();
  double* P = Pt + (size_t)blockIdx.x * (kDlIB * kDlIB);
  for (int e = tid; e < kDlIB * kDlIB; e += 64 * kDliWaves) {
    const int a = e % kDlIB, c = e / kDlIB;
    double sum = 0.0;
#pragma unroll
    for (int xl = 0; xl < 16; ++xl) sum = fma(Ws[xl][a], Zs[xl][c], sum);
    P[e] = sum;
  }
}
static_assert(64 * kDliWaves == 16 * kDlIB, "k_dli_cols stages one entry of the W tile and one of the Z tile per thread");

// Z_jj -= W_j' Z_Bj: the row tiles' parts added in tile order (lower triangle), the result stored at both places
__global__ __launch_bounds__(kDlIB * kDlIB) void k_dli_diag(int n, const int* __restrict__ blk, int j, double* Zt, const double* __restrict__ Pt) {
  if (j >= blk[0]) return;
  const int c0 = blk[1 + j], j1 = blk[2 + j], w = j1 - c0;
  const size_t ld = (size_t)n;
  const int ntile = (n - j1 + 15) / 16;
  const int a = threadIdx.x % kDlIB, c = threadIdx.x / kDlIB;
  if (a >= w || c > a) return;
  double s = 0.0;
  for (int t = 0; t < ntile; ++t) s += Pt[(size_t)t * (kDlIB * kDlIB) + threadIdx.x];
  const double v = Zt[(size_t)(c0 + c) * ld + c0 + a] - s;
  Zt[(size_t)(c0 + c) * ld + c0 + a] = v;
  Zt[(size_t)(c0 + a) * ld + c0 + c] = v;
}

// Z[perm[i], perm[j]] = Zt[i, j], and the count of the non-finite entries (integer atomics: exact in any order)
__global__ __launch_bounds__(256) void k_dli_out(int n, const int* __restrict__ perm, const double* __restrict__ Zt, double* __restrict__ Z, int64_t ldz,
                                                 unsigned long long* __restrict__ nonfinite) {
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  bool bad = false;
  if (i < n) {
    const double v = Zt[(size_t)j * n + i];
    Z[(size_t)perm[j] * (size_t)ldz + perm[i]] = v;
    bad = !isfinite(v);
  }
  const unsigned long long b = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(nonfinite, (unsigned long long)__popcll(b));
}

}  // namespace

void dense_ldlt_release(DenseLdltWork& D) {
  if (D.Zt) (void)hipFree(D.Zt);
  if (D.Pt) (void)hipFree(D.Pt);
  if (D.blk) (void)hipFree(D.blk);
  if (D.nonfinite) (void)hipFree(D.nonfinite);
  if (D.F) (void)hipFree(D.F);
  if (D.W) (void)hipFree(D.W);
  if (D.X) (void)hipFree(D.X);
  if (D.ipiv) (void)hipFree(D.ipiv);
  if (D.ptype) (void)hipFree(D.ptype);
  if (D.perm) (void)hipFree(D.perm);
  if (D.st) (void)hipFree(D.st);
  D = DenseLdltWork();
}

std::string dense_ldlt_alloc(DenseLdltWork& D, int64_t ns) {
  if (D.F && D.ns == ns) return "";
  dense_ldlt_release(D);
  D.ns = ns;
  const size_t n = (size_t)ns;
  std::string e = [&]() -> std::string {
    OKKT_HIP_TRY(hipMalloc((void**)&D.F, n * n * sizeof(double)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.W, n * kDlNB * sizeof(double)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.X, n * 12 * sizeof(double)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.ipiv, n * sizeof(int)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.ptype, n * sizeof(int)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.perm, n * sizeof(int)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.st, sizeof(DenseLdltState)));
    return "";
  }();
  if (!e.empty()) dense_ldlt_release(D);
  return e;
}

std::string dense_ldlt_factor(DenseLdltWork& D, hipStream_t st) {
  const int n = (int)D.ns;
  D.valid = false;
  hipLaunchKernelGGL(k_dl_init, dim3((n + 255) / 256), dim3(256), 0, st, n, D.perm, D.st);
  // panel p starts at column p (kDlNB - 1) at the earliest, and the part behind it is largest then
  for (int64_t p = 0; p * (kDlNB - 1) < n; ++p) {
    hipLaunchKernelGGL(k_dl_panel, dim3(1), dim3(kPanelThreads), 0, st, D.F, n, D.W, D.ipiv, D.ptype, D.perm, D.st);
    const int64_t rest = n - (p + 1) * (kDlNB - 1);
    if (rest <= 0) continue;
    const int64_t T = (rest + 63) / 64;
    hipLaunchKernelGGL(k_dl_trail, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, st, D.F, n, D.W, D.st);
  }
  OKKT_HIP_TRY(hipGetLastError());
  DenseLdltState h;
  OKKT_HIP_TRY(hipMemcpyAsync(&h, D.st, sizeof(h), hipMemcpyDeviceToHost, st));
  OKKT_HIP_TRY(hipStreamSynchronize(st));
  if (h.next != n) return "the dense factorisation stopped at column " + std::to_string(h.next) + " of " + std::to_string(n);
  for (int i = 0; i < 4; ++i) D.cnt[i] = h.cnt[i];
  D.valid = true;
  return "";
}

std::string dense_ldlt_solve_enqueue(DenseLdltWork& D, const double* d_r2, double* d_x2, int nr, int R, hipStream_t st) {
  if (R == 1) return solve_r<1>(D, d_r2, d_x2, nr, st);
  if (R == 2) return solve_r<2>(D, d_r2, d_x2, nr, st);
  return solve_r<4>(D, d_r2, d_x2, nr, st);
}

std::string dense_ldlt_inverse_enqueue(DenseLdltWork& D, double* d_Z, int64_t ld, hipStream_t st) {
  const int n = (int)D.ns;
  if (n <= 0) return "";
  const int maxb = (n + kDlIB - 2) / (kDlIB - 1);      // a block has kDlIB - 1 columns at the least (the last one apart)
  if (!D.Zt) {
    OKKT_HIP_TRY(hipMalloc((void**)&D.Zt, (size_t)n * n * sizeof(double)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.Pt, (size_t)((n + 15) / 16) * kDlIB * kDlIB * sizeof(double)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.blk, (size_t)(maxb + 2) * sizeof(int)));
    OKKT_HIP_TRY(hipMalloc((void**)&D.nonfinite, sizeof(unsigned long long)));
  }
  hipLaunchKernelGGL(k_dli_plan, dim3(1), dim3(64), 0, st, n, D.ptype, D.blk, D.nonfinite);
  for (int j = maxb - 1; j >= 0; --j) {
    // block j begins at column j (kDlIB - 1) at the earliest and ends kDlIB - 1 columns later at the earliest
    const int64_t below = std::max<int64_t>(0, (int64_t)n - (int64_t)(j + 1) * (kDlIB - 1));
    hipLaunchKernelGGL(k_dli_block, dim3((unsigned)(1 + (below + 255) / 256)), dim3(256), 0, st, D.F, n, D.ptype, D.blk, j, D.Zt, D.W);
    if (below > 0) hipLaunchKernelGGL(k_dli_cols, dim3((unsigned)((below + 15) / 16)), dim3(64 * kDliWaves), 0, st, n, D.blk, j, D.Zt, D.W, D.Pt);
    hipLaunchKernelGGL(k_dli_diag, dim3(1), dim3(kDlIB * kDlIB), 0, st, n, D.blk, j, D.Zt, D.Pt);
  }
  hipLaunchKernelGGL(k_dli_out, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, st, n, D.perm, D.Zt, d_Z, ld, D.nonfinite);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

}  // namespace okkt
