// Condition estimation and forward error bounds, gfx950.
//
// The Higham-Tisseur block 1-norm estimator (SIAM J. Matrix Anal. Appl. 21, 2000, Algorithm 2.4) applied to F^-1 (F symmetric:
// F^-T = F^-1) or, for the forward error bound, to diag(f) F^-1.  Its products are solve passes of the existing multi-right-hand-
// side path (api_condest.cpp); this file holds everything else, all of it bandwidth- or latency-bound:
//   - ||F||_1: exact row sums of |F| over the refinement's row-wise map (refine.h) plus the factorisation's diagonal shift, sized
//     as the residual kernels are (a lane group per short row, a workgroup per long row);
//   - after Y = op X: the column 1-norms, S = sign(Y), the +-1 dot products that tell parallel columns apart (exact integer counts);
//   - after Z = op' S: the row inf-norms h and a top-t selection by (h desc, row asc) over all rows and over the rows not yet used
//     (a bitmap of n bits);
//   - the unit-vector scatter of the next X, the replacement of a parallel sign column, the forward-error weights f.
// Every reduction runs in a fixed order over a grid that depends only on n, so a result is bitwise reproducible; maxima and the
// ordered selection are exact in any order.  One 256-thread workgroup per 256 rows.
#include <algorithm>
#include <climits>
#include <cmath>

#include "condest.h"

namespace okkt {

namespace {

#define CD_TRY(expr)                                                                        \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__);      \
  } while (0)

constexpr int kPS = 40;          // doubles per block partial
constexpr int kYQ = 37;          // quantities of the Y statistics: 4 norms, 1 flag, 16 + 16 dot products
constexpr double kNoRow = 9.0e15;   // the row of an empty candidate (above every row index; exact in double)

__device__ __forceinline__ double nmax(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
// candidate order: larger h first, then the lower row
__device__ __forceinline__ bool better(double va, double ia, double vb, double ib) { return va > vb || (va == vb && ia < ib); }

// sums (or maxima, bit q of maxmask) of quantity q = blockIdx.x over nb block partials of `stride` doubles: out[q]
__global__ __launch_bounds__(256) void k_cd_reduce(int64_t nb, int stride, unsigned maxmask, const double* __restrict__ part,
                                                   double* __restrict__ out) {
  __shared__ double sm[4];
  const int q = blockIdx.x;
  const bool mx = (maxmask >> q) & 1u;
  double a = 0.0;
  for (int64_t p = threadIdx.x; p < nb; p += 256) {
    const double v = part[p * stride + q];
    a = mx ? nmax(a, v) : a + v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v = __shfl_xor(a, o, 64);
    a = mx ? nmax(a, v) : a + v;
  }
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sm[0];
    for (int v = 1; v < 4; ++v) s = mx ? nmax(s, sm[v]) : s + sm[v];
    out[q] = s;
  }
}

// ---- ||F||_1 ----------------------------------------------------------------------------------------------------------------

__global__ void k_cd_shift(int64_t n, const int* __restrict__ perm, const double* __restrict__ diagadd, double* __restrict__ shift) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) shift[perm[k]] = diagadd[k];
}

// sum_j |F_ij| of the entries p0 + sub, p0 + sub + step, ...; the diagonal entry carries the shift; hasd: the diagonal was met
__device__ __forceinline__ void row_abs(int64_t row, int64_t p0, int64_t p1, int sub, int step, const int* __restrict__ col,
                                        const double* __restrict__ vals, double sh, double& s, int& hasd) {
  for (int64_t p = p0 + sub; p < p1; p += step) {
    const int c = col[p];
    const double a = c == row ? vals[p] + sh : vals[p];
    if (c == row) hasd = 1;
    s = s + fabs(a);
  }
}

template <int LPR>
__global__ __launch_bounds__(256) void k_cd_rowsum_short(int64_t n, const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                         const double* __restrict__ vals, const double* __restrict__ shift, int64_t long_min,
                                                         double* __restrict__ part) {
  __shared__ double sm[4];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t rc = row < n ? row : n - 1;
  const int64_t p0 = rowptr[rc], p1 = rowptr[rc + 1];
  const bool skip = p1 - p0 > long_min;
  const double sh = shift[rc];
  double s = 0.0;
  int hasd = 0;
  if (!skip) row_abs(rc, p0, p1, sub, LPR, col, vals, sh, s, hasd);
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) {
    s = s + __shfl_xor(s, o, 64);
    hasd |= __shfl_xor(hasd, o, 64);
  }
  double w = 0.0;
  if (sub == 0 && row < n && !skip) w = hasd ? s : s + fabs(sh);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w = nmax(w, __shfl_xor(w, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sm[0];
    for (int v = 1; v < 4; ++v) a = nmax(a, sm[v]);
    part[blockIdx.x * 2] = a;
    part[blockIdx.x * 2 + 1] = finite(a) ? 0.0 : 1.0;
  }
}

__global__ __launch_bounds__(256) void k_cd_rowsum_long(const int* __restrict__ long_rows, const int64_t* __restrict__ rowptr,
                                                        const int* __restrict__ col, const double* __restrict__ vals,
                                                        const double* __restrict__ shift, double* __restrict__ part) {
  __shared__ double sm[4];
  __shared__ int smd[4];
  const int64_t row = long_rows[blockIdx.x];
  const double sh = shift[row];
  double s = 0.0;
  int hasd = 0;
  row_abs(row, rowptr[row], rowptr[row + 1], threadIdx.x, 256, col, vals, sh, s, hasd);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s = s + __shfl_xor(s, o, 64);
    hasd |= __shfl_xor(hasd, o, 64);
  }
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = s; smd[threadIdx.x >> 6] = hasd; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sm[0];
    int d = smd[0];
    for (int v = 1; v < 4; ++v) { a = a + sm[v]; d |= smd[v]; }
    if (!d) a = a + fabs(sh);
    part[blockIdx.x * 2] = a;
    part[blockIdx.x * 2 + 1] = finite(a) ? 0.0 : 1.0;
  }
}

// ---- the estimator's blocks -------------------------------------------------------------------------------------------------

__global__ void k_cd_start(int64_t n, int t, double* __restrict__ X) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double inv = 1.0 / (double)n;
  const int64_t H = n < 4 ? n : 4;
  X[i] = inv;
  for (int j = 1; j < t; ++j) X[j * n + i] = cd_sign((uint64_t)j, j, i, H) * inv;
}

__global__ __launch_bounds__(256) void k_cd_ystats(int64_t n, int t, const double* __restrict__ Y, const double* __restrict__ f,
                                                   double* __restrict__ S, const double* __restrict__ Sold, int has_old,
                                                   double* __restrict__ SF, double* __restrict__ part, double* __restrict__ out) {
  __shared__ double sm[4][kYQ];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double q[kYQ];
#pragma unroll
  for (int k = 0; k < kYQ; ++k) q[k] = 0.0;
  if (i < n) {
    double s[4] = {0.0, 0.0, 0.0, 0.0}, so[4] = {0.0, 0.0, 0.0, 0.0};
    const double w = f ? f[i] : 1.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < t) {
        const double y = f ? w * Y[a * n + i] : Y[a * n + i];
        q[a] = fabs(y);
        if (!finite(y)) q[4] = 1.0;
        s[a] = y >= 0.0 ? 1.0 : -1.0;
        S[a * n + i] = s[a];
        if (f) SF[a * n + i] = w * s[a];
        if (has_old) so[a] = Sold[a * n + i];
        if (i < 4) out[kCdY + 37 + a * 4 + i] = s[a];
      }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        q[5 + a * 4 + b] = s[a] * s[b];
        q[21 + a * 4 + b] = s[a] * so[b];
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < kYQ; ++k) {
      const double v = __shfl_xor(q[k], o, 64);
      q[k] = k == 4 ? (q[k] > v ? q[k] : v) : q[k] + v;
    }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < kYQ; ++k) sm[wv][k] = q[k];
  __syncthreads();
  if (threadIdx.x < kYQ) {
    const int k = threadIdx.x;
    double a = sm[0][k];
    for (int v = 1; v < 4; ++v) a = k == 4 ? (a > sm[v][k] ? a : sm[v][k]) : a + sm[v][k];
    part[(size_t)blockIdx.x * kPS + k] = a;
  }
}

__global__ void k_cd_resample(int64_t n, int a, uint64_t draw, int cls, double* __restrict__ S, const double* __restrict__ f,
                              double* __restrict__ SF) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s = cd_sign(draw, cls, i, n < 4 ? n : 4);
  S[a * n + i] = s;
  if (f) SF[a * n + i] = f[i] * s;
}

// the t best of the workgroup's candidates (one per thread), best first; every thread gets the same lists
__device__ void block_top(double v, double idx, int t, double* ov, double* oi) {
  __shared__ double sv[4], si[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int r = 0; r < t; ++r) {
    double bv = v, bi = idx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double pv = __shfl_xor(bv, o, 64), pi = __shfl_xor(bi, o, 64);
      if (better(pv, pi, bv, bi)) { bv = pv; bi = pi; }
    }
    if (lane == 0) { sv[wv] = bv; si[wv] = bi; }
    __syncthreads();
    bv = sv[0]; bi = si[0];
    for (int w = 1; w < 4; ++w)
      if (better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
    __syncthreads();
    ov[r] = bv;
    oi[r] = bi;
    if (idx == bi) { v = -1.0; idx = kNoRow; }
  }
}

__global__ __launch_bounds__(256) void k_cd_zstats(int64_t n, int t, const double* __restrict__ Z, const uint32_t* __restrict__ used,
                                                   int64_t ind_best, double* __restrict__ part, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double h = -1.0, hv = -1.0, hi = kNoRow, uv = -1.0, ui = kNoRow, nf = 0.0;
  if (i < n) {
    h = 0.0;
    for (int a = 0; a < t; ++a) {
      const double z = fabs(Z[a * n + i]);
      if (!finite(z)) nf = 1.0;
      else h = z > h ? z : h;
    }
    if (nf == 0.0) {
      hv = h; hi = (double)i;
      if (!((used[i >> 5] >> (i & 31)) & 1u)) { uv = h; ui = (double)i; }
    }
    if (i == ind_best) out[kCdZ + 16] = nf != 0.0 ? -1.0 : h;
  }
  double av[4], ai[4], bv[4], bi[4];
  block_top(hv, hi, t, av, ai);
  block_top(uv, ui, t, bv, bi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nf = fmax(nf, __shfl_xor(nf, o, 64));
  __shared__ double snf[4];
  if ((threadIdx.x & 63) == 0) snf[threadIdx.x >> 6] = nf;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* p = part + (size_t)blockIdx.x * kPS;
    for (int r = 0; r < 4; ++r) {
      const bool ok = r < t;
      p[r] = ok ? av[r] : -1.0; p[4 + r] = ok ? ai[r] : kNoRow;
      p[8 + r] = ok ? bv[r] : -1.0; p[12 + r] = ok ? bi[r] : kNoRow;
    }
    p[16] = fmax(fmax(snf[0], snf[1]), fmax(snf[2], snf[3]));
  }
}

// insert (v, i) into the sorted list L of length t
__device__ __forceinline__ void list_insert(double* Lv, double* Li, int t, double v, double i) {
  if (!better(v, i, Lv[t - 1], Li[t - 1])) return;
  int r = t - 1;
  while (r > 0 && better(v, i, Lv[r - 1], Li[r - 1])) { Lv[r] = Lv[r - 1]; Li[r] = Li[r - 1]; --r; }
  Lv[r] = v; Li[r] = i;
}

// the block lists merged: out[kCdZ ..]; the row order is total, so the result does not depend on the merge order
__global__ __launch_bounds__(256) void k_cd_zfinal(int64_t nb, int t, const double* __restrict__ part, double* __restrict__ out) {
  double Av[4], Ai[4], Bv[4], Bi[4], nf = 0.0;
  for (int r = 0; r < 4; ++r) { Av[r] = -1.0; Ai[r] = kNoRow; Bv[r] = -1.0; Bi[r] = kNoRow; }
  for (int64_t p = threadIdx.x; p < nb; p += 256) {
    const double* q = part + p * kPS;
    for (int r = 0; r < t; ++r) {
      list_insert(Av, Ai, t, q[r], q[4 + r]);
      list_insert(Bv, Bi, t, q[8 + r], q[12 + r]);
    }
    nf = fmax(nf, q[16]);
  }
  // t rounds: every thread offers its head, the winner's owner moves on to its next entry
  double wv[4], wi[4];
  int ha = 0, hb = 0;
  for (int r = 0; r < t; ++r) {
    block_top(ha < t ? Av[ha] : -1.0, ha < t ? Ai[ha] : kNoRow, 1, wv, wi);
    if (threadIdx.x == 0) { out[kCdZ + r] = wv[0]; out[kCdZ + 4 + r] = wi[0]; }
    if (ha < t && Ai[ha] == wi[0] && wi[0] != kNoRow) ++ha;
    block_top(hb < t ? Bv[hb] : -1.0, hb < t ? Bi[hb] : kNoRow, 1, wv, wi);
    if (threadIdx.x == 0) { out[kCdZ + 8 + r] = wv[0]; out[kCdZ + 12 + r] = wi[0]; }
    if (hb < t && Bi[hb] == wi[0] && wi[0] != kNoRow) ++hb;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nf = fmax(nf, __shfl_xor(nf, o, 64));
  __shared__ double snf[4];
  if ((threadIdx.x & 63) == 0) snf[threadIdx.x >> 6] = nf;
  __syncthreads();
  if (threadIdx.x == 0) out[kCdZ + 17] = fmax(fmax(snf[0], snf[1]), fmax(snf[2], snf[3]));
}

__global__ void k_cd_scatter(int64_t n, int t, CdIdx ind, double* __restrict__ X, uint32_t* __restrict__ used) {
  const int a = threadIdx.x;
  if (a >= t) return;
  const int64_t i = ind.i[a];
  if (i < 0 || i >= n) return;
  X[a * n + i] = 1.0;
  atomicOr(&used[i >> 5], 1u << (i & 31));
}

// LAPACK's xSYRFS weights: f_i = |r_i| + nz eps den_i (+ nz safmin where den_i is tiny), nz = entries of row i + 1; ||x||_inf
__global__ __launch_bounds__(256) void k_cd_fweights(int64_t n, const int64_t* __restrict__ rowptr, const double* __restrict__ r,
                                                     const double* __restrict__ den, const double* __restrict__ x,
                                                     double* __restrict__ f, double* __restrict__ part) {
  __shared__ double sm[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double xm = 0.0;
  if (i < n) {
    const double eps = 0x1p-53, safmin = 0x1p-1022;
    const double nz = (double)(rowptr[i + 1] - rowptr[i] + 1);
    const double safe1 = nz * safmin, safe2 = safe1 / eps;
    const double d = den[i];
    f[i] = d > safe2 ? fabs(r[i]) + nz * eps * d : fabs(r[i]) + nz * eps * d + safe1;
    xm = fabs(x[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) xm = nmax(xm, __shfl_xor(xm, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = xm;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.x * kPS] = nmax(nmax(sm[0], sm[1]), nmax(sm[2], sm[3]));
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

std::string condest_alloc(int64_t n, CondestWork& W) {
  if (W.n == n && W.X) return std::string();
  condest_release(W);
  W.n = n;
  W.nb = (n + 255) / 256;
  auto alloc = [&](size_t bytes, void** out) -> std::string {
    void* p = nullptr;
    CD_TRY(hipMalloc(&p, std::max<size_t>(bytes, 64)));
    W.allocs.push_back(p);
    *out = p;
    return std::string();
  };
  const size_t blk = (size_t)4 * n * sizeof(double);
  // partials: the row kernels' nb blocks, or the norm's lane-group blocks (at most n / 4 + 1) plus one per long row
  const size_t npart = std::max<size_t>((size_t)W.nb * kPS, (size_t)2 * ((size_t)n / 4 + 2 + (size_t)n));
  std::string e;
  if (!(e = alloc(blk, (void**)&W.X)).empty() || !(e = alloc(blk, (void**)&W.Y)).empty() || !(e = alloc(blk, (void**)&W.S[0])).empty() ||
      !(e = alloc(blk, (void**)&W.S[1])).empty() || !(e = alloc(blk, (void**)&W.SF)).empty() || !(e = alloc(blk, (void**)&W.R)).empty() ||
      !(e = alloc(blk, (void**)&W.DEN)).empty() || !(e = alloc((size_t)n * 8, (void**)&W.f)).empty() ||
      !(e = alloc((size_t)n * 8, (void**)&W.shift)).empty() || !(e = alloc((size_t)((n + 31) / 32) * 4, (void**)&W.used)).empty() ||
      !(e = alloc(npart * 8, (void**)&W.part)).empty() || !(e = alloc((size_t)kCdOut * 8, (void**)&W.out)).empty()) {
    condest_release(W);
    return e;
  }
  return std::string();
}

void condest_release(CondestWork& W) {
  for (void* p : W.allocs) (void)hipFree(p);
  W = CondestWork();
}

void condest_norm1_enqueue(const RefineMap& M, CondestWork& W, const double* diagadd_perm, const int* perm, hipStream_t st) {
  const int64_t n = M.n;
  if (n == 0) return;
  hipLaunchKernelGGL(k_cd_shift, dim3(blocks(n)), dim3(256), 0, st, n, perm, diagadd_perm, W.shift);
  const dim3 b(256), gs((unsigned)M.nb_short);
  switch (M.lpr) {
    case 4: hipLaunchKernelGGL((k_cd_rowsum_short<4>), gs, b, 0, st, n, M.rowptr, M.col, M.vals, W.shift, M.long_min, W.part); break;
    case 8: hipLaunchKernelGGL((k_cd_rowsum_short<8>), gs, b, 0, st, n, M.rowptr, M.col, M.vals, W.shift, M.long_min, W.part); break;
    case 16: hipLaunchKernelGGL((k_cd_rowsum_short<16>), gs, b, 0, st, n, M.rowptr, M.col, M.vals, W.shift, M.long_min, W.part); break;
    case 32: hipLaunchKernelGGL((k_cd_rowsum_short<32>), gs, b, 0, st, n, M.rowptr, M.col, M.vals, W.shift, M.long_min, W.part); break;
    default: hipLaunchKernelGGL((k_cd_rowsum_short<64>), gs, b, 0, st, n, M.rowptr, M.col, M.vals, W.shift, M.long_min, W.part); break;
  }
  if (M.nlong)
    hipLaunchKernelGGL(k_cd_rowsum_long, dim3((unsigned)M.nlong), b, 0, st, M.long_rows, M.rowptr, M.col, M.vals, W.shift,
                       W.part + (size_t)M.nb_short * 2);
  hipLaunchKernelGGL(k_cd_reduce, dim3(2), dim3(256), 0, st, M.nb_short + M.nlong, 2, 3u, W.part, W.out + kCdN);
}

void condest_start_enqueue(CondestWork& W, int t, hipStream_t st) {
  if (W.n) hipLaunchKernelGGL(k_cd_start, dim3(blocks(W.n)), dim3(256), 0, st, W.n, t, W.X);
}

void condest_ystats_enqueue(CondestWork& W, int t, int cur, bool has_old, const double* f, hipStream_t st) {
  if (!W.n) return;
  hipLaunchKernelGGL(k_cd_ystats, dim3((unsigned)W.nb), dim3(256), 0, st, W.n, t, W.Y, f, W.S[cur], W.S[cur ^ 1], has_old ? 1 : 0, W.SF,
                     W.part, W.out);
  hipLaunchKernelGGL(k_cd_reduce, dim3(kYQ), dim3(256), 0, st, W.nb, kPS, 1u << 4, W.part, W.out + kCdY);
}

void condest_resample_enqueue(CondestWork& W, int cur, int a, uint64_t draw, int cls, const double* f, hipStream_t st) {
  if (W.n) hipLaunchKernelGGL(k_cd_resample, dim3(blocks(W.n)), dim3(256), 0, st, W.n, a, draw, cls, W.S[cur], f, W.SF);
}

void condest_zstats_enqueue(CondestWork& W, int t, int64_t ind_best, hipStream_t st) {
  if (!W.n) return;
  hipLaunchKernelGGL(k_cd_zstats, dim3((unsigned)W.nb), dim3(256), 0, st, W.n, t, W.Y, W.used, ind_best, W.part, W.out);
  hipLaunchKernelGGL(k_cd_zfinal, dim3(1), dim3(256), 0, st, W.nb, t, W.part, W.out);
}

void condest_scatter_enqueue(CondestWork& W, int t, const CdIdx& ind, hipStream_t st) {
  if (!W.n) return;
  (void)hipMemsetAsync(W.X, 0, (size_t)t * W.n * sizeof(double), st);
  hipLaunchKernelGGL(k_cd_scatter, dim3(1), dim3(64), 0, st, W.n, t, ind, W.X, W.used);
}

void condest_fweights_enqueue(const RefineMap& M, CondestWork& W, const double* r, const double* den, const double* x, hipStream_t st) {
  if (!W.n) return;
  hipLaunchKernelGGL(k_cd_fweights, dim3((unsigned)W.nb), dim3(256), 0, st, W.n, M.rowptr, r, den, x, W.f, W.part);
  hipLaunchKernelGGL(k_cd_reduce, dim3(1), dim3(256), 0, st, W.nb, kPS, 1u, W.part, W.out + kCdN + 2);
}

}  // namespace okkt
