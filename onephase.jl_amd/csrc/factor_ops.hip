// The factor as an operator, gfx950: products with the stored L and D, the copies that stop a solve between
// its sweeps, the quadratic form z' D z and the reductions of okkt_factor_error.
//
// u = L^T x: every pivot column is a dot product of its panel column with x gathered over the front's row list -- the access shape of
// the pivot report (pivots.hip): one wave per small front; a big front's columns in groups of kFoLtCols against chunks of kFoLtRows rows
// (the gathered x of a chunk is staged in LDS once and used by the group's columns), partial records, one merge pass.  One launch set,
// independent of the tree's levels.
// y = L v: rows collect from the columns of many fronts, so the products go up the tree like the forward sweep without its pivot chain:
// per level every front adds its children's contribution vectors (DevPlan::cv through rel, or through the inverted lists ea_ptr / ea_pos
// for the big fronts), its own pivots' part L[:, K] v_K -- a GEMV, nothing inside a front is sequential -- and leaves the rows below the
// pivot block as its own contribution vector.  One wave per small front (the front's vector in LDS); a big front's rows in blocks of
// kFoLRows against column blocks of kFoLCols (partial sums), then one merge pass per level.
// Panel reads are coalesced along the rows of a column (consecutive lanes, consecutive doubles); the columns of a front start at odd and
// even arena entries alike, so the loads are 8 bytes wide.
//
// Deterministic: no atomics; every output entry is owned by one thread or one wave that sums in a fixed order, so a result does not
// depend on the launch geometry or on the columns that share the pass.
// Compiled with -ffp-contract=off (Makefile): the double-double sums of the quadratic form need TwoSum as written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "dd_arith.h"
#include "factor_ops.h"

namespace okkt {

namespace {

template <bool ABS>
__device__ __forceinline__ double fo_abs(double x) { return ABS ? fabs(x) : x; }

// ---- u = L^T x ------------------------------------------------------------------------------------------------------------------

// small fronts: one wave per front; x over the front's rows in LDS, then column by column
template <int R, bool ABS>
__global__ __launch_bounds__(64) void k_fo_lt_small(const FoSmall* __restrict__ items, const double* __restrict__ arena, const int* __restrict__ rows_all,
                                                    const double* __restrict__ x, double* __restrict__ u, int64_t vs) {
  __shared__ double xg[R][kFoSmallMax];
  const FoSmall F = items[blockIdx.x];
  const int lane = threadIdx.x;
  const double* __restrict__ L = arena + F.L;
  const int* __restrict__ rows = rows_all + F.rows;
  for (int i = lane; i < F.f; i += 64) {
    const int g = rows[i];
#pragma unroll
    for (int q = 0; q < R; ++q) xg[q][i] = x[(size_t)q * vs + g];
  }
  __syncthreads();
  for (int lc = 0; lc < F.k; ++lc) {
    const double* __restrict__ c = L + (int64_t)lc * F.f;
    double a[R];
#pragma unroll
    for (int q = 0; q < R; ++q) a[q] = 0.0;
    for (int i = lc + 1 + lane; i < F.f; i += 64) {
      const double l = fo_abs<ABS>(c[i]);
#pragma unroll
      for (int q = 0; q < R; ++q) a[q] += l * xg[q][i];
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) a[q] += __shfl_xor(a[q], off, 64);
      if (lane == 0) u[(size_t)q * vs + F.col0 + lc] = xg[q][lc] + a[q];
    }
  }
}

// big fronts: a group of columns against a chunk of rows
template <int R, bool ABS>
__global__ __launch_bounds__(kFoThreads) void k_fo_lt_big(const FoLtBig* __restrict__ items, const double* __restrict__ arena, const int* __restrict__ rows_all,
                                                          const double* __restrict__ x, int64_t vs, double* __restrict__ part, int64_t ps) {
  __shared__ double xg[R][kFoLtRows];
  __shared__ double red[kFoThreads / 64][kFoLtCols][R];
  const FoLtBig T = items[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int* __restrict__ rows = rows_all + T.rows;
  const int nrow = T.r1 - T.r0;
  for (int i = t; i < nrow; i += kFoThreads) {
    const int g = rows[T.r0 + i];
#pragma unroll
    for (int q = 0; q < R; ++q) xg[q][i] = x[(size_t)q * vs + g];
  }
  __syncthreads();
  double a[kFoLtCols][R];
#pragma unroll
  for (int c = 0; c < kFoLtCols; ++c)
#pragma unroll
    for (int q = 0; q < R; ++q) a[c][q] = 0.0;
  const double* __restrict__ L = arena + T.L + (int64_t)T.c0 * T.f;
  for (int i = t; i < nrow; i += kFoThreads) {
    const int fr = T.r0 + i;        // front row
    double l[kFoLtCols];
#pragma unroll
    for (int c = 0; c < kFoLtCols; ++c) {
      // columns beyond the group and rows on or above a column's diagonal are not read (an entry above the diagonal was never written)
      const bool have = c < T.nc && fr > T.c0 + c;
      l[c] = have ? fo_abs<ABS>(L[(int64_t)c * T.f + fr]) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const double xv = xg[q][i];
#pragma unroll
      for (int c = 0; c < kFoLtCols; ++c) a[c][q] += l[c] * xv;
    }
  }
#pragma unroll
  for (int c = 0; c < kFoLtCols; ++c)
#pragma unroll
    for (int q = 0; q < R; ++q) {
      double v = a[c][q];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) red[wv][c][q] = v;
    }
  __syncthreads();
  if (t < kFoLtCols * R) {
    const int c = t / R, q = t % R;
    if (c < T.nc) {
      double v = red[0][c][q];
#pragma unroll
      for (int w = 1; w < kFoThreads / 64; ++w) v += red[w][c][q];
      part[(size_t)q * ps + T.part + (int64_t)c * T.nch] = v;
    }
  }
}

template <int R>
__global__ __launch_bounds__(kFoThreads) void k_fo_lt_merge(const FoLtMerge* __restrict__ items, int64_t nitems, const double* __restrict__ part, int64_t ps,
                                                            const double* __restrict__ x, double* __restrict__ u, int64_t vs) {
  const int64_t it = (int64_t)blockIdx.x * kFoThreads + threadIdx.x;
  if (it >= nitems) return;
  const FoLtMerge M = items[it];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    double a = 0.0;
    for (int c = 0; c < M.nch; ++c) a += part[(size_t)q * ps + M.part + c];
    u[(size_t)q * vs + M.out] = x[(size_t)q * vs + M.out] + a;
  }
}

// ---- y = L v --------------------------------------------------------------------------------------------------------------------

// small fronts of one level: one wave per front
template <int R, bool ABS>
__global__ __launch_bounds__(64) void k_fo_l_small(DevPlan P, const FoSmall* __restrict__ items, const double* __restrict__ v, double* __restrict__ y, int64_t vs) {
  __shared__ double acc[R][kFoSmallMax], vk[R][kFoSmallMax];
  const FoSmall F = items[blockIdx.x];
  const int lane = threadIdx.x;
  const int s = F.s;
  const double* __restrict__ L = P.arena + F.L;
  for (int i = lane; i < F.f; i += 64)
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const double vi = i < F.k ? v[(size_t)q * vs + F.col0 + i] : 0.0;
      vk[q][i] = vi;
      acc[q][i] = vi;         // the unit diagonal
    }
  __syncthreads();
  for (int64_t c = P.child_ptr[s]; c < P.child_ptr[s + 1]; ++c) {      // children in ascending order, one after the other: a fixed order per row
    const int ch = P.children[c];
    const int rc = (int)(P.rel_ptr[ch + 1] - P.rel_ptr[ch]);
    const int* __restrict__ rl = P.rel + P.rel_ptr[ch];
    const double* __restrict__ cvc = P.cv + P.cv_pos[ch];
    for (int ii = lane; ii < rc; ii += 64) {
      const int d = rl[ii];
#pragma unroll
      for (int q = 0; q < R; ++q) acc[q][d] += cvc[(size_t)q * P.cv_stride + ii];
    }
    __syncthreads();
  }
  double* __restrict__ cvs = P.cv + P.cv_pos[s];
  for (int i = lane; i < F.f; i += 64) {
    double a[R];
#pragma unroll
    for (int q = 0; q < R; ++q) a[q] = acc[q][i];
    const int nj = min(i, F.k);
    for (int j = 0; j < nj; ++j) {
      const double l = fo_abs<ABS>(L[(int64_t)j * F.f + i]);
#pragma unroll
      for (int q = 0; q < R; ++q) a[q] += l * vk[q][j];
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      if (i < F.k) y[(size_t)q * vs + F.col0 + i] = a[q];
      else cvs[(size_t)q * P.cv_stride + i - F.k] = a[q];
    }
  }
}

// big fronts of one level: a block of rows against a block of columns, one row per thread, eight columns' loads in flight
template <int R, bool ABS>
__global__ __launch_bounds__(kFoThreads) void k_fo_l_big(const FoLBig* __restrict__ items, const double* __restrict__ arena, const double* __restrict__ v, int64_t vs,
                                                         double* __restrict__ part, int64_t ps) {
  __shared__ double vk[R][kFoLCols];
  const FoLBig T = items[blockIdx.x];
  const int t = threadIdx.x;
  for (int j = t; j < T.nc; j += kFoThreads)
#pragma unroll
    for (int q = 0; q < R; ++q) vk[q][j] = v[(size_t)q * vs + T.col0 + T.c0 + j];
  __syncthreads();
  const int i = T.r0 + t;
  if (i >= T.r1) return;
  double a[R];
#pragma unroll
  for (int q = 0; q < R; ++q) a[q] = 0.0;
  const double* __restrict__ Lr = arena + T.L + (int64_t)T.c0 * T.f + i;
  const int nj = max(0, min(T.nc, i - T.c0));      // columns c0 + j < i: strictly below the diagonal
  int j = 0;
  for (; j + 8 <= nj; j += 8) {
    double l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) l[e] = fo_abs<ABS>(Lr[(int64_t)(j + e) * T.f]);
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int q = 0; q < R; ++q) a[q] += l[e] * vk[q][j + e];
  }
  for (; j < nj; ++j) {
    const double l = fo_abs<ABS>(Lr[(int64_t)j * T.f]);
#pragma unroll
    for (int q = 0; q < R; ++q) a[q] += l * vk[q][j];
  }
#pragma unroll
  for (int q = 0; q < R; ++q) part[(size_t)q * ps + T.part + i] = a[q];
}

template <int R>
__global__ __launch_bounds__(kFoThreads) void k_fo_l_merge(DevPlan P, const FoLMerge* __restrict__ items, const double* __restrict__ part, int64_t ps,
                                                           const double* __restrict__ v, double* __restrict__ y, int64_t vs) {
  const FoLMerge M = items[blockIdx.x];
  const int i = M.r0 + threadIdx.x;
  if (i >= min(M.f, M.r0 + kFoLRows)) return;
  double a[R];
#pragma unroll
  for (int q = 0; q < R; ++q) a[q] = i < M.k ? v[(size_t)q * vs + M.col0 + i] : 0.0;
  const int lim = min(i, M.k);
  for (int c0 = 0, cb = 0; c0 < lim; c0 += kFoLCols, ++cb)
#pragma unroll
    for (int q = 0; q < R; ++q) a[q] += part[(size_t)q * ps + M.part + (int64_t)cb * M.f + i];
  const int64_t e0 = P.ea_ptr[M.gcb + i], e1 = P.ea_ptr[M.gcb + i + 1];
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t pos = P.ea_pos[e];
#pragma unroll
    for (int q = 0; q < R; ++q) a[q] += P.cv[(size_t)q * P.cv_stride + pos];
  }
#pragma unroll
  for (int q = 0; q < R; ++q) {
    if (i < M.k) y[(size_t)q * vs + M.col0 + i] = a[q];
    else P.cv[(size_t)q * P.cv_stride + M.cv + i - M.k] = a[q];
  }
}

// ---- vector passes --------------------------------------------------------------------------------------------------------------

template <bool ABS>
__global__ __launch_bounds__(kFoThreads) void k_fo_d(int64_t n, int R, const double* __restrict__ d, double* __restrict__ w, int64_t vs) {
  const int64_t j = (int64_t)blockIdx.x * kFoThreads + threadIdx.x;
  if (j >= n) return;
  const double dj = fo_abs<ABS>(d[j]);
  for (int q = 0; q < R; ++q) w[(size_t)q * vs + j] = dj * w[(size_t)q * vs + j];
}

__global__ __launch_bounds__(kFoThreads) void k_fo_load(int64_t n, int nr, int R, const int* __restrict__ perm, const double* __restrict__ sc, int abs,
                                                        const double* __restrict__ x, int64_t stride, double* __restrict__ w, int64_t vs) {
  const int64_t j = (int64_t)blockIdx.x * kFoThreads + threadIdx.x;
  if (j >= n) return;
  const int64_t g = perm ? perm[j] : j;
  const double s = sc ? sc[g] : 1.0;
  for (int q = 0; q < R; ++q) {
    double val = 0.0;
    if (q < nr) {
      val = x[(size_t)q * stride + g];
      if (sc) val = val / s;
      if (abs) val = fabs(val);
    }
    w[(size_t)q * vs + j] = val;
  }
}

__global__ __launch_bounds__(kFoThreads) void k_fo_store(int64_t n, int nr, const int* __restrict__ perm, const double* __restrict__ sc,
                                                         const double* __restrict__ w, int64_t vs, double* __restrict__ y, int64_t stride) {
  const int64_t j = (int64_t)blockIdx.x * kFoThreads + threadIdx.x;
  if (j >= n) return;
  const int64_t g = perm ? perm[j] : j;
  const double s = sc ? sc[g] : 1.0;
  for (int q = 0; q < nr; ++q) {
    const double val = w[(size_t)q * vs + j];
    y[(size_t)q * stride + g] = sc ? val / s : val;
  }
}

// ---- the quadratic form ---------------------------------------------------------------------------------------------------------

// d z z as an unevaluated sum (hi, lo): z z and d (z z) are split exactly by fma, the product of d with the low part is rounded
// (a relative 2^-106 of the term)
__device__ __forceinline__ void fo_dzz(double d, double z, double& hi, double& lo) {
  const double p = z * z;
  const double e = fma(z, z, -p);
  hi = d * p;
  lo = fma(d, p, -hi) + d * e;
}

struct FoDD4 { double ph, pl, nh, nl; };

// the fixed tree of one workgroup: butterflies inside the waves, the four waves in order
__device__ __forceinline__ FoDD4 fo_block_sum(FoDD4 a, double (*sm)[4]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ph = __shfl_xor(a.ph, off, 64), pl = __shfl_xor(a.pl, off, 64), nh = __shfl_xor(a.nh, off, 64), nl = __shfl_xor(a.nl, off, 64);
    // both partners add the same two pairs; the lower lane's operand goes first on both sides so that they agree bit for bit
    const bool low = (threadIdx.x & off) == 0;
    double h0 = low ? a.ph : ph, l0 = low ? a.pl : pl;
    dd_add(h0, l0, low ? ph : a.ph, low ? pl : a.pl);
    double h1 = low ? a.nh : nh, l1 = low ? a.nl : nl;
    dd_add(h1, l1, low ? nh : a.nh, low ? nl : a.nl);
    a.ph = h0; a.pl = l0; a.nh = h1; a.nl = l1;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { sm[wv][0] = a.ph; sm[wv][1] = a.pl; sm[wv][2] = a.nh; sm[wv][3] = a.nl; }
  __syncthreads();
  FoDD4 r = {sm[0][0], sm[0][1], sm[0][2], sm[0][3]};
  for (int w = 1; w < kFoThreads / 64; ++w) {
    dd_add(r.ph, r.pl, sm[w][0], sm[w][1]);
    dd_add(r.nh, r.nl, sm[w][2], sm[w][3]);
  }
  return r;
}

__global__ __launch_bounds__(kFoThreads) void k_fo_quad(int64_t n, int nr, const double* __restrict__ d, const double* __restrict__ z, int64_t zs, FoQuad* __restrict__ out) {
  __shared__ double sm[kFoThreads / 64][4];
  for (int q = 0; q < nr; ++q) {
    FoDD4 a = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j = (int64_t)blockIdx.x * kFoThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kFoThreads) {
      const double dj = d[j];
      double hi, lo;
      fo_dzz(dj, z[(size_t)q * zs + j], hi, lo);
      if (dj > 0.0) dd_add(a.ph, a.pl, hi, lo);
      else if (dj < 0.0) dd_add(a.nh, a.nl, hi, lo);
    }
    a = fo_block_sum(a, sm);
    if (threadIdx.x == 0) { out[blockIdx.x].pos_h[q] = a.ph; out[blockIdx.x].pos_l[q] = a.pl; out[blockIdx.x].neg_h[q] = a.nh; out[blockIdx.x].neg_l[q] = a.nl; }
  }
}

// the blocks' records (one per thread) through the same tree; the result rounded once into pos_h / neg_h of record kFoRedBlocks
__global__ __launch_bounds__(kFoThreads) void k_fo_quad_final(int nr, FoQuad* __restrict__ io) {
  static_assert(kFoRedBlocks == kFoThreads, "one record per thread");
  __shared__ double sm[kFoThreads / 64][4];
  for (int q = 0; q < nr; ++q) {
    FoDD4 a = {io[threadIdx.x].pos_h[q], io[threadIdx.x].pos_l[q], io[threadIdx.x].neg_h[q], io[threadIdx.x].neg_l[q]};
    a = fo_block_sum(a, sm);
    if (threadIdx.x == 0) { io[kFoRedBlocks].pos_h[q] = a.ph + a.pl; io[kFoRedBlocks].neg_h[q] = a.nh + a.nl; }
  }
}

// ---- okkt_factor_error ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kFoThreads) void k_fo_err_init(int64_t n, int p0, int np, double* __restrict__ ones, double* __restrict__ zeros, double* __restrict__ V) {
  const int64_t i = (int64_t)blockIdx.x * kFoThreads + threadIdx.x;
  if (i >= n) return;
  ones[i] = 1.0;
  zeros[i] = 0.0;
  for (int p = 0; p < np; ++p) V[(size_t)p * n + i] = fo_probe(p0 + p, i);
}

// |x|, non-finite values as +Inf
__device__ __forceinline__ double fo_mag(double x) {
  const double a = fabs(x);
  return a < __builtin_inf() ? a : __builtin_inf();
}
__device__ __forceinline__ void fo_take(double& v, long long& r, double v2, long long r2) {
  if (r2 >= 0 && (r < 0 || v2 > v || (v2 == v && r2 < r))) { v = v2; r = r2; }
}
__device__ __forceinline__ double fo_max(double a, double b) { return b > a ? b : a; }

// thread j: the row perm[j] (the diagonal shift of the factorisation is kept in the permuted order)
__global__ __launch_bounds__(kFoThreads) void k_fo_err(int64_t n, int np, const int* __restrict__ perm, const double* __restrict__ shift, const double* __restrict__ fe,
                                                       const double* __restrict__ ae, const double* __restrict__ V, const double* __restrict__ dif, FoErr* __restrict__ out) {
  __shared__ double s_v[kFoThreads / 64], s_f[kFoThreads / 64], s_a[kFoThreads / 64];
  __shared__ long long s_r[kFoThreads / 64];
  double eta = 0.0, nf = 0.0, na = 0.0;
  long long row = -1;
  for (int64_t j = (int64_t)blockIdx.x * kFoThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kFoThreads) {
    const int64_t g = perm[j];
    const double sh = shift[j];
    const double f = fe[g] + fabs(sh), a = ae[g];
    nf = fo_max(nf, fo_mag(f));
    na = fo_max(na, fo_mag(a));
    const double den = f + a;
    for (int p = 0; p < np; ++p) {
      // dif = LDLT v - F0 v with F0 the matrix without the shift: F v - LDLT v = shift v - dif
      const double r = sh * V[(size_t)p * n + g] - dif[(size_t)p * n + g];
      const double ar = fabs(r);
      const double ratio = ar == 0.0 ? 0.0 : fo_mag(ar / den);
      fo_take(eta, row, ratio, (long long)g);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double v2 = __shfl_xor(eta, off, 64);
    const long long r2 = __shfl_xor(row, off, 64);
    fo_take(eta, row, v2, r2);
    nf = fo_max(nf, __shfl_xor(nf, off, 64));
    na = fo_max(na, __shfl_xor(na, off, 64));
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) { s_v[t >> 6] = eta; s_r[t >> 6] = row; s_f[t >> 6] = nf; s_a[t >> 6] = na; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kFoThreads / 64; ++w) { fo_take(eta, row, s_v[w], s_r[w]); nf = fo_max(nf, s_f[w]); na = fo_max(na, s_a[w]); }
    FoErr e;
    e.eta = eta; e.norm_f = nf; e.norm_a = na; e.row = row;
    out[blockIdx.x] = e;
  }
}

template <typename T>
std::string fo_upload(FactorOpsWork& W, T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  const size_t bytes = std::max<size_t>(src.size() * sizeof(T), 16);
  if (hipMalloc((void**)dst, bytes) != hipSuccess) return "hipMalloc failed";
  W.allocs.push_back(*dst);
  W.bytes += (int64_t)bytes;
  if (!src.empty() && hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return "upload failed";
  return "";
}

template <typename T>
std::string fo_alloc(FactorOpsWork& W, T** dst, int64_t count) {
  *dst = nullptr;
  const size_t bytes = std::max<size_t>((size_t)count * sizeof(T), 16);
  if (hipMalloc((void**)dst, bytes) != hipSuccess) return "hipMalloc failed";
  W.allocs.push_back(*dst);
  W.bytes += (int64_t)bytes;
  return "";
}

inline unsigned fo_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kFoThreads - 1) / kFoThreads); }

std::string fo_launch_error(const char* what) {
  const hipError_t he = hipGetLastError();
  if (he != hipSuccess) return std::string(what) + " launch failed: " + hipGetErrorString(he);
  return "";
}

template <int R, bool ABS>
std::string lt_enqueue(const Numeric& N, FactorOpsWork& W) {
  const DevPlan& d = N.d;
  hipStream_t st = N.stream;
  const int64_t vs = W.n;
  if (W.n_small > 0) k_fo_lt_small<R, ABS><<<dim3((unsigned)W.n_small), dim3(64), 0, st>>>(W.small, d.arena, d.rows, W.wa, W.wb, vs);
  if (W.n_lt_big > 0) k_fo_lt_big<R, ABS><<<dim3((unsigned)W.n_lt_big), dim3(kFoThreads), 0, st>>>(W.lt_big, d.arena, d.rows, W.wa, vs, W.lt_part, W.lt_parts);
  if (W.n_lt_merge > 0) k_fo_lt_merge<R><<<dim3(fo_grid(W.n_lt_merge)), dim3(kFoThreads), 0, st>>>(W.lt_merge, W.n_lt_merge, W.lt_part, W.lt_parts, W.wa, W.wb, vs);
  return fo_launch_error("L^T product");
}

template <int R, bool ABS>
std::string l_enqueue(const Numeric& N, FactorOpsWork& W) {
  const DevPlan& d = N.d;
  hipStream_t st = N.stream;
  const int64_t vs = W.n;
  for (int l = 0; l < W.nlevels; ++l) {
    const int64_t s0 = W.small_off[(size_t)l], ns = W.small_off[(size_t)l + 1] - s0;
    const int64_t b0 = W.l_big_off[(size_t)l], nb = W.l_big_off[(size_t)l + 1] - b0;
    const int64_t m0 = W.l_merge_off[(size_t)l], nm = W.l_merge_off[(size_t)l + 1] - m0;
    if (ns > 0) k_fo_l_small<R, ABS><<<dim3((unsigned)ns), dim3(64), 0, st>>>(d, W.small + s0, W.wb, W.wa, vs);
    if (nb > 0) k_fo_l_big<R, ABS><<<dim3((unsigned)nb), dim3(kFoThreads), 0, st>>>(W.l_big + b0, d.arena, W.wb, vs, W.l_part, W.l_parts);
    if (nm > 0) k_fo_l_merge<R><<<dim3((unsigned)nm), dim3(kFoThreads), 0, st>>>(d, W.l_merge + m0, W.l_part, W.l_parts, W.wb, W.wa, vs);
  }
  return fo_launch_error("L product");
}

}  // namespace

void factor_ops_release(FactorOpsWork& W) {
  for (void* p : W.allocs) (void)hipFree(p);
  W = FactorOpsWork();
}

std::string factor_ops_setup(const Symbolic& S, const Numeric& N, FactorOpsWork& W) {
  factor_ops_release(W);
  std::vector<int64_t> gcb((size_t)S.nsuper, -1);
  if (S.nsuper > 0 && hipMemcpy(gcb.data(), N.d.bigcol_base, (size_t)S.nsuper * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess)
    return "read of the extend-add list bases failed";
  FoPlan P;
  std::string e = factor_ops_build_plan(S, N.front_pos_host, gcb, N.small_max, P);
  if (!e.empty()) return e;
  W.n = S.n;
  W.nlevels = S.nlevels;
  W.small_off = P.small_off;
  W.l_big_off = P.l_big_off;
  W.l_merge_off = P.l_merge_off;
  W.n_small = (int64_t)P.small.size();
  W.n_lt_big = (int64_t)P.lt_big.size();
  W.n_lt_merge = (int64_t)P.lt_merge.size();
  W.lt_parts = std::max<int64_t>(P.lt_parts, 1);
  W.l_parts = std::max<int64_t>(P.l_parts, 1);
  if (!(e = fo_upload(W, &W.small, P.small)).empty()) return e;
  if (!(e = fo_upload(W, &W.lt_big, P.lt_big)).empty()) return e;
  if (!(e = fo_upload(W, &W.lt_merge, P.lt_merge)).empty()) return e;
  if (!(e = fo_upload(W, &W.l_big, P.l_big)).empty()) return e;
  if (!(e = fo_upload(W, &W.l_merge, P.l_merge)).empty()) return e;
  if (!(e = fo_alloc(W, &W.lt_part, W.lt_parts * kMaxRhs)).empty()) return e;
  if (!(e = fo_alloc(W, &W.l_part, W.l_parts * kMaxRhs)).empty()) return e;
  if (!(e = fo_alloc(W, &W.wa, S.n * kMaxRhs)).empty()) return e;
  if (!(e = fo_alloc(W, &W.wb, S.n * kMaxRhs)).empty()) return e;
  if (!(e = fo_alloc(W, &W.quad, kFoRedBlocks + 1)).empty()) return e;
  W.planned = true;
  return "";
}

std::string factor_ops_error_alloc(FactorOpsWork& W) {
  if (W.ev) return "";
  std::string e;
  if (!(e = fo_alloc(W, &W.ev, W.n * (5 + 3 * kMaxRhs))).empty()) return e;
  if (!(e = fo_alloc(W, &W.eom, 2 * kMaxRhs)).empty()) return e;
  return fo_alloc(W, &W.err, kFoRedBlocks);
}

void factor_ops_z_out(const Numeric& N, double* d_z, int64_t stride, int nr) {
  if (N.d.n <= 0 || nr <= 0) return;
  k_fo_store<<<dim3(fo_grid(N.d.n)), dim3(kFoThreads), 0, N.stream>>>(N.d.n, nr, nullptr, nullptr, N.d.zwork, N.d.xw_stride, d_z, stride);
}

void factor_ops_z_in(const Numeric& N, const double* d_z, int64_t stride, int nr, int R) {
  if (N.d.n <= 0) return;
  k_fo_load<<<dim3(fo_grid(N.d.n)), dim3(kFoThreads), 0, N.stream>>>(N.d.n, nr, R, nullptr, nullptr, 0, d_z, stride, N.d.zwork, N.d.xw_stride);
}

void factor_ops_quadform(const Numeric& N, FactorOpsWork& W, int nr) {
  k_fo_quad<<<dim3(kFoRedBlocks), dim3(kFoThreads), 0, N.stream>>>(N.d.n, nr, N.d.dvals, N.d.zwork, N.d.xw_stride, W.quad);
  k_fo_quad_final<<<dim3(1), dim3(kFoThreads), 0, N.stream>>>(nr, W.quad);
}

void factor_ops_load(const Numeric& N, FactorOpsWork& W, double* dst, const double* d_x, int64_t stride, int nr, int R, bool perm, const double* d_scale, bool abs) {
  if (W.n <= 0) return;
  k_fo_load<<<dim3(fo_grid(W.n)), dim3(kFoThreads), 0, N.stream>>>(W.n, nr, R, perm ? N.d.perm : nullptr, d_scale, abs ? 1 : 0, d_x, stride, dst, W.n);
}

void factor_ops_store(const Numeric& N, const FactorOpsWork& W, const double* src, double* d_y, int64_t stride, int nr, bool perm, const double* d_scale) {
  if (W.n <= 0 || nr <= 0) return;
  k_fo_store<<<dim3(fo_grid(W.n)), dim3(kFoThreads), 0, N.stream>>>(W.n, nr, perm ? N.d.perm : nullptr, d_scale, src, W.n, d_y, stride);
}

std::string factor_ops_lt(const Numeric& N, FactorOpsWork& W, int R, bool abs) {
  if (abs) return R == 1 ? lt_enqueue<1, true>(N, W) : (R == 2 ? lt_enqueue<2, true>(N, W) : lt_enqueue<4, true>(N, W));
  return R == 1 ? lt_enqueue<1, false>(N, W) : (R == 2 ? lt_enqueue<2, false>(N, W) : lt_enqueue<4, false>(N, W));
}

std::string factor_ops_l(const Numeric& N, FactorOpsWork& W, int R, bool abs) {
  if (abs) return R == 1 ? l_enqueue<1, true>(N, W) : (R == 2 ? l_enqueue<2, true>(N, W) : l_enqueue<4, true>(N, W));
  return R == 1 ? l_enqueue<1, false>(N, W) : (R == 2 ? l_enqueue<2, false>(N, W) : l_enqueue<4, false>(N, W));
}

void factor_ops_d(const Numeric& N, FactorOpsWork& W, int R, bool abs) {
  if (W.n <= 0) return;
  if (abs) k_fo_d<true><<<dim3(fo_grid(W.n)), dim3(kFoThreads), 0, N.stream>>>(W.n, R, N.d.dvals, W.wb, W.n);
  else k_fo_d<false><<<dim3(fo_grid(W.n)), dim3(kFoThreads), 0, N.stream>>>(W.n, R, N.d.dvals, W.wb, W.n);
}

void factor_ops_error_init(FactorOpsWork& W, int p0, int np, hipStream_t st) {
  if (W.n <= 0) return;
  k_fo_err_init<<<dim3(fo_grid(W.n)), dim3(kFoThreads), 0, st>>>(W.n, p0, np, W.ev, W.ev + W.n, W.ev + 5 * W.n);
}

void factor_ops_error_reduce(const Numeric& N, FactorOpsWork& W, int np, hipStream_t st) {
  const int64_t n = W.n;
  k_fo_err<<<dim3(kFoRedBlocks), dim3(kFoThreads), 0, st>>>(n, np, N.d.perm, N.d.diagadd, W.ev + 2 * n, W.ev + 3 * n, W.ev + 5 * n, W.ev + (5 + 2 * kMaxRhs) * n, W.err);
}

}  // namespace okkt
