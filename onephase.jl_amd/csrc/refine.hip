// Extra-precise residuals for iterative refinement, gfx950.
//
// r = b - A x for up to four right-hand sides per pass over A, A the symmetric matrix whose lower triangle the analysed CSC
// holds.  Every product a * x is split exactly by TwoProd (hi = a * x, lo = fma(a, x, -hi)) and accumulated in double-double
// with TwoSum; b enters the double-double sum before the one final rounding.  Alongside: (|A||x|)_i + |b_i| in plain double
// (only a denominator), the componentwise backward error omega = max_i |r_i| / (|A||x| + |b|)_i (0 / 0 = 0, c / 0 = inf,
// NaN where r_i or x_i is not finite) and ||r||_inf, as max-reductions over per-workgroup partials and one final pass.
//
// The same pass can store each row's denominator (|A||x|)_i + |b_i| (DenSet): the forward error bound of condest.hip weighs the
// residual with it.
//
// This file is compiled with -ffp-contract=off (Makefile): a contracted or reassociated TwoSum is no longer exact.  Every fma
// below is written out.
//
// Layout: a row-wise full-symmetric copy of the pattern (row pointers, 32-bit column indices, the index of each entry's value
// in nzval), built on the host on the first call after an analysis; each call gathers nzval once into row order, every pass
// then streams contiguous values and indices.  Rows of at most long_min entries: LPR lanes per row (LPR from the average row
// length, as k_seg_spmv picks it); longer rows (dense border rows, the 40 000-entry rows): one workgroup each.  Lane partial sums
// meet in a fixed tree, so r is bitwise reproducible and independent of how many right-hand sides share the pass.
#include <algorithm>
#include <cmath>

#include "dd_arith.h"
#include "refine.h"

namespace okkt {

namespace {

#define RF_TRY(expr)                                                                        \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__);      \
  } while (0)

// two_sum and dd_add: dd_arith.h
// (h, l) += a * x (TwoProd), den += |a| |x|
__device__ __forceinline__ void dd_madd(double& h, double& l, double& den, double a, double x) {
  const double p = a * x;
  const double q = fma(a, x, -p);
  dd_add(h, l, p, q);
  den = den + fabs(a) * fabs(x);
}
// max of two non-negative values; a NaN wins (a non-finite residual must reach the caller)
__device__ __forceinline__ double nmax(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

// r = b - (h + l) rounded once; ratio = |r| / (den + |b|) with 0 / 0 = 0.  xi = x_i: a non-finite x_i makes the ratio NaN even where
// no entry of A reads it (an empty row and column), so a non-finite solution never passes for a small omega
__device__ __forceinline__ void row_finish(double h, double l, double den, double b, double xi, double& r, double& ratio) {
  double s, e;
  two_sum(b, -h, s, e);
  e = e - l;
  r = s + e;
  const double ar = fabs(r);
  ratio = ar == 0.0 ? 0.0 : ar / (den + fabs(b));
  if (!(fabs(xi) <= 1.7976931348623157e308)) ratio = __builtin_nan("");
}

// per-workgroup maxima of (omega, |r|) for R right-hand sides into out[2 q], out[2 q + 1]; 256 threads = 4 waves of 64
template <int R>
__device__ __forceinline__ void block_max(double* w, double* ri, double* __restrict__ out) {
  __shared__ double sm[4][R][2];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int q = 0; q < R; ++q) {
      w[q] = nmax(w[q], __shfl_xor(w[q], o, 64));
      ri[q] = nmax(ri[q], __shfl_xor(ri[q], o, 64));
    }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < R; ++q) { sm[wv][q][0] = w[q]; sm[wv][q][1] = ri[q]; }
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < R; ++q) {
      double a = sm[0][q][0], b = sm[0][q][1];
      for (int v = 1; v < 4; ++v) { a = nmax(a, sm[v][q][0]); b = nmax(b, sm[v][q][1]); }
      out[2 * q] = a;
      out[2 * q + 1] = b;
    }
}

// rows of at most long_min entries: a group of LPR lanes per row; longer rows run the shuffles on an empty range (k_resid_long)
template <int LPR, int R, bool DEN>
__global__ __launch_bounds__(256) void k_resid_short(int64_t n, const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                     const double* __restrict__ vals, int64_t long_min, ResidSet S, DenSet Dn,
                                                     double* __restrict__ part) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t rc = row < n ? row : n - 1;
  const int64_t p0 = rowptr[rc], p1 = rowptr[rc + 1];
  const bool skip = p1 - p0 > long_min;
  double h[R], l[R], den[R];
#pragma unroll
  for (int q = 0; q < R; ++q) { h[q] = 0.0; l[q] = 0.0; den[q] = 0.0; }
  for (int64_t p = skip ? p1 : p0 + sub; p < p1; p += LPR) {
    const double a = vals[p];
    const int c = col[p];
#pragma unroll
    for (int q = 0; q < R; ++q) dd_madd(h[q], l[q], den[q], a, S.x[q][c]);
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1)
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const double ph = __shfl_xor(h[q], o, 64), pl = __shfl_xor(l[q], o, 64), pd = __shfl_xor(den[q], o, 64);
      dd_add(h[q], l[q], ph, pl);
      den[q] = den[q] + pd;
    }
  double w[R], ri[R];
  const bool own = sub == 0 && row < n && !skip;
#pragma unroll
  for (int q = 0; q < R; ++q) {
    w[q] = 0.0;
    ri[q] = 0.0;
    if (own) {
      double r, ratio;
      row_finish(h[q], l[q], den[q], S.b[q][row], S.x[q][row], r, ratio);
      S.r[q][row] = r;
      if (DEN) Dn.d[q][row] = den[q] + fabs(S.b[q][row]);
      w[q] = ratio;
      ri[q] = fabs(r);
    }
  }
  block_max<R>(w, ri, part + (size_t)blockIdx.x * 8);
}

// one workgroup per long row: 256 strided lanes, a butterfly inside each wave, the four waves added in order by thread 0
template <int R, bool DEN>
__global__ __launch_bounds__(256) void k_resid_long(const int* __restrict__ long_rows, const int64_t* __restrict__ rowptr,
                                                    const int* __restrict__ col, const double* __restrict__ vals, ResidSet S, DenSet Dn,
                                                    double* __restrict__ part) {
  __shared__ double sm[4][R][3];
  const int64_t row = long_rows[blockIdx.x];
  const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
  double h[R], l[R], den[R];
#pragma unroll
  for (int q = 0; q < R; ++q) { h[q] = 0.0; l[q] = 0.0; den[q] = 0.0; }
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const double a = vals[p];
    const int c = col[p];
#pragma unroll
    for (int q = 0; q < R; ++q) dd_madd(h[q], l[q], den[q], a, S.x[q][c]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const double ph = __shfl_xor(h[q], o, 64), pl = __shfl_xor(l[q], o, 64), pd = __shfl_xor(den[q], o, 64);
      dd_add(h[q], l[q], ph, pl);
      den[q] = den[q] + pd;
    }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < R; ++q) { sm[wv][q][0] = h[q]; sm[wv][q][1] = l[q]; sm[wv][q][2] = den[q]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = part + (size_t)blockIdx.x * 8;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      double hh = sm[0][q][0], ll = sm[0][q][1], dd = sm[0][q][2];
      for (int v = 1; v < 4; ++v) { dd_add(hh, ll, sm[v][q][0], sm[v][q][1]); dd = dd + sm[v][q][2]; }
      double r, ratio;
      row_finish(hh, ll, dd, S.b[q][row], S.x[q][row], r, ratio);
      S.r[q][row] = r;
      if (DEN) Dn.d[q][row] = dd + fabs(S.b[q][row]);
      out[2 * q] = ratio;
      out[2 * q + 1] = fabs(r);
    }
  }
}

// the maxima over all partials: om[q] = (omega, ||r||_inf)
__global__ __launch_bounds__(256) void k_resid_final(int64_t nb, int nr, const double* __restrict__ part, ResidSet S) {
  __shared__ double sm[4][4][2];
  double w[4] = {0.0, 0.0, 0.0, 0.0}, ri[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < nb; i += 256)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < nr) { w[q] = nmax(w[q], part[i * 8 + 2 * q]); ri[q] = nmax(ri[q], part[i * 8 + 2 * q + 1]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w[q] = nmax(w[q], __shfl_xor(w[q], o, 64));
      ri[q] = nmax(ri[q], __shfl_xor(ri[q], o, 64));
    }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < 4; ++q) { sm[wv][q][0] = w[q]; sm[wv][q][1] = ri[q]; }
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < nr) {
        double a = sm[0][q][0], b = sm[0][q][1];
        for (int v = 1; v < 4; ++v) { a = nmax(a, sm[v][q][0]); b = nmax(b, sm[v][q][1]); }
        S.om[q][0] = a;
        S.om[q][1] = b;
      }
}

__global__ void k_gather_vals(int64_t nnz, const int64_t* __restrict__ src, const double* __restrict__ nz, double* __restrict__ vals) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) vals[e] = nz[src[e]];
}
// entries listed more than once in the input: their sum in input order, from 0 (the order of the assembly's duplicate path)
__global__ void k_gather_dups(int64_t ndup, const int64_t* __restrict__ dup_e, const int64_t* __restrict__ dup_ptr,
                              const int64_t* __restrict__ dup_src, const double* __restrict__ nz, double* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ndup) return;
  double s = 0.0;
  for (int64_t p = dup_ptr[t]; p < dup_ptr[t + 1]; ++p) s = s + nz[dup_src[p]];
  vals[dup_e[t]] = s;
}

__global__ void k_refine_update(int64_t n, int nr, UpdateSet U) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q < nr) {
      const double x = U.x[q][i];
      U.xp[q][i] = x;
      U.x[q][i] = x + U.d[q][i];
    }
}

inline int pick_lanes(int64_t nnz, int64_t rows) {
  const double avg = rows > 0 ? (double)nnz / (double)rows : 1.0;
  return avg <= 5.0 ? 4 : (avg <= 10.0 ? 8 : (avg <= 24.0 ? 16 : (avg <= 56.0 ? 32 : 64)));
}

template <typename T>
std::string upload(RefineMap& M, const std::vector<T>& v, T** out) {
  void* p = nullptr;
  RF_TRY(hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)));
  M.allocs.push_back(p);
  if (!v.empty()) RF_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (T*)p;
  return std::string();
}

template <int R, bool DEN>
void launch_residual(const RefineMap& M, const ResidSet& S, const DenSet& D, hipStream_t st) {
  const dim3 b(256), gs((unsigned)M.nb_short);
  switch (M.lpr) {
    case 4: hipLaunchKernelGGL((k_resid_short<4, R, DEN>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, S, D, M.part); break;
    case 8: hipLaunchKernelGGL((k_resid_short<8, R, DEN>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, S, D, M.part); break;
    case 16: hipLaunchKernelGGL((k_resid_short<16, R, DEN>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, S, D, M.part); break;
    case 32: hipLaunchKernelGGL((k_resid_short<32, R, DEN>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, S, D, M.part); break;
    default: hipLaunchKernelGGL((k_resid_short<64, R, DEN>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, S, D, M.part); break;
  }
  if (M.nlong)
    hipLaunchKernelGGL((k_resid_long<R, DEN>), dim3((unsigned)M.nlong), b, 0, st, M.long_rows, M.rowptr, M.col, M.vals, S, D,
                       M.part + (size_t)M.nb_short * 8);
}

template <bool DEN>
void residual_enqueue(const RefineMap& M, const ResidSet& S, const DenSet& D, int nr, hipStream_t st) {
  if (nr <= 0) return;
  if (M.n == 0) {
    for (int q = 0; q < nr; ++q) (void)hipMemsetAsync(S.om[q], 0, 2 * sizeof(double), st);
    return;
  }
  switch (nr) {
    case 1: launch_residual<1, DEN>(M, S, D, st); break;
    case 2: launch_residual<2, DEN>(M, S, D, st); break;
    case 3: launch_residual<3, DEN>(M, S, D, st); break;
    default: launch_residual<4, DEN>(M, S, D, st); break;
  }
  hipLaunchKernelGGL(k_resid_final, dim3(1), dim3(256), 0, st, M.nb_short + M.nlong, std::min(nr, 4), M.part, S);
}

}  // namespace

std::string refine_map_build(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t base, RefineMap& M) {
  refine_map_release(M);
  const int64_t nnz_in = colptr[n] - base;
  // the (row >= column) pairs of the input, each once: first input entry, and the later entries of pairs listed more than once
  std::vector<int64_t> mark((size_t)n, -1), slot((size_t)n, -1);
  std::vector<int> mrow, mcol;
  std::vector<int64_t> msrc;
  std::vector<std::pair<int64_t, int64_t>> dupl;    // (pair, input entry), input order within a pair
  mrow.reserve((size_t)nnz_in); mcol.reserve((size_t)nnz_in); msrc.reserve((size_t)nnz_in);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t p = colptr[j] - base; p < colptr[j + 1] - base; ++p) {
      const int64_t i = rowval[p] - base;
      if (i < j) continue;   // upper-triangle entries are ignored, as in the analysis
      if (mark[(size_t)i] != j) {
        mark[(size_t)i] = j;
        slot[(size_t)i] = (int64_t)mrow.size();
        mrow.push_back((int)i); mcol.push_back((int)j); msrc.push_back(p);
      } else {
        dupl.emplace_back(slot[(size_t)i], p);
      }
    }
  std::vector<int64_t> mark_clear;
  mark.swap(mark_clear);
  const int64_t npair = (int64_t)mrow.size();
  // source lists of the repeated pairs: the first entry, then the others in input order
  std::vector<int64_t> dgrp((size_t)npair, -1), gptr(1, 0), gsrc;
  std::stable_sort(dupl.begin(), dupl.end(), [](const std::pair<int64_t, int64_t>& a, const std::pair<int64_t, int64_t>& b) { return a.first < b.first; });
  for (size_t t = 0; t < dupl.size();) {
    const int64_t m = dupl[t].first;
    dgrp[(size_t)m] = (int64_t)gptr.size() - 1;
    gsrc.push_back(msrc[(size_t)m]);
    for (; t < dupl.size() && dupl[t].first == m; ++t) gsrc.push_back(dupl[t].second);
    gptr.push_back((int64_t)gsrc.size());
  }
  // full-symmetric rows
  std::vector<int64_t> rowptr((size_t)n + 1, 0);
  for (int64_t m = 0; m < npair; ++m) {
    ++rowptr[(size_t)mrow[(size_t)m] + 1];
    if (mrow[(size_t)m] != mcol[(size_t)m]) ++rowptr[(size_t)mcol[(size_t)m] + 1];
  }
  for (int64_t i = 0; i < n; ++i) rowptr[(size_t)i + 1] += rowptr[(size_t)i];
  const int64_t nnz = rowptr[(size_t)n];
  std::vector<int> col((size_t)nnz);
  std::vector<int64_t> src((size_t)nnz), fill(rowptr.begin(), rowptr.end() - 1), dup_e, dup_ptr(1, 0), dup_src;
  auto put = [&](int64_t r, int c, int64_t m) {
    const int64_t e = fill[(size_t)r]++;
    col[(size_t)e] = c;
    src[(size_t)e] = msrc[(size_t)m];
    const int64_t g = dgrp[(size_t)m];
    if (g >= 0) {
      dup_e.push_back(e);
      dup_src.insert(dup_src.end(), gsrc.begin() + gptr[(size_t)g], gsrc.begin() + gptr[(size_t)g + 1]);
      dup_ptr.push_back((int64_t)dup_src.size());
    }
  };
  for (int64_t m = 0; m < npair; ++m) {
    put(mrow[(size_t)m], mcol[(size_t)m], m);
    if (mrow[(size_t)m] != mcol[(size_t)m]) put(mcol[(size_t)m], mrow[(size_t)m], m);
  }
  // row classes
  M.n = n;
  M.nnz = nnz;
  M.nnz_in = nnz_in;
  M.lpr = pick_lanes(nnz, n);
  M.long_min = std::max<int64_t>(256, 8 * (int64_t)M.lpr);
  std::vector<int> long_rows;
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[(size_t)i + 1] - rowptr[(size_t)i] > M.long_min) long_rows.push_back((int)i);
  M.nlong = (int64_t)long_rows.size();
  M.nb_short = n > 0 ? (n * M.lpr + 255) / 256 : 0;
  M.ndup = (int64_t)dup_e.size();
  std::string e;
  if (!(e = upload(M, rowptr, &M.rowptr)).empty() || !(e = upload(M, col, &M.col)).empty() || !(e = upload(M, src, &M.src)).empty() ||
      !(e = upload(M, long_rows, &M.long_rows)).empty()) { refine_map_release(M); return e; }
  if (M.ndup && (!(e = upload(M, dup_e, &M.dup_e)).empty() || !(e = upload(M, dup_ptr, &M.dup_ptr)).empty() ||
                 !(e = upload(M, dup_src, &M.dup_src)).empty())) { refine_map_release(M); return e; }
  // the value workspace and the partials: allocated, not uploaded
  auto alloc = [&](size_t bytes, double** out) -> std::string {
    void* p = nullptr;
    RF_TRY(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    M.allocs.push_back(p);
    *out = (double*)p;
    return std::string();
  };
  if (!(e = alloc((size_t)nnz * sizeof(double), &M.vals)).empty() ||
      !(e = alloc((size_t)(M.nb_short + M.nlong) * 8 * sizeof(double), &M.part)).empty()) { refine_map_release(M); return e; }
  M.ready = true;
  return std::string();
}

std::string refine_stage_alloc(RefineMap& M) {
  if (M.nz_stage) return std::string();
  void* p = nullptr;
  RF_TRY(hipMalloc(&p, std::max<size_t>((size_t)M.nnz_in * sizeof(double), 16)));
  M.allocs.push_back(p);
  M.nz_stage = (double*)p;
  return std::string();
}

void refine_map_release(RefineMap& M) {
  for (void* p : M.allocs) (void)hipFree(p);
  M = RefineMap();
}

void refine_gather_enqueue(const RefineMap& M, const double* d_nzval, hipStream_t st) {
  if (M.nnz > 0) {
    const int64_t nb = std::min<int64_t>((M.nnz + 255) / 256, 8192);
    hipLaunchKernelGGL(k_gather_vals, dim3((unsigned)nb), dim3(256), 0, st, M.nnz, M.src, d_nzval, M.vals);
  }
  if (M.ndup > 0)
    hipLaunchKernelGGL(k_gather_dups, dim3((unsigned)((M.ndup + 255) / 256)), dim3(256), 0, st, M.ndup, M.dup_e, M.dup_ptr, M.dup_src, d_nzval, M.vals);
}

void refine_residual_enqueue(const RefineMap& M, const ResidSet& S, int nr, hipStream_t st) {
  residual_enqueue<false>(M, S, DenSet{{nullptr, nullptr, nullptr, nullptr}}, nr, st);
}

void refine_residual_den_enqueue(const RefineMap& M, const ResidSet& S, const DenSet& D, int nr, hipStream_t st) {
  residual_enqueue<true>(M, S, D, nr, st);
}

void refine_update_enqueue(int64_t n, const UpdateSet& U, int nr, hipStream_t st) {
  if (n <= 0 || nr <= 0) return;
  hipLaunchKernelGGL(k_refine_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, std::min(nr, 4), U);
}

}  // namespace okkt
