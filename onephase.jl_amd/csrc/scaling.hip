// Symmetric equilibration on the device, gfx950.
//
// s starts at 1.  One sweep (Jacobi: every row from the old s): r_i = max_j (|a_ij| s_i) s_j over the finite entries of row i of the
// full symmetric matrix, the factorisation's diagonal shift added to a_ii first; s_i <- s_i / sqrt(r_i) where r_i is positive and finite,
// else s_i stays.  After the last sweep s_i = m 2^e (1/2 <= m < 1) is rounded to 2^(e-1) when m < fl(sqrt(1/2)), else to 2^e, the
// exponent clamped to [-510, 510]: scaling by powers of two is exact, so the factor of S F S is bitwise the factor of the prescaled
// matrix.  One more pass takes the row maxima with the final s; their extrema and the count of zero rows go through per-workgroup
// partials into four doubles that the factorisation reads with its pivot counts.
//
// The rows are those of the refinement's map (refine.h): values gathered once per factorisation into row order, duplicates summed.
// Row classes as in refine.hip: LPR lanes per row of at most long_min entries with a shuffle maximum, one workgroup per longer row.
// max is order-free: no atomics, two runs give identical bits.
//
// This file is compiled with -ffp-contract=off (Makefile): the products are rounded one by one in the order written, sqrt and the
// division are IEEE.
#include <algorithm>
#include <cmath>

#include "scaling.h"

namespace okkt {

namespace {

#define SC_TRY(expr)                                                                        \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__);      \
  } while (0)

constexpr double kDblMax = 1.7976931348623157e308;
constexpr double kSqrtHalf = 0.70710678118654757;     // fl(sqrt(1/2)) = 0x1.6a09e667f3bcdp-1

// one entry's candidate for the row maximum; a non-finite entry is skipped
__device__ __forceinline__ double row_cand(double r, double a, double si, double sj) {
  const double aa = fabs(a);
  if (!(aa <= kDblMax)) return r;
  const double v = (aa * si) * sj;
  return v > r ? v : r;
}
// UPDATE: the next s_i; else the row maximum itself
template <bool UPDATE>
__device__ __forceinline__ double row_result(double r, double si) {
  if (!UPDATE) return r;
  return (r > 0.0 && r <= kDblMax) ? si / sqrt(r) : si;
}

// rows of at most long_min entries: LPR lanes per row; longer rows run the shuffles on an empty range (k_scale_long)
template <int LPR, bool UPDATE>
__global__ __launch_bounds__(256) void k_scale_short(int64_t n, const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                     const double* __restrict__ vals, int64_t long_min, const double* __restrict__ shift,
                                                     const double* __restrict__ s_old, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sub = (int)(t % LPR);
  const int64_t rc = row < n ? row : n - 1;
  const int64_t p0 = rowptr[rc], p1 = rowptr[rc + 1];
  const bool skip = p1 - p0 > long_min;
  const double si = s_old[rc];
  double r = 0.0;
  for (int64_t p = skip ? p1 : p0 + sub; p < p1; p += LPR) {
    double a = vals[p];
    const int c = col[p];
    if (c == rc) a = a + shift[rc];
    r = row_cand(r, a, si, s_old[c]);
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) {
    const double v = __shfl_xor(r, o, 64);
    r = v > r ? v : r;
  }
  if (sub == 0 && row < n && !skip) out[row] = row_result<UPDATE>(r, si);
}

// one workgroup per long row: 256 strided lanes, a butterfly inside each wave, the four waves joined by thread 0
template <bool UPDATE>
__global__ __launch_bounds__(256) void k_scale_long(const int* __restrict__ long_rows, const int64_t* __restrict__ rowptr,
                                                    const int* __restrict__ col, const double* __restrict__ vals,
                                                    const double* __restrict__ shift, const double* __restrict__ s_old,
                                                    double* __restrict__ out) {
  __shared__ double sm[4];
  const int row = long_rows[blockIdx.x];
  const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
  const double si = s_old[row];
  double r = 0.0;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    double a = vals[p];
    const int c = col[p];
    if (c == row) a = a + shift[row];
    r = row_cand(r, a, si, s_old[c]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v = __shfl_xor(r, o, 64);
    r = v > r ? v : r;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sm[wv] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < 4; ++v) r = sm[v] > r ? sm[v] : r;
    out[row] = row_result<UPDATE>(r, si);
  }
}

__global__ void k_scale_fill(int64_t n, double v, double* __restrict__ s) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) s[i] = v;
}

// shift[original index] = the permuted diagadd of the factorisation
__global__ void k_scale_shift(int64_t n, const int* __restrict__ perm, const double* __restrict__ diagadd, double* __restrict__ shift) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) shift[perm[k]] = diagadd[k];
}

// s_i = m 2^e -> 2^(e - 1) when m < fl(sqrt(1/2)), else 2^e: integer exponent arithmetic (frexp / ldexp), no logarithm
__global__ void k_scale_round(int64_t n, double* __restrict__ s, int* __restrict__ expo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = s[i];
  int e = 0;
  if (v > 0.0 && v <= kDblMax) {
    const double m = frexp(v, &e);
    if (m < kSqrtHalf) e = e - 1;
    e = e < -kScaleExpMax ? -kScaleExpMax : (e > kScaleExpMax ? kScaleExpMax : e);
  }
  s[i] = ldexp(1.0, e);
  expo[i] = e;
}

// (min over the non-zero rows, max, zero rows, non-zero rows) of 256 values per lane set, joined over the workgroup
__device__ __forceinline__ void ext_join(double& mn, double& mx, double& nz, double& nn, double* __restrict__ out) {
  __shared__ double sm[4][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
    nz = nz + __shfl_xor(nz, o, 64);     // counts: exact in double
    nn = nn + __shfl_xor(nn, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { sm[wv][0] = mn; sm[wv][1] = mx; sm[wv][2] = nz; sm[wv][3] = nn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < 4; ++v) {
      mn = sm[v][0] < mn ? sm[v][0] : mn;
      mx = sm[v][1] > mx ? sm[v][1] : mx;
      nz = nz + sm[v][2];
      nn = nn + sm[v][3];
    }
    out[0] = mn; out[1] = mx; out[2] = nz; out[3] = nn;
  }
}

__global__ __launch_bounds__(256) void k_scale_ext_part(int64_t n, const double* __restrict__ rmax, double* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double mn = INFINITY, mx = 0.0, nz = 0.0, nn = 0.0;
  if (i < n) {
    const double r = rmax[i];
    if (r > 0.0) { mn = r; mx = r; nn = 1.0; }
    else nz = 1.0;
  }
  ext_join(mn, mx, nz, nn, part + (size_t)blockIdx.x * kScaleOut);
}

__global__ __launch_bounds__(256) void k_scale_ext_final(int64_t nb, const double* __restrict__ part, double* __restrict__ out) {
  double mn = INFINITY, mx = 0.0, nz = 0.0, nn = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += 256) {
    const double* p = part + b * kScaleOut;
    mn = p[0] < mn ? p[0] : mn;
    mx = p[1] > mx ? p[1] : mx;
    nz = nz + p[2];
    nn = nn + p[3];
  }
  ext_join(mn, mx, nz, nn, out);
}

// v'_e = (s_row v_e) s_col for every input entry, coalesced over the entries
__global__ void k_scale_values(int64_t nnz, const int* __restrict__ erow, const int* __restrict__ ecol, const double* __restrict__ s,
                               const double* __restrict__ v, double* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x)
    out[e] = (s[erow[e]] * v[e]) * s[ecol[e]];
}

// the shift the scaled assembly adds to pivot k: (s_g diagadd_k) s_g, g = perm[k]
__global__ void k_scale_dadd(int64_t n, const int* __restrict__ perm, const double* __restrict__ s, const double* __restrict__ diagadd,
                             double* __restrict__ dadd) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double sg = s[perm[k]];
  dadd[k] = (sg * diagadd[k]) * sg;
}

inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

template <bool UPDATE>
void launch_rows(const RefineMap& M, const double* shift, const double* s_old, double* out, hipStream_t st) {
  const dim3 b(256), gs((unsigned)M.nb_short);
  switch (M.lpr) {
    case 4: hipLaunchKernelGGL((k_scale_short<4, UPDATE>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, shift, s_old, out); break;
    case 8: hipLaunchKernelGGL((k_scale_short<8, UPDATE>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, shift, s_old, out); break;
    case 16: hipLaunchKernelGGL((k_scale_short<16, UPDATE>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, shift, s_old, out); break;
    case 32: hipLaunchKernelGGL((k_scale_short<32, UPDATE>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, shift, s_old, out); break;
    default: hipLaunchKernelGGL((k_scale_short<64, UPDATE>), gs, b, 0, st, M.n, M.rowptr, M.col, M.vals, M.long_min, shift, s_old, out); break;
  }
  if (M.nlong)
    hipLaunchKernelGGL((k_scale_long<UPDATE>), dim3((unsigned)M.nlong), b, 0, st, M.long_rows, M.rowptr, M.col, M.vals, shift, s_old, out);
}

}  // namespace

std::string scaling_alloc(ScalingWork& W, int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t base) {
  scaling_release(W);
  const int64_t nnz = n > 0 ? colptr[n] - base : 0;
  std::vector<int> erow((size_t)nnz), ecol((size_t)nnz);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t p = colptr[j] - base; p < colptr[j + 1] - base; ++p) {
      erow[(size_t)p] = (int)(rowval[p] - base);
      ecol[(size_t)p] = (int)j;
    }
  auto alloc = [&](size_t bytes, void** out) -> std::string {
    void* p = nullptr;
    SC_TRY(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    W.allocs.push_back(p);
    *out = p;
    return std::string();
  };
  W.nb_part = (n + 255) / 256;
  const size_t nd = (size_t)n * sizeof(double);
  std::string e;
  if (!(e = alloc(nd, (void**)&W.s[0])).empty() || !(e = alloc(nd, (void**)&W.s[1])).empty() || !(e = alloc(nd, (void**)&W.rmax)).empty() ||
      !(e = alloc((size_t)n * sizeof(int), (void**)&W.expo)).empty() || !(e = alloc(nd, (void**)&W.shift)).empty() ||
      !(e = alloc(nd, (void**)&W.dadd)).empty() || !(e = alloc((size_t)nnz * sizeof(int), (void**)&W.erow)).empty() ||
      !(e = alloc((size_t)nnz * sizeof(int), (void**)&W.ecol)).empty() || !(e = alloc((size_t)nnz * sizeof(double), (void**)&W.vals)).empty() ||
      !(e = alloc((size_t)std::max<int64_t>(W.nb_part, 1) * kScaleOut * sizeof(double), (void**)&W.part)).empty() ||
      !(e = alloc(kScaleOut * sizeof(double), (void**)&W.out)).empty()) {
    scaling_release(W);
    return e;
  }
  if (nnz > 0) {
    hipError_t he = hipMemcpy(W.erow, erow.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(W.ecol, ecol.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice);
    if (he != hipSuccess) { scaling_release(W); return std::string("upload of the entry indices: ") + hipGetErrorString(he); }
  }
  W.n = n;
  W.nnz_in = nnz;
  W.ready = true;
  return std::string();
}

void scaling_release(ScalingWork& W) {
  for (void* p : W.allocs) (void)hipFree(p);
  W.allocs.clear();
  W.ready = false;
  W.n = 0; W.nnz_in = 0; W.nb_part = 0;
  W.s[0] = W.s[1] = W.rmax = W.shift = W.dadd = W.vals = W.part = W.out = nullptr;
  W.expo = W.erow = W.ecol = nullptr;
  W.user_uploaded = false;
  W.valid = false;
  W.s_cur = nullptr;
}

void scaling_enqueue(ScalingWork& W, const RefineMap& M, const double* d_nzval, const double* diagadd_perm, const int* perm, hipStream_t st) {
  const int64_t n = W.n;
  W.s_cur = W.s[0];
  if (n <= 0) return;
  const dim3 b(256);
  hipLaunchKernelGGL(k_scale_shift, grid1(n), b, 0, st, n, perm, diagadd_perm, W.shift);
  refine_gather_enqueue(M, d_nzval, st);
  int cur = 0;
  if (W.mode == OKKT_SCALE_RUIZ) {
    hipLaunchKernelGGL(k_scale_fill, grid1(n), b, 0, st, n, 1.0, W.s[0]);
    for (int t = 0; t < W.sweeps; ++t) {
      launch_rows<true>(M, W.shift, W.s[cur], W.s[cur ^ 1], st);
      cur ^= 1;
    }
    hipLaunchKernelGGL(k_scale_round, grid1(n), b, 0, st, n, W.s[cur], W.expo);
  }
  const double* s = W.s[cur];
  W.s_cur = W.s[cur];
  launch_rows<false>(M, W.shift, s, W.rmax, st);
  hipLaunchKernelGGL(k_scale_ext_part, dim3((unsigned)W.nb_part), b, 0, st, n, W.rmax, W.part);
  hipLaunchKernelGGL(k_scale_ext_final, dim3(1), b, 0, st, W.nb_part, W.part, W.out);
  if (W.nnz_in > 0) {
    const int64_t nb = std::min<int64_t>((W.nnz_in + 255) / 256, 8192);
    hipLaunchKernelGGL(k_scale_values, dim3((unsigned)nb), b, 0, st, W.nnz_in, W.erow, W.ecol, s, d_nzval, W.vals);
  }
  hipLaunchKernelGGL(k_scale_dadd, grid1(n), b, 0, st, n, perm, s, diagadd_perm, W.dadd);
}

}  // namespace okkt
