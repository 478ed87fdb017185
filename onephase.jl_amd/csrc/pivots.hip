// Threshold pivot report: the column maxima of |L| below the diagonal and the rows that attain them, from one
// read of the factor's panels.  A (value, front row) pair is carried through lane exchanges, then through LDS; the larger value wins
// and, between equal values, the lower row: a total order, so the result does not depend on how the rows were dealt to the lanes, and
// no atomic is needed.  A NaN or an Inf counts as +Inf, so the first such row of a column wins it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "pivots.h"

namespace okkt {

namespace {

struct PvPair { double v; int r; };

__device__ __forceinline__ PvPair pv_none() { return {-1.0, INT_MAX}; }

// |x|, non-finite values as +Inf (neither a NaN nor an Inf is < Inf)
__device__ __forceinline__ double pv_mag(double x) {
  const double a = fabs(x);
  return a < __builtin_inf() ? a : __builtin_inf();
}

__device__ __forceinline__ void pv_take(PvPair& a, double v, int r) {
  if (v > a.v || (v == a.v && r < a.r)) { a.v = v; a.r = r; }
}

__device__ __forceinline__ PvPair pv_wave_reduce(PvPair a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double v = __shfl_xor(a.v, off, 64);
    const int r = __shfl_xor(a.r, off, 64);
    pv_take(a, v, r);
  }
  return a;
}

// g and the partner of permuted column `col` (front row list at `rows`), in the original numbering
__device__ __forceinline__ void pv_store(const PvPair& a, int col, const int* __restrict__ rows, const int* __restrict__ perm,
                                         double* __restrict__ g, int64_t* __restrict__ partner) {
  const int c = perm[col];
  const bool any = a.r != INT_MAX;
  g[c] = any ? a.v : 0.0;
  partner[c] = any ? (int64_t)perm[rows[a.r]] : (int64_t)-1;
}

// small fronts: one wave per front, looping over its columns (a column has fewer than small_max rows: one or two loads per lane)
__global__ __launch_bounds__(kPvThreads) void k_pv_small(const PvSmall* __restrict__ items, int64_t nitems, const double* __restrict__ arena,
                                                          const int* __restrict__ rows_all, const int* __restrict__ perm,
                                                          double* __restrict__ g, int64_t* __restrict__ partner) {
  const int lane = threadIdx.x & 63;
  const int64_t it = (int64_t)blockIdx.x * kPvWaves + (threadIdx.x >> 6);
  if (it >= nitems) return;
  const PvSmall F = items[it];
  const double* __restrict__ L = arena + F.L;
  const int* __restrict__ rows = rows_all + F.rows;
  for (int lc = 0; lc < F.k; ++lc) {
    const double* __restrict__ c = L + (int64_t)lc * F.f;
    PvPair a = pv_none();
    for (int i = lc + 1 + lane; i < F.f; i += 64) pv_take(a, pv_mag(c[i]), i);
    a = pv_wave_reduce(a);
    if (lane == 0) pv_store(a, F.col0 + lc, rows, perm, g, partner);
  }
}

// big fronts: one workgroup per chunk of a column.  A column starts at the odd or even arena entry lc * f + lc + 1: 16-byte loads on
// the aligned middle, single loads on the head and the tail.
__global__ __launch_bounds__(kPvThreads) void k_pv_big(const PvBig* __restrict__ items, const double* __restrict__ arena,
                                                        const int* __restrict__ rows_all, const int* __restrict__ perm,
                                                        double* __restrict__ g, int64_t* __restrict__ partner,
                                                        double* __restrict__ part_v, int* __restrict__ part_r) {
  __shared__ double sv[kPvWaves];
  __shared__ int sr[kPvWaves];
  const PvBig T = items[blockIdx.x];
  const int t = threadIdx.x;
  const int64_t lo = T.col + T.r0, hi = T.col + T.r1;      // arena entries [lo, hi)
  const int64_t alo = lo + (lo & 1), ahi = hi & ~(int64_t)1;   // the aligned middle [alo, ahi) (the arena itself is 256-byte aligned)
  PvPair a = pv_none();
  if (lo < hi) {
    if (t == 0 && (lo & 1)) pv_take(a, pv_mag(arena[lo]), T.r0);
    if (t == 1 && ahi < hi && ahi >= alo) pv_take(a, pv_mag(arena[ahi]), (int)(ahi - T.col));
    const double2* __restrict__ p2 = reinterpret_cast<const double2*>(arena + alo);
    const int64_t np = ahi > alo ? (ahi - alo) >> 1 : 0;
    const int r_alo = (int)(alo - T.col);
    for (int64_t q = t; q < np; q += kPvThreads) {
      const double2 x = p2[q];
      const int r = r_alo + 2 * (int)q;
      pv_take(a, pv_mag(x.x), r);
      pv_take(a, pv_mag(x.y), r + 1);
    }
  }
  a = pv_wave_reduce(a);
  if ((t & 63) == 0) { sv[t >> 6] = a.v; sr[t >> 6] = a.r; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < kPvWaves; ++w) pv_take(a, sv[w], sr[w]);
    if (T.part < 0) pv_store(a, T.out, rows_all + T.rows, perm, g, partner);
    else { part_v[T.part] = a.v; part_r[T.part] = a.r; }
  }
}

// columns of more than one chunk: their partial records, one thread per column
__global__ __launch_bounds__(kPvThreads) void k_pv_merge(const PvMerge* __restrict__ items, int64_t nitems, const double* __restrict__ part_v,
                                                          const int* __restrict__ part_r, const int* __restrict__ rows_all,
                                                          const int* __restrict__ perm, double* __restrict__ g, int64_t* __restrict__ partner) {
  const int64_t it = (int64_t)blockIdx.x * kPvThreads + threadIdx.x;
  if (it >= nitems) return;
  const PvMerge M = items[it];
  PvPair a = pv_none();
  for (int c = 0; c < M.nparts; ++c) pv_take(a, part_v[M.part0 + c], part_r[M.part0 + c]);
  pv_store(a, M.out, rows_all + M.rows, perm, g, partner);
}

// the variables of the Schur set (permuted columns c0 .. n - 1): g = 0, p = -1
__global__ void k_pv_fill(int c0, int n, const int* __restrict__ perm, double* __restrict__ g, int64_t* __restrict__ partner) {
  const int i = c0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = perm[i];
  g[c] = 0.0;
  partner[c] = -1;
}

// per block: columns with g > 1 / u, columns with g = +Inf, max g and the lowest original index that attains it
__global__ __launch_bounds__(kPvThreads) void k_pv_count(const double* __restrict__ g, int64_t n, double inv_u, PvCount* __restrict__ out) {
  __shared__ long long s_rej[kPvWaves], s_nf[kPvWaves], s_idx[kPvWaves];
  __shared__ double s_max[kPvWaves];
  long long rej = 0, nf = 0, idx = -1;
  double mx = -1.0;
  for (int64_t i = (int64_t)blockIdx.x * kPvThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPvThreads) {
    const double v = g[i];
    rej += v > inv_u;
    nf += v == __builtin_inf();
    if (v > mx) { mx = v; idx = i; }      // ascending i within a thread: the lowest index of a value comes first
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    rej += __shfl_xor(rej, off, 64);
    nf += __shfl_xor(nf, off, 64);
    const double v = __shfl_xor(mx, off, 64);
    const long long j = __shfl_xor(idx, off, 64);
    if (v > mx || (v == mx && j >= 0 && j < idx)) { mx = v; idx = j; }
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) { s_rej[t >> 6] = rej; s_nf[t >> 6] = nf; s_idx[t >> 6] = idx; s_max[t >> 6] = mx; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kPvWaves; ++w) {
      rej += s_rej[w];
      nf += s_nf[w];
      if (s_max[w] > mx || (s_max[w] == mx && s_idx[w] >= 0 && s_idx[w] < idx)) { mx = s_max[w]; idx = s_idx[w]; }
    }
    PvCount c;
    c.rejected = rej; c.nonfinite = nf; c.max_idx = idx; c.max_g = mx;
    out[blockIdx.x] = c;
  }
}

template <typename T>
std::string pv_upload(PivotWork& W, T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  const size_t bytes = std::max<size_t>(src.size() * sizeof(T), 8);
  if (hipMalloc((void**)dst, bytes) != hipSuccess) return "hipMalloc failed";
  W.allocs.push_back(*dst);
  W.bytes += (int64_t)bytes;
  if (!src.empty() && hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return "upload failed";
  return "";
}

template <typename T>
std::string pv_alloc(PivotWork& W, T** dst, int64_t count) {
  *dst = nullptr;
  const size_t bytes = std::max<size_t>((size_t)count * sizeof(T), 8);
  if (hipMalloc((void**)dst, bytes) != hipSuccess) return "hipMalloc failed";
  W.allocs.push_back(*dst);
  W.bytes += (int64_t)bytes;
  return "";
}

}  // namespace

void pivots_release(PivotWork& W) {
  for (void* p : W.allocs) (void)hipFree(p);
  W = PivotWork();
}

std::string pivots_setup(const Symbolic& S, const Numeric& N, PivotWork& W) {
  pivots_release(W);
  PvPlan P;
  std::string e = pivot_build_items(S, N.front_pos_host, N.small_max, N.schur_sn, P);
  if (!e.empty()) return e;
  if ((int64_t)P.big.size() > INT32_MAX) return "pivot report: too many column chunks for one launch";
  W.n = S.n;
  W.nschur = S.nschur;
  W.n_small = (int64_t)P.small.size();
  W.n_big = (int64_t)P.big.size();
  W.n_merge = (int64_t)P.merge.size();
  if (!(e = pv_upload(W, &W.small, P.small)).empty()) return e;
  if (!(e = pv_upload(W, &W.big, P.big)).empty()) return e;
  if (!(e = pv_upload(W, &W.merge, P.merge)).empty()) return e;
  if (!(e = pv_alloc(W, &W.g, S.n)).empty()) return e;
  if (!(e = pv_alloc(W, &W.partner, S.n)).empty()) return e;
  if (!(e = pv_alloc(W, &W.part_v, P.nparts)).empty()) return e;
  if (!(e = pv_alloc(W, &W.part_r, P.nparts)).empty()) return e;
  if (!(e = pv_alloc(W, &W.count, kPvCountBlocks)).empty()) return e;
  W.planned = true;
  return "";
}

std::string pivots_scan_enqueue(const Numeric& N, PivotWork& W, hipStream_t st) {
  const DevPlan& d = N.d;
  if (W.n_small > 0)
    k_pv_small<<<dim3((unsigned)((W.n_small + kPvWaves - 1) / kPvWaves)), dim3(kPvThreads), 0, st>>>(W.small, W.n_small, d.arena, d.rows, d.perm, W.g, W.partner);
  if (W.n_big > 0)
    k_pv_big<<<dim3((unsigned)W.n_big), dim3(kPvThreads), 0, st>>>(W.big, d.arena, d.rows, d.perm, W.g, W.partner, W.part_v, W.part_r);
  if (W.n_merge > 0)
    k_pv_merge<<<dim3((unsigned)((W.n_merge + kPvThreads - 1) / kPvThreads)), dim3(kPvThreads), 0, st>>>(W.merge, W.n_merge, W.part_v, W.part_r, d.rows, d.perm, W.g, W.partner);
  if (W.nschur > 0)
    k_pv_fill<<<dim3((unsigned)((W.nschur + kPvThreads - 1) / kPvThreads)), dim3(kPvThreads), 0, st>>>((int)(W.n - W.nschur), (int)W.n, d.perm, W.g, W.partner);
  const hipError_t he = hipGetLastError();
  if (he != hipSuccess) return std::string("pivot report launch failed: ") + hipGetErrorString(he);
  return "";
}

void pivots_count_enqueue(const PivotWork& W, double inv_u, hipStream_t st) {
  k_pv_count<<<dim3(kPvCountBlocks), dim3(kPvThreads), 0, st>>>(W.g, W.n, inv_u, W.count);
}

}  // namespace okkt
