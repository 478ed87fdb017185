// Vector kernels of GMRES-based iterative refinement, gfx950.
//
// The GMRES cycles of okkt_solve_gmres (api_refine.cpp) orthogonalise each new vector w = A F^-1 v_j against the basis V = [v_0 .. v_j]
// by classical Gram-Schmidt with one full reorthogonalisation (CGS2).  Per iteration three passes over V:
//   k_kry_pass<dots>        h1 = V^T w (w read once per chunk of 16 basis vectors)
//   k_kry_pass<orth, dots>  w = w - V h1, fused with the partial sums of h2 = V^T w
//   k_kry_pass<orth, norm>  w = w - V h2, fused with the partial sums of ||w||^2
// each followed by a one-wave-per-value final sum (k_kry_sum, k_kry_norm_final), and v_j+1 = w / h_j+1,j (k_kry_scale) once the host
// has read the column.  k_kry_combine forms V y for the correction.
//
// No floating-point atomics.  A pass runs nb workgroups per system (nb a function of n alone, <= 64, so <= 256 workgroups for four
// systems) over grid-stride loops; each workgroup's partial goes to its own slot of `part`, and the final kernel adds the nb partials
// of a value in a fixed butterfly.  A system's bits therefore depend neither on its slot nor on how many systems share the pass.
#include <algorithm>
#include <cmath>

#include "krylov.h"

namespace okkt {

namespace {

constexpr int kKryChunk = 16;   // basis vectors per accumulation chunk of a dot pass

// the sum of a[0..C) over the workgroup's 256 threads (4 waves of 64): a butterfly in each wave, the four waves added in order;
// thread t < cnt writes the sum of a[t] to out[t * nb]
template <int C>
__device__ __forceinline__ void block_sum(double* a, int cnt, double* __restrict__ out, int nb) {
  __shared__ double sm[4][C];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int u = 0; u < C; ++u) a[u] = a[u] + __shfl_xor(a[u], o, 64);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int u = 0; u < C; ++u) sm[wv][u] = a[u];
  __syncthreads();
  if ((int)threadIdx.x < cnt) {
    const int t = threadIdx.x;
    out[(size_t)t * nb] = ((sm[0][t] + sm[1][t]) + sm[2][t]) + sm[3][t];
  }
  __syncthreads();   // sm is reused by the next chunk
}

// One pass over the nv basis vectors of system blockIdx.y.
//   NEG:  w holds -w (the operator product comes from the residual kernel with b = 0); it is read negated
//   ORTH: w = w - V h (h = hin[s], v ascending), stored back
//   DOTS: partials of V^T w (after ORTH, if set) into part[s][v][blockIdx.x]; else partials of ||w||^2 into part[s][0][blockIdx.x]
template <bool NEG, bool ORTH, bool DOTS>
__global__ __launch_bounds__(256) void k_kry_pass(int64_t n, int nv, KrySet S, const double* __restrict__ hin, double* __restrict__ part,
                                                  int nb) {
  const int s = blockIdx.y;
  const double* __restrict__ V = S.v[s];
  double* __restrict__ w = S.w[s];
  const int64_t vs = S.vstride;
  const int64_t stride = (int64_t)nb * 256;
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double* out = part + (size_t)s * kKryCol * nb + blockIdx.x;
  const double* h = hin + (size_t)s * kKryCol;
  if (!DOTS) {
    double acc[1] = {0.0};
    for (int64_t i = i0; i < n; i += stride) {
      double x = NEG ? -w[i] : w[i];
      if (ORTH) {
        for (int v = 0; v < nv; ++v) x = x - h[v] * V[v * vs + i];
        w[i] = x;
      }
      acc[0] = acc[0] + x * x;
    }
    block_sum<1>(acc, 1, out, nb);
    return;
  }
  if (ORTH)
    for (int64_t i = i0; i < n; i += stride) {
      double x = NEG ? -w[i] : w[i];
      for (int v = 0; v < nv; ++v) x = x - h[v] * V[v * vs + i];
      w[i] = x;   // re-read below by this thread only
    }
  for (int c0 = 0; c0 < nv; c0 += kKryChunk) {
    double acc[kKryChunk];
#pragma unroll
    for (int u = 0; u < kKryChunk; ++u) acc[u] = 0.0;
    for (int64_t i = i0; i < n; i += stride) {
      const double x = (NEG && !ORTH) ? -w[i] : w[i];
#pragma unroll
      for (int u = 0; u < kKryChunk; ++u)
        if (c0 + u < nv) acc[u] = acc[u] + V[(c0 + u) * vs + i] * x;
    }
    block_sum<kKryChunk>(acc, std::min(kKryChunk, nv - c0), out + (size_t)c0 * nb, nb);
  }
}

// out[s][v] = the sum of part[s][v][0..nb) (nb <= 64: one partial per lane, a butterfly); grid (nv, nr), one wave each
__global__ __launch_bounds__(64) void k_kry_sum(int nb, const double* __restrict__ part, double* __restrict__ out) {
  const int v = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  double a = lane < nb ? part[((size_t)s * kKryCol + v) * nb + lane] : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);
  if (lane == 0) out[(size_t)s * kKryCol + v] = a;
}

// col[s][nv] = sqrt(sum of part[s][0][0..nb)); col[s][0..nv) = h1 + h2 (nv = 0: the norm alone, at index 0); grid (1, nr)
__global__ __launch_bounds__(64) void k_kry_norm_final(int nb, int nv, const double* __restrict__ part, const double* __restrict__ h1,
                                                       const double* __restrict__ h2, double* __restrict__ col) {
  const int s = blockIdx.y, lane = threadIdx.x;
  double a = lane < nb ? part[(size_t)s * kKryCol * nb + lane] : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);
  double* c = col + (size_t)s * kKryCol;
  if (lane == 0) c[nv] = sqrt(a);
  for (int t = lane; t < nv; t += 64) c[t] = h1[(size_t)s * kKryCol + t] + h2[(size_t)s * kKryCol + t];
}

__global__ __launch_bounds__(256) void k_kry_scale(int64_t n, int nr, KryScale S) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int s = 0; s < nr; ++s) {
    const double d = *S.div[s];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) S.dst[s][i] = S.src[s][i] / d;
  }
}

__global__ __launch_bounds__(256) void k_kry_combine(int64_t n, int nr, KryCombine C) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int s = 0; s < nr; ++s) {
    const double* __restrict__ V = C.v[s];
    const int m = C.m[s];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
      double u = 0.0;
      for (int k = 0; k < m; ++k) u = u + C.y[s][k] * V[k * C.vstride + i];
      C.u[s][i] = u;
    }
  }
}

inline unsigned grid_1d(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256)); }

}  // namespace

std::string krylov_alloc(int64_t n, int restart, KrylovWork& K) {
  if (K.V && K.n == n && K.restart >= restart) return std::string();
  krylov_release(K);
  const int64_t nv = (int64_t)(restart + 1) * 4 * n, nvec = 4 * n;
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048, 64));
  const int64_t total = nv + 7 * nvec + n + (int64_t)4 * kKryCol * nb + 3 * 4 * kKryCol + 16;
  double* p = nullptr;
  hipError_t e = hipMalloc((void**)&p, (size_t)std::max<int64_t>(total, 2) * sizeof(double));
  if (e != hipSuccess) return std::string("hipMalloc: ") + hipGetErrorString(e);
  K.n = n;
  K.restart = restart;
  K.nb = nb;
  K.V = p; p += nv;
  K.W = p; p += nvec;
  K.Z = p; p += nvec;
  K.P = p; p += nvec;
  K.B = p; p += nvec;
  K.R = p; p += nvec;
  K.U = p; p += nvec;
  K.XP = p; p += nvec;
  K.zero = p; p += n;
  K.part = p; p += (int64_t)4 * kKryCol * nb;
  K.h1 = p; p += 4 * kKryCol;
  K.h2 = p; p += 4 * kKryCol;
  K.col = p; p += 4 * kKryCol;
  K.om = p;
  K.bytes = total * (int64_t)sizeof(double);
  e = hipMemset(K.zero, 0, (size_t)std::max<int64_t>(n, 1) * sizeof(double));
  if (e != hipSuccess) { krylov_release(K); return std::string("hipMemset: ") + hipGetErrorString(e); }
  return std::string();
}

void krylov_release(KrylovWork& K) {
  if (K.V) (void)hipFree(K.V);
  K = KrylovWork();
}

void krylov_dots_enqueue(const KrylovWork& K, const KrySet& S, int nr, int nv, bool neg, hipStream_t st) {
  if (nr <= 0 || nv <= 0) return;
  const dim3 g((unsigned)K.nb, (unsigned)nr), b(256);
  if (neg) hipLaunchKernelGGL((k_kry_pass<true, false, true>), g, b, 0, st, K.n, nv, S, K.h1, K.part, K.nb);
  else hipLaunchKernelGGL((k_kry_pass<false, false, true>), g, b, 0, st, K.n, nv, S, K.h1, K.part, K.nb);
  hipLaunchKernelGGL(k_kry_sum, dim3((unsigned)nv, (unsigned)nr), dim3(64), 0, st, K.nb, K.part, K.h1);
}

void krylov_orth_dots_enqueue(const KrylovWork& K, const KrySet& S, int nr, int nv, bool neg, hipStream_t st) {
  if (nr <= 0 || nv <= 0) return;
  const dim3 g((unsigned)K.nb, (unsigned)nr), b(256);
  if (neg) hipLaunchKernelGGL((k_kry_pass<true, true, true>), g, b, 0, st, K.n, nv, S, K.h1, K.part, K.nb);
  else hipLaunchKernelGGL((k_kry_pass<false, true, true>), g, b, 0, st, K.n, nv, S, K.h1, K.part, K.nb);
  hipLaunchKernelGGL(k_kry_sum, dim3((unsigned)nv, (unsigned)nr), dim3(64), 0, st, K.nb, K.part, K.h2);
}

void krylov_orth_norm_enqueue(const KrylovWork& K, const KrySet& S, int nr, int nv, hipStream_t st) {
  if (nr <= 0) return;
  hipLaunchKernelGGL((k_kry_pass<false, true, false>), dim3((unsigned)K.nb, (unsigned)nr), dim3(256), 0, st, K.n, nv, S, K.h2, K.part, K.nb);
  hipLaunchKernelGGL(k_kry_norm_final, dim3(1, (unsigned)nr), dim3(64), 0, st, K.nb, nv, K.part, K.h1, K.h2, K.col);
}

void krylov_norm_enqueue(const KrylovWork& K, const KrySet& S, int nr, hipStream_t st) {
  if (nr <= 0) return;
  hipLaunchKernelGGL((k_kry_pass<false, false, false>), dim3((unsigned)K.nb, (unsigned)nr), dim3(256), 0, st, K.n, 0, S, K.h1, K.part, K.nb);
  hipLaunchKernelGGL(k_kry_norm_final, dim3(1, (unsigned)nr), dim3(64), 0, st, K.nb, 0, K.part, K.h1, K.h2, K.col);
}

void krylov_scale_enqueue(int64_t n, const KryScale& S, int nr, hipStream_t st) {
  if (n <= 0 || nr <= 0) return;
  hipLaunchKernelGGL(k_kry_scale, dim3(grid_1d(n)), dim3(256), 0, st, n, std::min(nr, 4), S);
}

void krylov_combine_enqueue(int64_t n, const KryCombine& C, int nr, hipStream_t st) {
  if (n <= 0 || nr <= 0) return;
  hipLaunchKernelGGL(k_kry_combine, dim3(grid_1d(n)), dim3(256), 0, st, n, std::min(nr, 4), C);
}

}  // namespace okkt
