// Vector kernels of the block shift-invert Krylov-Schur method of okkt_eigs, gfx950.
//
// A sweep of the method (api_eigs.cpp) appends a block Q of p <= 4 columns to the basis V, applies the operator in one solve pass
// (W = Op Q, kept as OV) and orthogonalises W against the whole of V by classical Gram-Schmidt with one full reorthogonalisation:
//   k_eig_pass<P, -, dots>     C1 = V' W, which is also the new block column of the projected matrix G (each basis vector is read once
//                              for all P columns; chunks of kEigChunk basis vectors run as workgroups of their own)
//   k_eig_pass<P, orth, dots>  W = W - V C1, fused with the partial sums of C2 = V' W
//   k_eig_pass<P, orth, norm>  W = W - V C2, fused with the partial sums of the column norms
// each followed by k_eig_sum, one wave per value.  The columns of the block are then orthogonalised one after the other against the
// accepted ones with the same three passes (P = 1, a basis of at most three vectors), k_eig_scale divides by the norm.
// k_eig_ritz forms the residual norms ||OV s - theta V s|| of the leading Ritz pairs in one pass over V and OV, k_eig_compress the
// out-of-place products V S and OV S of a restart, k_eig_fill the hashed start block; k_eig_pad, k_eig_restrict, k_eig_lambda_b and
// k_eig_finish are the vector work of pencil mode and of the returned vectors.
//
// No floating-point atomics.  A reduction pass over len rows runs nb = min(ceil(len / 512), 256) workgroups over grid-stride loops; the
// partial of workgroup b goes to slot b of its value and k_eig_sum adds the nb partials of a value in a fixed order (four per lane in
// ascending order, then a butterfly).  The bits of a sum therefore depend on len alone, not on how many columns or basis vectors share
// the pass.
#include <algorithm>
#include <cmath>

#include "eigs.h"

namespace okkt {

namespace {

constexpr int kEigChunk = 8;      // basis vectors per accumulation chunk of a projection
constexpr int kEigRitzChunk = 8;  // Ritz pairs per workgroup row of k_eig_ritz
constexpr int kEigKeepChunk = 12; // output columns per workgroup row of k_eig_compress

// the sums of a[0..C) over the workgroup's 256 threads (4 waves of 64): a butterfly in each wave, the four waves added in order;
// thread t < cnt writes the sum of a[t] to out[slot(t) * nb]
template <int C, class Slot>
__device__ __forceinline__ void eig_block_sum(double* a, int cnt, double* __restrict__ out, int nb, Slot slot) {
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
    out[(size_t)slot(t) * nb] = ((sm[0][t] + sm[1][t]) + sm[2][t]) + sm[3][t];
  }
  __syncthreads();   // sm is reused by the next chunk
}

__global__ __launch_bounds__(256) void k_eig_fill(int64_t len, int64_t ld, int p, uint64_t seed, uint64_t col0, double* __restrict__ dst) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int c = 0; c < p; ++c) {
    const uint64_t sc = eigs_mix(eigs_mix(seed) + col0 + (uint64_t)c);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) {
      const uint64_t hsh = eigs_mix(sc + (uint64_t)i);
      dst[c * ld + i] = ((double)(hsh >> 11) * 0x1p-52 - 1.0) + 0x1p-53;
    }
  }
}

// One pass over nv basis vectors V[v * ld + i] and the P columns W[c * ld + i], rows i < len.
//   ORTH: W = W - V h (h[v * 4 + c], v ascending), stored back
//   DOTS: partials of V' W (after ORTH, if set) into part[(v * 4 + c) * nb + blockIdx.x]; without ORTH the chunk of basis vectors is
//         blockIdx.y, with it the workgroup loops over the chunks (it re-reads only the rows it has just written)
//   else: partials of the squared column norms into part[c * nb + blockIdx.x]
template <int P, bool ORTH, bool DOTS>
__global__ __launch_bounds__(256) void k_eig_pass(int64_t len, int64_t ld, int nv, const double* __restrict__ V, double* W,
                                                  const double* __restrict__ h, double* __restrict__ part, int nb) {
  const int64_t stride = (int64_t)nb * 256;
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double* out = part + blockIdx.x;
  if (!DOTS) {
    double acc[P];
#pragma unroll
    for (int c = 0; c < P; ++c) acc[c] = 0.0;
    for (int64_t i = i0; i < len; i += stride) {
      double x[P];
#pragma unroll
      for (int c = 0; c < P; ++c) x[c] = W[c * ld + i];
      if (ORTH) {
        for (int v = 0; v < nv; ++v) {
          const double b = V[v * ld + i];
#pragma unroll
          for (int c = 0; c < P; ++c) x[c] = x[c] - h[v * 4 + c] * b;
        }
#pragma unroll
        for (int c = 0; c < P; ++c) W[c * ld + i] = x[c];
      }
#pragma unroll
      for (int c = 0; c < P; ++c) acc[c] = acc[c] + x[c] * x[c];
    }
    eig_block_sum<P>(acc, P, out, nb, [](int t) { return t; });
    return;
  }
  if (ORTH)
    for (int64_t i = i0; i < len; i += stride) {
      double x[P];
#pragma unroll
      for (int c = 0; c < P; ++c) x[c] = W[c * ld + i];
      for (int v = 0; v < nv; ++v) {
        const double b = V[v * ld + i];
#pragma unroll
        for (int c = 0; c < P; ++c) x[c] = x[c] - h[v * 4 + c] * b;
      }
#pragma unroll
      for (int c = 0; c < P; ++c) W[c * ld + i] = x[c];   // re-read below by this thread only
    }
  const int cbeg = ORTH ? 0 : (int)blockIdx.y * kEigChunk;
  const int cend = ORTH ? nv : std::min(nv, cbeg + kEigChunk);
  for (int c0 = cbeg; c0 < cend; c0 += kEigChunk) {
    double acc[kEigChunk * P];
#pragma unroll
    for (int u = 0; u < kEigChunk * P; ++u) acc[u] = 0.0;
    for (int64_t i = i0; i < len; i += stride) {
      double x[P];
#pragma unroll
      for (int c = 0; c < P; ++c) x[c] = W[c * ld + i];
#pragma unroll
      for (int u = 0; u < kEigChunk; ++u)
        if (c0 + u < nv) {
          const double b = V[(c0 + u) * ld + i];
#pragma unroll
          for (int c = 0; c < P; ++c) acc[u * P + c] = acc[u * P + c] + b * x[c];
        }
    }
    const int cnt = std::min(kEigChunk, nv - c0) * P;
    eig_block_sum<kEigChunk * P>(acc, cnt, out, nb, [c0](int t) { return (c0 + t / P) * 4 + t % P; });
  }
}

// out[off + val] = the sum of part[val][0..nb) (root: its square root), val = blockIdx.x * ystride + blockIdx.y; nb <= 256: four
// partials per lane in ascending order, then a butterfly; one wave each
__global__ __launch_bounds__(64) void k_eig_sum(int nb, int ystride, int root, const double* __restrict__ part, double* __restrict__ out) {
  const int val = blockIdx.x * ystride + blockIdx.y, lane = threadIdx.x;
  const double* p = part + (size_t)val * nb;
  double a = 0.0;
  for (int k = lane; k < nb; k += 64) a = a + p[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);
  if (lane == 0) out[val] = root ? sqrt(a) : a;
}

__global__ __launch_bounds__(256) void k_eig_scale(int64_t len, const double* src, double* dst, const double* __restrict__ div) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const double d = *div;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) dst[i] = src[i] / d;
}

struct EigPairs {
  const double* in[2];
  double* out[2];
};

// out[z][j][i] = sum_v in[z][v][i] S[v][j] (v ascending) for the columns j of chunk blockIdx.y; S[v * kEigMaxKeep + j]
__global__ __launch_bounds__(256) void k_eig_compress(int64_t len, int64_t ld, int m, int keep, EigPairs A, const double* __restrict__ S) {
  const double* __restrict__ in = A.in[blockIdx.z];
  double* __restrict__ out = A.out[blockIdx.z];
  const int j0 = (int)blockIdx.y * kEigKeepChunk;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) {
    double acc[kEigKeepChunk];
#pragma unroll
    for (int u = 0; u < kEigKeepChunk; ++u) acc[u] = 0.0;
    for (int v = 0; v < m; ++v) {
      const double b = in[v * ld + i];
#pragma unroll
      for (int u = 0; u < kEigKeepChunk; ++u)
        if (j0 + u < keep) acc[u] = acc[u] + b * S[v * kEigMaxKeep + j0 + u];
    }
#pragma unroll
    for (int u = 0; u < kEigKeepChunk; ++u)
      if (j0 + u < keep) out[(j0 + u) * ld + i] = acc[u];
  }
}

// partials of ||OV s_j - theta_j V s_j||^2 for the Ritz pairs j of chunk blockIdx.y into part[j * nb + blockIdx.x]
__global__ __launch_bounds__(256) void k_eig_ritz(int64_t len, int64_t ld, int m, int k, const double* __restrict__ V, const double* __restrict__ OV,
                                                  const double* __restrict__ S, const double* __restrict__ theta, double* __restrict__ part, int nb) {
  const int j0 = (int)blockIdx.y * kEigRitzChunk;
  const int64_t stride = (int64_t)nb * 256;
  double acc[kEigRitzChunk];
#pragma unroll
  for (int u = 0; u < kEigRitzChunk; ++u) acc[u] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) {
    double a[kEigRitzChunk], b[kEigRitzChunk];
#pragma unroll
    for (int u = 0; u < kEigRitzChunk; ++u) { a[u] = 0.0; b[u] = 0.0; }
    for (int v = 0; v < m; ++v) {
      const double x = V[v * ld + i], y = OV[v * ld + i];
#pragma unroll
      for (int u = 0; u < kEigRitzChunk; ++u)
        if (j0 + u < k) {
          const double s = S[v * kEigMaxKeep + j0 + u];
          a[u] = a[u] + y * s;
          b[u] = b[u] + x * s;
        }
    }
#pragma unroll
    for (int u = 0; u < kEigRitzChunk; ++u)
      if (j0 + u < k) {
        const double r = a[u] - theta[j0 + u] * b[u];
        acc[u] = acc[u] + r * r;
      }
  }
  eig_block_sum<kEigRitzChunk>(acc, std::min(kEigRitzChunk, k - j0), part + blockIdx.x, nb, [j0](int t) { return j0 + t; });
}

__global__ __launch_bounds__(256) void k_eig_pad(int64_t len, int64_t dim, int p, const double* __restrict__ x, double* __restrict__ P) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int c = 0; c < p; ++c)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += stride) P[c * dim + i] = i < len ? x[c * dim + i] : 0.0;
}

__global__ __launch_bounds__(256) void k_eig_restrict(int64_t len, int64_t dim, int p, const double* __restrict__ Y, double* __restrict__ dst) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int c = 0; c < p; ++c)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) dst[c * dim + i] = Y[c * dim + i];
}

__global__ __launch_bounds__(256) void k_eig_lambda_b(int64_t len, int64_t dim, int p, EigsLam L, const double* __restrict__ v, double* __restrict__ P) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int c = 0; c < p; ++c)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += stride) P[c * dim + i] = i < len ? L.lam[c] * v[c * dim + i] : 0.0;
}

// column blockIdx.x of v: the sum of squares and the first entry of largest modulus over the leading len rows (thread t takes the rows
// t, t + 256, ...; the 256 results are combined by a fixed tree), then all dim rows scaled by sign / norm
__global__ __launch_bounds__(256) void k_eig_finish(int64_t len, int64_t dim, double* v) {
  __shared__ double ss[256], mx[256];
  __shared__ long long ix[256];
  double* x = v + (size_t)blockIdx.x * dim;
  const int t = threadIdx.x;
  double s = 0.0, m = -1.0;
  long long im = -1;
  for (int64_t i = t; i < len; i += 256) {
    const double a = x[i];
    s = s + a * a;
    if (fabs(a) > m) { m = fabs(a); im = i; }
  }
  ss[t] = s; mx[t] = m; ix[t] = im;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      ss[t] = ss[t] + ss[t + o];
      const bool take = mx[t + o] > mx[t] || (mx[t + o] == mx[t] && ix[t + o] >= 0 && (ix[t] < 0 || ix[t + o] < ix[t]));
      if (take) { mx[t] = mx[t + o]; ix[t] = ix[t + o]; }
    }
    __syncthreads();
  }
  const double nrm = sqrt(ss[0]);
  const long long i0 = ix[0];
  const double flip = (i0 >= 0 && x[i0] < 0.0) ? -1.0 : 1.0;
  __syncthreads();   // x[i0] is read before any thread scales it
  for (int64_t i = t; i < dim; i += 256) x[i] = flip * (x[i] / nrm);
}

inline unsigned grid_1d(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024)); }

template <int P>
void pass_launch(const EigsWork& W, int64_t len, const double* V, int nv, double* Wc, int mode, const double* h, hipStream_t st) {
  const dim3 b(256);
  if (mode == 0)
    hipLaunchKernelGGL((k_eig_pass<P, false, true>), dim3((unsigned)W.nb, (unsigned)((nv + kEigChunk - 1) / kEigChunk)), b, 0, st, len, W.dim, nv, V, Wc,
                       h, W.part, W.nb);
  else if (mode == 1)
    hipLaunchKernelGGL((k_eig_pass<P, true, true>), dim3((unsigned)W.nb), b, 0, st, len, W.dim, nv, V, Wc, h, W.part, W.nb);
  else if (nv > 0)
    hipLaunchKernelGGL((k_eig_pass<P, true, false>), dim3((unsigned)W.nb), b, 0, st, len, W.dim, nv, V, Wc, h, W.part, W.nb);
  else
    hipLaunchKernelGGL((k_eig_pass<P, false, false>), dim3((unsigned)W.nb), b, 0, st, len, W.dim, nv, V, Wc, h, W.part, W.nb);
}

void pass_dispatch(const EigsWork& W, int64_t len, const double* V, int nv, double* Wc, int p, int mode, const double* h, hipStream_t st) {
  switch (p) {
    case 1: pass_launch<1>(W, len, V, nv, Wc, mode, h, st); break;
    case 2: pass_launch<2>(W, len, V, nv, Wc, mode, h, st); break;
    case 3: pass_launch<3>(W, len, V, nv, Wc, mode, h, st); break;
    default: pass_launch<4>(W, len, V, nv, Wc, mode, h, st); break;
  }
}

}  // namespace

std::string eigs_alloc(int64_t dim, int mb, EigsWork& W) {
  if (W.base && W.dim == dim && W.mb >= mb) return std::string();
  eigs_release(W);
  const int64_t ld = std::max<int64_t>(dim, 1);
  const int64_t nbasis = (int64_t)mb * ld;
  const int64_t npart = (int64_t)(mb * 4 + kEigMaxNev) * kEigMaxWg;
  const int64_t nsd = (int64_t)kEigMaxBasis * kEigMaxKeep + kEigMaxNev;
  const int64_t total = 4 * nbasis + 3 * 4 * ld + kEigMaxNev * ld + npart + 2 * (int64_t)mb * 4 + nsd + kEigOut;
  double* p = nullptr;
  hipError_t e = hipMalloc((void**)&p, (size_t)total * sizeof(double));
  if (e != hipSuccess) { (void)hipGetLastError(); return std::string("hipMalloc: ") + hipGetErrorString(e); }
  W.dim = dim;
  W.mb = mb;
  W.base = p;
  W.V[0] = p; p += nbasis;
  W.V[1] = p; p += nbasis;
  W.OV[0] = p; p += nbasis;
  W.OV[1] = p; p += nbasis;
  W.Q = p; p += 4 * ld;
  W.P = p; p += 4 * ld;
  W.Y = p; p += 4 * ld;
  W.X = p; p += kEigMaxNev * ld;
  W.part = p; p += npart;
  W.c1 = p; p += (int64_t)mb * 4;
  W.c2 = p; p += (int64_t)mb * 4;
  W.sd = p; p += nsd;
  W.out = p;
  W.bytes = total * (int64_t)sizeof(double);
  return std::string();
}

void eigs_release(EigsWork& W) {
  if (W.base) (void)hipFree(W.base);
  W = EigsWork();
}

void eigs_fill_enqueue(const EigsWork& W, int64_t len, double* dst, int p, uint64_t seed, uint64_t col0, hipStream_t st) {
  if (len <= 0 || p <= 0) return;
  hipLaunchKernelGGL(k_eig_fill, dim3(grid_1d(len)), dim3(256), 0, st, len, W.dim, std::min(p, kEigMaxBlock), seed, col0, dst);
}

void eigs_project_enqueue(const EigsWork& W, int64_t len, const double* V, int nv, const double* Wc, int p, hipStream_t st) {
  if (len <= 0 || p <= 0 || nv <= 0) return;
  p = std::min(p, kEigMaxBlock);
  pass_dispatch(W, len, V, nv, const_cast<double*>(Wc), p, 0, W.c1, st);
  hipLaunchKernelGGL(k_eig_sum, dim3((unsigned)nv, (unsigned)p), dim3(64), 0, st, W.nb, 4, 0, W.part, W.c1);
}

void eigs_orth_project_enqueue(const EigsWork& W, int64_t len, const double* V, int nv, double* Wc, int p, hipStream_t st) {
  if (len <= 0 || p <= 0 || nv <= 0) return;
  p = std::min(p, kEigMaxBlock);
  pass_dispatch(W, len, V, nv, Wc, p, 1, W.c1, st);
  hipLaunchKernelGGL(k_eig_sum, dim3((unsigned)nv, (unsigned)p), dim3(64), 0, st, W.nb, 4, 0, W.part, W.c2);
}

void eigs_orth_norm_enqueue(const EigsWork& W, int64_t len, const double* V, int nv, double* Wc, int p, int off, hipStream_t st) {
  if (len <= 0 || p <= 0) return;
  p = std::min(p, kEigMaxBlock);
  pass_dispatch(W, len, V, nv, Wc, p, 2, W.c2, st);
  hipLaunchKernelGGL(k_eig_sum, dim3((unsigned)p, 1), dim3(64), 0, st, W.nb, 1, 1, W.part, W.out + off);
}

void eigs_scale_enqueue(const EigsWork& W, int64_t len, const double* src, double* dst, int off, hipStream_t st) {
  if (len <= 0) return;
  hipLaunchKernelGGL(k_eig_scale, dim3(grid_1d(len)), dim3(256), 0, st, len, src, dst, W.out + off);
}

void eigs_compress_enqueue(const EigsWork& W, int64_t len, int m, int keep, const double* in0, double* out0, const double* in1, double* out1,
                           int cnt, hipStream_t st) {
  if (len <= 0 || m <= 0 || keep <= 0) return;
  keep = std::min(keep, kEigMaxKeep);
  EigPairs A;
  A.in[0] = in0; A.out[0] = out0;
  A.in[1] = cnt > 1 ? in1 : in0; A.out[1] = cnt > 1 ? out1 : out0;
  hipLaunchKernelGGL(k_eig_compress, dim3(grid_1d(len), (unsigned)((keep + kEigKeepChunk - 1) / kEigKeepChunk), (unsigned)(cnt > 1 ? 2 : 1)), dim3(256), 0,
                     st, len, W.dim, m, keep, A, W.sd);
}

void eigs_ritz_enqueue(const EigsWork& W, int64_t len, int m, int k, const double* V, const double* OV, hipStream_t st) {
  if (len <= 0 || m <= 0 || k <= 0) return;
  k = std::min(k, kEigMaxNev);
  hipLaunchKernelGGL(k_eig_ritz, dim3((unsigned)W.nb, (unsigned)((k + kEigRitzChunk - 1) / kEigRitzChunk)), dim3(256), 0, st, len, W.dim, m, k, V, OV, W.sd,
                     W.sd + (size_t)kEigMaxBasis * kEigMaxKeep, W.part, W.nb);
  hipLaunchKernelGGL(k_eig_sum, dim3((unsigned)k, 1), dim3(64), 0, st, W.nb, 1, 1, W.part, W.out);
}

void eigs_pad_enqueue(const EigsWork& W, int64_t len, const double* x, int p, hipStream_t st) {
  if (W.dim <= 0 || p <= 0) return;
  hipLaunchKernelGGL(k_eig_pad, dim3(grid_1d(W.dim)), dim3(256), 0, st, len, W.dim, std::min(p, kEigMaxBlock), x, W.P);
}

void eigs_restrict_enqueue(const EigsWork& W, int64_t len, double* dst, int p, hipStream_t st) {
  if (len <= 0 || p <= 0) return;
  hipLaunchKernelGGL(k_eig_restrict, dim3(grid_1d(len)), dim3(256), 0, st, len, W.dim, std::min(p, kEigMaxBlock), W.Y, dst);
}

void eigs_lambda_b_enqueue(const EigsWork& W, int64_t len, const double* v, int p, const EigsLam& L, hipStream_t st) {
  if (W.dim <= 0 || p <= 0) return;
  hipLaunchKernelGGL(k_eig_lambda_b, dim3(grid_1d(W.dim)), dim3(256), 0, st, len, W.dim, std::min(p, kEigMaxBlock), L, v, W.P);
}

void eigs_finish_enqueue(const EigsWork& W, int64_t len, double* v, int nvec, hipStream_t st) {
  if (W.dim <= 0 || nvec <= 0) return;
  hipLaunchKernelGGL(k_eig_finish, dim3((unsigned)std::min(nvec, kEigMaxNev)), dim3(256), 0, st, len, W.dim, v);
}

}  // namespace okkt
