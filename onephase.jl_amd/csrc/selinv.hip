// Selected inversion on the device: Z = F^-1 = L^-T D^-1 L^-1 on the stored supernodal pattern.
//
// A front with pivot columns P and off-diagonal rows R is taken in blocks of kSlB pivot columns, the last block first.  For block j
// (columns c0 .. c0 + w, rows below it B = c0 + w .. f, both front-local):
//   W_j   = L_{B,j} L_jj^-1
//   Z_Bj  = - Z_BB W_j
//   Z_jj  = L_jj^-T D_j^-1 L_jj^-1 - W_j' Z_Bj
// Z_BB is the trailing part of the front's dense inverse: the Z panel columns of the later blocks and Z_RR, which the front gathers
// from its ancestors' Z panels before its first block (R is a clique of the filled graph: every entry of Z_RR is stored in the panel
// of the supernode that owns its column).  The schedule walks the levels of the supernodal tree from the root down; a level is cut
// into chunks whose scratch (Z_RR, W, the partial products) fits a fixed budget, and every chunk runs a gather launch, a block-inverse
// launch, then two launches per block step.  No floating-point atomics and fixed summation orders: two calls on one factor give
// bitwise-identical Z.
#include <algorithm>
#include <cmath>

#include "selinv.h"

namespace okkt {

namespace {

// Z(i, j), i >= j global permuted indices, from the panel of the supernode that owns column j (NaN when (i, j) is not stored)
__device__ __forceinline__ double sl_lookup(const double* __restrict__ Z, const int64_t* __restrict__ zpos, const int* __restrict__ col2sn,
                                            const int* __restrict__ sn_col0, const int64_t* __restrict__ row_ptr, const int* __restrict__ rows,
                                            int i, int j) {
  const int t = col2sn[j];
  const int c0 = sn_col0[t], kt = sn_col0[t + 1] - c0;
  const int64_t rp = row_ptr[t];
  const int ft = (int)(row_ptr[t + 1] - rp);
  int pos;
  if (i < c0 + kt) {
    pos = i - c0;
  } else {
    int lo = kt, hi = ft;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rows[rp + mid] < i) lo = mid + 1; else hi = mid;
    }
    if (lo >= ft || rows[rp + lo] != i) return __builtin_nan("");
    pos = lo;
  }
  return Z[zpos[t] + pos + (int64_t)(j - c0) * ft];
}

// T = Z_RR of the front (both triangles): one workgroup per kSlGatherCols columns.  Columns that are pivots of the parent are read
// through the front's rel list (reverse extend-add); the others from the supernode that owns them.
__global__ void __launch_bounds__(256) k_sl_gather(const SlFront* __restrict__ fr, const SlItem* __restrict__ items, const double* __restrict__ Z,
                                                   const int64_t* __restrict__ zpos, const int* __restrict__ col2sn, const int* __restrict__ sn_col0,
                                                   const int64_t* __restrict__ row_ptr, const int* __restrict__ rows, const int64_t* __restrict__ rel_ptr,
                                                   const int* __restrict__ rel, double* __restrict__ scratch) {
  const SlItem it = items[blockIdx.x];
  const SlFront F = fr[it.slot];
  const int* R = rows + row_ptr[F.s] + F.k;
  const int* rl = rel + rel_ptr[F.s];
  double* T = scratch + F.T;
  int pk = 0, pf = 0;
  int64_t pz = 0;
  if (F.parent >= 0) {
    pk = sn_col0[F.parent + 1] - sn_col0[F.parent];
    pf = (int)(row_ptr[F.parent + 1] - row_ptr[F.parent]);
    pz = zpos[F.parent];
  }
  const int b1 = min(F.r, it.idx + kSlGatherCols);
  for (int b = it.idx; b < b1; ++b) {
    const int j = R[b];
    const int yb = rl[b];
    const bool in_parent = F.parent >= 0 && yb < pk;
    for (int a = b + threadIdx.x; a < F.r; a += blockDim.x) {
      double v;
      if (in_parent) v = Z[pz + rl[a] + (int64_t)yb * pf];
      else v = sl_lookup(Z, zpos, col2sn, sn_col0, row_ptr, rows, R[a], j);
      T[a + (int64_t)b * F.r] = v;
      T[b + (int64_t)a * F.r] = v;
    }
  }
}

// one workgroup per (front, block j): L_jj^-1 in LDS, W_j = L_{B,j} L_jj^-1, and Z_jj = L_jj^-T D_j^-1 L_jj^-1 (lower triangle)
__global__ void __launch_bounds__(256) k_sl_block(const SlFront* __restrict__ fr, const SlItem* __restrict__ items, const double* __restrict__ arena,
                                                  const double* __restrict__ dvals, double* __restrict__ Z, double* __restrict__ scratch) {
  __shared__ double Lb[kSlB][kSlB + 1];
  __shared__ double Li[kSlB][kSlB + 1];
  __shared__ double dinv[kSlB];
  const SlItem it = items[blockIdx.x];
  const SlFront F = fr[it.slot];
  const int c0 = it.idx * kSlB, w = min(kSlB, F.k - c0);
  const int64_t f = F.f;
  const double* L = arena + F.L;
  const int tid = threadIdx.x;
  for (int e = tid; e < kSlB * kSlB; e += blockDim.x) {
    const int x = e % kSlB, y = e / kSlB;
    Lb[x][y] = (x < w && y < x) ? L[(c0 + x) + (int64_t)(c0 + y) * f] : 0.0;
    Li[x][y] = (x == y && x < w) ? 1.0 : 0.0;
  }
  if (tid < w) dinv[tid] = 1.0 / dvals[F.col0 + c0 + tid];
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
  // Z_jj (lower): sum_{t >= x} Li[t][x] Li[t][y] / d_t, x >= y
  double* Zp = Z + F.Zp;
  for (int e = tid; e < w * w; e += blockDim.x) {
    const int x = e % w, y = e / w;
    if (x < y) continue;
    double s = 0.0;
    for (int t = x; t < w; ++t) s += Li[t][x] * Li[t][y] * dinv[t];
    Zp[(c0 + x) + (int64_t)(c0 + y) * f] = s;
  }
  // W_j rows below the block: one thread per row, kSlB columns
  double* Wp = scratch + F.W;
  for (int64_t x = c0 + w + tid; x < f; x += blockDim.x) {
    double acc[kSlB];
#pragma unroll
    for (int c = 0; c < kSlB; ++c) acc[c] = 0.0;
    for (int t = 0; t < w; ++t) {
      const double l = L[x + (int64_t)(c0 + t) * f];
#pragma unroll
      for (int c = 0; c < kSlB; ++c) acc[c] += l * Li[t][c];
    }
#pragma unroll
    for (int c = 0; c < kSlB; ++c)
      if (c < w) Wp[x + (int64_t)(c0 + c) * f] = acc[c];
  }
}

// one 64-row tile of Z_Bj = - Z_BB W_j for block j of its front, and the tile's partial W_j(tile)' Z_Bj(tile) for Z_jj.
// 256 threads, 4 x 4 outputs each; the reduction runs over the rows of B in 16-row slices through LDS.
constexpr int kSlKc = 16;
__global__ void __launch_bounds__(256) k_sl_cols(const SlFront* __restrict__ fr, const SlItem* __restrict__ items, int step, double* __restrict__ Z,
                                                 double* __restrict__ scratch) {
  __shared__ double sm[2 * kSlB * (kSlB + 1)];
  double(*As)[kSlB] = reinterpret_cast<double(*)[kSlB]>(sm);                        // [kSlKc][kSlB]: Z_BB(x, y), indexed [y][x]
  double(*Bs)[kSlB] = reinterpret_cast<double(*)[kSlB]>(sm + kSlKc * kSlB);         // [kSlKc][kSlB]: W(y, c)
  const SlItem it = items[blockIdx.x];
  const SlFront F = fr[it.slot];
  const int j = F.q - 1 - step;
  const int c0 = j * kSlB, w = min(kSlB, F.k - c0);
  const int j1 = c0 + w;
  const int f = F.f, k = F.k, r = F.r;
  const int x0 = j1 + it.idx * kSlB;
  const double* Zr = Z + F.Zp;
  const double* T = scratch + F.T;
  const double* Wp = scratch + F.W;
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.0;
  for (int y0 = j1; y0 < f; y0 += kSlKc) {
    // both operand slices: 1024 entries each, 4 per thread
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u;
      {
        const int xl = e % kSlB, yl = e / kSlB;
        const int x = x0 + xl, y = y0 + yl;
        double v = 0.0;
        if (x < f && y < f) {
          if (x >= k && y >= k) v = T[(x - k) + (int64_t)(y - k) * r];
          else if (x >= y) v = Zr[x + (int64_t)y * f];
          else v = Zr[y + (int64_t)x * f];
        }
        As[yl][xl] = v;
      }
      {
        const int yl = e % kSlKc, c = e / kSlKc;
        const int y = y0 + yl;
        Bs[yl][c] = (y < f && c < w) ? Wp[y + (int64_t)(c0 + c) * f] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int yl = 0; yl < kSlKc; ++yl) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[yl][ty * 4 + i];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = Bs[yl][tx * 4 + c];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] += a[i] * b[c];
    }
    __syncthreads();
  }
  // the tile of Z_Bj, and the partial for Z_jj from LDS copies of it and of W's rows
  double(*Zs)[kSlB + 1] = reinterpret_cast<double(*)[kSlB + 1]>(sm);
  double(*Ws)[kSlB + 1] = reinterpret_cast<double(*)[kSlB + 1]>(sm + kSlB * (kSlB + 1));
  double* Zw = Z + F.Zp;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int xl = ty * 4 + i, x = x0 + xl;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int cc = tx * 4 + c;
      const double v = (x < f && cc < w) ? -acc[i][c] : 0.0;
      Zs[xl][cc] = v;
      if (x < f && cc < w) Zw[x + (int64_t)(c0 + cc) * f] = v;
    }
  }
  for (int e = tid; e < kSlB * kSlB; e += blockDim.x) {
    const int xl = e % kSlB, c = e / kSlB, x = x0 + xl;
    Ws[xl][c] = (x < f && c < w) ? Wp[x + (int64_t)(c0 + c) * f] : 0.0;
  }
  __syncthreads();
  double* P = scratch + F.P + (int64_t)it.idx * kSlB * kSlB;
  double ps[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) ps[i][c] = 0.0;
#pragma unroll 2
  for (int xl = 0; xl < kSlB; ++xl) {
    double a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = Ws[xl][ty * 4 + i];
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = Zs[xl][tx * 4 + c];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) ps[i][c] += a[i] * b[c];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) P[(ty * 4 + i) + (tx * 4 + c) * kSlB] = ps[i][c];
}

// Z_jj -= sum of the row tiles' partials, in tile order (lower triangle); grid (fronts of the chunk, 16 slices of the block)
__global__ void __launch_bounds__(256) k_sl_diag_update(const SlFront* __restrict__ fr, int f_off, int step, double* __restrict__ Z,
                                                        const double* __restrict__ scratch) {
  const SlFront F = fr[f_off + blockIdx.x];
  const int j = F.q - 1 - step;
  if (j < 0) return;
  const int c0 = j * kSlB, w = min(kSlB, F.k - c0);
  const int m = F.f - (c0 + w);
  if (m <= 0) return;
  const int ntile = (m + kSlB - 1) / kSlB;
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int a = e % kSlB, c = e / kSlB;
  if (a >= w || c >= w || a < c) return;
  const double* P = scratch + F.P + e;
  double s = 0.0;
  for (int t = 0; t < ntile; ++t) s += P[(int64_t)t * kSlB * kSlB];
  Z[F.Zp + (c0 + a) + (int64_t)(c0 + c) * F.f] -= s;
}

// non-finite entries of the stored lower pattern of Z, one workgroup per column (integer atomics: the count is exact in any order)
__global__ void __launch_bounds__(256) k_sl_count(const double* __restrict__ Z, const int64_t* __restrict__ zpos, const int* __restrict__ col2sn,
                                                  const int* __restrict__ sn_col0, const int64_t* __restrict__ row_ptr,
                                                  unsigned long long* __restrict__ count) {
  const int j = blockIdx.x;
  const int t = col2sn[j];
  const int c = j - sn_col0[t];
  const int64_t f = row_ptr[t + 1] - row_ptr[t];
  const double* col = Z + zpos[t] + c * f;
  unsigned nf = 0;
  for (int64_t x = c + threadIdx.x; x < f; x += blockDim.x)
    if (!isfinite(col[x])) ++nf;
  __shared__ unsigned red[256];
  red[threadIdx.x] = nf;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0]) atomicAdd(count, (unsigned long long)red[0]);
}

__global__ void k_sl_export_diag(const double* __restrict__ Z, const int64_t* __restrict__ dpos, const int* __restrict__ perm, int64_t n,
                                 double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[perm[i]] = Z[dpos[i]];
}

__global__ void k_sl_export_pattern(const double* __restrict__ Z, const int64_t* __restrict__ zmap, int64_t nnz, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nnz) {
    const int64_t p = zmap[e];
    out[e] = p >= 0 ? Z[p] : __builtin_nan("");
  }
}

template <typename T>
std::string sl_upload(SelinvWork& W, T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  const size_t bytes = std::max<size_t>(src.size() * sizeof(T), 8);
  if (hipMalloc((void**)dst, bytes) != hipSuccess) return "hipMalloc failed";
  W.allocs.push_back(*dst);
  W.bytes += (int64_t)bytes;
  if (!src.empty() && hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return "upload failed";
  return "";
}

// front-local position of global row i in supernode t's row list, -1 when absent
int64_t sl_host_pos(const Symbolic& S, int t, int i) {
  const int c0 = S.sn_col0[t], kt = S.sn_col0[t + 1] - c0;
  if (i >= c0 && i < c0 + kt) return i - c0;
  const int* b = S.rows.data() + S.row_ptr[t] + kt;
  const int* e = S.rows.data() + S.row_ptr[t + 1];
  const int* p = std::lower_bound(b, e, i);
  if (p == e || *p != i) return -1;
  return kt + (p - b);
}

}  // namespace

void selinv_release(SelinvWork& W) {
  for (void* p : W.allocs) (void)hipFree(p);
  W = SelinvWork();
}

std::string selinv_setup(const Symbolic& S, const Numeric& N, const int64_t* colptr, const int64_t* rowval, SelinvWork& W, int skip_sn) {
  selinv_release(W);
  W.skip_sn = skip_sn;
  const int ns = S.nsuper;
  const int64_t n = S.n;
  auto fk = [&](int s, int& f, int& k) {
    f = (int)(S.row_ptr[s + 1] - S.row_ptr[s]);
    k = S.sn_col0[s + 1] - S.sn_col0[s];
  };
  // Z panels, packed (f x k each)
  W.zpos_host.assign(ns, 0);
  int64_t z = 0;
  for (int s = 0; s < ns; ++s) {
    int f, k;
    fk(s, f, k);
    W.zpos_host[s] = z;
    z += (int64_t)f * k;
  }
  W.z_doubles = z;
  // scratch of one front: Z_RR, W (panel shape), the partials of its widest block step
  auto need = [&](int s) {
    int f, k;
    fk(s, f, k);
    const int64_t r = f - k;
    return r * r + (int64_t)f * k + (int64_t)((f + kSlB - 1) / kSlB) * kSlB * kSlB;
  };
  int64_t budget = kSlChunkDoubles;
  for (int s = 0; s < ns; ++s) if (s != skip_sn) budget = std::max(budget, need(s));
  // levels from the root down, each cut into chunks within the budget
  std::vector<SlFront> fr;
  std::vector<SlItem> items;
  fr.reserve(ns);
  int64_t scratch_max = 0;
  double flops = 0;
  for (int l = S.nlevels - 1; l >= 0; --l) {
    int64_t p = S.level_ptr[l];
    const int64_t pe = S.level_ptr[l + 1];
    while (p < pe) {
      SlChunk C;
      C.f_off = (int)fr.size();
      int64_t used = 0;
      while (p < pe && (S.level_sn[p] == skip_sn || C.f_cnt == 0 || used + need(S.level_sn[p]) <= budget)) {
        const int s = S.level_sn[p++];
        if (s == skip_sn) continue;
        int f, k;
        fk(s, f, k);
        SlFront F;
        F.s = s; F.f = f; F.k = k; F.r = f - k; F.q = (k + kSlB - 1) / kSlB; F.col0 = S.sn_col0[s]; F.parent = S.sn_parent[s]; F.pad = 0;
        F.L = N.front_pos_host[s];
        F.Zp = W.zpos_host[s];
        F.T = used;
        F.W = F.T + (int64_t)F.r * F.r;
        F.P = F.W + (int64_t)f * k;
        used += need(s);
        fr.push_back(F);
        ++C.f_cnt;
      }
      if (C.f_cnt == 0) continue;      // the level held the skipped supernode alone
      scratch_max = std::max(scratch_max, used);
      C.g_off = (int64_t)items.size();
      for (int i = C.f_off; i < C.f_off + C.f_cnt; ++i)
        for (int b = 0; b < fr[i].r; b += kSlGatherCols) items.push_back({i, b});
      C.g_cnt = (int64_t)items.size() - C.g_off;
      C.w_off = (int64_t)items.size();
      for (int i = C.f_off; i < C.f_off + C.f_cnt; ++i) {
        C.nsteps = std::max(C.nsteps, fr[i].q);
        for (int j = 0; j < fr[i].q; ++j) items.push_back({i, j});
      }
      C.w_cnt = (int64_t)items.size() - C.w_off;
      for (int t = 0; t < C.nsteps; ++t) {
        C.z_off.push_back((int64_t)items.size());
        for (int i = C.f_off; i < C.f_off + C.f_cnt; ++i) {
          const SlFront& F = fr[i];
          const int j = F.q - 1 - t;
          if (j < 0) continue;
          const int w = std::min(kSlB, F.k - j * kSlB);
          const int m = F.f - (j * kSlB + w);
          flops += 2.0 * m * m * w + 2.0 * m * w * w;
          for (int tile = 0; tile * kSlB < m; ++tile) items.push_back({i, tile});
        }
        C.z_cnt.push_back((int64_t)items.size() - C.z_off.back());
      }
      W.chunks.push_back(std::move(C));
    }
  }
  if ((int)fr.size() != ns - (skip_sn >= 0 ? 1 : 0)) return "selected inversion: the level schedule does not cover every supernode";
  W.flops = flops;
  W.scratch_doubles = scratch_max;
  // diagonal positions and the map of the input entries (mirrored into the lower triangle of the permuted matrix)
  std::vector<int64_t> dpos(n), zmap;
  for (int64_t i = 0; i < n; ++i) {
    const int t = S.col2sn[i];
    int f, k;
    fk(t, f, k);
    const int64_t c = i - S.sn_col0[t];
    dpos[i] = W.zpos_host[t] + c + c * f;
  }
  const int64_t base = colptr[0];
  const int64_t nnz = colptr[n] - base;
  zmap.assign(nnz, -1);
  for (int64_t c = 0; c < n; ++c) {
    for (int64_t e = colptr[c] - base; e < colptr[c + 1] - base; ++e) {
      const int64_t rr = rowval[e] - base;
      if (rr < 0 || rr >= n) continue;
      int pi = S.iperm[rr], pj = S.iperm[c];
      if (pi < pj) std::swap(pi, pj);
      const int t = S.col2sn[pj];
      const int64_t pos = sl_host_pos(S, t, pi);
      if (pos < 0) continue;
      int f, k;
      fk(t, f, k);
      zmap[e] = W.zpos_host[t] + pos + (int64_t)(pj - S.sn_col0[t]) * f;
    }
  }
  std::string e;
  const size_t zb = (size_t)std::max<int64_t>(W.z_doubles, 1) * sizeof(double);
  const size_t sb = (size_t)std::max<int64_t>(W.scratch_doubles, 1) * sizeof(double);
  if (hipMalloc((void**)&W.Z, zb) != hipSuccess) return "Z arena: hipMalloc failed";
  W.allocs.push_back(W.Z);
  if (hipMalloc((void**)&W.scratch, sb) != hipSuccess) return "selected-inversion scratch: hipMalloc failed";
  W.allocs.push_back(W.scratch);
  if (hipMalloc((void**)&W.count, sizeof(unsigned long long)) != hipSuccess) return "hipMalloc failed";
  W.allocs.push_back(W.count);
  W.bytes += (int64_t)(zb + sb) + 8;
  if (hipMemset(W.Z, 0, zb) != hipSuccess) return "hipMemset failed";
  std::vector<int> col2sn(S.col2sn.begin(), S.col2sn.end());
  if (!(e = sl_upload(W, &W.zpos, W.zpos_host)).empty()) return e;
  if (!(e = sl_upload(W, &W.col2sn, col2sn)).empty()) return e;
  if (!(e = sl_upload(W, &W.fr, fr)).empty()) return e;
  if (!(e = sl_upload(W, &W.items, items)).empty()) return e;
  if (!(e = sl_upload(W, &W.dpos, dpos)).empty()) return e;
  if (!(e = sl_upload(W, &W.zmap, zmap)).empty()) return e;
  W.planned = true;
  return "";
}

std::string selinv_enqueue(const Numeric& N, SelinvWork& W) {
  const DevPlan& d = N.d;
  hipStream_t st = N.stream;
  (void)hipMemsetAsync(W.count, 0, sizeof(unsigned long long), st);
  for (const SlChunk& C : W.chunks) {
    if (C.g_cnt > 0)
      k_sl_gather<<<(unsigned)C.g_cnt, 256, 0, st>>>(W.fr, W.items + C.g_off, W.Z, W.zpos, W.col2sn, d.sn_col0, d.row_ptr, d.rows, d.rel_ptr, d.rel,
                                                     W.scratch);
    if (C.w_cnt > 0) k_sl_block<<<(unsigned)C.w_cnt, 256, 0, st>>>(W.fr, W.items + C.w_off, d.arena, d.dvals, W.Z, W.scratch);
    for (int t = 0; t < C.nsteps; ++t) {
      if (C.z_cnt[t] > 0) k_sl_cols<<<(unsigned)C.z_cnt[t], 256, 0, st>>>(W.fr, W.items + C.z_off[t], t, W.Z, W.scratch);
      k_sl_diag_update<<<dim3((unsigned)C.f_cnt, kSlB * kSlB / 256), 256, 0, st>>>(W.fr, C.f_off, t, W.Z, W.scratch);
    }
  }
  const int64_t n = (int64_t)N.d.n;
  if (n > 0) k_sl_count<<<(unsigned)n, 256, 0, st>>>(W.Z, W.zpos, W.col2sn, d.sn_col0, d.row_ptr, W.count);
  hipError_t he = hipGetLastError();
  if (he != hipSuccess) return std::string("selected inversion launch: ") + hipGetErrorString(he);
  return "";
}

void selinv_diag_enqueue(const Numeric& N, const SelinvWork& W, int64_t n, double* d_out, hipStream_t st) {
  if (n > 0) k_sl_export_diag<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(W.Z, W.dpos, N.d.perm, n, d_out);
}

void selinv_pattern_enqueue(const SelinvWork& W, int64_t nnz, double* d_out, hipStream_t st) {
  if (nnz > 0) k_sl_export_pattern<<<(unsigned)((nnz + 255) / 256), 256, 0, st>>>(W.Z, W.zmap, nnz, d_out);
}

}  // namespace okkt
