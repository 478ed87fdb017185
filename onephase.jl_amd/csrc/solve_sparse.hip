// Sparse right-hand sides, device side, gfx950.
//
// A pruned solve is the ordinary sweeps (solve.hip, unchanged kernels) launched on sublists of the level lists, between three small
// kernels of this file: k_sp_prepare zeroes what the sweeps would otherwise have computed as zero or would read from the previous solve
// (xwork on the pivot columns of the fronts the forward sweep runs, zwork on those only the backward sweep runs, the contribution
// vectors of the fringe), k_sp_scatter puts the non-zeros of b where solve_permute_in would have put them, k_sp_gather reads the wanted
// entries as solve_permute_out does.  Nothing here sums: the values are those of the dense solve, entry for entry.
#include "solve_sparse.h"

#include <algorithm>
#include <cstring>

namespace okkt {

#define OKKT_HIP_TRY(expr)                                                         \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess)                                                         \
      return std::string(#expr) + ": " + hipGetErrorString(e__);                   \
  } while (0)

typedef double d2_t __attribute__((ext_vector_type(2)));

// One workgroup per item = (front, kind, chunk of kSpChunk entries): zero that chunk of the front's pivot columns in xwork / zwork or of
// its contribution vector, for R right-hand sides.  16-byte stores between an 8-byte head and tail where the start is odd.  No atomics:
// every entry has one owner.
template <int R>
__global__ __launch_bounds__(256) void k_sp_prepare(DevPlan P, const int2* __restrict__ items) {
  const int2 it = items[blockIdx.x];
  const int s = it.x, kind = it.y & 3, chunk = it.y >> 2;
  const int col0 = P.sn_col0[s];
  const int k = P.sn_col0[s + 1] - col0;
  double* base;
  int64_t stride;
  int len;
  if (kind == kSpZeroCv) {
    base = P.cv + P.cv_pos[s];
    stride = P.cv_stride;
    len = (int)(P.row_ptr[s + 1] - P.row_ptr[s]) - k;
  } else {
    base = (kind == kSpZeroX ? P.xwork : P.zwork) + col0;
    stride = P.xw_stride;
    len = k;
  }
  const int lo = chunk * kSpChunk, hi = min(len, lo + kSpChunk);
  if (lo >= hi) return;
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < R; ++q) {
    double* p = base + (size_t)q * stride;
    const int a = lo + (int)(((uintptr_t)(p + lo) >> 3) & 1);      // first 16-byte aligned entry
    if (a > lo && tid == 0) p[lo] = 0.0;
    const int npair = (hi - a) / 2;
    for (int i = tid; i < npair; i += 256) *(d2_t*)(p + a + 2 * i) = (d2_t){0.0, 0.0};
    if (((hi - a) & 1) && tid == 0) p[hi - 1] = 0.0;
  }
}

// the entries of a batch's columns one after another: entry t belongs to column q with c[q] <= t < c[q + 1]
struct SpCols { int c[kMaxRhs + 1]; };

// xwork[q][pos[t]] = s_g * val[t], g = perm[pos[t]]: the value solve_permute_in stores there
template <bool SC>
__global__ __launch_bounds__(256) void k_sp_scatter(DevPlan P, const int* __restrict__ pos, SpCols C, const double* __restrict__ val, const double* __restrict__ sc) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= C.c[kMaxRhs]) return;
  int q = 0;
#pragma unroll
  for (int u = 1; u < kMaxRhs; ++u) q += t >= C.c[u];
  const int i = pos[t];
  const double v = val[t];
  P.xwork[(size_t)q * P.xw_stride + i] = SC ? v * sc[P.perm[i]] : v;
}

// out[q * stride + t] = s_g * xwork[q][pos[t]]: the value solve_permute_out stores at original index g = perm[pos[t]]
template <bool SC>
__global__ __launch_bounds__(256) void k_sp_gather(DevPlan P, const int* __restrict__ pos, int64_t nx, int nr, double* __restrict__ out, int64_t stride,
                                                   const unsigned long long* __restrict__ tmo, const double* __restrict__ sc) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nx) return;
  const int i = pos[t];
  const bool lost = __hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;      // as k_permute_out_r: no solution rather than a wrong one
  const double sg = SC ? sc[P.perm[i]] : 1.0;
  for (int q = 0; q < nr; ++q) {
    double v = lost ? __builtin_nan("") : P.xwork[(size_t)q * P.xw_stride + i];
    if (SC) v = v * sg;
    out[(size_t)q * stride + t] = v;
  }
}

void sparse_release(SparseWork& W) {
  if (W.pinned) (void)hipHostFree(W.pinned);
  if (W.d_lists) (void)hipFree(W.d_lists);
  if (W.d_xsel) (void)hipFree(W.d_xsel);
  if (W.d_ones) (void)hipFree(W.d_ones);
  if (W.copied) (void)hipEventDestroy(W.copied);
  W.pinned = W.d_lists = W.d_xsel = nullptr;
  W.d_ones = nullptr;
  W.copied = nullptr;
  W.cap = W.xsel_cap = W.ones_cap = 0;
  W.copy_pending = false;
  W.plan_analysis = -1;
  W.plan_arena = nullptr;
}

// where every unit stands in the schedules of the device plan
std::string sparse_plan_setup(const Symbolic& S, Numeric& N, SparseWork& W) {
  const int ns = S.nsuper;
  W.unit_pos.assign(ns, -1);
  W.unit_level.assign(ns, -1);
  W.unit_kind.assign(ns, -1);
  W.nsched = (int)N.sched_host.size();
  for (size_t l = 0; l < N.levels.size(); ++l) {
    for (int c = 0; c < 3; ++c) {
      const Segment& g = N.levels[l].seg[c];
      for (int q = 0; q < g.cnt; ++q) {
        const int s = N.sched_host[g.off + q];
        W.unit_pos[s] = g.off + q; W.unit_level[s] = (int)l; W.unit_kind[s] = (signed char)c;
      }
    }
    const SolveLevel& L = N.slevels[l];
    for (int q = 0; q < L.thin_cnt; ++q) {
      const int s = N.ssched_host[L.thin_off + q];
      W.unit_pos[s] = W.nsched + L.thin_off + q; W.unit_level[s] = (int)l; W.unit_kind[s] = 3;
    }
    for (int q = 0; q < L.wide_cnt; ++q) {
      const int s = N.ssched_host[L.wide_off + q];
      W.unit_pos[s] = W.nsched + L.wide_off + q; W.unit_level[s] = (int)l; W.unit_kind[s] = 4;
    }
  }
  for (int s = 0; s < ns; ++s)
    if (W.U.unit_root[s] == s && W.unit_kind[s] < 0) return "a unit of the analysis is in no schedule of the device plan";
  if (!W.copied) OKKT_HIP_TRY(hipEventCreateWithFlags(&W.copied, hipEventDisableTiming));
  return "";
}

namespace {
// the pinned buffer and its device twin hold at least `need` ints (grown; the stream is idle when they are replaced)
std::string reserve_lists(Numeric& N, SparseWork& W, int64_t need) {
  if (W.cap >= need) return "";
  OKKT_HIP_TRY(hipStreamSynchronize(N.stream));
  W.copy_pending = false;
  if (W.pinned) (void)hipHostFree(W.pinned);
  if (W.d_lists) (void)hipFree(W.d_lists);
  W.pinned = W.d_lists = nullptr;
  W.cap = 0;
  const int64_t cap = std::max<int64_t>(need + need / 2, 4096);
  OKKT_HIP_TRY(hipHostMalloc((void**)&W.pinned, (size_t)cap * sizeof(int), hipHostMallocDefault));
  OKKT_HIP_TRY(hipMalloc((void**)&W.d_lists, (size_t)cap * sizeof(int)));
  W.cap = cap;
  return "";
}

// the active units of one sweep in the order of the full lists, appended to `buf`; the level views that index them
void sublists(const Numeric& N, const SparseWork& W, std::vector<int> units, std::vector<int>& buf, std::vector<LevelSchedule>& lv, std::vector<SolveLevel>& sl) {
  std::sort(units.begin(), units.end(), [&](int a, int b) { return W.unit_pos[a] < W.unit_pos[b]; });
  lv = N.levels;
  sl = N.slevels;
  for (size_t l = 0; l < lv.size(); ++l) {      // (the bounds of a level hold for any part of it)
    for (int c = 0; c < 3; ++c) lv[l].seg[c].cnt = 0;
    sl[l].thin_cnt = sl[l].wide_cnt = 0;
  }
  const int base = (int)buf.size();
  for (int u : units) {
    const int at = (int)buf.size() - base, l = W.unit_level[u], kind = W.unit_kind[u];
    if (kind < 3) { Segment& g = lv[l].seg[kind]; if (!g.cnt++) g.off = at; }
    else if (kind == 3) { if (!sl[l].thin_cnt++) sl[l].thin_off = at; }
    else { if (!sl[l].wide_cnt++) sl[l].wide_off = at; }
    buf.push_back(u);
  }
}

void add_items(const Symbolic& S, const std::vector<int>& fronts, int kind, std::vector<int>& buf) {
  for (int s : fronts) {
    const int k = S.sn_col0[s + 1] - S.sn_col0[s];
    const int len = kind == kSpZeroCv ? (int)(S.row_ptr[s + 1] - S.row_ptr[s]) - k : k;
    for (int c = 0; c * kSpChunk < len; ++c) { buf.push_back(s); buf.push_back(kind | (c << 2)); }
  }
}
}  // namespace

std::string sparse_batch_enqueue(const Symbolic& S, Numeric& N, SparseWork& W, const SparseSets& A, const SparseScatter& sc, const double* d_val, const double* d_scale, int R) {
  hipStream_t st = N.stream;
  // one packed buffer: [forward sublists | backward sublists | prepare items (pairs) | scatter positions]
  std::vector<int> buf;
  std::vector<LevelSchedule> flv, blv;
  std::vector<SolveLevel> fsl, bsl;
  const int f_off = 0;
  if (!A.fwd_full) sublists(N, W, A.fwd_units, buf, flv, fsl);
  const int b_off = (int)buf.size();
  if (!A.bwd_full) sublists(N, W, A.bwd_units, buf, blv, bsl);
  if (buf.size() & 1) buf.push_back(0);      // the items are read as int2
  const int i_off = (int)buf.size();
  add_items(S, A.fwd_fronts, kSpZeroX, buf);
  add_items(S, A.bwd_only_fronts, kSpZeroZ, buf);
  add_items(S, A.fringe_fronts, kSpZeroCv, buf);
  const int n_items = ((int)buf.size() - i_off) / 2;
  const int p_off = (int)buf.size();
  buf.insert(buf.end(), sc.pos, sc.pos + sc.count);
  std::string e = reserve_lists(N, W, (int64_t)buf.size());
  if (!e.empty()) return e;
  if (W.copy_pending) { OKKT_HIP_TRY(hipEventSynchronize(W.copied)); W.copy_pending = false; }      // the last batch's copy has read the pinned buffer
  if (!buf.empty()) {
    std::memcpy(W.pinned, buf.data(), buf.size() * sizeof(int));
    OKKT_HIP_TRY(hipMemcpyAsync(W.d_lists, W.pinned, buf.size() * sizeof(int), hipMemcpyHostToDevice, st));
    OKKT_HIP_TRY(hipEventRecord(W.copied, st));
    W.copy_pending = true;
  }
  const DevPlan P = N.d;
  if (n_items > 0) {
    const int2* items = (const int2*)(W.d_lists + i_off);
    if (R == 1) hipLaunchKernelGGL(k_sp_prepare<1>, dim3(n_items), dim3(256), 0, st, P, items);
    else if (R == 2) hipLaunchKernelGGL(k_sp_prepare<2>, dim3(n_items), dim3(256), 0, st, P, items);
    else hipLaunchKernelGGL(k_sp_prepare<4>, dim3(n_items), dim3(256), 0, st, P, items);
  }
  if (sc.count > 0) {
    SpCols C;
    for (int q = 0; q <= kMaxRhs; ++q) C.c[q] = sc.col[q];
    const dim3 g((unsigned)((sc.count + 255) / 256)), b(256);
    if (d_scale) hipLaunchKernelGGL(k_sp_scatter<true>, g, b, 0, st, P, W.d_lists + p_off, C, d_val, d_scale);
    else hipLaunchKernelGGL(k_sp_scatter<false>, g, b, 0, st, P, W.d_lists + p_off, C, d_val, d_scale);
  }
  OKKT_HIP_TRY(hipGetLastError());
  if (A.fwd_full) e = solve_fwd_enqueue(N, 0, R);
  else e = solve_fwd_enqueue_lists(N, SweepLists{&flv, &fsl, W.d_lists + f_off, W.d_lists + f_off}, R);
  if (!e.empty()) return e;
  if (A.bwd_full) return solve_bwd_enqueue(N, 0, R);
  return solve_bwd_enqueue_lists(N, SweepLists{&blv, &bsl, W.d_lists + b_off, W.d_lists + b_off}, R);
}

void sparse_gather_enqueue(const Numeric& N, const int* d_xsel, int64_t nx, double* d_out, int64_t stride, int nr, const double* d_scale) {
  if (nx <= 0) return;
  const dim3 g((unsigned)((nx + 255) / 256)), b(256);
  if (d_scale) hipLaunchKernelGGL(k_sp_gather<true>, g, b, 0, N.stream, N.d, d_xsel, nx, nr, d_out, stride, N.d.counters + 5, d_scale);
  else hipLaunchKernelGGL(k_sp_gather<false>, g, b, 0, N.stream, N.d, d_xsel, nx, nr, d_out, stride, N.d.counters + 5, d_scale);
}

}  // namespace okkt
