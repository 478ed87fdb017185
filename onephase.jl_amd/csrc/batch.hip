// Uniform batches: B systems that share one analysed pattern, every front a small front (gfx950).
//
// The per-front code IS that of the single-system kernels: front_small_body, fs_small_body and bs_small_body of front_bodies.h, which
// k_front_small (numeric.hip), k_fs_small and k_bs_small (solve.hip) instantiate too, here in their forms without in-launch hand-offs
// (FLOW = false).  The kernels of this file add one grid coordinate: the item, whose values, shift, arena, D, counters and sweep vectors
// are reached through a DevPlan whose numeric pointers are moved to the item's slot (item_plan).  All index arrays are the plan's.
// The arithmetic of a small front does not depend on the block size (one update per element and pivot, children added one at a time
// in their fixed order, the duplicate path serial; the sweeps sum a row's terms in one thread, or in one wave in lane order), so item b
// is bit for bit what okkt_factor / okkt_solve compute for its values on a handle of their own, in both modes.
//
//   level mode: one launch per level of the task tree, grid = tasks of the level x B
//   item mode:  one workgroup per item runs every task of the plan in schedule order (children's contribution blocks and vectors pass
//               through the item's slot in HBM; the barrier at the end of a front orders the workgroup's stores before its later loads)
#include "batch.h"

#include <cstdlib>

#include "../../include/okkt.h"
#include "front_bodies.h"
#include "numeric.h"

namespace okkt {

#define OKKT_HIP_TRY(expr)                                                         \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess)                                                         \
      return std::string(#expr) + ": " + hipGetErrorString(e__);                   \
  } while (0)

// ------------------------------------------------------------------------------------------
// factorisation: front_small_body<TPB, false> on the item's plan, one call per task
// ------------------------------------------------------------------------------------------
// level mode: blockIdx.x = task of the level, blockIdx.y = item, or with an item list (the delta loop over the items of a KKT batch,
// DESIGN.md section 8.17, factors the still active items only) the slot items[blockIdx.y]; items = NULL is the identity
template <int TPB>
__global__ __launch_bounds__(TPB) void k_batch_front(DevPlan P0, BatchSlots S, const int* __restrict__ list, double tol, const double* __restrict__ vals, int64_t val_stride,
                                                     const int* __restrict__ items) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = items ? items[blockIdx.y] : (int)blockIdx.y;
  DevPlan P = item_plan(P0, S, b);
  P.vals = vals + (size_t)b * val_stride;
  unsigned pos = 0, neg = 0, zer = 0, bad = 0;
  front_small_body<TPB, false>(P, list[blockIdx.x], tol, sm, nullptr, 0, pos, neg, zer, bad);
  flush_counts(P, 0, pos, neg, zer, bad);
}

// level mode: the items' shifts and counters before the first level (diagadd[b][i] = shift[b] where the original index is below nshift)
__global__ __launch_bounds__(256) void k_batch_prepare(BatchSlots S, int n, const int* __restrict__ perm, const double* __restrict__ shift, int nshift,
                                                       const int* __restrict__ items) {
  const int b = items ? items[blockIdx.y] : (int)blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) S.diagadd[(size_t)b * n + i] = (shift && perm[i] < nshift) ? shift[b] : 0.0;
  if (blockIdx.x == 0 && threadIdx.x < kCountStride) S.counters[(size_t)b * kCountStride + threadIdx.x] = 0ull;
}

// item mode: blockIdx.x = item; the shift, the counters and every task of the plan, in the order of the schedule
template <int TPB>
__global__ __launch_bounds__(TPB) void k_batch_item_factor(DevPlan P0, BatchSlots S, const int* __restrict__ list, int ntasks, double tol, const double* __restrict__ vals,
                                                           int64_t val_stride, const double* __restrict__ shift, int nshift) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  DevPlan P = item_plan(P0, S, b);
  P.vals = vals + (size_t)b * val_stride;
  const double sh = shift ? shift[b] : 0.0;
  for (int i = threadIdx.x; i < P.n; i += TPB) P.diagadd[i] = (shift && P.perm[i] < nshift) ? sh : 0.0;
  if (threadIdx.x < kCountStride) atomicExch(&P.counters[threadIdx.x], 0ull);     // at the memory side, where the adds of the flush go
  __threadfence_block();
  __syncthreads();
  unsigned pos = 0, neg = 0, zer = 0, bad = 0;
  for (int t = 0; t < ntasks; ++t) front_small_body<TPB, false>(P, list[t], tol, sm, nullptr, 0, pos, neg, zer, bad);
  flush_counts(P, 0, pos, neg, zer, bad);
}

// ------------------------------------------------------------------------------------------
// solves, R right-hand sides: fs_small_body / bs_small_body<TPB, R, false> on the item's plan
// ------------------------------------------------------------------------------------------
template <int TPB, int R>
__global__ __launch_bounds__(TPB) void k_batch_fs(DevPlan P0, BatchSlots S, const int* __restrict__ list, int ldw) {
  extern __shared__ __attribute__((aligned(16))) double sm[];      // [R][ldw]
  const DevPlan P = item_plan(P0, S, blockIdx.y);
  fs_small_body<TPB, R, false>(P, list[blockIdx.x], ldw, sm, nullptr, 0);
}
template <int TPB, int R>
__global__ __launch_bounds__(TPB) void k_batch_bs(DevPlan P0, BatchSlots S, const int* __restrict__ list, int ldw) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const DevPlan P = item_plan(P0, S, blockIdx.y);
  bs_small_body<TPB, R, false>(P, list[blockIdx.x], ldw, sm);
}

// level mode: xwork[b][q][i] = rhs[b][r0 + q][perm[i]] for q < nr (zero for nr <= q < R)  /  sol[b][r0 + q][perm[i]] = xwork[b][q][i]
template <int R>
__global__ __launch_bounds__(256) void k_batch_permute_in(BatchSlots S, int n, const int* __restrict__ perm, const double* __restrict__ rhs, int64_t nrhs, int64_t r0, int nr) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int g = perm[i];
  double* x = S.xwork + (size_t)b * S.R * n;
  const double* src = rhs + ((size_t)b * nrhs + r0) * n;
#pragma unroll
  for (int q = 0; q < R; ++q) x[(size_t)q * n + i] = q < nr ? src[(size_t)q * n + g] : 0.0;
}
template <int R>
__global__ __launch_bounds__(256) void k_batch_permute_out(BatchSlots S, int n, const int* __restrict__ perm, double* __restrict__ sol, int64_t nrhs, int64_t r0, int nr) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int g = perm[i];
  const double* x = S.xwork + (size_t)b * S.R * n;
  double* dst = sol + ((size_t)b * nrhs + r0) * n;
#pragma unroll
  for (int q = 0; q < R; ++q)
    if (q < nr) dst[(size_t)q * n + g] = x[(size_t)q * n + i];
}

// item mode: gather, both sweeps over every task of the plan, scatter -- one workgroup per item.  (rhs may alias sol: an item reads all
// of its nr columns before it writes any of them, and no other workgroup touches them)
template <int TPB, int R>
__global__ __launch_bounds__(TPB) void k_batch_item_solve(DevPlan P0, BatchSlots S, const int* __restrict__ list, int ntasks, int ldw, const double* rhs, double* sol,
                                                          int64_t nrhs, int64_t r0, int nr) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  const DevPlan P = item_plan(P0, S, b);
  const int n = P.n;
  {
    const double* src = rhs + ((size_t)b * nrhs + r0) * n;
    for (int i = threadIdx.x; i < n; i += TPB) {
      const int g = P.perm[i];
#pragma unroll
      for (int q = 0; q < R; ++q) P.xwork[(size_t)q * P.xw_stride + i] = q < nr ? src[(size_t)q * n + g] : 0.0;
    }
  }
  __threadfence_block();
  __syncthreads();
  for (int t = 0; t < ntasks; ++t) fs_small_body<TPB, R, false>(P, list[t], ldw, sm, nullptr, 0);
  for (int t = ntasks - 1; t >= 0; --t) bs_small_body<TPB, R, false>(P, list[t], ldw, sm);
  {
    double* dst = sol + ((size_t)b * nrhs + r0) * n;
    for (int i = threadIdx.x; i < n; i += TPB) {
      const int g = P.perm[i];
#pragma unroll
      for (int q = 0; q < R; ++q)
        if (q < nr) dst[(size_t)q * n + g] = P.xwork[(size_t)q * P.xw_stride + i];
    }
  }
}

// okkt_batch_select: slot b -> the handle's own arena, D and shift
__global__ __launch_bounds__(256) void k_batch_select(DevPlan P, BatchSlots S, int64_t b, int64_t arena_len) {
  const size_t stride = (size_t)gridDim.x * 256;
  const double* a = S.arena + (size_t)b * S.arena_stride;
  const double* d = S.dvals + (size_t)b * S.n;
  const double* sh = S.diagadd + (size_t)b * S.n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)arena_len; i += stride) P.arena[i] = a[i];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)S.n; i += stride) { P.dvals[i] = d[i]; P.diagadd[i] = sh[i]; }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {
size_t lds_front(int maxf) { return ((size_t)(maxf | 1) * maxf + maxf) * sizeof(double); }

// the tasks of every level are one run of the schedule: with no big front, the three small classes of a level follow one another
struct LevelRun { int off, cnt, maxf; };
std::vector<LevelRun> level_runs(const Numeric& N) {
  std::vector<LevelRun> v;
  for (const LevelSchedule& L : N.levels) {
    LevelRun r{0, 0, 0};
    bool first = true;
    for (int c = 0; c < 3; ++c) {
      const Segment& g = L.seg[c];
      if (!g.cnt) continue;
      if (first) { r.off = g.off; first = false; }
      r.cnt += g.cnt;
      r.maxf = std::max(r.maxf, g.maxf);
    }
    if (r.cnt) v.push_back(r);
  }
  return v;
}

template <typename T>
bool dev_alloc(T** p, size_t count) {
  *p = nullptr;
  return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)) == hipSuccess;
}
}  // namespace

std::string batch_alloc(BatchWork& W, const Symbolic& S, int64_t arena_doubles, int64_t B, int64_t nrhs_max, bool* oom) {
  batch_free(W);
  *oom = false;
  const int R = batch_work_columns(nrhs_max);
  BatchSlots& s = W.s;
  s.n = S.n; s.sum_r = S.sum_r; s.R = R;
  s.arena_stride = batch_arena_stride(S, arena_doubles);
  W.arena_len = arena_doubles + 512 + (int64_t)S.max_front * 2;
  const size_t b = (size_t)B;
  const bool ok = dev_alloc(&s.arena, b * (size_t)s.arena_stride) && dev_alloc(&s.dvals, b * (size_t)S.n) && dev_alloc(&s.diagadd, b * (size_t)S.n) &&
                  dev_alloc(&s.xwork, b * R * (size_t)S.n) && dev_alloc(&s.zwork, b * R * (size_t)S.n) && dev_alloc(&s.cv, b * R * (size_t)S.sum_r) &&
                  dev_alloc(&s.counters, b * kCountStride) && dev_alloc(&W.shift, b) && dev_alloc(&W.items, b);
  if (!ok) {
    (void)hipGetLastError();
    batch_free(W);
    *oom = true;
    return "okkt_batch_reserve: " + std::to_string(B) + " slots of " + std::to_string(batch_slot_doubles(S, arena_doubles, R) * 8) + " bytes do not fit the device memory";
  }
  // D, the shift and the counters start from zero as the handle's own do; the arena is written before it is read
  OKKT_HIP_TRY(hipMemset(s.dvals, 0, std::max<size_t>(b * (size_t)S.n, 1) * sizeof(double)));
  OKKT_HIP_TRY(hipMemset(s.diagadd, 0, std::max<size_t>(b * (size_t)S.n, 1) * sizeof(double)));
  OKKT_HIP_TRY(hipMemset(s.counters, 0, b * kCountStride * sizeof(unsigned long long)));
  OKKT_HIP_TRY(hipStreamSynchronize(nullptr));
  // the fronts of more than about 90 rows need more dynamic LDS than the default limit: per reservation, on the handle's device, as
  // numeric_setup does for the single-system kernels
  const int big_lds = 160 * 1024 - 64;
  OKKT_HIP_TRY(hipFuncSetAttribute((const void*)k_batch_front<256>, hipFuncAttributeMaxDynamicSharedMemorySize, big_lds));
  OKKT_HIP_TRY(hipFuncSetAttribute((const void*)k_batch_item_factor<256>, hipFuncAttributeMaxDynamicSharedMemorySize, big_lds));
  W.B = B;
  W.nrhs_max = nrhs_max;
  W.factored_B = 0;
  return "";
}

void batch_free(BatchWork& W) {
  BatchSlots& s = W.s;
  for (void* p : {(void*)s.arena, (void*)s.dvals, (void*)s.diagadd, (void*)s.xwork, (void*)s.zwork, (void*)s.cv, (void*)s.counters, (void*)W.shift, (void*)W.items})
    if (p) (void)hipFree(p);
  s = BatchSlots();
  W.shift = nullptr;
  W.items = nullptr;
  ++W.generation;
  W.B = W.nrhs_max = W.factored_B = 0;
  W.mode_used = 0;
  W.inertia.clear();
  W.flags.clear();
}

bool batch_item_mode_ok(const Numeric& N) {
  // one epoch of contribution blocks (numeric_setup): a single level of tasks, or every level part of the one-launch range
  return N.levels.size() <= 1 || N.flow_levels == (int)N.levels.size();
}

int batch_pick_mode(const BatchWork& W, const Numeric& N, int64_t B) {
  (void)B;
  // the handle's forced mode, else the environment's; by itself level mode: no measured batch size at which item mode pays (batch.h)
  const int mode = W.mode != OKKT_BATCH_AUTO ? W.mode : W.env_mode;
  return mode == OKKT_BATCH_ITEM && batch_item_mode_ok(N) ? OKKT_BATCH_ITEM : OKKT_BATCH_LEVEL;
}

// No workgroup of a batch waits for another inside a launch: a grid of tasks x B is not resident as a whole, and the order in which
// workgroups are dispatched is undefined by contract, so a consumer could hold the slot its producer needs.  Dependencies are ordered
// by launch boundaries (level mode: children's levels are earlier launches on the stream) and by program order inside the one
// workgroup of an item (item mode: the schedule lists children's tasks before their parents'), and by nothing else.
std::string batch_factor_enqueue(Numeric& N, BatchWork& W, int mode, int64_t B, const double* d_vals, int64_t val_stride, bool shifted, int64_t nshift, double tol,
                                 const int* d_items) {
  const DevPlan P = N.d;
  hipStream_t st = N.stream;
  const double* d_shift = shifted ? W.shift : nullptr;
  const std::vector<LevelRun> runs = level_runs(N);
  if (mode == OKKT_BATCH_ITEM) {
    int maxf = 1, ntasks = 0;
    for (const LevelRun& r : runs) { maxf = std::max(maxf, r.maxf); ntasks += r.cnt; }
    const int* list = runs.empty() ? P.sched : P.sched + runs[0].off;
    if (maxf <= 32) hipLaunchKernelGGL(k_batch_item_factor<64>, dim3((unsigned)B), dim3(64), lds_front(maxf), st, P, W.s, list, ntasks, tol, d_vals, val_stride, d_shift, (int)nshift);
    else hipLaunchKernelGGL(k_batch_item_factor<256>, dim3((unsigned)B), dim3(256), lds_front(maxf), st, P, W.s, list, ntasks, tol, d_vals, val_stride, d_shift, (int)nshift);
  } else {
    hipLaunchKernelGGL(k_batch_prepare, dim3((unsigned)std::max<int64_t>((W.s.n + 255) / 256, 1), (unsigned)B), dim3(256), 0, st, W.s, (int)W.s.n, P.perm, d_shift, (int)nshift, d_items);
    for (const LevelRun& r : runs) {
      if (r.maxf <= 32) hipLaunchKernelGGL(k_batch_front<64>, dim3(r.cnt, (unsigned)B), dim3(64), lds_front(r.maxf), st, P, W.s, P.sched + r.off, tol, d_vals, val_stride, d_items);
      else hipLaunchKernelGGL(k_batch_front<256>, dim3(r.cnt, (unsigned)B), dim3(256), lds_front(r.maxf), st, P, W.s, P.sched + r.off, tol, d_vals, val_stride, d_items);
    }
  }
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

// level mode in its parts (the scenario batches of batch_schur.hip put the dense solve between the two sweeps): the gather of the
// right-hand sides, the levels upwards, the levels downwards, the scatter of the solutions
template <int R>
static void permute_in_r(Numeric& N, BatchWork& W, int64_t B, const double* d_rhs, int64_t nrhs, int64_t r0, int nr) {
  const int n = (int)W.s.n;
  hipLaunchKernelGGL(k_batch_permute_in<R>, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, N.stream, W.s, n, N.d.perm, d_rhs, nrhs, r0, nr);
}
template <int R>
static void permute_out_r(Numeric& N, BatchWork& W, int64_t B, double* d_sol, int64_t nrhs, int64_t r0, int nr) {
  const int n = (int)W.s.n;
  hipLaunchKernelGGL(k_batch_permute_out<R>, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, N.stream, W.s, n, N.d.perm, d_sol, nrhs, r0, nr);
}
template <int R>
static void fwd_r(Numeric& N, BatchWork& W, int64_t B) {
  const DevPlan P = N.d;
  hipStream_t st = N.stream;
  const std::vector<LevelRun> runs = level_runs(N);
  for (size_t l = 0; l < runs.size(); ++l) {      // forward: the levels upwards
    const LevelRun& r = runs[l];
    const size_t lds = (size_t)R * r.maxf * sizeof(double);
    if (r.maxf <= 32) hipLaunchKernelGGL((k_batch_fs<64, R>), dim3(r.cnt, (unsigned)B), dim3(64), lds, st, P, W.s, P.sched + r.off, r.maxf);
    else hipLaunchKernelGGL((k_batch_fs<256, R>), dim3(r.cnt, (unsigned)B), dim3(256), lds, st, P, W.s, P.sched + r.off, r.maxf);
  }
}
template <int R>
static void bwd_r(Numeric& N, BatchWork& W, int64_t B) {
  const DevPlan P = N.d;
  hipStream_t st = N.stream;
  const std::vector<LevelRun> runs = level_runs(N);
  for (size_t l = runs.size(); l-- > 0;) {        // backward: downwards
    const LevelRun& r = runs[l];
    const size_t lds = (size_t)R * r.maxf * sizeof(double);
    if (r.maxf <= 32) hipLaunchKernelGGL((k_batch_bs<64, R>), dim3(r.cnt, (unsigned)B), dim3(64), lds, st, P, W.s, P.sched + r.off, r.maxf);
    else hipLaunchKernelGGL((k_batch_bs<256, R>), dim3(r.cnt, (unsigned)B), dim3(256), lds, st, P, W.s, P.sched + r.off, r.maxf);
  }
}

#define OKKT_BATCH_BY_R(fn, ...)            \
  do {                                      \
    if (R == 1) fn<1>(__VA_ARGS__);         \
    else if (R == 2) fn<2>(__VA_ARGS__);    \
    else fn<4>(__VA_ARGS__);                \
  } while (0)

std::string batch_permute_in_enqueue(Numeric& N, BatchWork& W, int64_t B, const double* d_rhs, int64_t nrhs, int64_t r0, int nr, int R) {
  if (W.s.n > 0) OKKT_BATCH_BY_R(permute_in_r, N, W, B, d_rhs, nrhs, r0, nr);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}
std::string batch_permute_out_enqueue(Numeric& N, BatchWork& W, int64_t B, double* d_sol, int64_t nrhs, int64_t r0, int nr, int R) {
  if (W.s.n > 0) OKKT_BATCH_BY_R(permute_out_r, N, W, B, d_sol, nrhs, r0, nr);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}
std::string batch_fwd_enqueue(Numeric& N, BatchWork& W, int64_t B, int R) {
  OKKT_BATCH_BY_R(fwd_r, N, W, B);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}
std::string batch_bwd_enqueue(Numeric& N, BatchWork& W, int64_t B, int R) {
  OKKT_BATCH_BY_R(bwd_r, N, W, B);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

template <int R>
static std::string solve_enqueue_r(Numeric& N, BatchWork& W, int mode, int64_t B, const double* d_rhs, double* d_sol, int64_t nrhs, int64_t r0, int nr) {
  const DevPlan P = N.d;
  hipStream_t st = N.stream;
  const int n = (int)W.s.n;
  if (mode == OKKT_BATCH_ITEM) {
    const std::vector<LevelRun> runs = level_runs(N);
    int maxf = 1, ntasks = 0;
    for (const LevelRun& r : runs) { maxf = std::max(maxf, r.maxf); ntasks += r.cnt; }
    const int* list = runs.empty() ? P.sched : P.sched + runs[0].off;
    const size_t lds = (size_t)R * maxf * sizeof(double);
    if (maxf <= 32) hipLaunchKernelGGL((k_batch_item_solve<64, R>), dim3((unsigned)B), dim3(64), lds, st, P, W.s, list, ntasks, maxf, d_rhs, d_sol, nrhs, r0, nr);
    else hipLaunchKernelGGL((k_batch_item_solve<256, R>), dim3((unsigned)B), dim3(256), lds, st, P, W.s, list, ntasks, maxf, d_rhs, d_sol, nrhs, r0, nr);
  } else if (n > 0) {
    permute_in_r<R>(N, W, B, d_rhs, nrhs, r0, nr);
    fwd_r<R>(N, W, B);
    bwd_r<R>(N, W, B);
    permute_out_r<R>(N, W, B, d_sol, nrhs, r0, nr);
  }
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

std::string batch_solve_enqueue(Numeric& N, BatchWork& W, int mode, int64_t B, const double* d_rhs, double* d_sol, int64_t nrhs, int64_t r0, int nr, int R) {
  if (R == 1) return solve_enqueue_r<1>(N, W, mode, B, d_rhs, d_sol, nrhs, r0, nr);
  if (R == 2) return solve_enqueue_r<2>(N, W, mode, B, d_rhs, d_sol, nrhs, r0, nr);
  return solve_enqueue_r<4>(N, W, mode, B, d_rhs, d_sol, nrhs, r0, nr);
}

std::string batch_select_enqueue(Numeric& N, BatchWork& W, int64_t b) {
  const int64_t len = W.arena_len;      // what the handle's own arena holds (numeric_setup)
  const unsigned grid = (unsigned)std::min<int64_t>(2048, std::max<int64_t>((len + 1023) / 1024, 1));
  hipLaunchKernelGGL(k_batch_select, dim3(grid), dim3(256), 0, N.stream, N.d, W.s, b, len);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

}  // namespace okkt
