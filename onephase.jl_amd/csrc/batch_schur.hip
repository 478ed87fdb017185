// Scenario batches: B items in Schur mode on one analysed pattern (gfx950).  The interiors are the level mode
// of the uniform batches (batch.hip); this file is the item coordinate on the Schur front -- its assembly, the gather and the put of the
// sweeps -- and the two sums over the items.  The assembly of a column is the single-system body itself (assemble_column of
// front_bodies.h) on a DevPlan pointed at the item's slot (item_plan), not code of this file; the gather of a row still repeats fwd_gather.
//
// No workgroup waits for another inside a launch: no flags, no spins.  Every dependency -- the interiors before the Schur fronts, the
// fronts before the group partials, the partials before the sum, the sum before the dense factor -- is a launch boundary on the handle's
// stream, for the reason written at batch_factor_enqueue (batch.hip).
//
// The sums have ONE order, whatever the device or ns: P_g = the sequential sum, from 0.0, over the items kSchurBatchGroup * g ..
// min(kSchurBatchGroup * g + kSchurBatchGroup - 1, B - 1) in item order; the result is ((P_0 + P_1) + ... + P_{G-1}), then the caller's
// addend last.  No atomics.
#include "batch_schur.h"

#include <cstdlib>

#include "../../include/okkt.h"
#include "front_bodies.h"
#include "numeric.h"

namespace okkt {

static_assert(kSchurBatchGroup == OKKT_SBATCH_GROUP, "the group size of the sums is a constant of the interface");

#define OKKT_HIP_TRY(expr)                                                         \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess)                                                         \
      return std::string(#expr) + ": " + hipGetErrorString(e__);                   \
  } while (0)

// ------------------------------------------------------------------------------------------
// k_batch_schur_assemble: grid (ceil(ns / 4), B), one wave per (column of the Schur front, item), the column in LDS and written once:
// the LDS branch of k_big_assemble<true> (numeric.hip) on the item's plan -- assemble_column<true, true> of front_bodies.h, so item b's S_b
// is bit for bit okkt_factor_schur's
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_schur_assemble(DevPlan P0, BatchSlots S, int s, int lcol, const double* __restrict__ vals, int64_t val_stride) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y;
  DevPlan P = item_plan(P0, S, b);
  P.vals = vals + (size_t)b * val_stride;
  const int col0 = P.sn_col0[s];
  const int k = P.sn_col0[s + 1] - col0;
  const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
  const int pc = blockIdx.x * 4 + wv;
  if (pc >= f) return;
  const int nrow = f - pc;
  if (nrow > lcol) return;      // (never: lcol >= ns; a column that does not fit is not written rather than written out of bounds)
  double* col = P.arena + P.front_pos[s] + (size_t)pc * f + pc + cb_off(P, s, pc, k);
  double* buf = sm + (size_t)wv * lcol;
  assemble_column<true, true>(P, s, pc, f, k, col0, buf);
  for (int i = lane; i < nrow; i += 64) col[i] = buf[i];
}

// ------------------------------------------------------------------------------------------
// the sums over the items.  Stage one: thread t of group g adds entry t of the group's items, in item order, from 0.0; neighbouring
// threads read neighbouring entries.  tri_ns > 0: the entries are those of an ns x ns column-major matrix and only its lower triangle
// is summed.  Stage two: one thread per entry over the G partials, then the addend
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_schur_partial(const double* __restrict__ src, int64_t item_stride, int64_t len, int tri_ns, int B, double* __restrict__ part) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= len) return;
  if (tri_ns > 0 && t % tri_ns < t / tri_ns) return;
  const int g = blockIdx.y;
  const int b0 = g * kSchurBatchGroup, b1 = min(b0 + kSchurBatchGroup, B);
  double acc = 0.0;
  for (int b = b0; b < b1; ++b) acc += src[(size_t)b * item_stride + t];
  part[(size_t)g * len + t] = acc;
}

// S = ((P_0 + P_1) + ...) (+ add): both triangles written from the one sum of the lower entry, so S is bitwise symmetric
__global__ __launch_bounds__(256) void k_batch_schur_sum(const double* __restrict__ part, int G, int ns, const double* __restrict__ add, int64_t ld, double* __restrict__ out) {
  const int64_t len = (int64_t)ns * ns;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= len) return;
  const int i = (int)(t % ns), j = (int)(t / ns);
  if (i < j) return;
  double acc = part[t];
  for (int g = 1; g < G; ++g) acc = acc + part[(size_t)g * len + t];
  if (add) acc = acc + add[(size_t)j * ld + i];
  out[(size_t)j * ns + i] = acc;
  out[(size_t)i * ns + j] = acc;
}

// the same rule on vectors: out[t] = ((P_0[t] + P_1[t]) + ...) (+ add[t])
__global__ __launch_bounds__(256) void k_batch_schur_vsum(const double* __restrict__ part, int G, int64_t len, const double* __restrict__ add, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= len) return;
  double acc = part[t];
  for (int g = 1; g < G; ++g) acc = acc + part[(size_t)g * len + t];
  if (add) acc = acc + add[t];
  out[t] = acc;
}

// ------------------------------------------------------------------------------------------
// k_batch_schur_gather: the item coordinate on k_schur_gather (solve.hip).  The body from "w[q] =" to the end of the loop over the records
// is a COPY of fwd_gather<R> (solve.hip): a change to either must be made to both (tests/test_gpu_schur_batch.py compares r2 bit for bit).
// The one copy left in the batch kernels: a call of fwd_gather, which the compiler optimises on its own with w behind a pointer before it
// inlines it, costs the R = 4 form 110 registers against 88 and one wave of occupancy
// ------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void k_batch_schur_gather(DevPlan P, BatchSlots S, int64_t gcb, int col0, int ns, int nr, double* __restrict__ r2i, double* __restrict__ items,
                                                            int64_t nrhs, int64_t r0) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= ns) return;
  const int b = blockIdx.y;
  const double* __restrict__ xwork = S.xwork + (size_t)b * S.R * S.n;
  const double* __restrict__ cv = S.cv + (size_t)b * S.R * S.sum_r;
  double w[R];
#pragma unroll
  for (int q = 0; q < R; ++q) w[q] = xwork[(size_t)q * P.xw_stride + col0 + r];
  const int64_t q0 = P.ea_ptr[gcb + r], q1 = P.ea_ptr[gcb + r + 1];
  for (int64_t e = q0; e < q1; e += 8) {
    int64_t pos[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pos[u] = P.ea_pos[min(e + u, q1 - 1)];
    double v[8][R];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < R; ++q) v[u][q] = cv[(size_t)q * P.cv_stride + pos[u]];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (e + u < q1) {
#pragma unroll
        for (int q = 0; q < R; ++q) w[q] += v[u][q];
      }
  }
  // (end of the copy)
#pragma unroll
  for (int q = 0; q < R; ++q) {
    r2i[((size_t)b * 4 + q) * ns + r] = q < nr ? w[q] : 0.0;
    if (items && q < nr) items[((size_t)b * nrhs + r0 + q) * ns + r] = w[q];
  }
}

// the item coordinate on k_schur_put (solve.hip): the one x2 into the Schur columns of every item's xwork
template <int R>
__global__ __launch_bounds__(256) void k_batch_schur_put(DevPlan P, BatchSlots S, int col0, int ns, int nr, const double* __restrict__ x2) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= ns) return;
  double* xwork = S.xwork + (size_t)blockIdx.y * S.R * S.n;
#pragma unroll
  for (int q = 0; q < R; ++q) xwork[(size_t)q * P.xw_stride + col0 + r] = q < nr ? x2[(size_t)q * ns + r] : 0.0;
}

// item b's S_b: the lower triangle of its assembled front (column-major, leading dimension ns) -> full symmetric, leading dimension ld
__global__ __launch_bounds__(256) void k_batch_schur_export(const double* __restrict__ F, int ns, double* __restrict__ out, int64_t ld) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)ns * ns) return;
  const int i = (int)(t % ns), j = (int)(t / ns);
  out[(size_t)j * ld + i] = i >= j ? F[(size_t)j * ns + i] : F[(size_t)i * ns + j];
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {
template <typename T>
bool dev_alloc(T** p, size_t count) {
  *p = nullptr;
  return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)) == hipSuccess;
}
int groups_of(int64_t B) { return (int)((B + kSchurBatchGroup - 1) / kSchurBatchGroup); }
unsigned blocks_of(int64_t len) { return (unsigned)std::max<int64_t>((len + 255) / 256, 1); }
}  // namespace

std::string schur_batch_alloc(SchurBatchWork& W, const Symbolic& S, const Numeric& N, int64_t B, int64_t nrhs_max, bool* oom) {
  schur_batch_free(W);
  std::string e = batch_alloc(W.w, S, N.arena_doubles, B, nrhs_max, oom);
  if (!e.empty()) return e;
  const int64_t ns = S.nschur;
  const size_t G = (size_t)groups_of(B);
  const bool ok = dev_alloc(&W.sum, (size_t)ns * ns) && dev_alloc(&W.part, G * (size_t)ns * ns) && dev_alloc(&W.r2i, (size_t)B * 4 * ns) &&
                  dev_alloc(&W.r2p, G * 4 * (size_t)ns) && dev_alloc(&W.r2, 4 * (size_t)ns);
  if (ok) e = dense_ldlt_alloc(W.dl, ns);
  if (!ok || !e.empty()) {
    (void)hipGetLastError();
    schur_batch_free(W);
    *oom = true;
    return "okkt_schur_batch_reserve: the sum buffers and the dense factor of a set of " + std::to_string(ns) + " (" + std::to_string(G) + " groups) do not fit the device memory";
  }
  if (getenv("OKKT_DEBUG_POISON")) {
    // debug, as numeric_setup's own arena: the items' arenas (the strict upper triangles of the fronts are never written), the partials
    // (their upper triangles neither) and the items' r2 start as NaNs -- a kernel that reads what it should not shows up
    OKKT_HIP_TRY(hipMemset(W.w.s.arena, 0xFF, (size_t)B * (size_t)W.w.s.arena_stride * sizeof(double)));
    OKKT_HIP_TRY(hipMemset(W.part, 0xFF, std::max<size_t>(G * (size_t)ns * ns, 1) * sizeof(double)));
    OKKT_HIP_TRY(hipMemset(W.r2i, 0xFF, std::max<size_t>((size_t)B * 4 * ns, 1) * sizeof(double)));
    OKKT_HIP_TRY(hipStreamSynchronize(nullptr));
  }
  W.ns = ns;
  W.schur_sn = N.schur_sn;
  W.front_pos = N.front_pos_host[(size_t)N.schur_sn];
  W.gcb = N.schur_gcb;
  return "";
}

void schur_batch_free(SchurBatchWork& W) {
  batch_free(W.w);
  for (void* p : {(void*)W.sum, (void*)W.part, (void*)W.r2i, (void*)W.r2p, (void*)W.r2})
    if (p) (void)hipFree(p);
  W.sum = W.part = W.r2i = W.r2p = W.r2 = nullptr;
  dense_ldlt_release(W.dl);
  W.ns = 0;
  W.schur_sn = -1;
  W.dense_ok = false;
}

std::string schur_batch_assemble_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_vals, int64_t val_stride) {
  const int f = (int)W.ns;
  const int lcol = std::max(256, (f + 63) / 64 * 64);      // as numeric_factor_enqueue sizes it for k_big_assemble<true>; at most 64 KiB for ns <= 2048
  hipLaunchKernelGGL(k_batch_schur_assemble, dim3((unsigned)((f + 3) / 4), (unsigned)B), dim3(256), (size_t)4 * lcol * sizeof(double), N.stream, N.d, W.w.s, W.schur_sn, lcol,
                     d_vals, val_stride);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

std::string schur_batch_sum_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_add, int64_t ld, double* d_out) {
  const int ns = (int)W.ns;
  const int64_t len = (int64_t)ns * ns;
  const int G = groups_of(B);
  hipLaunchKernelGGL(k_batch_schur_partial, dim3(blocks_of(len), (unsigned)G), dim3(256), 0, N.stream, W.w.s.arena + W.front_pos, W.w.s.arena_stride, len, ns, (int)B, W.part);
  hipLaunchKernelGGL(k_batch_schur_sum, dim3(blocks_of(len)), dim3(256), 0, N.stream, W.part, G, ns, d_add, ld, d_out);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

std::string schur_batch_export_enqueue(Numeric& N, SchurBatchWork& W, int64_t b, double* d_S, int64_t ld) {
  const int ns = (int)W.ns;
  hipLaunchKernelGGL(k_batch_schur_export, dim3(blocks_of((int64_t)ns * ns)), dim3(256), 0, N.stream, W.w.s.arena + (size_t)b * W.w.s.arena_stride + W.front_pos, ns, d_S, ld);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

std::string schur_batch_gather_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, double* d_items, int64_t nrhs, int64_t r0, int nr, int R) {
  const int ns = (int)W.ns, col0 = N.d.n - ns;
  const dim3 g((unsigned)((ns + 255) / 256), (unsigned)B), t(256);
  if (R == 1) hipLaunchKernelGGL(k_batch_schur_gather<1>, g, t, 0, N.stream, N.d, W.w.s, W.gcb, col0, ns, nr, W.r2i, d_items, nrhs, r0);
  else if (R == 2) hipLaunchKernelGGL(k_batch_schur_gather<2>, g, t, 0, N.stream, N.d, W.w.s, W.gcb, col0, ns, nr, W.r2i, d_items, nrhs, r0);
  else hipLaunchKernelGGL(k_batch_schur_gather<4>, g, t, 0, N.stream, N.d, W.w.s, W.gcb, col0, ns, nr, W.r2i, d_items, nrhs, r0);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

std::string schur_batch_r2sum_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_add, double* d_out, int nr, int R) {
  (void)R;
  const int64_t len = (int64_t)nr * W.ns;      // the first nr of an item's four columns
  const int G = groups_of(B);
  hipLaunchKernelGGL(k_batch_schur_partial, dim3(blocks_of(len), (unsigned)G), dim3(256), 0, N.stream, W.r2i, 4 * W.ns, len, 0, (int)B, W.r2p);
  hipLaunchKernelGGL(k_batch_schur_vsum, dim3(blocks_of(len)), dim3(256), 0, N.stream, W.r2p, G, len, d_add, d_out);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

std::string schur_batch_put_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_x2, int nr, int R) {
  const int ns = (int)W.ns, col0 = N.d.n - ns;
  const dim3 g((unsigned)((ns + 255) / 256), (unsigned)B), t(256);
  if (R == 1) hipLaunchKernelGGL(k_batch_schur_put<1>, g, t, 0, N.stream, N.d, W.w.s, col0, ns, nr, d_x2);
  else if (R == 2) hipLaunchKernelGGL(k_batch_schur_put<2>, g, t, 0, N.stream, N.d, W.w.s, col0, ns, nr, d_x2);
  else hipLaunchKernelGGL(k_batch_schur_put<4>, g, t, 0, N.stream, N.d, W.w.s, col0, ns, nr, d_x2);
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

}  // namespace okkt
