// The per-front device bodies that the single-system kernels and the batch kernels both run (gfx950), one definition each:
//   front_small_body<TPB, FLOW>     the fronts of a small-front task, assembled, factored and written back from LDS
//                                   (k_front_small of numeric.hip; k_batch_front, k_batch_item_factor of batch.hip)
//   fs_small_body<TPB, R, FLOW>     the forward sweep over the fronts of a task  (k_fs_small of solve.hip; k_batch_fs, k_batch_item_solve)
//   bs_small_body<TPB, R, FLOW>     the backward sweep                           (k_bs_small of solve.hip; k_batch_bs, k_batch_item_solve)
//   assemble_column<LDS, BATCH>     one column of a big front, with its tuning constants
//                                   (k_big_assemble of numeric.hip; k_batch_schur_assemble of batch_schur.hip)
// with the in-launch hand-offs of the FLOW forms, and item_plan, which points a DevPlan at the slot of a batch item: the bodies read
// every numeric array through the plan, so an item of a batch runs the very instructions of a handle of its own (DESIGN.md sections
// 8.15 and 8.16; tests/test_gpu_batch.py and tests/test_gpu_schur_batch.py compare the two bit for bit).
#pragma once
#include "batch.h"
#include "front_device.h"

namespace okkt {

// the plan as item b sees it: numeric state in the item's slot, no limits on the counts (a batch has no early exit).  vals is the caller's
__device__ __forceinline__ DevPlan item_plan(DevPlan P, const BatchSlots& S, int b) {
  P.arena = S.arena + (size_t)b * S.arena_stride;
  P.dvals = S.dvals + (size_t)b * S.n;
  P.diagadd = S.diagadd + (size_t)b * S.n;
  P.xwork = S.xwork + (size_t)b * S.R * S.n;
  P.zwork = S.zwork + (size_t)b * S.R * S.n;
  P.cv = S.cv + (size_t)b * S.R * S.sum_r;
  P.counters = S.counters + (size_t)b * kCountStride;
  P.want_pos = P.want_neg = -1;
  return P;
}

// ------------------------------------------------------------------------------------------
// small fronts: one workgroup, front resident in LDS
// ------------------------------------------------------------------------------------------
// FLOW (round 3): the tasks of SEVERAL levels in one launch.  `list` holds them level by level, so a task's children tasks have
// lower block indices (dispatch order = dependency order: a waiting workgroup never keeps its producers from being scheduled).
// A task raises flags[root] = epoch once its last front is in HBM; a parent waits on the flag of every child that lies outside
// its own index range.  The contribution blocks travel with agent-scope (sc1) accesses, which the memory side serves: no
// release / acquire fences.  A banded KKT system (BASELINE config 2) is factored by one launch instead of one per level.
__device__ __forceinline__ void flow_st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double flow_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// bounded: a hand-off that never comes ends the wait instead of hanging the GPU -- and is counted as a non-finite pivot (`bad`,
// slot 0 word 3) and in the time-out word (slot 0 word 5): the factorisation reports a wrong inertia, solves return NaN
__device__ __forceinline__ void flow_wait_task(const int* flag, int value, unsigned long long* counters) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < value && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(1);
    if (spins >= (1 << 22)) { atomicAdd(&counters[3], 1ull); atomicExch(&counters[5], 1ull); }
  }
  __syncthreads();
}
__device__ __forceinline__ void flow_signal(int* flag, int value) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave: its stores have been acknowledged
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the task of root s_root: the fronts task_lo[root] .. root in postorder, children's contribution blocks pass through HBM (the
// barrier at the end of an iteration makes the workgroup's stores visible to its own later loads).  sm: (f | 1) * f + f doubles of
// LDS for the largest front; the pivots are counted into pos .. bad, which the caller flushes
template <int TPB, bool FLOW>
__device__ __forceinline__ void front_small_body(const DevPlan& P, int s_root, double tol, double* sm, const int* flags, int wait_epoch, unsigned& pos, unsigned& neg,
                                                 unsigned& zer, unsigned& bad) {
  constexpr int G = TPB / 32;
  const int tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
  const int t_lo = P.task_lo[s_root];
  for (int s = t_lo; s <= s_root; ++s) {
    const int col0 = P.sn_col0[s];
    const int k = P.sn_col0[s + 1] - col0;
    const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
    const int ldf = f | 1;
    double* F = sm;
    double* wcol = sm + (size_t)ldf * f;
    double* front = P.arena + P.front_pos[s];

    for (int i = tid; i < ldf * f; i += TPB) F[i] = 0.0;
    __syncthreads();
    // original matrix entries of this supernode's columns
    {
      const int64_t e0 = P.aent_ptr[s], e1 = P.aent_ptr[s + 1];
      if (!P.has_dup) {
        for (int64_t e = e0 + tid; e < e1; e += TPB) {
          const int dst = (int)P.aent_dst[e];      // f <= 136 here: the offset fits in 32 bits
          const int lc = dst / f, lr = dst - lc * f;
          F[lr + lc * ldf] = P.vals[P.aent_src[e]];
        }
      } else if (tid == 0) {
        for (int64_t e = e0; e < e1; ++e) {
          const int dst = (int)P.aent_dst[e];
          const int lc = dst / f, lr = dst - lc * f;
          F[lr + lc * ldf] += P.vals[P.aent_src[e]];
        }
      }
    }
    __syncthreads();
    for (int j = tid; j < k; j += TPB) F[j + j * ldf] += P.diagadd[col0 + j];
    __syncthreads();
    // extend-add of the children's contribution blocks, one child at a time (fixed order)
    for (int64_t q = P.child_ptr[s]; q < P.child_ptr[s + 1]; ++q) {
      const int c = P.children[q];
      const int kc = P.sn_col0[c + 1] - P.sn_col0[c];
      const int fc = (int)(P.row_ptr[c + 1] - P.row_ptr[c]);
      const int rc = fc - kc;
      const double* C = P.arena + P.front_pos[c] + P.cb_shift[c];      // only the child's contribution block (columns >= kc) is read
      const int* rl = P.rel + P.rel_ptr[c];
      if (FLOW && c < t_lo) flow_wait_task(flags + c, wait_epoch, P.counters);      // a child task of this launch (workgroup-uniform)
      for (int jj = grp; jj < rc; jj += G) {
        const int pj = rl[jj];
        const double* Ccol = C + (size_t)(kc + jj) * fc + kc;
        for (int ii = jj + lane; ii < rc; ii += 32) F[rl[ii] + pj * ldf] += FLOW ? flow_ld(Ccol + ii) : Ccol[ii];
      }
      __syncthreads();
    }
    ldl_partial_lds<TPB>(F, wcol, ldf, f, k);
    // write back: L panel (rows >= col), contribution block (lower), D, inertia counts
    for (int c = grp; c < f; c += G) {
      double* dst = front + (size_t)c * f + cb_off(P, s, c, k);
      if (FLOW && c >= k) { for (int i = c + lane; i < f; i += 32) flow_st(dst + i, F[i + c * ldf]); }
      else for (int i = c + lane; i < f; i += 32) dst[i] = F[i + c * ldf];
    }
    for (int j = tid; j < k; j += TPB) {
      const double d = F[j + j * ldf];
      P.dvals[col0 + j] = d;
      classify_pivot(d, tol, pos, neg, zer, bad);
    }
    if (FLOW) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next front of the task reads this contribution block back
    __threadfence_block();
    __syncthreads();
  }
}

// ---- in-launch hand-offs between the workgroups of one front (round 3): a level's two dependent launches become one.
// Producer workgroups have LOWER block indices than their consumers (dispatch order = dependency order, so a waiting
// consumer never keeps its producer from being scheduled); the protocol is the MI355X guide's: every storing wave drains its
// stores, the workgroup meets at a barrier, one lane releases at agent scope and then raises the flag / counter; the consumer
// polls with relaxed agent-scope loads (bounded: a hand-off that never arrives ends the wait instead of hanging the GPU and
// raises the plan's time-out word, which turns the solution into NaN in k_permute_out_r), acquires once, and only then reads the data.
// The handed-off bytes are a few hundred doubles per front: they are written and read with agent-scope (sc1) accesses, which
// bypass the CU's L1 and are served by the memory side -- no release / acquire fences (an agent release writes back the whole L2,
// an acquire invalidates the whole L1: 2 - 7 us each, per workgroup, measured as a net loss on the fused sweeps).
__device__ __forceinline__ void st_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void front_signal_store(int* flag, int value) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave: its sc1 stores have been acknowledged
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// waits until *flag >= value (monotonic flags); the payload is then read with ld_agent only.  `tmo` (slot 0, word 5 of the plan's
// counters): raised when a wait runs into its bound; the last kernel of a solve (k_permute_out_r) then returns NaN instead of a
// solution that was computed from data that had not arrived
__device__ __forceinline__ void front_wait(const int* flag, int value, unsigned long long* tmo = nullptr) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < value && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(2);
    if (spins >= (1 << 22) && tmo) atomicExch(tmo, 1ull);
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// small fronts, the sweeps: the front's vector in LDS, sm = [R][ldw], R right-hand sides
// ------------------------------------------------------------------------------------------
// FLOW: the tasks of several levels in one launch (see front_small_body): a task waits for the flags of its children tasks,
// contribution vectors travel with agent-scope accesses
template <int TPB, int R, bool FLOW>
__device__ __forceinline__ void fs_small_body(const DevPlan& P, int s_root, int ldw, double* sm, const int* flags, int wait_epoch) {
  const int tid = threadIdx.x;
  const int t_lo = P.task_lo[s_root];
  for (int s = t_lo; s <= s_root; ++s) {      // the task's fronts, children first
    const int col0 = P.sn_col0[s];
    const int k = P.sn_col0[s + 1] - col0;
    const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
    const double* L = P.arena + P.front_pos[s];
    for (int i = tid; i < f; i += TPB)
#pragma unroll
      for (int q = 0; q < R; ++q) sm[q * ldw + i] = i < k ? P.xwork[(size_t)q * P.xw_stride + col0 + i] : 0.0;
    __syncthreads();
    for (int64_t c = P.child_ptr[s]; c < P.child_ptr[s + 1]; ++c) {
      const int ch = P.children[c];
      const int rc = (int)(P.rel_ptr[ch + 1] - P.rel_ptr[ch]);
      const int* rl = P.rel + P.rel_ptr[ch];
      const double* cvc = P.cv + P.cv_pos[ch];
      if (FLOW && ch < t_lo) front_wait(flags + ch, wait_epoch, P.counters + 5);
      for (int ii = tid; ii < rc; ii += TPB) {
        const int d = rl[ii];
#pragma unroll
        for (int q = 0; q < R; ++q) sm[q * ldw + d] += FLOW ? ld_agent(cvc + (size_t)q * P.cv_stride + ii) : cvc[(size_t)q * P.cv_stride + ii];
      }
      __syncthreads();
    }
    // unit lower triangular k x k
    for (int j = 0; j < k; ++j) {
      const double* col = L + (size_t)j * f;
      for (int i = j + 1 + tid; i < k; i += TPB) {
        const double l = col[i];
#pragma unroll
        for (int q = 0; q < R; ++q) sm[q * ldw + i] -= l * sm[q * ldw + j];
      }
      __syncthreads();
    }
    // rows below the pivot block: contribution vector for the parent
    double* cvs = P.cv + P.cv_pos[s];
    for (int i = k + tid; i < f; i += TPB) {
      double acc[R];
#pragma unroll
      for (int q = 0; q < R; ++q) acc[q] = sm[q * ldw + i];
      for (int j = 0; j < k; ++j) {
        const double l = L[(size_t)j * f + i];
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] -= l * sm[q * ldw + j];
      }
#pragma unroll
      for (int q = 0; q < R; ++q) { if (FLOW) st_agent(cvs + (size_t)q * P.cv_stride + i - k, acc[q]); else cvs[(size_t)q * P.cv_stride + i - k] = acc[q]; }
    }
    // z = D^-1 y
    for (int j = tid; j < k; j += TPB) {
      const double d = P.dvals[col0 + j];
#pragma unroll
      for (int q = 0; q < R; ++q) P.zwork[(size_t)q * P.xw_stride + col0 + j] = sm[q * ldw + j] / d;
    }
    if (FLOW) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __threadfence_block();
    __syncthreads();
  }
}

// FLOW: the ancestors' solution, which another workgroup of the launch has written, is read with agent-scope loads
template <int TPB, int R, bool FLOW>
__device__ __forceinline__ void bs_small_body(const DevPlan& P, int s_root, int ldw, double* sm) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NW = TPB / 64;
  for (int s = s_root; s >= P.task_lo[s_root]; --s) {      // the task's fronts, parents first
    const int col0 = P.sn_col0[s];
    const int k = P.sn_col0[s + 1] - col0;
    const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
    const double* L = P.arena + P.front_pos[s];
    const int* rows = P.rows + P.row_ptr[s];
    for (int i = tid; i < f; i += TPB) {
      const int g = rows[i];     // rows[i] = col0 + i for i < k: this front's z; beyond: the ancestors' solution
      const double* src = i < k ? P.zwork : P.xwork;
#pragma unroll
      for (int q = 0; q < R; ++q) sm[q * ldw + i] = (FLOW && i >= k) ? ld_agent(src + (size_t)q * P.xw_stride + g) : src[(size_t)q * P.xw_stride + g];
    }
    __syncthreads();
    // rhs_j = z_j - sum_{i >= k} L[i, j] * x_i
    for (int j = wv; j < k; j += NW) {
      const double* col = L + (size_t)j * f;
      double acc[R];
#pragma unroll
      for (int q = 0; q < R; ++q) acc[q] = 0.0;
      for (int i = k + lane; i < f; i += 64) {
        const double l = col[i];
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] += l * sm[q * ldw + i];
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        double a = acc[q];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) sm[q * ldw + j] -= a;
      }
    }
    __syncthreads();
    // unit upper triangular (L11^T) k x k, column oriented
    for (int j = k - 1; j >= 0; --j) {
      for (int i = tid; i < j; i += TPB) {
        const double l = L[(size_t)i * f + j];
#pragma unroll
        for (int q = 0; q < R; ++q) sm[q * ldw + i] -= l * sm[q * ldw + j];
      }
      __syncthreads();
    }
    for (int j = tid; j < k; j += TPB)
#pragma unroll
      for (int q = 0; q < R; ++q) { if (FLOW) st_agent(P.xwork + (size_t)q * P.xw_stride + col0 + j, sm[q * ldw + j]); else P.xwork[(size_t)q * P.xw_stride + col0 + j] = sm[q * ldw + j]; }
    if (FLOW) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __threadfence_block();
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// big fronts: one column of the assembly
// ------------------------------------------------------------------------------------------
// Each front column is owned by exactly one wave, which applies the contributions in list order:
// deterministic, no atomics, no workgroup barriers.
// column pc of front s accumulated in `buf` (buf[0] = row pc): zero, A entries, delta, children's contributions in
// their fixed order.  LDS = true: buf is the wave's LDS column; false: the HBM column itself.
// extend-add items whose records and first rows are in flight together (round 5: packed 32-byte records, 4 / 8 / 16 items measured: 2047 / 2058 /
// 2485 us of assembly per S-metric factorisation -- the kernels are not bound by the record fetches)
#ifndef OKKT_ASM_BATCH
#define OKKT_ASM_BATCH 4
#endif
#ifndef OKKT_ASM_BATCH_CHUNKED
#define OKKT_ASM_BATCH_CHUNKED 4
#endif
#ifndef OKKT_ASM_UNROLL
#define OKKT_ASM_UNROLL 4
#endif
constexpr int kAsmBatch = OKKT_ASM_BATCH, kAsmBatchChunked = OKKT_ASM_BATCH_CHUNKED;
constexpr int kAsmUnroll = OKKT_ASM_UNROLL;      // 64-row groups of an item whose index and value loads are in flight together (round 6: 8 instead of 4 is SLOWER -- S-metric 17.3 against 17.1 ms, S-C5 3.95 / 3.87: the registers cost waves, and waves are what hides the latency here)
template <bool LDS, bool BATCH>
__device__ __forceinline__ void assemble_column(const DevPlan& P, int s, int pc, int f, int k, int col0, double* __restrict__ buf) {
  const int lane = threadIdx.x & 63;
  const int nrow = f - pc;
  for (int i = lane; i < nrow; i += 64) buf[i] = 0.0;
  __threadfence_block();
  if (pc < k) {
    const int64_t e0 = P.aent_ptr[s];
    const int ne = (int)(P.aent_ptr[s + 1] - e0);
    const int64_t* dstv = P.aent_dst + e0;
    // range of this column's entries: precomputed on the host (two binary searches = ~25 dependent loads otherwise)
    const int64_t gcol = P.bigcol_base[s] + pc;
    const int lo = (int)(P.acol_lo[gcol] - e0);
    const int hi = pc + 1 < f ? (int)(P.acol_lo[gcol + 1] - e0) : ne;
    const int64_t base = (int64_t)pc * f + pc;     // dstv holds offsets in the front; entry (row, pc) sits at pc * f + row (past 2^31 above 46 340 rows)
    if (!P.has_dup) {
      for (int e = lo + lane; e < hi; e += 64) buf[(int)(dstv[e] - base)] = P.vals[P.aent_src[e0 + e]];
    } else if (lane == 0) {
      for (int e = lo; e < hi; ++e) buf[(int)(dstv[e] - base)] += P.vals[P.aent_src[e0 + e]];
    }
    __threadfence_block();
    if (lane == 0) buf[0] += P.diagadd[col0 + pc];
    __threadfence_block();
  }
  const int64_t gc = P.bigcol_base[s] + pc;
  // one precomputed record per item (source column in the arena, rel list, lengths): the per-child metadata
  // would cost two more dependent memory round trips per item; the next record is fetched while the current
  // item is applied
  const int64_t q0 = P.ea_ptr[gc], q1 = P.ea_ptr[gc + 1];
  // Items are applied strictly in order (same destination column), but their loads need not wait for each other:
  // four items at a time have their records, and then the first 64 rows of their index and source columns, in
  // flight together (clamped addresses, no branches); most items of the lower levels are no longer than that.
  constexpr int NB4 = kAsmBatch;
  if constexpr (!BATCH) {
    // long columns (upper levels, bandwidth-bound): one item after the other, the next record fetched meanwhile
    int64_t src_n = 0, rel_n = 0;
    int rc_n = 0, jj_n = 0;
    if (q0 < q1) { const EaRec r = P.ea_rec[q0]; src_n = r.src; rel_n = r.rel; rc_n = r.rc; jj_n = r.jj; }
    for (int64_t q = q0; q < q1; ++q) {
      const int rc = rc_n, jj = jj_n;
      const int* rl = P.rel + rel_n;
      const double* Ccol = P.arena + src_n;
      if (q + 1 < q1) { const EaRec r = P.ea_rec[q + 1]; src_n = r.src; rel_n = r.rel; rc_n = r.rc; jj_n = r.jj; }
      int ii = jj + lane;
      for (; ii + 64 * (kAsmUnroll - 1) < rc; ii += 64 * kAsmUnroll) {
        int d[kAsmUnroll];
        double v[kAsmUnroll], o[kAsmUnroll];
#pragma unroll
        for (int u = 0; u < kAsmUnroll; ++u) d[u] = rl[ii + 64 * u] - pc;
#pragma unroll
        for (int u = 0; u < kAsmUnroll; ++u) { v[u] = Ccol[ii + 64 * u]; o[u] = buf[d[u]]; }
#pragma unroll
        for (int u = 0; u < kAsmUnroll; ++u) buf[d[u]] = o[u] + v[u];
      }
      for (; ii < rc; ii += 64) buf[rl[ii] - pc] += Ccol[ii];
      __threadfence_block();
    }
    return;
  }
  for (int64_t q = q0; q < q1; q += NB4) {
    int64_t src[NB4], rel[NB4];
    int rc[NB4], jj[NB4];
#pragma unroll
    for (int u = 0; u < NB4; ++u) {
      const EaRec r = P.ea_rec[min(q + u, q1 - 1)];
      src[u] = r.src; rel[u] = r.rel; rc[u] = r.rc; jj[u] = r.jj;
    }
    int d[NB4];
    double v[NB4];
#pragma unroll
    for (int u = 0; u < NB4; ++u) {
      const int ii = min(jj[u] + lane, rc[u] - 1);
      d[u] = P.rel[rel[u] + ii] - pc;
      v[u] = P.arena[src[u] + ii];
    }
#pragma unroll
    for (int u = 0; u < NB4; ++u) {
      if (q + u < q1) {       // wave-uniform
        if (jj[u] + lane < rc[u]) buf[d[u]] += v[u];
        const int* rl = P.rel + rel[u];
        const double* Ccol = P.arena + src[u];
        int ii = jj[u] + 64 + lane;
        for (; ii + 64 * (kAsmUnroll - 1) < rc[u]; ii += 64 * kAsmUnroll) {
          int dd[kAsmUnroll];
          double vv[kAsmUnroll], oo[kAsmUnroll];
#pragma unroll
          for (int w = 0; w < kAsmUnroll; ++w) dd[w] = rl[ii + 64 * w] - pc;
#pragma unroll
          for (int w = 0; w < kAsmUnroll; ++w) { vv[w] = Ccol[ii + 64 * w]; oo[w] = buf[dd[w]]; }
#pragma unroll
          for (int w = 0; w < kAsmUnroll; ++w) buf[dd[w]] = oo[w] + vv[w];
        }
        for (; ii < rc[u]; ii += 64) buf[rl[ii] - pc] += Ccol[ii];
        __threadfence_block();
      }
    }
  }
}

}  // namespace okkt
