// Dataflow factorisation of the big fronts of one level: ONE persistent launch instead of one launch per block column and kernel.
//
// Replaces, for the fronts above small_max rows, the per-step sequence k_big_diag2 -> k_big_trsm -> k_big_syrk of numeric.hip (the
// reference reaches the same arithmetic through CHOLMOD's numeric factorisation, /root/reference/src/linear_system_solvers/julia.jl:21-97).
// The level's fronts are cut into 128 x 128 tiles; dataflow_sched.cpp turns the blocked right-looking LDL^T into tasks D (diagonal
// tile), T (tile of the panel below it) and U (update of a trailing tile by one or two panels) and orders them in ONE queue.
// Every workgroup of this launch is a worker: pop the next task, wait until the tile states it depends on have been published
// (bounded spin on agent-scope loads), run the task's body, publish the new state of its tile.  No kernel boundaries and no
// stream events between the steps: the diagonal block of block column q + 1 starts as soon as ITS tile has received panel q,
// while the rest of panel q's update is still running on the other CUs.
//
// Hand-off protocol (MI355X guide, "Workgroup dispatch, XCD placement & inter-workgroup visibility"): a producer writes every
// byte that another task reads with sc1 (write-through) stores, every storing wave drains its stores (s_waitcnt vmcnt(0)), the
// workgroup meets at a barrier, one lane publishes the tile state with an agent-scope store.  A consumer polls the state with
// agent-scope loads from one lane, that lane runs an agent-scope acquire (invalidates the CU's L1) and drains it, the workgroup
// meets at a barrier, and only then loads -- plain loads and LDS-DMA.
//
// The arithmetic per entry is the sequence of the per-step kernels (same bodies, same order of the panels per tile): the factor
// is bitwise the same, which is how the GPU tests pin this path (tests/test_gpu_dataflow.py).
#include "front_device.h"
#include "df_fragments.h"
#include "../../include/okkt.h"

#include <algorithm>
#include <type_traits>
#include <cstdio>
#include <cstdlib>

namespace okkt {

#define OKKT_HIP_TRY(expr)                                                         \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess)                                                         \
      return std::string(#expr) + ": " + hipGetErrorString(e__);                   \
  } while (0)

typedef double d2_t __attribute__((ext_vector_type(2)));
constexpr int kDfThreadsC = 512;   // threads of a worker
#ifndef OKKT_DF_STAGES
#define OKKT_DF_STAGES 2
#endif
#ifndef OKKT_DF_KC
#define OKKT_DF_KC 32
#endif
#ifndef OKKT_DF_STAGGER
#define OKKT_DF_STAGGER 1
#endif
constexpr bool kDfStagger = OKKT_DF_STAGGER != 0;   // waves 4 - 7 of a worker request the next operand chunk half a chunk behind waves 0 - 3
#ifndef OKKT_DF_LOG_BUILD
#define OKKT_DF_LOG_BUILD 0
#endif
// the per-task time stamps (OKKT_DEBUG_DATAFLOW=16 + OKKT_DF_LOG) and the switches that skip task bodies (1 / 2 / 4) are instrumentation of the
// same kind: with them compiled out S-metric is 1.6 % faster (17.06 against 17.33 ms), S-C3 0.8 %, S-C5 1.6 % (82 instead of 101 scalar-register
// spills, a shorter instruction stream).  libonephase_kkt_log.so (the product kernel + this instrumentation) has them;
// OKKT_DEBUG_DATAFLOW=8 (synchronise and report every launch) works everywhere.
constexpr bool kDfLog = OKKT_DF_LOG_BUILD != 0;
#ifndef OKKT_DF_MULTI
#define OKKT_DF_MULTI 1
#endif
// update tasks that carry several row tiles (OKKT_DF_ROWS, OKKT_DF_ROWS_BIG: measured slower since round 4) need a second set of C-tile registers in the
// update role.  -DOKKT_DF_MULTI=0 leaves it out; measured (round 6, four A/B pairs on one box): the kernel WITH it is the faster one -- S-metric 17.07 against
// 17.17 ms, S-C3 2.95 against 2.99 -- register allocation, not logic: kept
constexpr bool kDfMulti = OKKT_DF_MULTI != 0;
#ifndef OKKT_DF_CONTIG
#define OKKT_DF_CONTIG 1
#endif
// update tasks: a lane's eight column fragments are eight NEIGHBOURING columns (4 x ds_read_b128 instead of 4 x ds_read2_b64 per k-step) and the operand
// ring has a conflict-free image of its own (df_fragments.h); bitwise equal.  -DOKKT_DF_CONTIG=0: the earlier map and the kSyrkLd ring, for A/B runs
constexpr int kDfContig = OKKT_DF_CONTIG != 0 ? 1 : 0;
static_assert(kDfFragLdOld == kSyrkLd, "df_fragments.h describes the earlier ring with kSyrkLd");
static_assert(df_ring_rot(kDfContig, 1) == 0, "the LDS-DMA of df_syrk_tiles fetches a panel column lane-linearly");
constexpr int kDfDiagMfmaWaves = 6;   // MFMA waves of the diagonal-block factorisation in a worker (four or six: the same time)
constexpr int kDfKC = OKKT_DF_KC;           // panel columns per ring slot of the update tasks
constexpr int kDfStages = OKKT_DF_STAGES;   // operand ring of the update tasks: 16-column chunks in LDS (one workgroup per CU: nobody else covers a chunk that is late)

// 16-byte write-through store (global_store_dwordx4 ... sc1): the C tiles leave the CU at the rate of plain stores and are
// visible to every other CU once the storing wave's vmcnt has drained
__device__ __forceinline__ void st_sc1_f64x2(double* p, d2_t v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ int ld_state(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// first row / column of block b of a front with KB pivot blocks: 128 b inside the pivot block, k + 128 (b - KB) behind it
__device__ __forceinline__ int df_block_lo(int b, int KB, int k, int f) { return b < KB ? b * 128 : min(k + (b - KB) * 128, f); }

// ---- T: rows [r0, rlim) (at most 128) of the panel below diagonal block q ---------------------------------------------------
// k_big_trsm's body (front_device.h: trsm_body) for a workgroup of eight waves, 16 rows each; every load behind the task's
// acquire is a plain load, W and L leave with sc1 stores.
__device__ __forceinline__ void df_trsm_tile(const DevPlan& P, int s, int q, int r0, int rlim, double* sm) {
  constexpr int NBLK = 4, NB = 128, NPAIR = NBLK * (NBLK + 1) / 2;
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));      // opaque: nothing derived from the lane id is hoisted out of the worker's loop and kept live across the other roles
  const int tid = tid_, lane = tid & 63, wv = tid >> 6;
  const int col0 = P.sn_col0[s];
  const int k = P.sn_col0[s + 1] - col0;
  const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
  const int j0 = q * NB;
  const int nb = min(NB, k - j0);
  double* F = P.arena + P.front_pos[s];
  double* Wb = P.wbuf + P.wbuf_pos[s] + (size_t)j0 * f;
  const double* X = P.invl + P.invl_pos[s] + (size_t)q * NB * NB;
  double* rdv = sm + NPAIR * kIB * kIB;
  const int row = r0 + wv * 16 + (lane & 15);
  const int rowc = min(row, f - 1);
  const bool valid = row < rlim;
  const int lk = lane >> 4, li = lane & 3;
  double t[NBLK * 8];
#pragma unroll
  for (int qq = 0; qq < NBLK * 8; ++qq) {
    const int c = 4 * qq + lk;
    t[qq] = keep_f64(F[(size_t)(j0 + min(c, nb - 1)) * f + rowc], c < nb && valid);
  }
  {
    const int e = tid * 2;                 // 2 consecutive rows of one column per thread and block
    const int cc = e / kIB, rr = e - cc * kIB;
#pragma unroll
    for (int bi = 0; bi < NBLK; ++bi)
#pragma unroll
      for (int bp = 0; bp <= bi; ++bp) {
        double v[2];
        const int gr = bi * kIB + rr, gc = bp * kIB + cc;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const double* src = bp == bi ? X + (gr + u) + (size_t)gc * NB
                                       : F + (size_t)(j0 + min(gc, nb - 1)) * f + j0 + min(gr + u, nb - 1);
          v[u] = keep_f64(*src, gr + u < nb && gc < nb);
        }
        double* dst = sm + (bi * (bi + 1) / 2 + bp) * kIB * kIB + e;
        dst[0] = v[0]; dst[1] = v[1];
      }
    if (tid < NB) rdv[tid] = tid < nb ? 1.0 / P.dvals[col0 + j0 + tid] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int bi = 0; bi < NBLK; ++bi) {
#pragma unroll
    for (int bp = 0; bp < bi; ++bp) {
      const double* Lb = sm + (bi * (bi + 1) / 2 + bp) * kIB * kIB;
#pragma unroll
      for (int gp = 0; gp < 8; ++gp)
#pragma unroll
        for (int g = 0; g < 8; ++g)
          t[bi * 8 + gp] = __builtin_amdgcn_mfma_f64_4x4x4f64(Lb[(gp * 4 + li) + (g * 4 + lk) * kIB], t[bp * 8 + g], t[bi * 8 + gp], 0, 0, 1 /* neg A */);
    }
    const double* Xb = sm + (bi * (bi + 1) / 2 + bi) * kIB * kIB;
    double wt[8];
#pragma unroll
    for (int gp = 0; gp < 8; ++gp) {
      wt[gp] = 0.0;
#pragma unroll
      for (int g = 0; g <= gp; ++g)   // X_ii is lower triangular
        wt[gp] = __builtin_amdgcn_mfma_f64_4x4x4f64(Xb[(gp * 4 + li) + (g * 4 + lk) * kIB], t[bi * 8 + g], wt[gp], 0, 0, 0);
    }
#pragma unroll
    for (int gp = 0; gp < 8; ++gp) t[bi * 8 + gp] = wt[gp];
  }
  if (valid) {
#pragma unroll
    for (int qq = 0; qq < NBLK * 8; ++qq) {
      const int c = 4 * qq + lk;
      if (c < nb) {
        st_agent_f64(&Wb[(size_t)c * f + row], t[qq]);
        st_agent_f64(&F[(size_t)(j0 + c) * f + row], t[qq] * rdv[c]);
      }
    }
  }
}

// a wait inside a task (the diagonal block a TL task solves against): the worker's protocol -- wave 0 polls (bounded), acquires, the
// workgroup meets.  false: the launch is stopping (delta loop) or a wait has run into its bound
__device__ __forceinline__ bool df_await(const DevPlan& P, const int* state, int least, int* flag) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave == 0) {
    int ok = 1, spins = 0;
    long long t0w = 0;
    for (;;) {
      if (__builtin_amdgcn_readfirstlane(ld_state(state)) >= least) break;
      const int stop = P.want_neg >= 0 ? __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&P.counters[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
      const int dead = __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&P.counters[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (stop | dead) { ok = 0; break; }
      if (wait_expired(spins, t0w)) {
        if ((threadIdx.x & 63) == 0) atomicExch(&P.counters[5], 1ull);
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *flag = ok;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*flag) != 0;
}

// ---- TL: the last update of tile (i, q) (panel q - 1) and T(i, q) in one task, q >= 1 ------------------------------------------------
// A block row below the chain's advances one block column per chain step: T(i, q - 1) -> U(i, q; panel q - 1) -> T(i, q), two tasks and two
// hand-offs (30 + 27 + 2 x 3 us) per 63-us step -- every row was as slow as the chain itself, any queueing made it slower, and the chain
// waits for the rows that enter its cone: the root of the metric workload ran at 87 - 94 us per block column while updates were
// plentiful.  Here the update runs in the panel solve's own register layout (a wave owns 16 rows x 128 columns: the 16 x 4 strips are
// the accumulators, W(i, q - 1) in the same layout is the B operand, L(q, q - 1) staged in LDS the A operand: 1024 MFMAs per wave) and
// BEFORE D(q) has arrived -- the task is popped when its tile has received panel q - 2 and block rows i and q of panel q - 1 are there,
// waits for D(q) inside like TU, stages the diagonal block's pieces over the L image and solves.  The products reach every entry in
// ascending panel order, k ascending within the panel, as in the update task: bitwise the same tile, then df_trsm_tile's solve.
// W and L leave through LDS as 16-byte write-through stores (the 8-byte ones of df_trsm_tile cost 9 us per tile).
constexpr int kTlLd = 132;           // leading dimension of the L(q, q - 1) image: the four k-slices of an A fragment on disjoint banks
constexpr size_t kDfTlLds = std::max((size_t)128 * kTlLd * sizeof(double), (size_t)(128 * kSyrkLd + 128) * sizeof(double));
__device__ __forceinline__ bool df_tl_tile(const DevPlan& P, int s, int q, int r0, int rlim, const int* dstate, int* s_flag, double* sm, long long* marks) {
  constexpr int NBLK = 4, NB = 128, NPAIR = NBLK * (NBLK + 1) / 2;
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));
  const int tid = tid_, lane = tid & 63, wv = tid >> 6;
  const int col0 = P.sn_col0[s];
  const int k = P.sn_col0[s + 1] - col0;
  const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
  const int j0 = q * NB;
  const int nb = min(NB, k - j0);
  double* F = P.arena + P.front_pos[s];
  double* Wb = P.wbuf + P.wbuf_pos[s] + (size_t)j0 * f;
  const double* Wprev = Wb - (size_t)NB * f;              // W of panel q - 1 (a whole block column)
  const double* X = P.invl + P.invl_pos[s] + (size_t)q * NB * NB;
  const int trow = wv * 16 + (lane & 15);
  const int row = r0 + trow;
  const int rowc = min(row, f - 1);
  const bool valid = row < rlim;
  const int lk = lane >> 4, li = lane & 3;
  double t[NBLK * 8], w[NBLK * 8];
#pragma unroll
  for (int qq = 0; qq < NBLK * 8; ++qq) {
    const int c = 4 * qq + lk;
    t[qq] = keep_f64(F[(size_t)(j0 + min(c, nb - 1)) * f + rowc], c < nb && valid);
    w[qq] = keep_f64(Wprev[(size_t)c * f + rowc], valid);
  }
  // L(q, q - 1): rows [j0, j0 + nb) of panel q - 1, entry (c, kk) at c + kk * kTlLd
  {
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int idx = it * kDfThreadsC + tid;
      const int kk = idx >> 6, c2 = (idx & 63) * 2;
      const double* src = F + (size_t)(j0 - NB + kk) * f + j0;
      d2_t v;
      v[0] = keep_f64(src[min(c2, nb - 1)], c2 < nb);
      v[1] = keep_f64(src[min(c2 + 1, nb - 1)], c2 + 1 < nb);
      __builtin_memcpy(sm + (size_t)kk * kTlLd + c2, &v, 16);
    }
  }
  __syncthreads();
  if (marks && tid == 0) marks[0] = wall_clock64();        // operands in registers and LDS
  // t(rows, c) -= sum_kk W(rows, kk) L(c, kk): k-strips ascending, the order of the update task's k-steps
  // (fully unrolled: a rolled loop over g indexes w[] dynamically, which puts the array into scratch memory -- a scratch load and a
  // vmcnt(0) per 64 MFMAs)
#pragma unroll
  for (int g = 0; g < NBLK * 8; ++g) {
#pragma unroll
    for (int gp = 0; gp < NBLK * 8; ++gp)
      t[gp] = __builtin_amdgcn_mfma_f64_4x4x4f64(sm[(gp * 4 + li) + (size_t)(g * 4 + lk) * kTlLd], w[g], t[gp], 0, 0, 1 /* neg A */);
  }
  if (marks && tid == 0) marks[1] = wall_clock64();        // tile updated
  if (!df_await(P, dstate, q + 1, s_flag)) return false;   // D(q); the barrier inside: every wave is done with the L image
  if (marks && tid == 0) marks[2] = wall_clock64();        // D(q) has arrived
  double* rdv = sm + NPAIR * kIB * kIB;
  {
    const int e = tid * 2;
    const int cc = e / kIB, rr = e - cc * kIB;
#pragma unroll
    for (int bi = 0; bi < NBLK; ++bi)
#pragma unroll
      for (int bp = 0; bp <= bi; ++bp) {
        double v[2];
        const int gr = bi * kIB + rr, gc = bp * kIB + cc;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const double* src = bp == bi ? X + (gr + u) + (size_t)gc * NB
                                       : F + (size_t)(j0 + min(gc, nb - 1)) * f + j0 + min(gr + u, nb - 1);
          v[u] = keep_f64(*src, gr + u < nb && gc < nb);
        }
        double* dst = sm + (bi * (bi + 1) / 2 + bp) * kIB * kIB + e;
        dst[0] = v[0]; dst[1] = v[1];
      }
    if (tid < NB) rdv[tid] = tid < nb ? 1.0 / P.dvals[col0 + j0 + tid] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int bi = 0; bi < NBLK; ++bi) {
#pragma unroll
    for (int bp = 0; bp < bi; ++bp) {
      const double* Lb = sm + (bi * (bi + 1) / 2 + bp) * kIB * kIB;
#pragma unroll
      for (int gp = 0; gp < 8; ++gp)
#pragma unroll
        for (int g = 0; g < 8; ++g)
          t[bi * 8 + gp] = __builtin_amdgcn_mfma_f64_4x4x4f64(Lb[(gp * 4 + li) + (g * 4 + lk) * kIB], t[bp * 8 + g], t[bi * 8 + gp], 0, 0, 1 /* neg A */);
    }
    const double* Xb = sm + (bi * (bi + 1) / 2 + bi) * kIB * kIB;
    double wt[8];
#pragma unroll
    for (int gp = 0; gp < 8; ++gp) {
      wt[gp] = 0.0;
#pragma unroll
      for (int g = 0; g <= gp; ++g)   // X_ii is lower triangular
        wt[gp] = __builtin_amdgcn_mfma_f64_4x4x4f64(Xb[(gp * 4 + li) + (g * 4 + lk) * kIB], t[bi * 8 + g], wt[gp], 0, 0, 0);
    }
#pragma unroll
    for (int gp = 0; gp < 8; ++gp) t[bi * 8 + gp] = wt[gp];
  }
  const double myrd = tid < NB ? rdv[tid] : 0.0;
  __syncthreads();                       // every wave is done with the staged blocks and the reciprocals
  double* Wl = sm;                       // [128 panel columns][kSyrkLd]: W(r0 + r, j0 + p) at p * kSyrkLd + r
  double* rd2 = sm + (size_t)128 * kSyrkLd;
#pragma unroll
  for (int qq = 0; qq < NBLK * 8; ++qq) Wl[(size_t)(4 * qq + lk) * kSyrkLd + trow] = t[qq];      // rows past the block are zero
  if (tid < NB) rd2[tid] = myrd;
  __syncthreads();
  if (marks && tid == 0) marks[3] = wall_clock64();        // solved, W in LDS
  {
    const int nrow = min(rlim - r0, 128);
    for (int idx = tid; idx < (nb << 6); idx += kDfThreadsC) {
      const int p = idx >> 6, x2 = (idx & 63) * 2;
      d2_t wv2;
      __builtin_memcpy(&wv2, Wl + (size_t)p * kSyrkLd + x2, 16);
      const double rp = rd2[p];
      const d2_t l = (d2_t){wv2[0] * rp, wv2[1] * rp};
      double* wdst = Wb + (size_t)p * f + r0 + x2;
      double* ldst = F + (size_t)(j0 + p) * f + r0 + x2;
      if (x2 + 1 < nrow) { st_sc1_f64x2(wdst, wv2); st_sc1_f64x2(ldst, l); }
      else if (x2 < nrow) { st_agent_f64(wdst, wv2[0]); st_agent_f64(ldst, l[0]); }
    }
  }
  return true;
}

// ---- TU: T(q + 1, q) and the update of the diagonal tile (q + 1, q + 1) by panel q in one task -------------------------------
// The two steps between the diagonal blocks of consecutive block columns.  The task is popped beside D(q): the rows of tile
// (q + 1, q) and the diagonal tile are in flight while D(q) runs; then the task waits for D(q) (second wait, same protocol as the
// worker's), solves its 128 rows like df_trsm_tile, keeps W in LDS (128 x 128, the layout of the trailing update's operand
// slots; L = W * (1 / d) is formed on the fly, the very product that is stored) and applies it to the diagonal tile with the
// trailing update's MFMA loop.  Same operations per entry in the same order as T followed by U: bitwise the same numbers.
//
// Both steps run at the FP64 matrix rate of ONE CU (7 us for the rows, 9 - 11 us for the ten 32 x 32 sub-tiles of the lower
// triangle), so the block row may be split between two workers (`part`):
//   part 1 (task TA): rows [r0, r0 + 64) -- solves them, stores their W and L (half state 1), updates the sub-tiles that need
//                     nothing else ((0,0), (1,0), (1,1) of the 4 x 4 grid), stores them (half state 2: published by the worker);
//   part 2 (task TU): rows [r0 + 64, rlim) -- solves them, fetches the W of the upper rows once half state 1 is seen, updates the
//                     seven sub-tiles of its rows, takes the three of part 1 from memory (half state 2) and goes on as the
//                     unsplit task does (the diagonal block's factorisation from LDS, or the tile's publication);
//   part 0: everything in one task (block rows of at most 64 rows, OKKT_DF_SPLIT_TU=0).
// The half state lives in the unused upper slot (q, q + 1) of the front's tile states.
// units (row block | column half-block << 2 of the 4 x 8 grid of 32 x 16 units; 255 = none) per part, wave and slot: see df_tu_tile
__device__ const unsigned char kTuUnits[3][8][3] = {
    {{0, 10, 19}, {4, 14, 23}, {1, 18, 27}, {5, 22, 31}, {9, 3, 255}, {13, 7, 255}, {2, 11, 255}, {6, 15, 255}},
    {{0, 255, 255}, {4, 255, 255}, {1, 255, 255}, {5, 255, 255}, {9, 255, 255}, {13, 255, 255}, {255, 255, 255}, {255, 255, 255}},
    {{18, 2, 255}, {22, 6, 255}, {19, 10, 255}, {23, 14, 255}, {27, 3, 255}, {31, 7, 255}, {255, 11, 255}, {255, 15, 255}}};
constexpr size_t kDfTuLds = ((size_t)128 * kSyrkLd + 128) * sizeof(double);
constexpr int kDfTileLd = 130;       // leading dimension of the diagonal tile handed from TU to D through LDS (even: 16-byte rows pairs stay aligned)
__device__ __forceinline__ bool df_tu_tile(const DevPlan& P, int s, int q, int r0, int rlim, const int* dstate, int dval, int* diag_state, int* row_state, int* half_state, int part,
                                           bool with_d, int* s_flag, double* sm, long long* marks) {
  constexpr int NBLK = 4, NB = 128, NPAIR = NBLK * (NBLK + 1) / 2;
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));
  const int tid = tid_, lane = tid & 63, wv = tid >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(wv);
  const int col0 = P.sn_col0[s];
  const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
  const int j0 = q * NB;
  // q + 1 < KB: panel q is a whole block column (nb = 128)
  double* F = P.arena + P.front_pos[s];
  double* Wb = P.wbuf + P.wbuf_pos[s] + (size_t)j0 * f;
  const double* X = P.invl + P.invl_pos[s] + (size_t)q * NB * NB;
  double* rdv = sm + NPAIR * kIB * kIB;
  // the rows this task solves: sixteen per wave, eight waves for a whole block row, four for a half
  const int roff = part == 2 ? 64 : 0;
  const int hrows = part == 0 ? 128 : 64;
  const bool solver = part == 0 || wave < 4;
  const int trow = roff + (part == 0 ? wv : (wv & 3)) * 16 + (lane & 15);      // row of the tile
  const int row = r0 + trow;
  const int rowc = min(row, f - 1);
  const bool valid = solver && row < rlim;
  const int lk = lane >> 4, li = lane & 3;
  const int l15 = lane & 15, l4 = lane >> 4;
  double t[NBLK * 8];
#pragma unroll
  for (int qq = 0; qq < NBLK * 8; ++qq) t[qq] = 0.0;
  if (solver) {
#pragma unroll
    for (int qq = 0; qq < NBLK * 8; ++qq) {
      const int c = 4 * qq + lk;
      t[qq] = keep_f64(F[(size_t)(j0 + c) * f + rowc], valid);
    }
  }
  // The diagonal tile (rows and columns [r0, rlim)) is updated in UNITS of 32 rows x 16 columns -- 8 MFMAs per k-step of four
  // panel columns, 4096 cycles of the SIMD's matrix pipe (1.75 us).  Only the lower triangle counts: 20 units of 32, dealt over the
  // waves so that every SIMD (waves w and w + 4 share one: scripts/simd_probe.hip) has TWO waves issuing -- one wave alone gets an
  // FP64 MFMA through every 32 cycles instead of every 16 (measured here: 512 MFMAs of one wave 6.9 us; the 64 x 32 pieces of the
  // first version, one or two per SIMD, took 10.7 us for the tile):
  //   part 0: 3, 3, 3, 3, 2, 2, 2, 2 units per wave (five per SIMD);
  //   part 1: its six units (row blocks 0 and 1) on waves 0-5;
  //   part 2: the six units of its own rows and columns on waves 0-5 (slot 0: they run while the workgroup waits for the other
  //           half's W), the eight left of them on waves 0-7 (slot 1).
  constexpr int NU = 3;
  int ucode[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) ucode[u] = __builtin_amdgcn_readfirstlane((int)kTuUnits[part][wave][u]);
  auto unit_on = [&](int u) { return ucode[u] != 255 && r0 + 32 * (ucode[u] & 3) < rlim && r0 + 16 * (ucode[u] >> 2) < rlim; };
  double acc[NU][4][2];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
#pragma unroll
    for (int cg = 0; cg < 4; ++cg) { acc[u][cg][0] = 0.0; acc[u][cg][1] = 0.0; }
    if (!unit_on(u)) continue;
    const int r = r0 + 32 * (ucode[u] & 3) + 2 * l15;
    const int rcl = min(r, f - 2);
    const int shift = r - rcl;
#pragma unroll
    for (int cg = 0; cg < 4; ++cg) {
      const int c = r0 + 16 * (ucode[u] >> 2) + cg * 4 + l4;
      const double* colp = F + (size_t)min(c, rlim - 1) * f;      // (columns of a pivot tile: clamped inside the panel)
      d2_t v;
      __builtin_memcpy(&v, colp + rcl, 16);
      const double e0 = shift == 0 ? v[0] : v[1];
      acc[u][cg][0] = keep_f64(e0, r < rlim && c < rlim && r >= c);
      acc[u][cg][1] = keep_f64(v[1], shift == 0 && r + 1 < rlim && c < rlim && r + 1 >= c);
    }
  }
  // a wait inside the task (the diagonal block of panel q; the other half's states): the worker's protocol, one flag word per wait
  auto await = [&](const int* state, int least, int* flag, int poller) -> bool {
    if (wave == poller) {
      int ok = 1, spins = 0;
      long long t0w = 0;
      for (;;) {
        if (__builtin_amdgcn_readfirstlane(ld_state(state)) >= least) break;
        const int stop = P.want_neg >= 0 ? __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&P.counters[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
        const int dead = __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&P.counters[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (stop | dead) { ok = 0; break; }
        if (wait_expired(spins, t0w)) {
          if (lane == 0) atomicExch(&P.counters[5], 1ull);
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      *flag = ok;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*flag) != 0;
  };
  if (!await(dstate, dval, s_flag, 0)) return false;
  if (marks && tid == 0) marks[0] = wall_clock64();        // D(q) has arrived
  {
    const int e = tid * 2;
    const int cc = e / kIB, rr = e - cc * kIB;
#pragma unroll
    for (int bi = 0; bi < NBLK; ++bi)
#pragma unroll
      for (int bp = 0; bp <= bi; ++bp) {
        double v[2];
        const int gr = bi * kIB + rr, gc = bp * kIB + cc;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const double* src = bp == bi ? X + (gr + u) + (size_t)gc * NB : F + (size_t)(j0 + gc) * f + j0 + gr + u;
          v[u] = *src;
        }
        double* dst = sm + (bi * (bi + 1) / 2 + bp) * kIB * kIB + e;
        dst[0] = v[0]; dst[1] = v[1];
      }
    if (tid < NB) rdv[tid] = 1.0 / P.dvals[col0 + j0 + tid];
  }
  __syncthreads();
#ifdef OKKT_TU_STAGE_MARK
  if (marks && tid == 0) marks[1] = wall_clock64();        // (variant build) the staged blocks are in LDS
#define OKKT_TU_SKIP_MARK1 1
#endif
  if (solver) {
#pragma unroll
    for (int bi = 0; bi < NBLK; ++bi) {
#pragma unroll
      for (int bp = 0; bp < bi; ++bp) {
        const double* Lb = sm + (bi * (bi + 1) / 2 + bp) * kIB * kIB;
#pragma unroll
        for (int gp = 0; gp < 8; ++gp)
#pragma unroll
          for (int g = 0; g < 8; ++g)
            t[bi * 8 + gp] = __builtin_amdgcn_mfma_f64_4x4x4f64(Lb[(gp * 4 + li) + (g * 4 + lk) * kIB], t[bp * 8 + g], t[bi * 8 + gp], 0, 0, 1 /* neg A */);
      }
      const double* Xb = sm + (bi * (bi + 1) / 2 + bi) * kIB * kIB;
      double wt[8];
#pragma unroll
      for (int gp = 0; gp < 8; ++gp) {
        wt[gp] = 0.0;
#pragma unroll
        for (int g = 0; g <= gp; ++g)
          wt[gp] = __builtin_amdgcn_mfma_f64_4x4x4f64(Xb[(gp * 4 + li) + (g * 4 + lk) * kIB], t[bi * 8 + g], wt[gp], 0, 0, 0);
      }
#pragma unroll
      for (int gp = 0; gp < 8; ++gp) t[bi * 8 + gp] = wt[gp];
    }
  }
#ifndef OKKT_TU_SKIP_MARK1
  if (marks && tid == 0) marks[1] = wall_clock64();        // rows solved
#endif
  const double myrd = tid < NB ? rdv[tid] : 0.0;
  __syncthreads();                       // every wave is done with the staged blocks and the reciprocals
  double* Wl = sm;                       // [128 panel columns][kSyrkLd]: W(r0 + r, j0 + p) at p * kSyrkLd + r
  double* rd2 = sm + (size_t)128 * kSyrkLd;
  if (solver) {
#pragma unroll
    for (int qq = 0; qq < NBLK * 8; ++qq) Wl[(size_t)(4 * qq + lk) * kSyrkLd + trow] = t[qq];      // rows past the block are zero
  }
  if (tid < NB) rd2[tid] = myrd;
  __syncthreads();
  if (marks && tid == 0 && part == 0) marks[2] = wall_clock64();        // W in LDS (a split task: the hand-over of the upper rows' W, below)
  // W and L = W D^-1 of the task's rows leave from LDS: 16-byte write-through stores of two consecutive rows, 1 KiB (512 B for
  // a half) of one column per wave instruction (the 8-byte sc1 stores straight from the solve's register layout took 9 us of the 42
  // between two diagonal blocks).
  auto store_wl = [&](int first_thread, int nthreads) {
    const int nrow = min(rlim - r0, roff + hrows);
    const int sh = part == 0 ? 6 : 5;                      // log2 of the row pairs per column
    if (tid < first_thread || tid >= first_thread + nthreads) return;
    for (int idx = tid - first_thread; idx < (128 << sh); idx += nthreads) {
      const int p = idx >> sh, x2 = roff + (idx & ((1 << sh) - 1)) * 2;
      d2_t w;
      __builtin_memcpy(&w, Wl + (size_t)p * kSyrkLd + x2, 16);
      const double rp = rd2[p];
      const d2_t l = (d2_t){w[0] * rp, w[1] * rp};
      double* wdst = Wb + (size_t)p * f + r0 + x2;
      double* ldst = F + (size_t)(j0 + p) * f + r0 + x2;
      if (x2 + 1 < nrow) { st_sc1_f64x2(wdst, w); st_sc1_f64x2(ldst, l); }
      else if (x2 < nrow) { st_agent_f64(wdst, w[0]); st_agent_f64(ldst, l[0]); }
    }
  };
  // the update of unit u: the operand fragments of the next k-step are requested before the products of the current one are issued
  auto update_unit = [&](auto uc) {
    constexpr int u = decltype(uc)::value;
    if (!unit_on(u)) return;
    const double* bw = Wl + 32 * (ucode[u] & 3) + 2 * l15;
    const double* bl = Wl + 16 * (ucode[u] >> 2) + (lane & 3);
    double nrd, nav[4];
    d2_t nbv;
    auto fetch = [&](int kk) {
      nrd = rd2[kk * 4 + l4];
      __builtin_memcpy(&nbv, bw + (kk * 4 + l4) * kSyrkLd, 16);
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) nav[cg] = bl[(kk * 4 + l4) * kSyrkLd + cg * 4];
    };
    fetch(0);
#pragma unroll 4
    for (int kk = 0; kk < NB / 4; ++kk) {
      double av[4];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const d2_t bv = nbv;
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) av[cg] = nav[cg] * nrd;
      fetch(min(kk + 1, NB / 4 - 1));
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) {
        acc[u][cg][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[cg], bv[0], acc[u][cg][0], 0, 0, 1 /* neg A */);
        acc[u][cg][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[cg], bv[1], acc[u][cg][1], 0, 0, 1 /* neg A */);
      }
    }
  };
  if (part == 1) {
    // the other half waits for these rows: out, drained, published
    store_wl(0, kDfThreadsC);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave == 0) __hip_atomic_store(half_state, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (marks && tid == 0) marks[2] = wall_clock64();      // W and L of the upper rows stored, drained, published
    update_unit(std::integral_constant<int, 0>());
  } else if (part == 2) {
    // W and L of these rows to memory (every wave its share: one wave alone has 64 stores in flight at most and took 8 us over
    // them); then waves 0-5 the units of its own rows and columns, wave 7 the wait for the other half's W
    store_wl(6 * 64, 128);
    update_unit(std::integral_constant<int, 0>());
    if (!await(half_state, 1, s_flag + 1, 0)) return false;
    if (marks && tid == 0) marks[2] = wall_clock64();      // ... and seen by the other half
    // W of the upper 64 rows (the column operand of this half's sub-tiles left of the diagonal) from memory into the image
#pragma unroll 4
    for (int it = 0; it < 8; ++it) {
      const int idx = it * kDfThreadsC + tid;
      const int p = idx >> 5, x2 = (idx & 31) * 2;
      d2_t w;
      __builtin_memcpy(&w, Wb + (size_t)p * f + r0 + x2, 16);
      __builtin_memcpy(Wl + (size_t)p * kSyrkLd + x2, &w, 16);
    }
    __syncthreads();
    update_unit(std::integral_constant<int, 1>());
  } else {
    update_unit(std::integral_constant<int, 0>());
    update_unit(std::integral_constant<int, 1>());
    update_unit(std::integral_constant<int, 2>());
  }
  // the wave's units to memory (write-through) ...
  auto store_piece = [&]() {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (!unit_on(u)) continue;
      const int r = r0 + 32 * (ucode[u] & 3) + 2 * l15;
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) {
        const int c = r0 + 16 * (ucode[u] >> 2) + cg * 4 + l4;
        if (c >= rlim) continue;
        double* colp = F + (size_t)c * f;
        if (r + 1 < rlim && r >= c) {
          st_sc1_f64x2(colp + r, (d2_t){acc[u][cg][0], acc[u][cg][1]});
        } else {
          if (r < rlim && r >= c) st_agent_f64(colp + r, acc[u][cg][0]);
          if (r + 1 < rlim && r + 1 >= c) st_agent_f64(colp + r + 1, acc[u][cg][1]);
        }
      }
    }
  };
  // ... or into the LDS tile the diagonal-block factorisation reads (column-major, leading dimension kDfTileLd, over the W image)
  auto piece_to_lds = [&]() {
    double* Tl = sm;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (!unit_on(u)) continue;
      const int r = 32 * (ucode[u] & 3) + 2 * l15;
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) {
        const int c = 16 * (ucode[u] >> 2) + cg * 4 + l4;
        const d2_t v = (d2_t){acc[u][cg][0], acc[u][cg][1]};
        __builtin_memcpy(Tl + (size_t)c * kDfTileLd + r, &v, 16);
      }
    }
  };
  if (part == 1) {
    // sub-tiles (0,0), (1,0), (1,1): to memory; the worker drains, meets and publishes half state 2
    if (marks && tid == 0) marks[3] = wall_clock64();
    store_piece();
    return true;
  }
  if (!with_d) {
    // the diagonal tile first: it is what D(q + 1) waits for.  Every storing wave drains, the workgroup meets, one wave publishes.
    store_piece();
    if (part == 2 && !await(half_state, 2, s_flag + 2, 0)) return false;      // ... the other half's sub-tiles are part of the tile
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave == 0) __hip_atomic_store(diag_state, dval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // tile (q + 1, q + 1) has received panel q (= q + 1 tasks)
    if (marks && tid == 0) marks[3] = wall_clock64();      // diagonal tile updated and published
    if (part == 0) store_wl(0, kDfThreadsC);
  } else {
    // TU(q) + D(q + 1) in one task: the block row's W and L go out (the other rows' updates of block column q + 1 wait for them:
    // stored ahead of the tile update they delayed it by 10 us, published from inside the factorisation they came 4 us late --
    // both measured slower on S-C3), then the updated diagonal tile is handed to the diagonal-block factorisation through LDS
    // -- no trip through HBM, no hand-off
    if (marks && tid == 0) marks[3] = wall_clock64();      // diagonal tile updated
    if (part == 0) store_wl(0, kDfThreadsC);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();                     // every wave has read its part of the W image
    piece_to_lds();
    if (part == 2) {
      if (!await(half_state, 2, s_flag + 2, 0)) return false;
      // the other half's sub-tiles: rows and columns [0, 64) of the tile, from memory
      double* Tl = sm;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int idx = it * kDfThreadsC + tid;
        const int c = idx >> 5, x2 = (idx & 31) * 2;
        d2_t v;
        __builtin_memcpy(&v, F + (size_t)(r0 + c) * f + r0 + x2, 16);
        v[0] = keep_f64(v[0], x2 >= c);
        v[1] = keep_f64(v[1], x2 + 1 >= c);
        __builtin_memcpy(Tl + (size_t)c * kDfTileLd + x2, &v, 16);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave == 0) __hip_atomic_store(row_state, dval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // tile (q + 1, q): W and L of the block row are in memory
  }
  return true;
}

// ---- U: tiles (i .. i + R - 1, j) -= W[rows, j0 .. j0 + nb) * L[columns of block j, j0 .. j0 + nb)^T ------------------------------
// k_big_syrk's tile (numeric.hip: 128 x 128 per workgroup of 2 x 4 waves, v_mfma_f64_4x4x4 with neg-A, both operand panels through
// an LDS-DMA ring of two 16-column chunks) with a row limit (the last pivot block of a front may be shorter than 128 rows) and sc1
// stores of the C tile.  One workgroup per CU has nobody to hide a tile's prologue (C tile: 6 us until it has landed, 4 us for the
// first operand chunk behind it) and epilogue, so a bulk task carries R row tiles of one tile column as ONE stream of operand
// chunks: the C tile of the next row block is requested while the current one is in its main loop (raw pairs in registers, masked
// when the accumulators switch), its first operand chunk follows the last chunk of the current tile through the ring, and the
// stores of a finished tile drain behind the next tile's first chunk.
// kDfContig (default): the loop is bound by the CU's LDS pipe; this is the LDS ARRAY's side of that bound.  With the earlier map the eight column fragments of a lane lie 4 doubles apart and come
// as 4 x ds_read2_b64 (8 array cycles each, against 4 for a ds_read_b128 of the same bytes), and at kSyrkLd = 144 every row read is 2-way bank-conflicted.
// Here the wave's columns are renamed so that a lane's fragments are 64 contiguous bytes, and the ring has its own two images (df_fragments.h): per
// k-step 6 conflict-free ds_read_b128, 24 instead of 40 + 8 array cycles, no VALU added.  Measured (profiles/contiguous_fragments_ab.txt): LDS-array cycles
// of the launch - 41 %, conflict share 0.143 -> 0.011, the chunk 10 268 -> 9 771 cycles, S-metric 18.09 -> 17.85 ms -- the array was part of the wait, not all.
// KC / STAGES: panel columns per ring slot and slots (32 x 2 for the one-workgroup-per-CU worker; 16 x 2 = 72 KB was the 128-VGPR
// bulk kernel's of the two-kernel form, scripts/experiments/r05_two_kernel_form.patch); MULTI: a task may carry several row tiles
// (the next C tile in a second register set); STAGGER: see below.
template <int KC, int STAGES, bool MULTI, bool STAGGER>
__device__ __forceinline__ void df_syrk_tiles(const DevPlan& P, int s, int j0, int nb, int i, int R_, int j, int KB, int k, double* sm, long long* marks, int* pub0 = nullptr, int pub_stride = 0, int pub_val = 0) {
  constexpr int NW = kSyrkNW;
  constexpr int kDfKC = KC;
  const int R = MULTI ? R_ : 1;
  constexpr int DMA = 2 * (kDfKC / NW);   // LDS-DMA instructions per wave and chunk
  constexpr int WCW = 128 / (NW / 2);   // columns per wave
  constexpr int NCG = WCW / 4;          // 4-column groups per wave
  constexpr int LDW = df_ring_ld_w(kDfContig), LDL = df_ring_ld_l(kDfContig), SLOT = df_ring_slot_doubles(kDfContig, kDfKC);      // the ring's images: df_fragments.h
  static_assert(WCW == 32 && NCG == 8, "df_fragments.h: 2 x 4 waves of 64 rows x 32 columns");
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));      // opaque: nothing derived from the lane id is hoisted out of the worker's loop and kept live across the other roles
  const int tid = tid_, lane = tid & 63, wv = tid >> 6;
  const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
  const int ct0 = df_block_lo(j, KB, k, f), clim = df_block_lo(j + 1, KB, k, f);
  const int cbase = ct0 + (wv >> 1) * WCW;
  double* F = P.arena + P.front_pos[s];
  double* Fc = F + (j >= KB ? P.cb_shift[s] : 0);      // the tile column's base: a block of the contribution block lives in the shared region
  const double* Wcol = P.wbuf + P.wbuf_pos[s] + (size_t)j0 * f + lane * 2;
  const double* Lg = F + (size_t)j0 * f + ct0 + lane * 2;
  const int l15 = lane & 15, l4 = lane >> 4;
  auto col_of = [&](int cg) { return cbase + df_frag_acc_col(kDfContig, lane, cg); };      // the column of accumulator group cg in this lane
  const int nchunk = (nb + kDfKC - 1) / kDfKC;
  const int total = R * nchunk;
  // operand chunk g of the stream: chunk g % nchunk of row tile g / nchunk
  auto issue = [&](int g) {
    const int r = g / nchunk, ch = g - r * nchunk;
    const double* Wg = Wcol + df_block_lo(i + r, KB, k, f);
    double* slot = sm + (size_t)(g % STAGES) * SLOT;
#pragma unroll
    for (int qq = 0; qq < kDfKC / NW; ++qq) {
      const int prow = qq * NW + wv;
      const int p = ch * kDfKC + prow;
      const double* wsrc = p < nb ? Wg + (size_t)p * f : P.zero_page + lane * 2;
      const double* lsrc = p < nb ? Lg + (size_t)p * f : P.zero_page + lane * 2;
      __builtin_amdgcn_global_load_lds(wsrc, (lds_void_t*)(slot + prow * LDW), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(lsrc, (lds_void_t*)(slot + kDfKC * LDW + prow * LDL), 16, 0, 0);
    }
  };
  // raw C pairs of a row tile (clamped addresses, no branches) and the masks that turn them into accumulators
  d2_t raw[NCG][2];
  auto load_c = [&](int r) {
    const int rbase = df_block_lo(i + r, KB, k, f) + (wv & 1) * 64;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c = col_of(cg);
      const double* colp = Fc + (size_t)min(c, clim - 1) * f;      // (clamped inside the tile column: a pivot block never reads past its panel)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rr = rbase + 2 * l15 + 32 * h;
        __builtin_memcpy(&raw[cg][h], colp + min(rr, f - 2), 16);
      }
    }
  };
  double acc[NCG][4];
  auto mask_c = [&](int r) {
    const int rbase = df_block_lo(i + r, KB, k, f) + (wv & 1) * 64;
    const int rlim = df_block_lo(i + r + 1, KB, k, f);
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c = col_of(cg);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rr = rbase + 2 * l15 + 32 * h;
        const int shift = rr - min(rr, f - 2);      // 0 in the interior, 1 when rr is the last row, >= 2 outside
        const double e0 = shift == 0 ? raw[cg][h][0] : raw[cg][h][1];
        acc[cg][2 * h] = keep_f64(e0, rr < rlim && c < clim && rr >= c);
        acc[cg][2 * h + 1] = keep_f64(raw[cg][h][1], shift == 0 && rr + 1 < rlim && c < clim && rr + 1 >= c);
      }
    }
  };
  load_c(0);
  asm volatile("" ::: "memory");
  mask_c(0);
#pragma unroll
  for (int g = 0; g < STAGES - 1; ++g) if (g < total) issue(g);
  // pub0 (round 6): a row tile of a multi-tile task is published as soon as its stores have drained -- behind the wait of the first chunk
  // iteration of the NEXT row tile -- instead of with the whole task (the caller then publishes the last row tile only): the tiles of a pair
  // used to become visible one tile's time late
  int pend_r = -1;
  int plain_until = 0;                     // chunks up to this one are waited for with vmcnt(0): ordinary loads / stores sit between the operand requests
  const int pre = min(2, nchunk - 1);      // chunk of a tile behind whose operand request the next tile's C is requested
  int r = 0, ch = 0;
  for (int g = 0; g < total; ++g) {
    {
      // chunk g has landed once only the chunks requested after it (at most STAGES - 2) are still outstanding
      const int later = g < plain_until ? 0 : min(STAGES - 2, total - 1 - g);
      if (later >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * DMA) : "memory");
      else if (later == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if constexpr (MULTI) {
      if (pend_r >= 0) {      // every wave's stores of that row tile have drained behind this iteration's vmcnt(0)
        if (tid == 0) __hip_atomic_store(pub0 + (size_t)pend_r * pub_stride, pub_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pend_r = -1;
      }
    }
    if (marks && g == 0 && tid == 0) { marks[0] = wall_clock64(); marks[3] = -(long long)clock64(); }       // C tile and the first operand chunk have landed; shader clock at the start of the main loop
    // the slot written next was last read one iteration ago; everyone is past that barrier.  Waves k and k + 4 share a SIMD and run
    // the same program: waves 0 - 3 request the next chunk right here, waves 4 - 7 in the middle of their MFMAs, so that one wave's
    // LDS-DMA issue (8 requests with their address arithmetic: ~ 1 200 cycles of a 10 500-cycle chunk) falls into its partner's
    // matrix work instead of both stalling the SIMD's matrix pipe at the same time (MI355X guide, two waves per SIMD, item 9)
    const bool late = STAGGER && wv >= 4;
    const bool more = g + STAGES - 1 < total;
    if (more && !late) issue(g + STAGES - 1);
    if constexpr (MULTI) { if (ch == pre && r + 1 < R) { load_c(r + 1); plain_until = g + STAGES; } }
    const int rt0 = df_block_lo(i + r, KB, k, f), rlim = df_block_lo(i + r + 1, KB, k, f);
    const int rbase = rt0 + (wv & 1) * 64;
    const bool active = !(rbase + 63 < cbase) && rbase < rlim && cbase < clim;
    if (active) {
      const double* slot = sm + (size_t)(g % STAGES) * SLOT;
      const double* bw = slot + (wv & 1) * 64 + 2 * l15;
      const double* bl = slot + kDfKC * kSyrkLd + (wv >> 1) * WCW + (lane & 3);      // (bw, bl: the earlier ring, OKKT_DF_CONTIG=0)
      if constexpr (kDfContig) {
        // a k-step: the four row fragments and the eight column fragments as 2 + 4 sixteen-byte reads (df_fragments.h)
  #pragma unroll
        for (int kk = 0; kk < kDfKC / 4; ++kk) {
          if (kk == (KC / 8) && more && late) issue(g + STAGES - 1);
          d2_t bq[2];
  #pragma unroll
          for (int h = 0; h < 2; ++h) bq[h] = *(const d2_t*)(slot + df_frag_b_off(kDfContig, wv, lane, kk, 2 * h));
  #pragma unroll
          for (int half = 0; half < NCG / 4; ++half) {
            d2_t aq[2];
  #pragma unroll
            for (int h = 0; h < 2; ++h) aq[h] = *(const d2_t*)(slot + df_frag_a_off(kDfContig, kDfKC, wv, lane, kk, half * 4 + 2 * h));
  #pragma unroll
            for (int qq = 0; qq < 4; ++qq)
  #pragma unroll
              for (int rb = 0; rb < 4; ++rb)
                acc[half * 4 + qq][rb] = __builtin_amdgcn_mfma_f64_4x4x4f64(aq[qq >> 1][qq & 1], bq[rb >> 1][rb & 1], acc[half * 4 + qq][rb], 0, 0, 1 /* neg A */);
          }
        }
      } else {
  #pragma unroll
        for (int kk = 0; kk < kDfKC / 4; ++kk) {
          if (kk == (KC / 8) && more && late) issue(g + STAGES - 1);
          double bv[4];
  #pragma unroll
          for (int rb = 0; rb < 4; ++rb) bv[rb] = bw[(kk * 4 + l4) * kSyrkLd + (rb & 1) + 32 * (rb >> 1)];
  #pragma unroll
          for (int half = 0; half < NCG / 4; ++half) {
            double av[4];
  #pragma unroll
            for (int qq = 0; qq < 4; ++qq) av[qq] = bl[(kk * 4 + l4) * kSyrkLd + (half * 4 + qq) * 4];
  #pragma unroll
            for (int qq = 0; qq < 4; ++qq)
  #pragma unroll
              for (int rb = 0; rb < 4; ++rb)
                acc[half * 4 + qq][rb] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[qq], bv[rb], acc[half * 4 + qq][rb], 0, 0, 1 /* neg A */);
          }
        }
      }
    } else if (more && late) issue(g + STAGES - 1);      // a wave without a piece of this tile still stages its rows
    if (++ch == nchunk) {
      if (marks && g == total - 1 && tid == 0) { marks[1] = wall_clock64(); marks[3] += (long long)clock64(); }      // main loop done: marks[3] = shader cycles of the main loop
      // the row tile is done: store it (write-through, not waited for here) and switch to the next one's accumulators
      if (active) {
        // (contiguous map: the eight column addresses are formed here, from a lane id read afresh -- hoisted out of the chunk loop they do
        // not fit beside the accumulators, and a reload from scratch in front of every store waits for the store before it)
        int lane_s = lane;
        if constexpr (kDfContig) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_s));
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) {
          const int c = kDfContig ? cbase + df_frag_acc_col(kDfContig, lane_s, cg) : col_of(cg);
          if (c >= clim) continue;
          double* colp = Fc + (size_t)c * f;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int rr = rbase + 2 * l15 + 32 * h;
            if (rr + 1 < rlim && rr >= c) {
              st_sc1_f64x2(colp + rr, (d2_t){acc[cg][2 * h], acc[cg][2 * h + 1]});
            } else {
              if (rr < rlim && rr >= c) st_agent_f64(colp + rr, acc[cg][2 * h]);
              if (rr + 1 < rlim && rr + 1 >= c) st_agent_f64(colp + rr + 1, acc[cg][2 * h + 1]);
            }
          }
        }
      }
      ch = 0;
      plain_until = g + STAGES;
      if constexpr (MULTI) { if (pub0 && r + 1 < R) pend_r = r; }
      ++r;
      if constexpr (MULTI) { if (r < R) mask_c(r); }
    }
  }
  if (marks && tid == 0) marks[2] = wall_clock64();        // stores issued
  // the ring's slots are reused by the next task of this workgroup: every wave is done reading them behind the caller's barrier
}

constexpr int kDfThreads = kDfThreadsC;
constexpr size_t kDfLds = std::max(std::max(std::max(std::max(OKKT_DIAG2_LDS_DOUBLES(kMW) * sizeof(double), kDfTuLds), (size_t)kDfStages * df_ring_slot_doubles(kDfContig, kDfKC) * sizeof(double)), kDfTlLds), (size_t)128 * kDfTileLd * sizeof(double));   // diag2_body's and df_tu_tile's; the other roles need less

// counters[5] = a wait ran into its bound, three seconds of wall clock (or another worker's did): every worker leaves, the factorisation
// fails with "a hand-off timed out" and the solves return NaN -- never numbers computed from tiles that had not arrived
__global__ __launch_bounds__(kDfThreads, 1) void k_front_dataflow(DevPlan P, const DfTask* __restrict__ tasks, int ntasks, int* __restrict__ head, double tol, int drop, int dbg, long long* __restrict__ tlog) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ int s_ctl[8];
  const int tid = threadIdx.x;
  if constexpr (!kDfLog) { tlog = nullptr; dbg = 0; }      // (the product library: no instrumentation in the kernel)
  // The scheduling code runs on WAVE 0 as a whole (a wave-uniform branch, every lane polls the same words): with an `if (tid == 0)`
  // around it hipcc threads the branch through the loop header, the structurizer turns the worker's loop into two nested loops and
  // lanes 1 .. 63 of wave 0 run ahead into the next s_barrier while lane 0 is masked off -- the workgroup hangs (round 4, first run)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int t_ahead = -1;      // wave 0: the queue position taken while the previous task's stores were draining
  for (;;) {
    if (wave == 0) {
      int t = t_ahead;
      if (t_ahead < 0) {
        if ((tid & 63) == 0) t = atomicAdd(head, 1);
        t = __builtin_amdgcn_readfirstlane(t);
      }
      int ok = 1;
      // a retry of the delta loop whose pivot counts already decide a wrong inertia: nothing more is started (the workers leave
      // within one task's time; the launches of the levels above return at their first pop)
      if (P.want_neg >= 0 && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&P.counters[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) ok = 0;
      if (tlog && t < ntasks && (tid & 63) == 0) { tlog[(size_t)t * 8] = wall_clock64(); tlog[(size_t)t * 8 + 3] = blockIdx.x; }
      if (t < ntasks && ok) {
        const DfTask tk = tasks[t];
        const int s = __builtin_amdgcn_readfirstlane(tk.front), type_nq = __builtin_amdgcn_readfirstlane(tk.type_nq), ij = __builtin_amdgcn_readfirstlane(tk.ij), q0 = __builtin_amdgcn_readfirstlane(tk.q0);
        const int type = type_nq & 255, nq = (type_nq >> 8) & 255, rows = max(type_nq >> 16, 1), i = ij & 0xffff, j = ij >> 16;
        const int k = P.sn_col0[s + 1] - P.sn_col0[s];
        const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
        const int KB = (k + 127) >> 7;
        const int TB = KB + ((f - k + 127) >> 7);
        const int* st = P.df_state + P.df_state_pos[s];
        // the tile states the task waits for, one per lane of the wave: (address, least value); the other lanes hold a condition
        // that is always true
        const int ln = tid & 63;
        const int* addr = st;
        int need = -(1 << 30);
        if (type == kDfD) { if (ln == 0) { addr = st + (size_t)i * TB + i; need = i; } }
        else if (type == kDfT) {
          if (ln == 0) { addr = st + (size_t)j * TB + j; need = j + 1; }
          if (ln == 1) { addr = st + (size_t)i * TB + j; need = j; }
        } else if (type == kDfTL) {      // tile (i, q) with panel q - 2 applied, block rows i and q of panel q - 1; D(q) is awaited inside the task
          if (ln == 0) { addr = st + (size_t)i * TB + j; need = j - 1; }
          if (ln == 1) { addr = st + (size_t)i * TB + (j - 1); need = j; }
          if (ln == 2) { addr = st + (size_t)j * TB + (j - 1); need = j; }
        } else if (type == kDfTU || type == kDfTA) {      // the tiles (q + 1, q) and (q + 1, q + 1), q = j; D(q) is awaited inside the task
          if (ln == 0) { addr = st + (size_t)i * TB + j; need = j; }
          if (ln == 1) { addr = st + (size_t)i * TB + i; need = j; }
        } else {
          const int ql = q0 + nq - 1;
          if (ln < rows) { addr = st + (size_t)(i + ln) * TB + ql; need = ql + 1; }                   // row operands
          else if (ln < 2 * rows) { addr = st + (size_t)(i + ln - rows) * TB + j; need = q0; }        // the tiles themselves
          else if (ln == 2 * rows) { addr = st + (size_t)j * TB + ql; need = ql + 1; }                // column operand
        }
        if (drop && ln == 0) need += 1 << 20;      // tests: a hand-off that never comes
        int spins = 0;
        long long t0w = 0;
        for (;;) {
          if (__builtin_amdgcn_ballot_w64(ld_state(addr) >= need) == ~0ull) break;
          // the stop flag of the delta loop (retries only) and the time-out word end every wait
          const int stop = P.want_neg >= 0 ? __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&P.counters[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
          const int dead = __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&P.counters[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          if (stop | dead) { ok = 0; break; }
          if (wait_expired(spins, t0w)) {
            if (ln == 0) atomicExch(&P.counters[5], 1ull);
            ok = 0;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tlog && (tid & 63) == 0) tlog[(size_t)t * 8 + 1] = wall_clock64();
      }
      s_ctl[0] = t; s_ctl[1] = ok;       // every lane of the wave writes the same two words
    }
    __syncthreads();
    const int t = __builtin_amdgcn_readfirstlane(s_ctl[0]);
    if (t >= ntasks || __builtin_amdgcn_readfirstlane(s_ctl[1]) == 0) return;
    const DfTask tk = tasks[t];
    const int s = __builtin_amdgcn_readfirstlane(tk.front);
    const int type_nq = __builtin_amdgcn_readfirstlane(tk.type_nq);
    const int ij = __builtin_amdgcn_readfirstlane(tk.ij);
    const int q0 = __builtin_amdgcn_readfirstlane(tk.q0);
    const int type = type_nq & 255, nq = (type_nq >> 8) & 255, rows = max(type_nq >> 16, 1), i = ij & 0xffff, j = ij >> 16;
    const int k = P.sn_col0[s + 1] - P.sn_col0[s];
    const int f = (int)(P.row_ptr[s + 1] - P.row_ptr[s]);
    const int KB = (k + 127) >> 7;
    const int TB = KB + ((f - k + 127) >> 7);
    int* st = P.df_state + P.df_state_pos[s];
    int* mine;
    int newv, npub = 1;
    if (type == kDfD) {
      if (!(dbg & 1)) diag2_body<true, kDiag2MW, kDfDiagMfmaWaves>(P, s, i, 128, tol, sm, nullptr, 0, tlog ? tlog + (size_t)t * 8 + 4 : nullptr);
      mine = st + (size_t)i * TB + i; newv = i + 1;
    } else if (type == kDfT) {
      if (!(dbg & 2)) df_trsm_tile(P, s, j, df_block_lo(i, KB, k, f), df_block_lo(i + 1, KB, k, f), sm);
      mine = st + (size_t)i * TB + j; newv = j + 1;
    } else if (type == kDfTL) {
      if (!df_tl_tile(P, s, j, df_block_lo(i, KB, k, f), df_block_lo(i + 1, KB, k, f), st + (size_t)j * TB + j, &s_ctl[2], sm, tlog ? tlog + (size_t)t * 8 + 4 : nullptr)) return;
      mine = st + (size_t)i * TB + j; newv = j + 1;
    } else if (type == kDfTU || type == kDfTA) {
      // nq & 2: D(q + 1) is part of the task (the updated diagonal tile reaches it through LDS); nq & 4: the lower half of a split block
      // row (the upper half is the TA task right before it in the queue)
      const bool with_d = type == kDfTU && (nq & 2);
      const int part = type == kDfTA ? 1 : ((nq & 4) ? 2 : 0);
      int* hs = st + (size_t)j * TB + i;          // the unused upper slot (q, q + 1): the state of the upper half
      if (!df_tu_tile(P, s, j, df_block_lo(i, KB, k, f), df_block_lo(i + 1, KB, k, f), st + (size_t)j * TB + j, j + 1, st + (size_t)i * TB + i, st + (size_t)i * TB + j, hs, part, with_d,
                      &s_ctl[2], sm, tlog ? tlog + (size_t)t * 8 + 4 : nullptr)) return;
      if (type == kDfTA) {
        mine = hs; newv = 2;
      } else if (with_d) {
        diag2_body<true, kDiag2MW, kDfDiagMfmaWaves>(P, s, i, 128, tol, sm, sm, kDfTileLd);
        mine = st + (size_t)i * TB + i; newv = i + 1;          // tile (q + 1, q) was published inside the task
      } else {
        mine = st + (size_t)i * TB + j; newv = j + 1;
      }
    } else {
      const int j0 = q0 * 128;
      mine = st + (size_t)i * TB + j; newv = q0 + nq; npub = rows;
      if (!(dbg & 4)) {
        if (kDfMulti && rows > 1 && P.df_early_pub) {      // the row tiles but the last are published from inside the task, as their stores drain
          df_syrk_tiles<kDfKC, kDfStages, kDfMulti, kDfStagger>(P, s, j0, min(nq * 128, k - j0), i, rows, j, KB, k, sm, tlog ? tlog + (size_t)t * 8 + 4 : nullptr, mine, TB, newv);
          mine += (size_t)(rows - 1) * TB; npub = 1;
        } else df_syrk_tiles<kDfKC, kDfStages, kDfMulti, kDfStagger>(P, s, j0, min(nq * 128, k - j0), i, rows, j, KB, k, sm, tlog ? tlog + (size_t)t * 8 + 4 : nullptr);
      }
    }
    // the next queue position is requested now: the atomic's round trip (1 us) runs beside the drain of this task's stores
    int t_pre = 0;
    if (wave == 0 && (tid & 63) == 0) t_pre = atomicAdd(head, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave: its sc1 stores have been acknowledged
    __syncthreads();                                      // ... and every wave is done with the LDS of this task and with s_ctl
    if (tlog && tid == 0) tlog[(size_t)t * 8 + 2] = wall_clock64();
    if (wave == 0) {      // lane r publishes row tile r of the task (one tile for every kind but the bulk updates)
      const int ln = tid & 63;
      if (ln < npub) __hip_atomic_store(mine + (size_t)ln * TB, newv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      t_ahead = __builtin_amdgcn_readfirstlane(t_pre);
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

const char* df_build_flags() {
  return kDfLog ? "log=1" : "log=0";
}

std::string df_setup(Numeric& N) {
  DevPlan& d = N.d;
  const int ns = d.nsuper;
  N.df_tasks = nullptr; N.df_heads = nullptr; N.n_df_heads = 0; N.df_state_ints = 0;
  d.df_state = nullptr; d.df_state_pos = nullptr;
  if (!N.dataflow || N.nb != 128) return "";
  std::vector<int64_t> spos(ns, -1);
  int64_t total = 0;
  std::vector<DfTask> all;
  std::vector<DfTask> q;
  int nheads = 0;
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) == hipSuccess) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount; }
  N.df_workers = getenv("OKKT_DF_WORKERS") ? std::max(1, atoi(getenv("OKKT_DF_WORKERS"))) : ncu;
  N.df_group = getenv("OKKT_DF_GROUP") ? std::max(1, std::min(atoi(getenv("OKKT_DF_GROUP")), 16)) : 4;
  N.df_fuse_d = getenv("OKKT_DF_FUSE_D") ? atoi(getenv("OKKT_DF_FUSE_D")) : 1;
  N.df_split_tu = getenv("OKKT_DF_SPLIT_TU") ? atoi(getenv("OKKT_DF_SPLIT_TU")) : 1;
  N.df_fuse_tl = getenv("OKKT_DF_FUSE_TL") ? atoi(getenv("OKKT_DF_FUSE_TL")) : 1;
  d.df_early_pub = getenv("OKKT_DF_EARLY_PUB") ? atoi(getenv("OKKT_DF_EARLY_PUB")) : 1;      // multi-tile update tasks publish every row tile as its stores drain (round 6; 0: with the task)
  N.df_rows = (kDfMulti && getenv("OKKT_DF_ROWS")) ? std::max(1, std::min(atoi(getenv("OKKT_DF_ROWS")), 8)) : 1;
  OKKT_HIP_TRY(hipFuncSetAttribute((const void*)k_front_dataflow, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64));
  auto do_sched = [&](std::vector<LevelSchedule>& levels) {
    for (LevelSchedule& L : levels) {
      Segment& g = L.seg[3];
      g.df_off = -1; g.df_cnt = 0; g.df_head = -1; g.df_flops = 0;
      if (g.cnt == 0) continue;
      std::vector<DfFront> fronts;
      for (int a = 0; a < g.cnt; ++a) {
        const int s = N.sched_host[g.off + a];
        const int f = N.sn_f[s], k = N.sn_k[s];
        fronts.push_back({s, f, k});
        if (spos[s] < 0) {
          const int64_t TB = (k + 127) / 128 + (f - k + 127) / 128;
          spos[s] = total;
          total += TB * TB;
        }
        g.df_flops += (double)k * f * f - (double)k * k * f + (double)k * k * k / 3.0;
      }
      double model = 0;
      df_build_queue(fronts, N.df_workers, N.df_group, N.df_rows, N.df_fuse_d != 0, N.df_split_tu != 0, q, &model, N.df_fuse_tl != 0, kDfMulti);
      g.df_off = (int64_t)all.size();
      g.df_cnt = (int)q.size();
      g.df_head = nheads++;
      all.insert(all.end(), q.begin(), q.end());
      if (getenv("OKKT_DEBUG_FRONTS")) fprintf(stderr, "okkt: dataflow level: %d fronts (largest %d x %d), %d tasks, model %.0f us\n", g.cnt, g.maxf, g.maxk, g.df_cnt, model);
    }
  };
  do_sched(N.levels);
  do_sched(N.levels_top);
  N.n_df_heads = nheads;
  N.df_state_ints = total;
  auto up = [&](const void* src, size_t bytes, void** out) -> std::string {
    void* p = nullptr;
    OKKT_HIP_TRY(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    N.allocations.push_back(p);
    if (bytes) OKKT_HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *out = p;
    return "";
  };
  std::string e;
  if (!(e = up(spos.data(), spos.size() * sizeof(int64_t), (void**)&d.df_state_pos)).empty()) return e;
  if (!(e = up(all.data(), all.size() * sizeof(DfTask), (void**)&N.df_tasks)).empty()) return e;
  if (total + (int64_t)nheads * kDfHeadStride >= (int64_t)1 << 31) return "dataflow: tile states beyond 2^31";
  {
    void* p = nullptr;      // tile states, then the queue heads: one fill per factorisation clears both
    const size_t bytes = ((size_t)total + (size_t)nheads * kDfHeadStride + 16) * sizeof(int);
    OKKT_HIP_TRY(hipMalloc(&p, bytes));
    N.allocations.push_back(p);
    OKKT_HIP_TRY(hipMemset(p, 0, bytes));
    // the handle's streams are non-blocking: nothing else orders this null-stream fill before the first factorisation's own clear and
    // launch (dalloc() documents the same race for its zero fills; advisor, round 5)
    OKKT_HIP_TRY(hipStreamSynchronize(nullptr));
    d.df_state = (int*)p;
    N.df_heads = d.df_state + total;
  }
  return "";
}

std::string df_launch(Numeric& N, const DevPlan& P, const Segment& g, hipStream_t st, double tol) {
  if (g.df_cnt <= 0) return "";
  static const int drop = getenv("OKKT_DEBUG_DROP_HANDOFF") ? atoi(getenv("OKKT_DEBUG_DROP_HANDOFF")) : 0;
  static const int dbg_env = getenv("OKKT_DEBUG_DATAFLOW") ? atoi(getenv("OKKT_DEBUG_DATAFLOW")) : 0;   // 1 / 2 / 4: skip the bodies of D / T / U (wrong results), 8: synchronise and report every launch, 16: per-task time stamps appended to $OKKT_DF_LOG
  static const int dbg = kDfLog ? dbg_env : (dbg_env & 8);
  static const bool warned = [] {
    if (!kDfLog && (dbg_env & ~8)) fprintf(stderr, "okkt: OKKT_DEBUG_DATAFLOW=%d: the task log and the body switches are compiled into libonephase_kkt_log.so only (OKKT_LIB_PATH); ignored here\n", dbg_env);
    return true;
  }();
  (void)warned;
  const int grid = std::min(g.df_cnt, N.df_workers);
  long long* tlog = nullptr;
  if (dbg & 16) { OKKT_HIP_TRY(hipMalloc((void**)&tlog, (size_t)g.df_cnt * 8 * sizeof(long long))); OKKT_HIP_TRY(hipMemsetAsync(tlog, 0, (size_t)g.df_cnt * 8 * sizeof(long long), st)); }   // debug only: per task pop / ready / end ticks (10 ns) and the worker
  hipLaunchKernelGGL(k_front_dataflow, dim3(grid), dim3(kDfThreads), kDfLds, st, P, N.df_tasks + g.df_off, g.df_cnt, N.df_heads + g.df_head * kDfHeadStride, tol, (drop & 4) ? 1 : 0, dbg, tlog);
  if (dbg & 24) {
    hipError_t e2 = hipStreamSynchronize(st);
    fprintf(stderr, "okkt: dataflow launch of %d tasks on %d workers: %s\n", g.df_cnt, grid, hipGetErrorString(e2));
  }
  if (tlog) {
    std::vector<long long> hl((size_t)g.df_cnt * 8);
    std::vector<DfTask> ht((size_t)g.df_cnt);
    OKKT_HIP_TRY(hipMemcpy(hl.data(), tlog, hl.size() * sizeof(long long), hipMemcpyDeviceToHost));
    OKKT_HIP_TRY(hipMemcpy(ht.data(), N.df_tasks + g.df_off, ht.size() * sizeof(DfTask), hipMemcpyDeviceToHost));
    (void)hipFree(tlog);
    const char* path = getenv("OKKT_DF_LOG");
    if (FILE* fp = fopen(path ? path : "/tmp/okkt_df_log.txt", "a")) {
      fprintf(fp, "# launch %d tasks %d workers (index front type i j q0 nq worker pop ready end [10 ns ticks])\n", g.df_cnt, grid);
      for (int t = 0; t < g.df_cnt; ++t)
        fprintf(fp, "%d %d %d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld\n", t, ht[t].front, ht[t].type_nq & 255, ht[t].ij & 0xffff, ht[t].ij >> 16, ht[t].q0, ht[t].type_nq >> 8,
                hl[(size_t)t * 8 + 3], hl[(size_t)t * 8], hl[(size_t)t * 8 + 1], hl[(size_t)t * 8 + 2], hl[(size_t)t * 8 + 4], hl[(size_t)t * 8 + 5], hl[(size_t)t * 8 + 6], hl[(size_t)t * 8 + 7]);
      fclose(fp);
    }
  }
  OKKT_HIP_TRY(hipGetLastError());
  return "";
}

}  // namespace okkt

// the maps of df_fragments.h as this library's kernel was compiled with them (host only; tests/test_dataflow_fragments.py)
extern "C" int64_t okkt_debug_dataflow_fragment(int32_t map, int32_t what, int32_t wave, int32_t lane, int32_t kk, int32_t idx) {
  using namespace okkt;
  if (map < 0) map = kDfContig;
  if (map > 1 || wave < 0 || wave >= 8 || lane < 0 || lane >= 64 || kk < 0 || kk >= kDfKC / 4 || idx < 0 || idx >= 8) return OKKT_ERR_INVALID;
  switch (what) {
    case 0: return df_frag_acc_col(map, lane, idx);
    case 1: return df_frag_a_col(map, lane, idx);
    case 2: return df_frag_a_off(map, kDfKC, wave, lane, kk, idx);
    case 3: return idx < 4 ? df_frag_b_off(map, wave, lane, kk, idx) : OKKT_ERR_INVALID;
    case 4: return df_ring_rot(map, 4 * kk + (lane >> 4));
    case 5: {
      const int64_t geo[8] = {df_ring_ld_w(map), df_ring_ld_l(map), df_ring_slot_doubles(map, kDfKC), kDfKC, kDfStages, kDfContig, (int64_t)kDfLds, kSyrkLd};
      return geo[idx];
    }
  }
  return OKKT_ERR_INVALID;
}
