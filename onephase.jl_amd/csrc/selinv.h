// Selected inversion (selinv.hip): the entries of Z = F^-1 on the stored supernodal pattern of the factor,
// computed top-down over the supernodal tree.  The state lives on the solver handle (SelinvWork), not in DevPlan: the factorisation
// and solve kernels are unchanged by it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "numeric.h"
#include "symbolic.h"

namespace okkt {

constexpr int kSlB = 64;                       // pivot columns per block step of a front
constexpr int kSlGatherCols = 8;               // columns of the gathered Z_RR per workgroup
constexpr int64_t kSlChunkDoubles = 1 << 25;   // scratch of one chunk of a level (256 MiB), raised to the largest single front's need

// one front in the top-down schedule: its panels and its slices of the chunk's scratch (doubles)
struct SlFront {
  int64_t L;    // factor panel (arena offset, f rows x k columns, leading dimension f)
  int64_t Zp;   // Z panel (Z arena offset, same shape)
  int64_t T;    // Z_RR gathered from the ancestors, r x r, both triangles
  int64_t W;    // W = L_{below block} L_jj^-1 for every block j, panel shape
  int64_t P;    // partial products W_j' Z_j of the row tiles, kSlB x kSlB each
  int s, f, k, r, q, col0, parent, pad;
};
static_assert(sizeof(SlFront) == 72, "host and device agree on the record");

struct SlItem { int slot, idx; };

struct SlChunk {
  int f_off = 0, f_cnt = 0;                  // its fronts in SelinvWork::fr
  int64_t g_off = 0, g_cnt = 0;              // gather items
  int64_t w_off = 0, w_cnt = 0;              // block-inverse items
  int nsteps = 0;
  std::vector<int64_t> z_off, z_cnt;         // per block step: column-product items
};

struct SelinvWork {
  bool planned = false;
  int64_t analysis = -1;        // okkt_solver_s::n_analyze_calls the plan belongs to
  const double* arena = nullptr;  // ... and the front arena (a new device plan gets a new one)
  int64_t factor_seq = -1;      // the factorisation Z was computed from (-1: none)
  int skip_sn = -1;             // the supernode the plan leaves out of the block steps (the Schur front, section 8.10; -1: none)
  int64_t dense_seq = -1;       // Schur route: the okkt_schur_factor whose S^-1 seeded Z
  int64_t z_doubles = 0, scratch_doubles = 0, bytes = 0;
  double flops = 0;             // products of the block steps (2 m^2 w + 2 m w^2 per step), informational
  double* Z = nullptr;
  double* scratch = nullptr;
  int64_t* zpos = nullptr;      // [nsuper] Z panel bases
  int* col2sn = nullptr;        // [n]
  SlFront* fr = nullptr;        // [nsuper] in schedule order
  SlItem* items = nullptr;
  int64_t* dpos = nullptr;      // [n] Z offset of the diagonal entry of permuted column i
  int64_t* zmap = nullptr;      // [nnz_in] Z offset of each input entry (mirrored), -1: outside the pattern
  unsigned long long* count = nullptr;
  std::vector<int64_t> zpos_host;
  std::vector<SlChunk> chunks;
  std::vector<void*> allocs;
};

// host plan and allocations for the current analysis (colptr / rowval: the analysed input pattern, index base = colptr[0])
// skip_sn: a root supernode whose Z panel the caller fills before selinv_enqueue (the Schur front of the Schur route); it gets a panel
// and no block step
std::string selinv_setup(const Symbolic& S, const Numeric& N, const int64_t* colptr, const int64_t* rowval, SelinvWork& W, int skip_sn = -1);
void selinv_release(SelinvWork& W);
// Z from the factor in N (enqueued on N.stream) and the count of its non-finite entries into W.count (no synchronisation)
std::string selinv_enqueue(const Numeric& N, SelinvWork& W);
// diag(Z) in original order / Z at every input entry (NaN outside the pattern), on `st`
void selinv_diag_enqueue(const Numeric& N, const SelinvWork& W, int64_t n, double* d_out, hipStream_t st);
void selinv_pattern_enqueue(const SelinvWork& W, int64_t nnz, double* d_out, hipStream_t st);

}  // namespace okkt
