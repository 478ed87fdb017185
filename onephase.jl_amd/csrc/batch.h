// Uniform batches: B systems on one analysed pattern.  The slots of the items (batch.hip allocates and
// launches, api_batch.cpp is the C ABI) and the host-side description of the grids (batch_shape: no device, also what
// okkt_batch_query answers from).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "symbolic.h"

namespace okkt {

struct Numeric;

// why a plan takes no batch (okkt.h: OKKT_BATCH_*), and the grids of one that does
struct BatchShape {
  int reason = 0;
  int levels = 0, max_front = 0;
  int64_t tasks = 0;
  std::vector<int> level_cnt, level_maxf;      // tasks and largest front per level of the task tree
};
// S analysed; small_max as numeric_setup clamps it.  Fills levels / tasks from the units of form_front_units (the ones the device
// schedule is made of); reason = OKKT_BATCH_BIG_FRONTS when a front is larger than small_max (the counts are then not filled)
void batch_shape(const Symbolic& S, int small_max, BatchShape& out);
// doubles of one slot: arena_doubles as the device plan allocates them (or the dense bound), R work columns (1, 2 or 4)
int64_t batch_slot_doubles(const Symbolic& S, int64_t arena_doubles, int R);
inline int batch_work_columns(int64_t nrhs_max) { return nrhs_max >= 3 ? 4 : (int)std::max<int64_t>(nrhs_max, 1); }
inline int64_t batch_arena_stride(const Symbolic& S, int64_t arena_doubles) { return (arena_doubles + 512 + (int64_t)S.max_front * 2 + 1) & ~(int64_t)1; }

// OKKT_BATCH_AUTO is level mode.  Measured (profiles/batch_throughput.json): level mode is ahead at every batch
// size up to 4096 on the hanging chain (by 1.4 x at B = 4096, by 12 x at B = 64); on S-tiny item mode only draws level at B = 4096
// (3.54 against 3.49 M systems/s, the device times equal): no measured case where item mode pays, so it is taken only when forced

// per-item state in HBM; item b of an array starts at base + b * stride
struct BatchSlots {
  double* arena = nullptr;   int64_t arena_stride = 0;
  double* dvals = nullptr;   // stride n
  double* diagadd = nullptr; // stride n
  double* xwork = nullptr;   // stride R * n
  double* zwork = nullptr;
  double* cv = nullptr;      // stride R * sum_r
  unsigned long long* counters = nullptr;   // stride kCountStride: pos, neg, zero, nonfinite
  int64_t n = 0, sum_r = 0;
  int R = 0;
};

struct BatchWork {
  BatchSlots s;
  int64_t B = 0, nrhs_max = 0;
  int64_t generation = 0;        // counts the reservations made and released: what holds state of its own per slot (kkt_batch.hip) compares it
  int64_t arena_len = 0;         // doubles of the handle's own arena (the copy of okkt_batch_select)
  int64_t factored_B = 0;        // items of the last okkt_factor_batch (0: none)
  int mode = 0, env_mode = 0, mode_used = 0;   // mode forced by okkt_batch_set_mode (0 = none), by OKKT_BATCH_MODE at the reservation, mode of the last factorisation
  double* shift = nullptr;       // [B] the items' shifts on the device
  int* items = nullptr;          // [B] the slots of a factorisation over an item list (solver_factor_batch_device with items)
  std::vector<int64_t> inertia;  // [factored_B][4]
  std::vector<int> flags;
  std::vector<unsigned long long> raw;
  // the device plan the slots were sized and laid out for (okkt_batch_reserve): a plan rebuilt since with another layout -- a partition
  // set on the analysed handle -- makes the reservation stale, and every batch call refuses it (api_batch.cpp, batch_ready)
  int64_t plan_arena_doubles = 0, plan_tasks = 0;
  int plan_levels = 0;
  // the grids of the analysed pattern, counted once per analysis (okkt_stats.n_analyze_calls) and small_front_max
  BatchShape shape;
  int64_t shape_analysis = -1;
  int shape_small_max = 0;
};

std::string batch_alloc(BatchWork& W, const Symbolic& S, int64_t arena_doubles, int64_t B, int64_t nrhs_max, bool* oom);
void batch_free(BatchWork& W);
// item mode needs every contribution block in a place of its own for the whole factorisation (numeric_setup gives that to plans
// whose levels run as one epoch)
bool batch_item_mode_ok(const Numeric& N);
int batch_pick_mode(const BatchWork& W, const Numeric& N, int64_t B);
// all on N.stream, no synchronisation.  d_shift: W.shift filled by the caller (NULL: zero shift).  d_items (level mode only): B slots;
// grid item j works on slot d_items[j] -- its values at d_vals + slot * val_stride, its shift W.shift[slot]; NULL: slot j
std::string batch_factor_enqueue(Numeric& N, BatchWork& W, int mode, int64_t B, const double* d_vals, int64_t val_stride, bool shifted,
                                 int64_t nshift, double tol, const int* d_items = nullptr);
// right-hand sides r0 .. r0 + nr of every item (R = 1, 2 or 4 columns carried); rhs / sol [B][nrhs][n]
std::string batch_solve_enqueue(Numeric& N, BatchWork& W, int mode, int64_t B, const double* d_rhs, double* d_sol, int64_t nrhs, int64_t r0,
                                int nr, int R);
std::string batch_select_enqueue(Numeric& N, BatchWork& W, int64_t b);
// the parts of a level-mode solve, for callers that put work of their own between the sweeps (batch_schur.hip): xwork <- rhs, the levels
// upwards, the levels downwards, sol <- xwork
std::string batch_permute_in_enqueue(Numeric& N, BatchWork& W, int64_t B, const double* d_rhs, int64_t nrhs, int64_t r0, int nr, int R);
std::string batch_fwd_enqueue(Numeric& N, BatchWork& W, int64_t B, int R);
std::string batch_bwd_enqueue(Numeric& N, BatchWork& W, int64_t B, int R);
std::string batch_permute_out_enqueue(Numeric& N, BatchWork& W, int64_t B, double* d_sol, int64_t nrhs, int64_t r0, int nr, int R);

}  // namespace okkt
