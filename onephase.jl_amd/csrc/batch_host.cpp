// Uniform batches, host side: the grids of a batch from the analysed pattern alone -- what okkt_batch_query
// answers, also on handles without a device, and what the sanitizer driver runs.
#include "batch.h"
#include "batch_schur.h"

#include "../../include/okkt.h"
#include "solve_sparse.h"

namespace okkt {

void batch_shape(const Symbolic& S, int small_max, BatchShape& out) {
  out = BatchShape();
  out.max_front = (int)S.max_front;
  const int ns = S.nsuper;
  for (int s = 0; s < ns; ++s)
    if (S.row_ptr[s + 1] - S.row_ptr[s] > small_max) { out.reason = OKKT_BATCH_BIG_FRONTS; return; }
  // the units of the device schedule (numeric_setup): with small fronts only, every unit is a workgroup task, and a level of the
  // schedule holds the units of one height
  FrontUnits U;
  form_front_units(S, small_max, U);
  for (int s = 0; s < ns; ++s)
    if (U.unit_root[s] == s) out.levels = std::max(out.levels, U.ulevel[s] + 1);
  out.level_cnt.assign((size_t)out.levels, 0);
  out.level_maxf.assign((size_t)out.levels, 0);
  for (int s = 0; s < ns; ++s) {
    const int l = U.ulevel[U.unit_root[s]];
    out.level_maxf[(size_t)l] = std::max(out.level_maxf[(size_t)l], (int)(S.row_ptr[s + 1] - S.row_ptr[s]));
    if (U.unit_root[s] != s) continue;
    ++out.level_cnt[(size_t)l];
    ++out.tasks;
  }
}

int64_t batch_slot_doubles(const Symbolic& S, int64_t arena_doubles, int R) {
  // arena, D, shift, x and z of the sweeps, contribution vectors, one line of counters
  return batch_arena_stride(S, arena_doubles) + 2 * S.n + (int64_t)R * (2 * S.n + S.sum_r) + 16;
}

// ---- scenario batches ------------------------------------------------------------------------------------
void schur_batch_shape(const Symbolic& S, int small_max, SchurBatchShape& out) {
  out = SchurBatchShape();
  out.ns = S.nschur;
  if (S.nschur <= 0) { out.reason = OKKT_SBATCH_NO_SET; return; }
  const int ns = S.nsuper, schur_sn = ns - 1;      // the Schur front: the last supernode, a unit that no schedule holds
  for (int s = 0; s < schur_sn; ++s) out.max_front = std::max(out.max_front, (int)(S.row_ptr[s + 1] - S.row_ptr[s]));
  if (out.max_front > small_max) { out.reason = OKKT_SBATCH_BIG_FRONTS; return; }
  if (S.nschur > kSchurBatchMaxSet) { out.reason = OKKT_SBATCH_SET_TOO_LARGE; return; }
  FrontUnits U;
  form_front_units(S, small_max, U);
  for (int s = 0; s < schur_sn; ++s) {
    if (U.unit_root[s] != s) continue;
    out.levels = std::max(out.levels, U.ulevel[s] + 1);
    ++out.tasks;
  }
}

int64_t schur_batch_item_doubles(int64_t ns, int R) {
  return (int64_t)R * ns + (ns * ns + 4 * ns + kSchurBatchGroup - 1) / kSchurBatchGroup;
}

int64_t schur_batch_shared_doubles(int64_t ns) {
  // the sum, r2 / x2; the dense factor: F, the panel W, the solves' vectors X, the pivot arrays (three ints per column)
  return ns * ns + 4 * ns + ns * ns + ns * kDlNB + 12 * ns + 2 * ns;
}

}  // namespace okkt
