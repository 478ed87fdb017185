// Uniform batches, host side: the grids of a batch from the analysed pattern alone -- what okkt_batch_query
// answers, also on handles without a device, and what the sanitizer driver runs.
#include "batch.h"

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

}  // namespace okkt
