// Scenario batches: B items in Schur mode on one analysed pattern [[A11 A12]; [A21 A22]] -- every item factors
// its A11 and assembles its S_b, the S_b are summed in a fixed order, one dense factor of the sum solves the linking system of the
// arrowhead matrix.  The items' slots are a BatchWork (batch.hip: the interior is the level mode of the uniform batches); this header
// adds what all items share.  batch_schur.hip allocates and launches, api_batch_schur.cpp is the C ABI, the shape comes from
// batch_host.cpp (no device).
#pragma once
#include <cstdint>
#include <string>

#include "batch.h"
#include "dense_ldlt.h"

namespace okkt {

struct Numeric;

// the sums run over groups of this many items (OKKT_SBATCH_GROUP in okkt.h: a constant of the interface)
constexpr int kSchurBatchGroup = 32;

// why a plan takes no scenario batch (okkt.h: OKKT_SBATCH_*), and the grids of the interior of one that does
struct SchurBatchShape {
  int reason = 0;
  int levels = 0, max_front = 0;      // of the interior: the Schur front is in no level and under no bound
  int64_t tasks = 0, ns = 0;
};
// S analysed, not partitioned; small_max as numeric_setup clamps it.  reason: OKKT_SBATCH_OK, _NO_SET, _BIG_FRONTS (an interior front
// above small_max), _SET_TOO_LARGE (ns above the bound of the column-in-LDS assembly), in this order
void schur_batch_shape(const Symbolic& S, int small_max, SchurBatchShape& out);
constexpr int kSchurBatchMaxSet = 2048;
// doubles of one item beyond its slot: its right-hand side of the linking system, its share of the group partials (a started group counts whole)
int64_t schur_batch_item_doubles(int64_t ns, int R);
// doubles all items share: the sum, r2 / x2, the dense factor's buffers
int64_t schur_batch_shared_doubles(int64_t ns);

struct SchurBatchWork {
  BatchWork w;                   // the items' slots; w.factored_B: items of the last okkt_factor_schur_batch
  int64_t ns = 0;
  int64_t front_pos = 0;         // the Schur front in an item's arena (the single-system plan's place)
  int64_t gcb = 0;               // its first column in the extend-add lists
  int schur_sn = -1;
  double* sum = nullptr;         // ns x ns: the sum of the items' S_b handed out by okkt_schur_batch_get(-1), both triangles
  double* part = nullptr;        // [G][ns x ns]: the group partials of the sum (lower triangles)
  double* r2i = nullptr;         // [B][4][ns]: the items' right-hand sides of the linking system
  double* r2p = nullptr;         // [G][4][ns]: their group partials
  double* r2 = nullptr;          // [4][ns]: the summed right-hand side, overwritten by x2
  DenseLdltWork dl;              // the batch's own dense factor (the handle's is not touched)
  bool dense_ok = false;         // dl is the factor of the last factorisation's sum
  SchurBatchShape shape;
  int64_t shape_analysis = -1;
  int shape_small_max = 0;
};

// slots as batch_alloc lays them out, then the shared buffers
std::string schur_batch_alloc(SchurBatchWork& W, const Symbolic& S, const Numeric& N, int64_t B, int64_t nrhs_max, bool* oom);
void schur_batch_free(SchurBatchWork& W);

// all on N.stream, no synchronisation, every dependency a launch boundary
// the Schur fronts of items 0 .. B-1 behind their interiors (batch_factor_enqueue in level mode comes first)
std::string schur_batch_assemble_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_vals, int64_t val_stride);
// d_out (ns x ns, leading dimension ns, both triangles) = ((P_0 + P_1) + ... + P_{G-1}) (+ S_add), P_g the sequential sum from 0.0 over
// the items of group g; d_add: full symmetric, leading dimension ld (its lower triangle is read), or NULL
std::string schur_batch_sum_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_add, int64_t ld, double* d_out);
// item b's S_b, full and symmetric, leading dimension ld
std::string schur_batch_export_enqueue(Numeric& N, SchurBatchWork& W, int64_t b, double* d_S, int64_t ld);
// the items' r2 (behind the forward sweep) into W.r2i, and into d_items [B][nrhs][ns] at columns r0 .. r0 + nr if given
std::string schur_batch_gather_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, double* d_items, int64_t nrhs, int64_t r0, int nr, int R);
// d_out[q][ns] (q < nr) = the sum of W.r2i by the grouping rule (+ d_add[q][ns])
std::string schur_batch_r2sum_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_add, double* d_out, int nr, int R);
// x2 [nr][ns] into the Schur columns of every item's xwork (zeros for the padding columns)
std::string schur_batch_put_enqueue(Numeric& N, SchurBatchWork& W, int64_t B, const double* d_x2, int nr, int R);

}  // namespace okkt
