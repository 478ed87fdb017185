// The attempts of ipopt_strategy! (delta_strategy.jl:37-114) as a sequence known before any of them is factored.  All three delta loops
// step it: the serial one and the one that factors `width` attempts at a time (kkt.hip), and the one over the
// items of a KKT batch (kkt_batch.hip, section 8.17) -- so their doubles are the same because the code is.  Host code only, no device
// and no handle: the sanitizer driver runs it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/okkt.h"

namespace okkt {

// the reference's defaults: what okkt_kkt_default_pars hands out
inline okkt_kkt_pars default_kkt_pars() {
  okkt_kkt_pars P;
  P.delta_start = 1e-6;                 // parameters.jl:147-158
  P.delta_min = 1e-12;
  P.delta_max = 1e50;
  P.delta_inc = 8.0;
  P.delta_dec = 1.0 / M_PI;
  P.delta_zero = 0.0;
  P.ItRefine_Num = 3;                   // parameters.jl:20
  P.max_it = 500;                       // delta_strategy.jl:40
  return P;
}

struct DeltaSeq {
  double tau = 0.0, delta = 0.0, delta_prev = 0.0;
  bool zero_first = false;
  int it = 0;
  // tau from diag_min: a positive tau means the first attempt is delta_zero, outside the loop, and tau = 0 afterwards
  void start(double diag_min, double delta_prev_, const okkt_kkt_pars& P) {
    tau = 1.5 * diag_min;
    delta = P.delta_zero;
    delta_prev = delta_prev_;
    zero_first = tau > 0.0;
    if (zero_first) tau = 0.0;
    it = 0;
  }
  // the next attempt: its delta, and whether it is one of the loop (the delta_max exit applies to those only); false: max_it is used up
  bool next(const okkt_kkt_pars& P, double* d, bool* in_loop) {
    if (zero_first) { zero_first = false; *d = P.delta_zero; *in_loop = false; return true; }
    if (it >= P.max_it) return false;
    ++it;
    if (it == 1) delta = delta_prev != 0.0 ? std::max(P.delta_min - tau, delta_prev * P.delta_dec) : P.delta_start - tau;
    else delta = delta * P.delta_inc;
    *d = delta;
    *in_loop = true;
    return true;
  }
};

// One round of the loop over items, as bookkeeping: every active item has made the attempt cand[b] (in_loop[b]) and flag[b] says whether
// its inertia was right.  Counts the attempt, records delta, closes the items that end (first success: status 1; first attempt of the
// loop beyond delta_max: status 0) and lists the failed ones (they are scanned for diagonal dominance whether they go on or not).
struct ItemsLoop {
  std::vector<int32_t> active, failed;
  void start(int64_t B) {
    active.resize((size_t)B);
    for (int64_t b = 0; b < B; ++b) active[(size_t)b] = (int32_t)b;
    failed.clear();
  }
  void close_round(const double* cand, const char* in_loop, const int32_t* flag, double delta_max, int32_t* status, int32_t* num_fac, double* delta_out) {
    std::vector<int32_t> next;
    failed.clear();
    for (const int32_t b : active) {
      ++num_fac[b];
      delta_out[b] = cand[b];
      if (flag[b] == 1) { status[b] = 1; continue; }
      failed.push_back(b);
      if (in_loop[b] && cand[b] > delta_max) { status[b] = 0; continue; }      // :failure: the complete factor of this delta stays in the slot
      next.push_back(b);
    }
    active.swap(next);
  }
};

}  // namespace okkt
