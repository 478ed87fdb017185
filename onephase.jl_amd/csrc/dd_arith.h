// Double-double building blocks of the extra-precise device sums (refine.hip, factor_ops.hip).  A file that includes this is compiled
// with -ffp-contract=off (Makefile): a contracted or reassociated TwoSum is no longer exact.
#pragma once
#include <hip/hip_runtime.h>

namespace okkt {

// Knuth's TwoSum: s + e == a + b exactly, for any order of magnitude of a and b
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
// (h, l) += (p, q) in double-double
__device__ __forceinline__ void dd_add(double& h, double& l, double p, double q) {
  double s, e;
  two_sum(h, p, s, e);
  e = e + (l + q);
  h = s + e;
  l = e - (h - s);
}

}  // namespace okkt
