// dgp_qmc.h -- what the two sweeps over randomly shifted Richtmyer rules share (dgp_orthant.hip, dgp_counts.hip): the weight of a
// point, the clamp of a draw and the size limits of a call.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace dgp {

constexpr long OR_MAX_M = 16384;
constexpr long OR_MAX_POINTS = 1L << 20;
constexpr double OR_YMAX = 38.0;  // |y| clamp: Phi(-38) = 3e-316

// The weight of point n in dimension i: |2 frac(n g + D) - 1| with the product and the sum rounded once each, as numpy rounds
// them.  The pragma, not the _rn intrinsics: those are plain operators here and contract to one fma like any others, which
// moved x by an ulp -- 6e-12 of a weight near 0 -- and an estimate by 2e-10 relative.
__device__ __forceinline__ double or_weight(double n, double g, double shift) {
#pragma clang fp contract(off)
  double x = n * g;
  x = x + shift;
  x = x - floor(x);
  return fabs(2.0 * x - 1.0);
}

inline bool or_sizes_ok(int64_t m, int nlevels, int nshifts, int64_t npoints) {
  return m >= 1 && m <= OR_MAX_M && nlevels >= 1 && nlevels <= 64 && nshifts >= 2 && nshifts <= 64 && npoints >= 1 &&
         npoints <= OR_MAX_POINTS;
}

}  // namespace dgp
