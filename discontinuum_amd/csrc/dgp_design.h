// dgp_design.h -- what the two gain-map passes share: dgp_design.hip (dense covariance) and dgp_design_stream.hip (covariance
// produced panel by panel).  The tile shape, the lane read and the prep rule for v'_c are used by both; the register-resident
// power sums and the series fold are the streamed pass's copy of the two loops sv_sums_kernel keeps in its own text -- called from
// here they changed that kernel's register allocation, and its generated code stays what it was.
#pragma once
#include "dgp_common.h"

namespace dgp {

constexpr int SV_CAND = 64;           // candidates of a workgroup's wave: a lane each
constexpr int SV_DAYS = 16;           // days of a tile
constexpr int SV_LD = SV_CAND + 1;    // leading dimension of the staged tile [SV_DAYS][SV_LD]

__device__ __forceinline__ double sv_readlane(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// r (0 on entry) = 1 / sqrt(v'_c); left 0 where v'_c is not > 0 (v is then set to 0), NaN where it is NaN (NaN in, NaN out)
__device__ __forceinline__ void sv_inv_sd(double& v, double& r) {
  if (v > 0.0)
    r = 1.0 / sqrt(v);
  else if (v != v)
    r = v;
  else
    v = 0.0;
}

// S[k] += pw b^(k+1) for k < K (rounded up to a multiple of four: sums past K within the last four are computed and never used)
template <int KT>
__device__ __forceinline__ void sv_add_day(double (&S)[KT], int K, double pw, double b) {
#pragma unroll
  for (int k4 = 0; k4 < KT; k4 += 4) {
    if (k4 < K) {  // wave-uniform
#pragma unroll
      for (int k = k4; k < k4 + 4; ++k) {
        pw *= b;
        S[k] += pw;
      }
    }
  }
}

// sum_{k < K} (s2)^(k+1) / (k+1)! S[k]^2
template <int KT>
__device__ __forceinline__ double sv_series(const double (&S)[KT], int K, double s2) {
  double coef = 1.0, gain = 0.0;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {
      coef *= s2 / (double)(k + 1);
      gain += coef * (S[k] * S[k]);
    }
  }
  return gain;
}

}  // namespace dgp
