// dgp_orthant.hip -- orthant probabilities P(lo <= f <= hi), f ~ N(0, L L^T), by Genz's separation of variables over a randomly
// shifted Richtmyer rule with the periodising tent transform (dgp_orthant_probability): the distribution function of a period's
// maximum (minimum) of the latent posterior.  The estimator, fixed so that a numpy restatement walks the same points:
//     w_{n,s,i} = |2 frac(n g_i + D_{s,i}) - 1|,  n = 1 .. N  (product and sum rounded once each: no contraction)
//   per (s, n), i = 0 .. m-1 in order:
//     c = sum_{j<i} L_ij y_j,  a = (lo_i - c) / L_ii,  b = (hi_i - c) / L_ii
//     a + b > 0 (the interval's centre lies in the upper half: the upper tail is the nearer one):
//              A = Phi(-b), B = Phi(-a), d = max(B - A, 0), t = min(A + (1 - w) d, 1), y_i = -clamp(Phi^-1(t), -38, 38)
//     otherwise  A = Phi(a),  B = Phi(b),  d = max(B - A, 0), t = min(A + w d, 1),       y_i =  clamp(Phi^-1(t), -38, 38)
//     p *= d
//   estimate of shift s = mean_n p;  prob = mean_s;  se = sample standard deviation over the shifts / sqrt(S).
// Phi(x) = erfc(-x / sqrt 2) / 2 and Phi^-1(t) = -Phi^-1(1 - t) for t > 1/2 (1 - t is exact there), so neither d nor t nor the
// library ever holds 1 - tiny; d < 0 (lo > hi) counts as 0; a point whose d
// underflows keeps p = 0 and a finite y (the clamp), so nothing non-finite reaches a sum; (-inf, +inf) gives d = 1 exactly
// and still draws y = Phi^-1(w).
//
// Schedule.  Points do not interact: ONE workgroup owns OR_PC = 128 points of one (level, shift) and walks the dimensions in
// blocks of OR_DB = 64 by itself; grid = (point chunks, shifts, levels), no synchronisation between workgroups.  Per block k:
//   1. offsets  c[i][pt] = sum_{j < 64 k} L[64 k + i][j] Y[j][pt]  on the plain MFMA tile core (TileGemm 64 x 128, A = rows of L,
//      B = the workgroup's own Y slice read transposed); the k-range stops before the diagonal block.  The accumulators land in
//      the 64 x 128 LDS stage (which is also the core's operand image: the product is finished before the stage is written);
//   2. the 64 sequential steps on the vector pipe, one point per lane (waves 0 and 1): slot [i][pt] of the stage holds c and
//      is overwritten by y_i; the row of L_kk reaches the lanes through uniform loads;
//   3. the stage goes to rows [64 k, 64 k + 64) of the workgroup's Y slice ([dimension][128 points]) for the later products.
// The workgroup reads back global memory that it wrote itself: step 3 ends with a device-scope fence and a barrier before the
// next block's operand loads (plain global loads into registers -- the direct-to-LDS core is not used here).
// The factor is read as psd_safe_factor leaves it: inside the lower triangle of the diagonal 128-blocks and in the blocks below
// the block diagonal only; the sweep stops at m.  Per-workgroup partial sums (fixed tree), then one reduce launch: no
// floating-point atomics, repeated calls are bitwise equal.
#include "../../include/dgp_hip.h"
#include "dgp_gemm.h"
#include "dgp_plan.h"
#include "dgp_qmc.h"  // or_weight, OR_YMAX, the size limits

namespace dgp {

namespace {

constexpr int OR_DB = 64;    // dimensions per block (divides the factor's 128-blocks)
constexpr int OR_PC = 128;   // points per workgroup

using OrG = TileGemm<double, true, false, OR_DB, OR_PC>;
static_assert(OrG::SMEM_ELEMS <= OR_DB * OR_PC, "the tile core's operand image must fit the stage it shares");

__device__ __forceinline__ double or_phi(double x) { return 0.5 * erfc(-0.70710678118654752440 * x); }

// One step of the recurrence from the standardised limits a <= b and the weight w: -> d, and y by reference.  No contraction
// either: every operation is rounded as the restatement rounds it.  Kept out of line: inlined into the sweep's loops the
// polynomial constants of erfc and Phi^-1 are hoisted into registers, a few hundred of them, and the kernel spills at one wave
// per SIMD.
__device__ __noinline__ double or_step(double a, double b, double w, double& y) {
#pragma clang fp contract(off)
  const bool flip = a + b > 0.0;
  const double A = or_phi(flip ? -b : a), B = or_phi(flip ? -a : b);
  const double d = fmax(B - A, 0.0);
  if (flip) w = 1.0 - w;
  const double wd = w * d;
  const double tt = fmin(A + wd, 1.0);
  // Phi^-1 through the lower half only: 1 - t is exact for t >= 1/2, so no 1 - tiny reaches the library's normcdfinv
  const bool upper = tt > 0.5;
  const double z = fmin(fmax(normcdfinv(upper ? 1.0 - tt : tt), -OR_YMAX), OR_YMAX);
  y = flip != upper ? -z : z;
  return d;
}

// work area: Y slices [wg][M64][OR_PC] doubles, then partial[level][shift][chunk]
__global__ __launch_bounds__(256, 2) void orthant_sweep_kernel(const double* __restrict__ L, long ld, int m, const double* __restrict__ lo,
                                                           const double* __restrict__ hi, const double* __restrict__ gen,
                                                           const double* __restrict__ shift, int npoints, double* Yall,
                                                           double* __restrict__ partial) {
  __shared__ double stage[OR_DB * OR_PC];
  const int t = threadIdx.x;
  const int chunk = blockIdx.x, s = blockIdx.y, lev = blockIdx.z;
  const long wg = ((long)lev * gridDim.y + s) * gridDim.x + chunk;
  const long M64 = ((long)m + OR_DB - 1) / OR_DB * OR_DB;
  double* Y = Yall + wg * M64 * OR_PC;
  const double* lo_l = lo + (long)lev * m;
  const double* hi_l = hi + (long)lev * m;
  const double* sh = shift + (long)s * m;
  const long n0 = (long)chunk * OR_PC + t;  // this lane's point (t < OR_PC), n = n0 + 1
  const double nn = (double)(n0 + 1);
  double p = 1.0;

  for (int k0 = 0; k0 < m; k0 += OR_DB) {
    // 1. conditional offsets of the block's rows
    if (k0 == 0) {
      for (int e = t; e < OR_DB * OR_PC; e += 256) stage[e] = 0.0;
    } else {
      typename OrG::acc_t acc[OrG::MI][OrG::NI];
      OrG::zero(acc);
      OrG::run(L + (long)k0 * ld, ld, Y, (long)OR_PC, k0 / 16, stage, acc);
      __syncthreads();  // every wave is done with the operand image
      OrG::foreach (acc, [&](int r, int c, double& v) { stage[r * OR_PC + c] = v; });
    }
    __syncthreads();
    // 2. the sequential steps of the diagonal block, one point per lane
    const int rows = min(OR_DB, m - k0);
    if (t < OR_PC) {
#pragma unroll 1
      for (int i = 0; i < rows; ++i) {
        const double* Lrow = L + (long)(k0 + i) * ld + k0;
        double c = stage[i * OR_PC + t];
#pragma unroll 4
        for (int j = 0; j < i; ++j) c = fma(Lrow[j], stage[j * OR_PC + t], c);
        const double lii = Lrow[i];
        const double a = (lo_l[k0 + i] - c) / lii, b = (hi_l[k0 + i] - c) / lii;
        const double w = or_weight(nn, gen[k0 + i], sh[k0 + i]);
        double y;
        p *= or_step(a, b, w, y);
        stage[i * OR_PC + t] = y;
      }
    }
    __syncthreads();
    // 3. the block's y to the workgroup's slice, visible to its own later operand loads
    if (k0 + OR_DB < m) {
      double* Yk = Y + (long)k0 * OR_PC;
      for (int e = t; e < OR_DB * OR_PC; e += 256) Yk[e] = stage[e];
      __threadfence();
    }
    __syncthreads();
  }

  // partial sum of the chunk's points in a fixed tree
  if (t < OR_PC) stage[t] = n0 < npoints ? p : 0.0;
  __syncthreads();
  for (int h = OR_PC / 2; h > 0; h >>= 1) {
    if (t < h) stage[t] += stage[t + h];
    __syncthreads();
  }
  if (t == 0) partial[wg] = stage[0];
}

// one thread per level: the shifts' estimates (chunks ascending), their mean and its standard error
__global__ void orthant_reduce_kernel(const double* __restrict__ partial, int nchunks, int nshifts, int nlevels, int npoints,
                                      double* __restrict__ prob, double* __restrict__ se) {
  const int lev = blockIdx.x * blockDim.x + threadIdx.x;
  if (lev >= nlevels) return;
  const double* pl = partial + (long)lev * nshifts * nchunks;
  double mean = 0.0;
  for (int s = 0; s < nshifts; ++s) {
    double e = 0.0;
    for (int c = 0; c < nchunks; ++c) e += pl[(long)s * nchunks + c];
    mean += e / (double)npoints;
  }
  mean /= (double)nshifts;
  double ss = 0.0;
  for (int s = 0; s < nshifts; ++s) {
    double e = 0.0;
    for (int c = 0; c < nchunks; ++c) e += pl[(long)s * nchunks + c];
    const double dv = e / (double)npoints - mean;
    ss += dv * dv;
  }
  prob[lev] = mean;
  se[lev] = sqrt(ss / (double)(nshifts - 1)) / sqrt((double)nshifts);
}

}  // namespace

}  // namespace dgp

using namespace dgp;

extern "C" {

size_t dgp_orthant_probability_workspace_bytes(int64_t m, int nlevels, int nshifts, int64_t npoints) {
  if (!or_sizes_ok(m, nlevels, nshifts, npoints)) return 0;
  const size_t chunks = (size_t)((npoints + OR_PC - 1) / OR_PC), wgs = chunks * (size_t)nshifts * (size_t)nlevels;
  const size_t M64 = (size_t)round_up(m, OR_DB);
  return wgs * (M64 * OR_PC + 1) * sizeof(double);
}

int dgp_orthant_probability(const double* L, int64_t m, int64_t ld, const double* lo, const double* hi, int nlevels, const double* gen,
                            const double* shift, int nshifts, int64_t npoints, void* work, size_t work_bytes, double* prob, double* se,
                            void* stream) {
  if (!L || !lo || !hi || !gen || !shift || !prob || !se) return fail(DGP_E_ARG, "dgp_orthant_probability: null argument");
  if (!or_sizes_ok(m, nlevels, nshifts, npoints))
    return fail(DGP_E_ARG, "dgp_orthant_probability: bad size (1 <= m <= 16384, 1 <= nlevels <= 64, 2 <= nshifts <= 64, "
                           "1 <= npoints <= 2^20)");
  if (ld < round_up(m, DGP_TILE_HOST) || (ld & 1) != 0 || ((uintptr_t)L & 15) != 0)
    return fail(DGP_E_ARG, "dgp_orthant_probability: ld must be even and at least the padded m, the factor 16-byte aligned");
  if (!work || work_bytes < dgp_orthant_probability_workspace_bytes(m, nlevels, nshifts, npoints))
    return fail(DGP_E_WORKSPACE, "dgp_orthant_probability: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_orthant_probability: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (int)((npoints + OR_PC - 1) / OR_PC);
  const size_t wgs = (size_t)chunks * (size_t)nshifts * (size_t)nlevels;
  double* Y = (double*)work;
  double* partial = Y + wgs * (size_t)round_up(m, OR_DB) * OR_PC;
  orthant_sweep_kernel<<<dim3((unsigned)chunks, (unsigned)nshifts, (unsigned)nlevels), 256, 0, s>>>(L, (long)ld, (int)m, lo, hi, gen, shift,
                                                                                                (int)npoints, Y, partial);
  int rc = (int)hipGetLastError();
  if (rc == 0) {
    orthant_reduce_kernel<<<1, 64, 0, s>>>(partial, chunks, nshifts, nlevels, (int)npoints, prob, se);
    rc = (int)hipGetLastError();
  }
  return wrap(rc, "dgp_orthant_probability");
}

}  // extern "C"
