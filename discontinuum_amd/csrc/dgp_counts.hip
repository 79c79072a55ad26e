// dgp_counts.hip -- exceedance-count and longest-spell histograms of joint paths f ~ N(0, L L^T) over the randomly shifted
// Richtmyer rules of the orthant sweep (dgp_path_counts): how many of a period's points lie beyond a threshold, and the longest
// run of consecutive such points.  Neither has a closed form or a separation of variables: paths are drawn, compared, counted.
// The estimator, fixed so that a numpy restatement walks the same points (tests/count_helpers.py):
//     w_{n,s,i} = |2 frac(n g_i + D_{s,i}) - 1|,  n = 1 .. N           (or_weight: product and sum rounded once each)
//     y_i = clamp(Phi^-1(w), -38, 38)                                  (through the lower half: w > 1/2 -> -Phi^-1(1 - w))
//     f_i = sum_{j <= i} L_ij y_j
//     e_i = above ? f_i > c_{l,i} : f_i < c_{l,i}                      (a NaN threshold never counts)
//     N_l = sum_i e_i,   R_l = the longest run of consecutive e_i = 1, a run being broken at i when link[i] == 0
//     count_hist[l][s][N_l] += 1,  spell_hist[l][s][R_l] += 1          (int32; everything after that is the host's)
// Nothing is truncated, so the draws of a point do not depend on each other: the paths of a block of rows are one triangular
// product, and one sweep serves every level, because the path does not depend on the level.
//
// Schedule.  ONE workgroup owns CT_PC = 128 points of one shift and a chunk of at most CT_LC = 16 levels; grid = (point chunks,
// shifts, level chunks), no synchronisation between workgroups.
//   0. its slice Y[round_up(m, 128)][128] of the draws goes to the work area once (m x 128 evaluations of Phi^-1; rows >= m zero),
//      followed by a device-scope fence and a barrier: the workgroup reads back what it wrote itself;
//   1. per block of CT_DB = 128 rows: f = L[k0 .. k0 + 128, 0 .. k0 + 128) Y on the plain MFMA tile core (TileGemm 128 x 128, A =
//      rows of L, B = the slice read transposed).  The k-range runs THROUGH the block's own columns: the zeros above the diagonal
//      inside a diagonal 128-block make that exact, and the 64 sequential vector steps of the orthant sweep disappear;
//   2. the accumulators pass through the 64 x 128 LDS stage (also the core's operand image: the product is finished first) in
//      two halves of 64 rows -- waves 0, 1 hold the first, waves 2, 3 the second --, and one lane per (point, half of the level
//      chunk) walks each half's rows in order: (N, current run, best run) of 8 levels in registers;
//   3. after the last block every lane adds 1 into its levels' two histograms: integer atomics, whose result has no order.
// Why 128 rows and not the orthant sweep's 64: the sweep is bound by the operand traffic from L2, not by the MFMA pipe -- per
// block of rows a workgroup reads the rows of L and ALL of its slice up to the diagonal, so the slice is re-read m / rows
// times; 128 rows halve that (measured at m = 8760, 16 x 4096 points: see EXPERIMENTS.md) while the stage stays at 64 KiB and
// two workgroups fit a CU.
// The factor is read as psd_safe_factor leaves it: inside the lower triangle of the diagonal 128-blocks and in the blocks below
// the block diagonal only.  The tile core loads whole 128-row blocks, so rows [m, round_up(m, 128)) of the padded buffer are
// loaded with the last block and their products discarded: no value in a row >= m reaches a result.  No floating-point atomics;
// repeated calls give identical integers; a level's histograms depend neither on the other levels nor on their chunking.
#include "../../include/dgp_hip.h"
#include "../../include/dgp_hip_ext2.h"
#include "dgp_gemm.h"
#include "dgp_plan.h"
#include "dgp_qmc.h"

namespace dgp {

namespace {

constexpr int CT_DB = 128;  // rows per block: the factor's own 128-blocks
constexpr int CT_SR = 64;   // rows of the LDS stage: a block's accumulators pass through it in two halves
constexpr int CT_PC = 128;  // points per workgroup
constexpr int CT_LC = 16;   // levels per workgroup: two halves of CT_LH, one per half of the workgroup
constexpr int CT_LH = CT_LC / 2;

using CtG = TileGemm<double, true, false, CT_DB, CT_PC>;
static_assert(CtG::SMEM_ELEMS <= CT_SR * CT_PC, "the tile core's operand image must fit the stage it shares");
static_assert(CT_DB == 2 * CT_SR, "waves 0, 1 hold the accumulators of the block's first half of rows, waves 2, 3 of the second");

// y = clamp(Phi^-1(w), -38, 38) through the lower half only: 1 - w is exact for w >= 1/2, w = 0 gives -38
// Kept out of line: inlined, the polynomial constants of Phi^-1 are hoisted into registers and the kernel spills.
__device__ __noinline__ double ct_draw(double w) {
  const bool upper = w > 0.5;
  const double z = fmin(fmax(normcdfinv(upper ? 1.0 - w : w), -OR_YMAX), OR_YMAX);
  return upper ? -z : z;
}

// work area: Y slices [wg][round_up(m, CT_DB)][CT_PC] doubles
__global__ __launch_bounds__(256, 2) void path_counts_kernel(const double* __restrict__ L, long ld, int m, const double* __restrict__ thr,
                                                         int nlevels, int above, const int* __restrict__ link,
                                                         const double* __restrict__ gen, const double* __restrict__ shift,
                                                         int npoints, double* Yall, int* count_hist, int* spell_hist) {
  __shared__ double stage[CT_SR * CT_PC];
  const int t = threadIdx.x, pt = t & (CT_PC - 1);
  const int half = __builtin_amdgcn_readfirstlane(t >> 7);  // wave-uniform: waves 0, 1 -> 0; waves 2, 3 -> 1
  const int chunk = blockIdx.x, s = blockIdx.y, lc = blockIdx.z;
  const int nshifts = gridDim.y;
  const long wg = ((long)lc * nshifts + s) * gridDim.x + chunk;
  const long MB = ((long)m + CT_DB - 1) / CT_DB * CT_DB;
  double* Y = Yall + wg * MB * CT_PC;
  const double* sh = shift + (long)s * m;
  const long n0 = (long)chunk * CT_PC + pt;  // this lane's point, n = n0 + 1
  const int lev0 = lc * CT_LC + half * CT_LH;
  const int nl = min(CT_LH, nlevels - lev0);  // <= 0: this half has no level

  // 0. the draws of the workgroup's points, [dimension][point]
  {
    const double nn = (double)(n0 + 1);
    for (long i = t >> 7; i < MB; i += 2)
      Y[i * CT_PC + pt] = i < m ? ct_draw(or_weight(nn, gen[i], sh[i])) : 0.0;
    __threadfence();
  }
  __syncthreads();

  int cnt[CT_LH], cur[CT_LH], best[CT_LH];
#pragma unroll
  for (int l = 0; l < CT_LH; ++l) cnt[l] = cur[l] = best[l] = 0;

  for (int k0 = 0; k0 < m; k0 += CT_DB) {
    // 1. the block's rows of the paths
    typename CtG::acc_t acc[CtG::MI][CtG::NI];
    CtG::zero(acc);
    CtG::run(L + (long)k0 * ld, ld, Y, (long)CT_PC, (k0 + CT_DB) / 16, stage, acc);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r0 = k0 + h * CT_SR, rows = min(CT_SR, m - r0);
      if (rows <= 0) break;  // (uniform)
      __syncthreads();  // every wave is done with the operand image, or with the first half of the rows
      CtG::foreach (acc, [&](int r, int c, double& v) {
        if ((r >> 6) == h) stage[(r & (CT_SR - 1)) * CT_PC + c] = v;
      });
      __syncthreads();
      // 2. compare and count, one lane per (point, half of the levels)
      if (nl > 0) {
#pragma unroll 1
        for (int i = 0; i < rows; ++i) {
          const double f = stage[i * CT_PC + pt];
          const bool linked = link == nullptr || link[r0 + i] != 0;
          const double* ci = thr + (long)lev0 * m + (r0 + i);
#pragma unroll
          for (int l = 0; l < CT_LH; ++l)
            if (l < nl) {
              const double c = ci[(long)l * m];
              const bool e = above ? f > c : f < c;
              cur[l] = e ? (linked ? cur[l] + 1 : 1) : 0;
              cnt[l] += e ? 1 : 0;
              best[l] = max(best[l], cur[l]);
            }
        }
      }
    }
    __syncthreads();  // the stage becomes the operand image again
  }

  // 3. one count per (level, point) into each histogram
  if (n0 < npoints) {
#pragma unroll
    for (int l = 0; l < CT_LH; ++l)
      if (l < nl) {
        const long base = ((long)(lev0 + l) * nshifts + s) * ((long)m + 1);
        atomicAdd(count_hist + base + cnt[l], 1);
        atomicAdd(spell_hist + base + best[l], 1);
      }
  }
}

}  // namespace

}  // namespace dgp

using namespace dgp;

extern "C" {

size_t dgp_path_counts_workspace_bytes(int64_t m, int nlevels, int nshifts, int64_t npoints) {
  if (!or_sizes_ok(m, nlevels, nshifts, npoints)) return 0;
  const size_t chunks = (size_t)((npoints + CT_PC - 1) / CT_PC), lchunks = (size_t)((nlevels + CT_LC - 1) / CT_LC);
  return chunks * (size_t)nshifts * lchunks * (size_t)round_up(m, CT_DB) * CT_PC * sizeof(double);
}

int dgp_path_counts(const double* L, int64_t m, int64_t ld, const double* thr, int nlevels, int above, const int32_t* link,
                    const double* gen, const double* shift, int nshifts, int64_t npoints, void* work, size_t work_bytes,
                    int32_t* count_hist, int32_t* spell_hist, void* stream) {
  if (!L || !thr || !gen || !shift || !count_hist || !spell_hist) return fail(DGP_E_ARG, "dgp_path_counts: null argument");
  if (!or_sizes_ok(m, nlevels, nshifts, npoints))
    return fail(DGP_E_ARG, "dgp_path_counts: bad size (1 <= m <= 16384, 1 <= nlevels <= 64, 2 <= nshifts <= 64, "
                           "1 <= npoints <= 2^20)");
  if (ld < round_up(m, DGP_TILE_HOST) || (ld & 1) != 0 || ((uintptr_t)L & 15) != 0)
    return fail(DGP_E_ARG, "dgp_path_counts: ld must be even and at least the padded m, the factor 16-byte aligned");
  if (!work || work_bytes < dgp_path_counts_workspace_bytes(m, nlevels, nshifts, npoints))
    return fail(DGP_E_WORKSPACE, "dgp_path_counts: workspace missing or too small");
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_path_counts: the work area must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t hist_bytes = (size_t)nlevels * (size_t)nshifts * (size_t)(m + 1) * sizeof(int32_t);
  int rc = (int)hipMemsetAsync(count_hist, 0, hist_bytes, s);
  if (rc == 0) rc = (int)hipMemsetAsync(spell_hist, 0, hist_bytes, s);
  if (rc == 0) {
    const unsigned chunks = (unsigned)((npoints + CT_PC - 1) / CT_PC), lchunks = (unsigned)((nlevels + CT_LC - 1) / CT_LC);
    path_counts_kernel<<<dim3(chunks, (unsigned)nshifts, lchunks), 256, 0, s>>>(L, (long)ld, (int)m, thr, nlevels, above != 0 ? 1 : 0, link,
                                                                               gen, shift, (int)npoints, (double*)work, count_hist,
                                                                               spell_hist);
    rc = (int)hipGetLastError();
  }
  return wrap(rc, "dgp_path_counts");
}

}  // extern "C"
