// dgp_aggregate.hip -- exact moments of period sums of a transformed Gaussian posterior (dgp_period_moments).
//
// f ~ N(mu, C) over m points (C: the matrix dgp_posterior_cov leaves; only its lower triangle is read), a
// data-space value c_i = exp(s f_i + t) (mode 1) or s f_i + t (mode 0), weights w_i, and group ids g_i (non-decreasing,
// -1 = excluded).  With mu_i already mapped (mu_i <- s mu_i + t) and s2 = s^2:
//     mode 1:  a_i = w_i exp(mu_i + s2 C_ii / 2),  mean_g = sum_{i in g} a_i,
//              cov_gh = sum_{i in g} sum_{j in h} a_i a_j expm1(s2 C_ij)
//     mode 0:  a_i = w_i,                         mean_g = sum_{i in g} w_i mu_i,
//              cov_gh = sum_{i in g} sum_{j in h} a_i a_j s2 C_ij
// (C_ii + extra_var_i on the diagonal).  Four launches (a tiny init, then three passes), gridDim.z = sites, no floating-point
// atomics:
//   prep    one thread per point: a_i, the mean term, and each group's column range [start, end) (integer atomics)
//   rows    one workgroup per (128-row block, group): Y[i][g] = sum_{j in g} a_j phi(C_ij).  Columns j <= i are read as
//           C[i][j] (row-contiguous: a wave per row, lanes along j); columns j > i as C[j][i], a row segment of a lower
//           tile (lanes along i).  Every C element (i, j), i != j, is read twice in all.
//   reduce  one workgroup per (64 columns h, group g): cov_gh = sum_{i in g} a_i Y[i][h] for h >= g, written to both
//           (g, h) and (h, g) -- the output is exactly symmetric; mean_g beside it.
// Every sum runs in a fixed order, so results are bitwise repeatable and a site's numbers do not depend on its batch.
//
// dgp_posterior_period_moments: the same moments with C = K(Xs, Xs) - V^T V (V = L^-1 K(X, Xs), left in the work area by the
// prediction's first stages) folded in tile by tile and never stored.  The rows pass is replaced by ppm_rows_kernel:
//   one workgroup per (128-row block I, group h) -- a block whose rows all lie in groups above h (excluded rows included)
//   writes zeros to Y[., h] and leaves: the reduce pass only needs Y[i][h] for h >= g(i), and reads the rest times a_i = 0 --
//   looping over h's 64-column tiles J in ascending order:
//     acc = V_I^T V_J   (the tile-GEMM core of posterior_cov_kernel, TileGemm, on 128 x 64 tiles: 64 accumulator registers
//                        per lane, so that the per-entry epilogue below fits beside them at two workgroups per CU without
//                        spilling -- on 128 x 128 tiles the 128 accumulators left too little room in fp64)
//     per 16 x 16 sub-tile of acc: C_ij = k(x_i, x_j) - acc_ij (+ extra_var_i on the diagonal), a_j phi(C_ij) for the
//     columns j of group h (a select: anything else -- pad, excluded, other groups -- adds an exact zero), summed over
//     the sub-tile's columns by a fixed butterfly, then over the two wave columns and the tiles J in order.
//   k(x_i, x_j) is gram_sym_kernel's evaluation (per-point features in LDS, the model's pair<false>); the row strip stays
//   in LDS for the whole loop, the column strip of each J goes into the operand tiles the k-loop has just finished with.
// Visits about m^2 / 2 (1 + 1/P) entries, 2 N flop each on the MFMA pipe; no floating-point atomics.
#include <climits>

#include "dgp_common.h"
#include "dgp_gemm_dma.h"
#include "dgp_gram_shared.h"
#include "dgp_stream.h"
#include "dgp_models.h"

namespace dgp {

namespace {

constexpr int PM_ROWS = 128;  // rows of a workgroup of the rows pass (== DGP_TILE_HOST, the cov buffer's block size)
constexpr int PM_COLS = 64;   // columns of a tile of the streamed rows pass (ppm_rows_kernel)

// per-site work area, in doubles: a[M], mean term[M], Y[M x P], then 2 P ints (group start / end)
__host__ __device__ inline long pm_site_doubles(long M, int P) { return 2 * M + M * (long)P + P; }

template <int MODE>
__device__ __forceinline__ double pm_phi(double s2, double x) {
  if constexpr (MODE == 1)
    return expm1(s2 * x);
  else
    return s2 * x;
}

__device__ __forceinline__ double pm_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ void pm_range(const int* se, int g, int& c0, int& c1) {
  c0 = se[2 * g];
  c1 = se[2 * g + 1];
  if (c1 <= c0) c0 = c1 = 0;  // empty group (start still INT_MAX)
}

__global__ __launch_bounds__(256) void pm_init_kernel(double* work, long ws, long M, int P) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  int* se = (int*)(work + (long)blockIdx.z * ws + 2 * M + M * (long)P);
  se[2 * g] = INT_MAX;
  se[2 * g + 1] = 0;
}

// C_jj of site z sits at diag[z dsite + j dstep]: the diagonal of the dense covariance (dsite = M M, dstep = M + 1), or the
// predicted variance the streamed pass finds in its work area (dsite = that area's site stride, dstep = 1)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void pm_prep_kernel(const T* __restrict__ diag, long dsite, long dstep, long M, int m, int P,
                                                      const T* __restrict__ mu, const double* __restrict__ scale2,
                                                      const double* __restrict__ w, const int* __restrict__ group,
                                                      const T* __restrict__ ev, double* work, long ws) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  double* a = work + (long)z * ws;
  double* am = a + M;
  int* se = (int*)(a + 2 * M + M * (long)P);
  double av = 0.0, amv = 0.0;
  if (j < m) {
    const long k = (long)z * m + j;
    const int g = group[k];
    if (g >= 0 && g < P) {
      const double wj = w[k], muj = (double)mu[k];
      if constexpr (MODE == 1) {
        double cjj = (double)diag[(long)z * dsite + j * dstep];
        if (ev) cjj += (double)ev[k];
        av = wj * exp(muj + 0.5 * scale2[z] * cjj);
        amv = av;
      } else {
        av = wj;
        amv = wj * muj;
      }
      atomicMin(&se[2 * g], (int)j);
      atomicMax(&se[2 * g + 1], (int)j + 1);
    }
  }
  a[j] = av;
  am[j] = amv;
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void pm_rows_kernel(const T* __restrict__ cov, long M, int m, int P,
                                                      const double* __restrict__ scale2, const T* __restrict__ ev,
                                                      double* __restrict__ work, long ws) {
  const int rb = blockIdx.x, g = blockIdx.y, z = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* C = cov + (long)z * M * M;
  double* base = work + (long)z * ws;
  const double* a = base;
  double* Y = base + 2 * M;
  int c0, c1;
  pm_range((const int*)(base + 2 * M + M * (long)P), g, c0, c1);
  const double s2 = scale2[z];
  const T* evz = ev ? ev + (long)z * m : nullptr;
  const int r0 = rb * PM_ROWS;
  __shared__ double low[PM_ROWS], up[2][PM_ROWS];

  // j <= i: a wave per row, lanes along the row
  for (int ii = wave; ii < PM_ROWS; ii += 4) {
    const int i = r0 + ii;
    double acc = 0.0;
    if (i < m) {
      const T* row = C + (long)i * M;
      const double evi = evz ? (double)evz[i] : 0.0;
      const int split = min(c1, i + 1);
      for (int j = c0 + lane; j < split; j += 64) {
        double x = (double)row[j];
        if (j == i) x += evi;
        acc += a[j] * pm_phi<MODE>(s2, x);
      }
    }
    acc = pm_wave_sum(acc);
    if (lane == 0) low[ii] = acc;
  }

  // j > i: C[j][i], a row segment of a lower tile; lanes along i, two threads per row
  {
    const int ii = tid & (PM_ROWS - 1), half = tid >> 7;
    const int i = r0 + ii;
    double acc = 0.0;
    if (i < m) {
      const T* col = C + i;
#pragma unroll 4
      for (int j = max(c0, i + 1) + half; j < c1; j += 2) acc += a[j] * pm_phi<MODE>(s2, (double)col[(long)j * M]);
    }
    up[half][ii] = acc;
  }
  __syncthreads();
  if (tid < PM_ROWS && r0 + tid < m) Y[(long)(r0 + tid) * P + g] = low[tid] + (up[0][tid] + up[1][tid]);
}

__global__ __launch_bounds__(256) void pm_reduce_kernel(long M, int P, const double* __restrict__ work, long ws,
                                                        double* __restrict__ mean_out, double* __restrict__ cov_out) {
  const int hc = blockIdx.x, g = blockIdx.y, z = blockIdx.z;
  if (hc > 0 && hc * 64 + 63 < g) return;  // every h of this chunk is < g: the (h, g) workgroup writes those entries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* a = work + (long)z * ws;
  const double* am = a + M;
  const double* Y = a + 2 * M;
  int c0, c1;
  pm_range((const int*)(a + 2 * M + M * (long)P), g, c0, c1);
  __shared__ double red[4][64];
  __shared__ double mred[256];
  const int h = hc * 64 + lane;
  double acc = 0.0;
  if (h < P) {
#pragma unroll 4
    for (int i = c0 + wave; i < c1; i += 4) acc += a[i] * Y[(long)i * P + h];
  }
  red[wave][lane] = acc;
  if (hc == 0) {
    double s = 0.0;
    for (int i = c0 + tid; i < c1; i += 256) s += am[i];
    mred[tid] = s;
  }
  __syncthreads();
  if (wave == 0 && h < P && h >= g) {
    const double v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    double* out = cov_out + (long)z * P * P;
    out[(long)g * P + h] = v;
    out[(long)h * P + g] = v;
  }
  if (hc == 0) {
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) mred[tid] += mred[tid + s];
      __syncthreads();
    }
    if (tid == 0) mean_out[(long)z * P + g] = mred[0];
  }
}

// Workgroups per CU the streamed rows kernel is compiled for: two, except for the two fp64 evaluators whose covariance
// evaluation is too large for the registers two workgroups leave beside the accumulators (measured at two: rating 84 bytes
// of scratch per lane, loadest d = 6 12 bytes) -- they get one, and the register file of a whole SIMD, instead of spilling.
template <typename T, typename Mod>
struct PpmOcc {
  static constexpr int value = 2;
};
template <>
struct PpmOcc<double, Rating<double>> {
  static constexpr int value = 1;
};
template <>
struct PpmOcc<double, Loadest<double, 6>> {
  static constexpr int value = 1;
};

// Y[i][h] = sum_{j in h} a_j phi(C_ij), C = K(Xs, Xs) - V^T V from V (N x Mp, site stride wbs) and the test points' SoA
// coordinates Xst (d x Mp, same stride); see the file header.
template <typename T, typename Mod, int MODE>
__global__ __launch_bounds__(256, (PpmOcc<T, Mod>::value)) void ppm_rows_kernel(const T* __restrict__ V, long N, long Mp, int m, int P,
                                                          const T* __restrict__ Xst, long wbs, const PreBatch<Mod> pb,
                                                          const double* __restrict__ scale2, const int* __restrict__ group,
                                                          const T* __restrict__ ev, double* __restrict__ work, long ws) {
  using K = TileCore<T, false, false, PM_ROWS, PM_COLS>;  // the register-staged core (TileGemm) on 128 x 64 tiles
  using G = typename K::G;
  static_assert(!K::DMA && G::MI == 4 && G::NI == 2, "128 x 64 tile, 2 x 2 waves of 64 x 32");
  static_assert(Mod::NF * PM_COLS * sizeof(T) + PM_COLS * sizeof(double) <= K::SMEM_ELEMS * sizeof(T),
                "the column strip does not fit the operand tiles");
  const int rb = blockIdx.x, h = blockIdx.y, z = blockIdx.z;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int r0 = rb * PM_ROWS;
  const int* gz = group + (long)z * m;
  exp_table_init<T>();
  // rows of this block in a group <= h: otherwise no entry of Y[., h] here is ever read (the barrier also publishes the table)
  int need = 0;
  if (t < PM_ROWS && r0 + t < m) {
    const int g = gz[r0 + t];
    need = g >= 0 && g <= h;
  }
  double* base = work + (long)z * ws;
  const double* a = base;
  double* Y = base + 2 * Mp;
  if (!__syncthreads_or(need)) {
    // The reduce pass reads Y[i][h] for every i in a group's column range, excluded points included (a_i = 0 there): a
    // block of excluded points inside a range -- a gap of 128 or more -- must still leave numbers, not the work area's past
    if (t < PM_ROWS && r0 + t < m) Y[(long)(r0 + t) * P + h] = 0.0;
    return;
  }

  __shared__ __attribute__((aligned(16))) T smem[K::SMEM_ELEMS];
  __shared__ T sfi[Mod::NF][PM_ROWS];
  __shared__ double red[2][PM_ROWS];
  V = site(V, wbs);
  Xst = site(Xst, wbs);
  int c0, c1;
  pm_range((const int*)(base + 2 * Mp + Mp * (long)P), h, c0, c1);
  const T* evz = ev ? ev + (long)z * m : nullptr;
  const double s2 = scale2[z];
  const typename Mod::Pre& pre = pb.get();
  if (t < PM_ROWS) {
    T x[Mod::NX], f[Mod::NF];
#pragma unroll
    for (int c = 0; c < Mod::NX; ++c) x[c] = Xst[(long)c * Mp + r0 + t];
    Mod::features(x, pre, f);
#pragma unroll
    for (int c = 0; c < Mod::NF; ++c) sfi[c][t] = f[c];
  }
  // (the first barrier of the k-loop publishes the row strip)
  T(*sfj)[PM_COLS] = reinterpret_cast<T(*)[PM_COLS]>(smem);
  double* saj = reinterpret_cast<double*>(smem + Mod::NF * PM_COLS);
  const int wm = (w >> 1) * (PM_ROWS / 2), wn = (w & 1) * (PM_COLS / 2);
  double racc = 0.0;  // thread t < 128: row r0 + t
  T dummy[Mod::NTHETA];
  for (int jb = c0 / PM_COLS; jb * PM_COLS < c1; ++jb) {
    typename G::acc_t acc[G::MI][G::NI];
    G::zero(acc);
    K::run(V + r0, Mp, V + (long)jb * PM_COLS, Mp, (int)(N / 16), smem, acc);
    __syncthreads();  // every wave is done with the operand tiles
    if (t < PM_COLS) {
      const int j = jb * PM_COLS + t;
      T x[Mod::NX], f[Mod::NF];
#pragma unroll
      for (int c = 0; c < Mod::NX; ++c) x[c] = Xst[(long)c * Mp + j];
      Mod::features(x, pre, f);
#pragma unroll
      for (int c = 0; c < Mod::NF; ++c) sfj[c][t] = f[c];
      saj[t] = (j < m && gz[j] == h) ? a[j] : 0.0;
    }
    __syncthreads();
    // One entry at a time, features from LDS per entry.  The loops over the 16-row groups, a group's sub-tiles and a lane's
    // four entries of a sub-tile stay rolled: the next group / sub-tile / entry is rotated to the front (register moves), so
    // that the accumulators and the four row sums keep constant indices and only ONE covariance evaluation is in flight --
    // unrolled, the compiler interleaves several and spills in fp64 (measured: 172-408 bytes per lane with four in flight).
#pragma unroll 1
    for (int mi = 0; mi < G::MI; ++mi) {
      typename G::acc_t row[G::NI];  // this 16-row group's sub-tiles; the later groups move up
#pragma unroll
      for (int k = 0; k < G::NI; ++k) row[k] = acc[0][k];
#pragma unroll
      for (int q = 0; q + 1 < G::MI; ++q)
#pragma unroll
        for (int k = 0; k < G::NI; ++k) acc[q][k] = acc[q + 1][k];
      dgp_d4 part = {0.0, 0.0, 0.0, 0.0};  // the row sums of this lane's four rows r, rotated with the entries
#pragma unroll 1
      for (int ni = 0; ni < G::NI; ++ni) {
        typename G::acc_t cur = row[0];
#pragma unroll
        for (int k = 0; k + 1 < G::NI; ++k) row[k] = row[k + 1];
        const int cj = wn + ni * 16 + (lane & 15);
        const long gj = (long)jb * PM_COLS + cj;
        T fj[Mod::NF];
#pragma unroll
        for (int c = 0; c < Mod::NF; ++c) fj[c] = sfj[c][cj];
        const double aj = saj[cj];
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const double vr = (double)cur[0];
          cur = cur.yzwx;
          const int ri = wm + mi * 16 + Mfma<T>::crow(lane, r);
          const long gi = (long)r0 + ri;
          T fi[Mod::NF];
#pragma unroll
          for (int c = 0; c < Mod::NF; ++c) fi[c] = sfi[c][ri];
          double cij = (double)Mod::template pair<false>(fi, fj, pre, T(0), dummy) - vr;
          if (gi == gj && evz && gi < m) cij += (double)evz[gi];
          const double v = aj * pm_phi<MODE>(s2, cij);
          part.x += aj != 0.0 ? v : 0.0;
          part = part.yzwx;  // four rotations per sub-tile: back in row order
        }
      }
      // the 16 columns of the sub-tile (lanes of one lane >> 4 group), a fixed butterfly
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double pr = part[r];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) pr += __shfl_xor(pr, off, 64);
        if ((lane & 15) == 0) red[w & 1][wm + mi * 16 + Mfma<T>::crow(lane, r)] = pr;
      }
    }
    __syncthreads();
    if (t < PM_ROWS) racc += red[0][t] + red[1][t];
    // (the next tile's k-loop starts with a barrier before anything rewrites the operand tiles or red)
  }
  if (t < PM_ROWS && r0 + t < m) Y[(long)(r0 + t) * P + h] = gz[r0 + t] >= 0 ? racc : 0.0;
}

template <typename T, int MODE>
int period_moments_mode(const T* cov, long M, int m, int B, const T* mu, const double* scale2, const double* w,
                        const int* group, int P, const T* ev, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  const long ws = pm_site_doubles(M, P);
  pm_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P);
  pm_prep_kernel<T, MODE><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(cov, M * M, M + 1, M, m, P, mu, scale2,
                                                                                          w, group, ev, work, ws);
  pm_rows_kernel<T, MODE><<<dim3((unsigned)(M / PM_ROWS), (unsigned)P, (unsigned)B), 256, 0, s>>>(cov, M, m, P, scale2, ev, work, ws);
  pm_reduce_kernel<<<dim3((unsigned)((P + 63) / 64), (unsigned)P, (unsigned)B), 256, 0, s>>>(M, P, work, ws, mean_out, cov_out);
  return (int)hipGetLastError();
}

// ---- the same moments on R = B^T B (B: nrows x m conditioning rows) without ever forming R (dgp_lowrank_period_moments).
// R_ij is a product of nrows terms, so nothing is read twice and nothing is stored: one thread per point forms R_ii for the
// prep pass (left where Y will be), then one workgroup per (64-row block I, group h) -- a block past h's last column writes
// zeros and leaves, as in the streamed pass -- holds its rows' B_ti in LDS, lanes along i, and walks h's columns 8 at a time,
// the four waves taking the 8-column tiles in turn: the columns' B_tj are wave-uniform loads, 8 accumulators per lane, t
// ascending (fused multiply-adds: R_ij and R_ji are the same bits), then a_j phi(R_ij) into the lane's sum; the waves' sums are
// added in a fixed order.  The reduce pass is pm_reduce_kernel.
constexpr int LR_ROWS = 64;  // rows of a workgroup
constexpr int LR_COLS = 8;   // columns of a wave's tile

__global__ __launch_bounds__(256) void lr_diag_kernel(const double* __restrict__ rows, int nrows, long M, int m, int P, double* work,
                                                      long ws) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  double r = 0.0;
  if (j < m)
    for (int t = 0; t < nrows; ++t) {
      const double b = rows[((long)z * nrows + t) * m + j];
      r = __builtin_fma(b, b, r);
    }
  work[(long)z * ws + 2 * M + j] = r;
}

template <int MODE>
__global__ __launch_bounds__(256) void lr_rows_kernel(const double* __restrict__ rows, int nrows, long M, int m, int P,
                                                      const double* __restrict__ scale2, const int* __restrict__ group,
                                                      double* __restrict__ work, long ws) {
  const int rb = blockIdx.x, h = blockIdx.y, z = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* base = work + (long)z * ws;
  const double* a = base;
  double* Y = base + 2 * M;
  int c0, c1;
  pm_range((const int*)(base + 2 * M + M * (long)P), h, c0, c1);
  const int r0 = rb * LR_ROWS, i = r0 + lane;
  if (r0 >= c1) {  // every row lies in a group above h, is excluded or is pad: the reduce pass reads these times a_i = 0 or not at all
    if (tid < LR_ROWS) Y[(long)i * P + h] = 0.0;
    return;
  }
  extern __shared__ __attribute__((aligned(16))) char lr_smem[];
  double* bi = (double*)lr_smem;        // [nrows][LR_ROWS]: B[t][r0 + lane]
  double* part = bi + nrows * LR_ROWS;  // [4][LR_ROWS]
  const double* bz = rows + (long)z * nrows * m;
  for (int t = wave; t < nrows; t += 4) bi[t * LR_ROWS + lane] = i < m ? bz[(long)t * m + i] : 0.0;
  __syncthreads();
  const double s2 = scale2[z];
  double acc = 0.0;
  for (int j0 = c0 / LR_COLS * LR_COLS + wave * LR_COLS; j0 < c1; j0 += 4 * LR_COLS) {
    double x[LR_COLS];
#pragma unroll
    for (int u = 0; u < LR_COLS; ++u) x[u] = 0.0;
    const bool whole = j0 + LR_COLS <= m;
    for (int t = 0; t < nrows; ++t) {
      const double bv = bi[t * LR_ROWS + lane];
      const double* br = bz + (long)t * m + j0;
#pragma unroll
      for (int u = 0; u < LR_COLS; ++u) x[u] = __builtin_fma(bv, whole || j0 + u < m ? br[u] : 0.0, x[u]);
    }
#pragma unroll
    for (int u = 0; u < LR_COLS; ++u) {
      const int j = j0 + u;
      if (j >= c0 && j < c1) acc += a[j] * pm_phi<MODE>(s2, x[u]);  // wave-uniform
    }
  }
  part[wave * LR_ROWS + lane] = acc;
  __syncthreads();
  if (tid < LR_ROWS) {
    const double v = ((part[lane] + part[LR_ROWS + lane]) + part[2 * LR_ROWS + lane]) + part[3 * LR_ROWS + lane];
    Y[(long)i * P + h] = i < m && group[(long)z * m + i] >= 0 ? v : 0.0;
  }
}

template <int MODE>
int lowrank_period_moments_mode(const double* rows, int nrows, long M, int m, int B, const double* mu, const double* scale2,
                                const double* w, const int* group, int P, double* work, double* mean_out, double* cov_out,
                                hipStream_t s) {
  const long ws = pm_site_doubles(M, P);
  pm_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P);
  lr_diag_kernel<<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(rows, nrows, M, m, P, work, ws);
  // R_ii sits at the head of Y (site stride ws, step 1) until the rows pass overwrites it
  pm_prep_kernel<double, MODE><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work + 2 * M, ws, 1, M, m, P, mu, scale2, w,
                                                                                               group, nullptr, work, ws);
  const size_t lds = ((size_t)nrows + 4) * LR_ROWS * sizeof(double);
  lr_rows_kernel<MODE><<<dim3((unsigned)(M / LR_ROWS), (unsigned)P, (unsigned)B), 256, lds, s>>>(rows, nrows, M, m, P, scale2, group, work, ws);
  pm_reduce_kernel<<<dim3((unsigned)((P + 63) / 64), (unsigned)P, (unsigned)B), 256, 0, s>>>(M, P, work, ws, mean_out, cov_out);
  return (int)hipGetLastError();
}

}  // namespace

static size_t period_moments_workspace_bytes(long m, int P, int B) {
  return sizeof(double) * (size_t)B * (size_t)pm_site_doubles(round_up(m, DGP_TILE_HOST), P);
}

// exact mean / covariance of period sums of exp(s f + t) (mode 1) or s f + t (mode 0), f ~ N(mu, C)
template <typename T>
static int period_moments(int mode, const T* cov, long m, int B, const T* mu, const double* scale2, const double* w, const int* group,
                   int P, const T* ev, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  return mode == 1 ? period_moments_mode<T, 1>(cov, M, (int)m, B, mu, scale2, w, group, P, ev, work, mean_out, cov_out, s)
                   : period_moments_mode<T, 0>(cov, M, (int)m, B, mu, scale2, w, group, P, ev, work, mean_out, cov_out, s);
}

namespace {
template <typename T, int MODE>
int posterior_period_moments_mode(int model, int d, const T* V, long N, long Mp, int m, int B, const T* Xst, const T* var, long wbs,
                                  const double* theta, const T* mu, const double* scale2, const double* w, const int* group, int P,
                                  const T* ev, double* work, double* mean_out, double* cov_out, hipStream_t s, void* pre_scratch) {
  const int nt = model_ntheta(model, d);
  if (nt < 0) return -2;
  const long ws = pm_site_doubles(Mp, P);
  pm_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work, ws, Mp, P);
  pm_prep_kernel<T, MODE><<<dim3((unsigned)((Mp + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(var, wbs, 1, Mp, m, P, mu, scale2, w,
                                                                                           group, ev, work, ws);
  const dim3 grid((unsigned)(Mp / PM_ROWS), (unsigned)P, (unsigned)B);
  DGP_DISPATCH_MODEL(model, d, (ppm_rows_kernel<T, M, MODE><<<grid, 256, 0, s>>>(
                                   V, N, Mp, m, P, Xst, wbs, prepare_batch<M>(theta, nt, B, pre_scratch, false, s), scale2, group,
                                   ev, work, ws)));
  pm_reduce_kernel<<<dim3((unsigned)((P + 63) / 64), (unsigned)P, (unsigned)B), 256, 0, s>>>(Mp, P, work, ws, mean_out, cov_out);
  return (int)hipGetLastError();
}
}  // namespace

// the same moments with C = K(Xs, Xs) - V^T V never stored: V (N x M), the test points' SoA coordinates Xst (d x M) and their
// predicted variance var (M) as the prediction leaves them in its work area (site stride wbs elements); `work` as above
// (period_moments_workspace_bytes); pre_scratch: the plan's hyperparameter scratch, already filled by this call's gram_cross
template <typename T>
static int posterior_period_moments(int mode, int model, int d, const T* V, long N, long m, int B, const T* Xst, const T* var, long wbs,
                                    const double* theta, const T* mu, const double* scale2, const double* w, const int* group, int P,
                                    const T* ev, double* work, double* mean_out, double* cov_out, hipStream_t s, void* pre_scratch) {
  const long Mp = round_up(m, DGP_TILE_HOST);
  return mode == 1 ? posterior_period_moments_mode<T, 1>(model, d, V, N, Mp, (int)m, B, Xst, var, wbs, theta, mu, scale2, w, group,
                                                          P, ev, work, mean_out, cov_out, s, pre_scratch)
                   : posterior_period_moments_mode<T, 0>(model, d, V, N, Mp, (int)m, B, Xst, var, wbs, theta, mu, scale2, w, group,
                                                          P, ev, work, mean_out, cov_out, s, pre_scratch);
}

}  // namespace dgp

using namespace dgp;

// streamed period moments: dgp_stream.h's areas without a panel (the pass forms its rows of C on the fly), then the moment
// pass's work area
template <typename T>
static int post_period(dgp_plan* p, const double* theta, const void* Xs, int64_t m, int mode, const void* mu, const double* scale2,
                       const double* w, const int32_t* group, int P, const void* ev, void* work, double* mean_out, double* cov_out,
                       hipStream_t s) {
  double* pm = (double*)posterior_areas<T>(p, m, work, 0).own;
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, pm, s)) return rc;
  return posterior_period_moments<T>(mode, p->model, p->d, ps.V, p->N, (long)m, p->B, ps.Xst, ps.var, ps.wbs, theta, (const T*)mu, scale2, w,
                                     group, P, (const T*)ev, pm, mean_out, cov_out, s, p->pre);
}

extern "C" {

size_t dgp_period_moments_workspace_bytes(int64_t m, int ngroups, int batch) {
  if (m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535 || batch <= 0 || batch > DGP_MAX_BATCH_SITES) return 0;
  return period_moments_workspace_bytes(m, ngroups, batch);
}

int dgp_period_moments(int dtype, int mode, const void* cov, int64_t m, int batch, const void* mu, const double* scale2,
                       const double* w, const int32_t* group, int ngroups, const void* extra_var, void* work,
                       size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_period_moments: dtype must be 0 (f64) or 1 (f32)");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_period_moments: mode must be 0 (linear) or 1 (log)");
  if (!cov || !mu || !scale2 || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_period_moments: null argument");
  if (m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535 || batch <= 0 || batch > DGP_MAX_BATCH_SITES)
    return fail(DGP_E_ARG, "dgp_period_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= batch <= 1024)");
  if (!work || work_bytes < period_moments_workspace_bytes(m, ngroups, batch))
    return fail(DGP_E_WORKSPACE, "dgp_period_moments: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64
                     ? period_moments<double>(mode, (const double*)cov, m, batch, (const double*)mu, scale2, w, group, ngroups,
                                              (const double*)extra_var, (double*)work, mean_out, cov_out, s)
                     : period_moments<float>(mode, (const float*)cov, m, batch, (const float*)mu, scale2, w, group, ngroups,
                                             (const float*)extra_var, (double*)work, mean_out, cov_out, s);
  return wrap(rc, "dgp_period_moments");
}

int dgp_lowrank_period_moments(int mode, const double* rows, int nrows, int64_t m, int batch, const double* mu, const double* scale2,
                               const double* w, const int32_t* group, int ngroups, void* work, size_t work_bytes, double* mean_out,
                               double* cov_out, void* stream) {
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_lowrank_period_moments: mode must be 0 (linear) or 1 (log)");
  if (!rows || !mu || !scale2 || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_lowrank_period_moments: null argument");
  if (m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535 || nrows < 1 || nrows > 64 || batch <= 0 || batch > DGP_MAX_BATCH_SITES)
    return fail(DGP_E_ARG,
                "dgp_lowrank_period_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nrows <= 64, 1 <= batch <= 1024)");
  if (!work || work_bytes < period_moments_workspace_bytes(m, ngroups, batch))
    return fail(DGP_E_WORKSPACE, "dgp_lowrank_period_moments: workspace missing or too small");
  if (((uintptr_t)work & 7) != 0) return fail(DGP_E_ARG, "dgp_lowrank_period_moments: the work area must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long M = round_up(m, DGP_TILE_HOST);
  const int rc = mode == 1 ? lowrank_period_moments_mode<1>(rows, nrows, M, (int)m, batch, mu, scale2, w, group, ngroups, (double*)work,
                                                            mean_out, cov_out, s)
                           : lowrank_period_moments_mode<0>(rows, nrows, M, (int)m, batch, mu, scale2, w, group, ngroups, (double*)work,
                                                            mean_out, cov_out, s);
  return wrap(rc, "dgp_lowrank_period_moments");
}

size_t dgp_posterior_period_moments_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups) {
  if (!p || m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535) return 0;
  return posterior_head_bytes(p, m, 0) + period_moments_workspace_bytes(m, ngroups, p->B);
}

int dgp_posterior_period_moments(dgp_plan* p, const double* theta, const void* Xs, int64_t m, int mode, const void* mu,
                                 const double* scale2, const double* w, const int32_t* group, int ngroups, const void* extra_var,
                                 void* work, size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_posterior_period_moments: mode must be 0 (linear) or 1 (log)");
  if (!theta || !Xs || !mu || !scale2 || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_posterior_period_moments: null argument");
  if (m <= 0 || m > (1 << 20) || ngroups <= 0 || ngroups > 65535)
    return fail(DGP_E_ARG, "dgp_posterior_period_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535)");
  if (int rc = need_factor(p, "dgp_posterior_period_moments", "call dgp_factorize")) return rc;
  DGP_CHECK_PLAN(p);
  if (!work || work_bytes < dgp_posterior_period_moments_workspace_bytes(p, m, ngroups))
    return fail(DGP_E_WORKSPACE, "dgp_posterior_period_moments: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, post_period<double>(p, theta, Xs, m, mode, mu, scale2, w, group, ngroups, extra_var, work, mean_out, cov_out, s),
                              post_period<float>(p, theta, Xs, m, mode, mu, scale2, w, group, ngroups, extra_var, work, mean_out, cov_out, s));
  return wrap(rc, "dgp_posterior_period_moments");
}

}  // extern "C"
