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
#include <climits>

#include "dgp_common.h"
#include "dgp_internal.h"

namespace dgp {

namespace {

constexpr int PM_ROWS = 128;  // rows of a workgroup of the rows pass (== DGP_TILE_HOST, the cov buffer's block size)

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

template <typename T, int MODE>
__global__ __launch_bounds__(256) void pm_prep_kernel(const T* __restrict__ cov, long M, int m, int P, const T* __restrict__ mu,
                                                      const double* __restrict__ scale2, const double* __restrict__ w,
                                                      const int* __restrict__ group, const T* __restrict__ ev, double* work,
                                                      long ws) {
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
        double cjj = (double)cov[(long)z * M * M + j * M + j];
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

template <typename T, int MODE>
int period_moments_mode(const T* cov, long M, int m, int B, const T* mu, const double* scale2, const double* w,
                        const int* group, int P, const T* ev, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  const long ws = pm_site_doubles(M, P);
  pm_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P);
  pm_prep_kernel<T, MODE><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(cov, M, m, P, mu, scale2, w, group,
                                                                                          ev, work, ws);
  pm_rows_kernel<T, MODE><<<dim3((unsigned)(M / PM_ROWS), (unsigned)P, (unsigned)B), 256, 0, s>>>(cov, M, m, P, scale2, ev, work, ws);
  pm_reduce_kernel<<<dim3((unsigned)((P + 63) / 64), (unsigned)P, (unsigned)B), 256, 0, s>>>(M, P, work, ws, mean_out, cov_out);
  return (int)hipGetLastError();
}

}  // namespace

size_t period_moments_workspace_bytes(long m, int P, int B) {
  return sizeof(double) * (size_t)B * (size_t)pm_site_doubles(round_up(m, DGP_TILE_HOST), P);
}

template <typename T>
int period_moments(int mode, const T* cov, long m, int B, const T* mu, const double* scale2, const double* w, const int* group,
                   int P, const T* ev, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  return mode == 1 ? period_moments_mode<T, 1>(cov, M, (int)m, B, mu, scale2, w, group, P, ev, work, mean_out, cov_out, s)
                   : period_moments_mode<T, 0>(cov, M, (int)m, B, mu, scale2, w, group, P, ev, work, mean_out, cov_out, s);
}

template int period_moments<double>(int, const double*, long, int, const double*, const double*, const double*, const int*, int,
                                    const double*, double*, double*, double*, hipStream_t);
template int period_moments<float>(int, const float*, long, int, const float*, const double*, const double*, const int*, int,
                                   const float*, double*, double*, double*, hipStream_t);

}  // namespace dgp
