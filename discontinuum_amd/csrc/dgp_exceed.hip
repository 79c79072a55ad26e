// dgp_exceed.hip -- exact moments of threshold-exceedance counts of a Gaussian posterior (dgp_exceedance_moments).
//
// f ~ N(mu, C) over m points (C: the matrix dgp_posterior_cov leaves; only its lower triangle is read), per level l a
// threshold u_il in model space, weights w_i and group ids g_i (non-decreasing, -1 = excluded).  With
//     sigma_i^2 = C_ii (+ extra_var_i),  z_il = (mu_i - u_il) / sigma_i,  p_il = Phi(z_il),  rho_ij = C_ij / (sigma_i sigma_j)
// the count N_g = sum_{i in g} w_i 1[f_i > u_il] has
//     mean_g = sum_{i in g} w_i p_il,   cov_gh = sum_{i in g} sum_{j in h} w_i w_j D(z_il, z_jl, rho_ij),
//     D(h, k, rho) = Phi2(h, k; rho) - Phi(h) Phi(k)  (= p (1 - p) on the diagonal).
//
// The pair function is Genz's bivariate normal algorithm (Numerical computation of rectangular bivariate and trivariate
// normal and t probabilities, Statistics and Computing 14, 2004) rearranged to return D:
//   |rho| < 0.925   D = asin(rho) / (4 pi) sum_n w_n exp((s_n h k - (h^2 + k^2) / 2) / (1 - s_n^2)),  s_n = sin(asin(rho) (1 +- x_n) / 2),
//                   Gauss-Legendre with 6 (|rho| < 0.3), 12 (< 0.75) or 20 nodes: the integral IS D, nothing is subtracted; every
//                   exponent is <= 0 (exp_nonpos).  The two nodes +-x_n share sin / cos of asin(rho) / 2 and asin(rho) x_n / 2
//                   (angle addition; all angles below 0.6, so a short Taylor polynomial needs no range reduction), and
//                   1 - s_n^2 is the square of the angle's cosine, which the same products give without cancellation.
//   0.925 <= |rho| < 1  the expansion about |rho| = 1 plus a 20-node rule for its remainder.
//   |rho| = 1       min(Phi(h), Phi(k)) - Phi(h) Phi(k)  /  max(0, Phi(h) + Phi(k) - 1) - Phi(h) Phi(k).
// What depends on rho alone -- the nodes' sines and 1 / (1 - s_n^2), the expansion's abscissae and roots -- is computed once
// per pair, in the node loop, whose inner loop runs over the levels of the chunk (LC = 8, 4, 2 or 1 levels in registers).
//
// Launches (gridDim.z = sites), no floating-point atomics: a tiny init and a prep once, then per chunk of levels
//   prep    one thread per point: w_i (0 if excluded), 1 / sigma_i, z_il and p_il for every level, each group's column range.
//           A point is DECIDED at a level when sigma_i^2 <= 0 or u_il = +-inf: z = +-inf (a tie mu = u is "not exceeded"),
//           p = 1 / 0 and D = 0 with every other point; so is an excluded point (w = 0).  NaN stays NaN.
//   pairs   one workgroup per (64-row block, group h): Y[l][i][h] = sum_j w_j D(z_il, z_jl, rho_ij) over the j of h that the
//           reduce needs -- j < i for g(i) = h, read as C[i][j] (a wave per row, lanes along j); all j of h for g(i) < h, read
//           as C[j][i] (lanes along i, the four waves take every fourth j); nothing for g(i) > h.  Every unordered pair is
//           evaluated once.  Lanes of a wave see neighbouring points, hence similar rho: the branch on |rho| is mostly
//           wave-uniform.
//   reduce  one workgroup per (64 columns h, level, group g): cov_gh = sum_{i in g} w_i Y[l][i][h] for h > g, twice that plus
//           sum_i w_i^2 p_il (1 - p_il) for h = g, written to (g, h) and (h, g) from one value; mean_g beside it.
// Every sum runs in a fixed order: bitwise repeatable, and a site's numbers do not depend on its batch.  All arithmetic
// after the loads of C and mu is double.
#include <climits>

#include "dgp_bvn.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

__global__ __launch_bounds__(256) void ex_init_kernel(double* work, long ws, long M, int P, int L) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  const ExWork wk(work, ws, M, P, L);
  wk.se[2 * g] = INT_MAX;
  wk.se[2 * g + 1] = 0;
}

// C_jj of site z sits at diag[z dsite + j dstep]: the diagonal of the dense covariance (dsite = M M, dstep = M + 1), or the
// predicted variance the streamed pass finds in its work area (dsite = that area's site stride, dstep = 1)
template <typename T>
__global__ __launch_bounds__(256) void ex_prep_kernel(const T* __restrict__ diag, long dsite, long dstep, long M, int m, int P, int L,
                                                      const T* __restrict__ mu, const double* __restrict__ thresh,
                                                      const double* __restrict__ w, const int* __restrict__ group,
                                                      const T* __restrict__ ev, double* work, long ws) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  const ExWork wk(work, ws, M, P, L);
  bool in = false;
  double wj = 0.0, sinv = 0.0, var = 0.0, muj = 0.0;
  if (j < m) {
    const long k = (long)z * m + j;
    const int g = group[k];
    if (g >= 0 && g < P) {
      in = true;
      wj = w[k];
      muj = (double)mu[k];
      var = (double)diag[(long)z * dsite + j * dstep];
      if (ev) var += (double)ev[k];
      sinv = var > 0.0 ? 1.0 / sqrt(var) : (var != var ? var : 0.0);
      atomicMin(&wk.se[2 * g], (int)j);
      atomicMax(&wk.se[2 * g + 1], (int)j + 1);
    }
  }
  wk.w[j] = wj;
  wk.sinv[j] = sinv;
  for (int l = 0; l < L; ++l) {
    double zl = -INFINITY;  // excluded / pad: decided, p = 0
    if (in) {
      const double u = thresh[((long)z * L + l) * m + j];
      if (var <= 0.0 || isinf(u))
        zl = (muj != muj || u != u) ? __builtin_nan("") : (muj > u ? INFINITY : -INFINITY);
      else
        zl = (muj - u) * sinv;
    }
    wk.z[(long)l * M + j] = zl;
    wk.p[(long)l * M + j] = ex_phi(zl);
  }
}

// levels l0 .. l0 + LC of Y; see the file header
template <typename T, int LC>
__global__ __launch_bounds__(256) void ex_pairs_kernel(const T* __restrict__ cov, long M, int m, int P, int L, int l0,
                                                       const int* __restrict__ group, double* __restrict__ work, long ws) {
  const int rb = blockIdx.x, h = blockIdx.y, z = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ExWork wk(work, ws, M, P, L);
  const int r0 = rb * EX_ROWS;
  int c0, c1;
  ex_range(wk.se, h, c0, c1);
  if (r0 >= c1) {  // every row here lies in a later group (or h is empty): nothing the reduce uses, but it reads numbers
    if (tid < EX_ROWS)
#pragma unroll
      for (int l = 0; l < LC; ++l) wk.Y[((long)l * M + r0 + tid) * P + h] = 0.0;
    return;
  }
  ex_tables_init();
  __shared__ double low[LC][EX_ROWS], up[4][LC][EX_ROWS];
  const T* C = cov + (long)z * M * M;
  const int* gz = group + (long)z * m;
  const double* zs = wk.z + (long)l0 * M;
  const double* ps = wk.p + (long)l0 * M;
  __syncthreads();

  // g(i) = h: the j < i of the group, C[i][j]; a wave per row, lanes along the row
  for (int ii = wave; ii < EX_ROWS; ii += 4) {
    const int i = r0 + ii;
    double acc[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) acc[l] = 0.0;
    if (i < m && gz[i] == h) {
      const T* row = C + (long)i * M;
      const double si = wk.sinv[i];
      double zi[LC], pi[LC];
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        zi[l] = zs[(long)l * M + i];
        pi[l] = ps[(long)l * M + i];
      }
      for (int j = c0 + lane; j < i; j += 64) {
        double zj[LC], pj[LC], D[LC];
#pragma unroll
        for (int l = 0; l < LC; ++l) {
          zj[l] = zs[(long)l * M + j];
          pj[l] = ps[(long)l * M + j];
        }
        bvn_excess<LC>(zi, zj, pi, pj, (double)row[j] * si * wk.sinv[j], D);
        const double wj = wk.w[j];
#pragma unroll
        for (int l = 0; l < LC; ++l) acc[l] = __builtin_fma(wj, D[l], acc[l]);
      }
    }
#pragma unroll
    for (int l = 0; l < LC; ++l) {
      const double v = ex_wave_sum(acc[l]);
      if (lane == 0) low[l][ii] = v;
    }
  }

  // 0 <= g(i) < h: every j of the group (all beyond i), C[j][i]; lanes along i, wave q takes j = c0 + q, c0 + q + 4, ...
  {
    const int i = r0 + lane;
    double acc[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) acc[l] = 0.0;
    const int gi = i < m ? gz[i] : -1;
    if (gi >= 0 && gi < h) {
      const T* col = C + i;
      const double si = wk.sinv[i];
      double zi[LC], pi[LC];
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        zi[l] = zs[(long)l * M + i];
        pi[l] = ps[(long)l * M + i];
      }
      for (int j = c0 + wave; j < c1; j += 4) {
        double zj[LC], pj[LC], D[LC];
#pragma unroll
        for (int l = 0; l < LC; ++l) {
          zj[l] = zs[(long)l * M + j];
          pj[l] = ps[(long)l * M + j];
        }
        bvn_excess<LC>(zi, zj, pi, pj, (double)col[(long)j * M] * si * wk.sinv[j], D);
        const double wj = wk.w[j];
#pragma unroll
        for (int l = 0; l < LC; ++l) acc[l] = __builtin_fma(wj, D[l], acc[l]);
      }
    }
#pragma unroll
    for (int l = 0; l < LC; ++l) up[wave][l][lane] = acc[l];
  }
  __syncthreads();
  if (tid < EX_ROWS)
#pragma unroll
    for (int l = 0; l < LC; ++l)
      wk.Y[((long)l * M + r0 + tid) * P + h] = low[l][tid] + ((up[0][l][tid] + up[1][l][tid]) + (up[2][l][tid] + up[3][l][tid]));
}

// blockIdx.x = (64-column chunk of h) * LC + level of the chunk
__global__ __launch_bounds__(256) void ex_reduce_kernel(long M, int P, int L, int l0, int LC, double* __restrict__ work, long ws,
                                                        double* __restrict__ mean_out, double* __restrict__ cov_out) {
  const int hc = blockIdx.x / LC, lc = blockIdx.x % LC, g = blockIdx.y, z = blockIdx.z;
  if (hc > 0 && hc * 64 + 63 < g) return;  // every h of this chunk is < g: the (h, g) workgroup writes those entries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ExWork wk(work, ws, M, P, L);
  const double* Y = wk.Y + (long)lc * M * P;
  const double* p = wk.p + (long)(l0 + lc) * M;
  int c0, c1;
  ex_range(wk.se, g, c0, c1);
  __shared__ double red[4][64];
  __shared__ double mred[256], dred[256];
  const int h = hc * 64 + lane;
  double acc = 0.0;
  if (h < P) {
#pragma unroll 4
    for (int i = c0 + wave; i < c1; i += 4) acc += wk.w[i] * Y[(long)i * P + h];
  }
  red[wave][lane] = acc;
  const bool own = g >= hc * 64 && g < hc * 64 + 64;  // this workgroup holds (g, g): it needs the diagonal terms
  if (hc == 0 || own) {
    double s = 0.0, d = 0.0;
    for (int i = c0 + tid; i < c1; i += 256) {
      const double wi = wk.w[i], pi = p[i];
      s += wi * pi;
      d += wi * wi * (pi * (1.0 - pi));
    }
    mred[tid] = s;
    dred[tid] = d;
  }
  __syncthreads();
  if (hc == 0 || own) {
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        mred[tid] += mred[tid + s];
        dred[tid] += dred[tid + s];
      }
      __syncthreads();
    }
  }
  if (wave == 0 && h < P && h >= g) {
    double v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    if (h == g) v = 2.0 * v + dred[0];
    double* out = cov_out + ((long)z * L + l0 + lc) * P * P;
    out[(long)g * P + h] = v;
    out[(long)h * P + g] = v;
  }
  if (hc == 0 && tid == 0) mean_out[((long)z * L + l0 + lc) * P + g] = mred[0];
}

template <typename T, int LC>
void ex_chunk(const T* cov, long M, int m, int B, int P, int L, int l0, const int* group, double* work, long ws, double* mean_out,
              double* cov_out, hipStream_t s) {
  ex_pairs_kernel<T, LC><<<dim3((unsigned)(M / EX_ROWS), (unsigned)P, (unsigned)B), 256, 0, s>>>(cov, M, m, P, L, l0, group, work, ws);
  exceedance_reduce(M, B, P, L, l0, LC, work, mean_out, cov_out, s);
}

__global__ __launch_bounds__(256) void ex_debug_kernel(const double* __restrict__ h, const double* __restrict__ k,
                                                       const double* __restrict__ rho, long count, double* __restrict__ out) {
  ex_tables_init();
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const double hv[1] = {h[i]}, kv[1] = {k[i]}, ph[1] = {ex_phi(hv[0])}, pk[1] = {ex_phi(kv[0])};
  double D[1];
  bvn_excess<1>(hv, kv, ph, pk, rho[i], D);
  out[i] = D[0];
}

}  // namespace

size_t exceedance_moments_workspace_bytes(long m, int P, int L, int B) {
  return sizeof(double) * (size_t)B * (size_t)ex_site_doubles(round_up(m, DGP_TILE_HOST), P, L);
}

template <typename T>
void exceedance_prepare(const T* diag, long dsite, long dstep, long m, int B, const T* mu, const double* thresh, int L, const double* w,
                        const int* group, int P, const T* ev, double* work, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const long ws = ex_site_doubles(M, P, L);
  ex_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P, L);
  ex_prep_kernel<T><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(diag, dsite, dstep, M, (int)m, P, L, mu, thresh, w,
                                                                                    group, ev, work, ws);
}

void exceedance_reduce(long M, int B, int P, int L, int l0, int LC, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  ex_reduce_kernel<<<dim3((unsigned)(((P + 63) / 64) * LC), (unsigned)P, (unsigned)B), 256, 0, s>>>(M, P, L, l0, LC, work,
                                                                                                  ex_site_doubles(M, P, L), mean_out,
                                                                                                  cov_out);
}

// exact mean / covariance of the counts sum_{i in g} w_i 1[f_i > u_il], f ~ N(mu, C), per level l.  thresh [B][L][m] in model
// space; mean_out [B][L][P], cov_out [B][L][P][P]; `work`: exceedance_moments_workspace_bytes
template <typename T>
static int exceedance_moments(const T* cov, long m, int B, const T* mu, const double* thresh, int L, const double* w, const int* group,
                              int P, const T* ev, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const long ws = ex_site_doubles(M, P, L);
  exceedance_prepare<T>(cov, M * M, M + 1, m, B, mu, thresh, L, w, group, P, ev, work, s);
  level_chunks(L, [&](int l0, auto width) {
    ex_chunk<T, decltype(width)::value>(cov, M, (int)m, B, P, L, l0, group, work, ws, mean_out, cov_out, s);
    return 0;
  });
  return (int)hipGetLastError();
}

template void exceedance_prepare<double>(const double*, long, long, long, int, const double*, const double*, int, const double*, const int*,
                                         int, const double*, double*, hipStream_t);
template void exceedance_prepare<float>(const float*, long, long, long, int, const float*, const double*, int, const double*, const int*,
                                        int, const float*, double*, hipStream_t);

// out[i] = Phi2(h_i, k_i; rho_i) - Phi(h_i) Phi(k_i): the pair function of the pass above, pointwise
static int debug_bvn_excess(const double* h, const double* k, const double* rho, long count, double* out, hipStream_t s) {
  ex_debug_kernel<<<dim3((unsigned)((count + 255) / 256)), 256, 0, s>>>(h, k, rho, count, out);
  return (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

extern "C" {

size_t dgp_exceedance_moments_workspace_bytes(int64_t m, int ngroups, int nlevels, int batch) {
  if (!ex_sizes_ok(m, ngroups, nlevels, batch)) return 0;
  return exceedance_moments_workspace_bytes(m, ngroups, nlevels, batch);
}

int dgp_exceedance_moments(int dtype, const void* cov, int64_t m, int batch, const void* mu, const double* thresh, int nlevels,
                           const double* w, const int32_t* group, int ngroups, const void* extra_var, void* work,
                           size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_exceedance_moments: dtype must be 0 (f64) or 1 (f32)");
  if (!cov || !mu || !thresh || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_exceedance_moments: null argument");
  if (!ex_sizes_ok(m, ngroups, nlevels, batch))
    return fail(DGP_E_ARG,
                "dgp_exceedance_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nlevels <= 64, 1 <= batch <= 1024)");
  if (!work || work_bytes < exceedance_moments_workspace_bytes(m, ngroups, nlevels, batch))
    return fail(DGP_E_WORKSPACE, "dgp_exceedance_moments: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64
                     ? exceedance_moments<double>((const double*)cov, m, batch, (const double*)mu, thresh, nlevels, w, group, ngroups,
                                                  (const double*)extra_var, (double*)work, mean_out, cov_out, s)
                     : exceedance_moments<float>((const float*)cov, m, batch, (const float*)mu, thresh, nlevels, w, group, ngroups,
                                                 (const float*)extra_var, (double*)work, mean_out, cov_out, s);
  return wrap(rc, "dgp_exceedance_moments");
}

int dgp_debug_bvn_excess(const double* h, const double* k, const double* rho, int64_t count, double* out, void* stream) {
  if (!h || !k || !rho || !out || count <= 0 || count > (1ll << 31))
    return fail(DGP_E_ARG, "dgp_debug_bvn_excess: null argument / bad count");
  return wrap(debug_bvn_excess(h, k, rho, count, out, (hipStream_t)stream), "dgp_debug_bvn_excess");
}

}  // extern "C"
