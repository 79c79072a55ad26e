// dgp_exceed_stream.hip -- the moments of dgp_exceedance_moments straight from the held factorisation, with the posterior
// covariance C = K(Xs, Xs) - V^T V produced R rows at a time and never stored whole (dgp_posterior_exceedance_moments).
//
// The front end, the panels and their invariants are dgp_stream.h's.  Launches (gridDim.z = sites, one stream, no
// floating-point atomics):
//   init, prep   dgp_exceed.hip's, once; the diagonal is the predicted variance (sigma never comes from the panel)
//   per chunk of levels (8 / 4 / 2 / 1, a function of L alone):
//     zero       Y[l][i][h] = 0 for the levels of the chunk: the reduce pass finds numbers wherever it reads, whatever the work
//                area held before and however many excluded rows a panel has
//     per panel, in ascending order:
//       gram, cov   the panel of C
//       pairs       one workgroup per (64-row block below the panel's end, group h): Y[l][i][h] += sum_j w_j D(z_il, z_jl, rho_ij)
//                   over the j of h that ex_pairs_kernel takes for row i and whose pair (i, j) lies in this panel: for g(i) = h
//                   the j < i, when i is a row of the panel (read as C[i][j]); for g(i) < h the j of h among the panel's rows
//                   (read as C[j][i]).  One workgroup owns an entry of Y in a launch and the launches are ordered: a plain
//                   read-modify-write, every sum in a fixed order.
//     reduce     dgp_exceed.hip's
// Repeated calls are bitwise equal and a site's numbers do not depend on its batch; different R regroup the sums over j.
// The quadrature never runs beside live MFMA accumulators: it reads C back from the panel (L2 / HBM, R M elements).
#include "dgp_bvn.h"
#include "dgp_stream.h"

namespace dgp {

namespace {

__global__ __launch_bounds__(256) void exs_zero_kernel(double* work, long ws, long M, int P, int L, int LC) {
  const ExWork wk(work, ws, M, P, L);
  const long count = (long)LC * M * P;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) wk.Y[i] = 0.0;
}

// levels l0 .. l0 + LC of Y, the pairs of the panel of rows [p0, p1) (row i of C at panel[(i - p0) M]); see the file header
template <typename T, int LC>
__global__ __launch_bounds__(256) void exs_pairs_kernel(const T* __restrict__ panel, long pstride, long M, int m, int P, int L, int l0,
                                                        int p0, int p1, const int* __restrict__ group, double* __restrict__ work,
                                                        long ws) {
  const int rb = blockIdx.x, h = blockIdx.y, z = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ExWork wk(work, ws, M, P, L);
  const int r0 = rb * EX_ROWS;
  int c0, c1;
  ex_range(wk.se, h, c0, c1);
  const int j0 = c0 > p0 ? c0 : p0, j1 = c1 < p1 ? c1 : p1;  // the j of h among the panel's rows
  const bool lowp = r0 >= p0 && r0 < c1 && r0 + EX_ROWS > c0;  // rows of the panel that may lie in h
  const bool upp = j0 < j1 && r0 < c0;                        // rows of earlier groups, and h has rows in the panel
  if (!lowp && !upp) return;
  ex_tables_init();
  __shared__ double low[LC][EX_ROWS], up[4][LC][EX_ROWS];
  const T* C = panel + (long)z * pstride;
  const int* gz = group + (long)z * m;
  const double* zs = wk.z + (long)l0 * M;
  const double* ps = wk.p + (long)l0 * M;
  __syncthreads();

  // g(i) = h, i a row of the panel: the j < i of the group, C[i][j]; a wave per row, lanes along the row
  for (int ii = wave; ii < EX_ROWS; ii += 4) {
    const int i = r0 + ii;
    double acc[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) acc[l] = 0.0;
    if (lowp && i < m && gz[i] == h) {
      const T* row = C + (long)(i - p0) * M;
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

  // 0 <= g(i) < h: the j of the group among the panel's rows (all beyond i), C[j][i]; lanes along i, wave q takes
  // j = j0 + q, j0 + q + 4, ...
  {
    const int i = r0 + lane;
    double acc[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) acc[l] = 0.0;
    const int gi = i < m ? gz[i] : -1;
    if (upp && gi >= 0 && gi < h) {
      const T* col = C + i;
      const double si = wk.sinv[i];
      double zi[LC], pi[LC];
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        zi[l] = zs[(long)l * M + i];
        pi[l] = ps[(long)l * M + i];
      }
      for (int j = j0 + wave; j < j1; j += 4) {
        double zj[LC], pj[LC], D[LC];
#pragma unroll
        for (int l = 0; l < LC; ++l) {
          zj[l] = zs[(long)l * M + j];
          pj[l] = ps[(long)l * M + j];
        }
        bvn_excess<LC>(zi, zj, pi, pj, (double)col[(long)(j - p0) * M] * si * wk.sinv[j], D);
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
      wk.Y[((long)l * M + r0 + tid) * P + h] += low[l][tid] + ((up[0][l][tid] + up[1][l][tid]) + (up[2][l][tid] + up[3][l][tid]));
}

template <typename T, int LC>
int exs_chunk(const Posterior<T>& ps, long R, T* panel, long pstride, int P, int L, int l0, const int* group, double* work, long ws,
              double* mean_out, double* cov_out) {
  const long M = ps.M;
  const int B = ps.p->B;
  hipStream_t s = ps.s;
  const long count = (long)LC * M * P;
  const long zb = (count + 255) / 256;
  exs_zero_kernel<<<dim3((unsigned)(zb < 65536 ? zb : 65536), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P, L, LC);
  const int rc = ps.panels(R, panel, pstride, [&](long p0, long p1) {
    exs_pairs_kernel<T, LC><<<dim3((unsigned)(p1 / EX_ROWS), (unsigned)P, (unsigned)B), 256, 0, s>>>(panel, pstride, M, (int)ps.m, P, L, l0,
                                                                                                   (int)p0, (int)p1, group, work, ws);
  });
  if (rc) return rc;
  exceedance_reduce(M, B, P, L, l0, LC, work, mean_out, cov_out, s);
  return (int)hipGetLastError();
}

}  // namespace

// The exceedance moments with C produced R rows at a time into `panel` (site stride pstride) and never stored whole; every
// chunk of levels produces all panels again.  `work` as for exceedance_moments
template <typename T>
static int posterior_exceedance_moments(const Posterior<T>& ps, const T* mu, const double* thresh, int L, const double* w,
                                        const int* group, int P, const T* ev, long R, T* panel, long pstride, double* work,
                                        double* mean_out, double* cov_out) {
  const long ws = (long)(exceedance_moments_workspace_bytes(ps.m, P, L, 1) / sizeof(double));
  exceedance_prepare<T>(ps.var, ps.wbs, 1, ps.m, ps.p->B, mu, thresh, L, w, group, P, ev, work, ps.s);
  if (int rc = ps.zero_noise()) return rc;
  const int rc = level_chunks(L, [&](int l0, auto width) {
    return exs_chunk<T, decltype(width)::value>(ps, R, panel, pstride, P, L, l0, group, work, ws, mean_out, cov_out);
  });
  return rc ? rc : (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

// streamed exceedance moments: dgp_stream.h's areas with one covariance panel of R x M elements per site, then the moment pass's
// work area
static size_t exceed_panel_bytes(const dgp_plan* p, int64_t m, int panel_rows) {
  return panel_bytes(p, m, panel_rows, round_up(m, DGP_TILE_HOST));
}
template <typename T>
static int post_exceed(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* thresh, int L,
                       const double* w, const int32_t* group, int P, const void* ev, int panel_rows, void* work, double* mean_out,
                       double* cov_out, hipStream_t s) {
  const PosteriorAreas<T> A = posterior_areas<T>(p, m, work, exceed_panel_bytes(p, m, panel_rows));
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, A.own, s)) return rc;
  return posterior_exceedance_moments<T>(ps, (const T*)mu, thresh, L, w, group, P, (const T*)ev, panel_rows, A.panel, A.pstride,
                                         (double*)A.own, mean_out, cov_out);
}

extern "C" {

size_t dgp_posterior_exceedance_moments_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups, int nlevels, int panel_rows) {
  if (!p || !ex_sizes_ok(m, ngroups, nlevels, p->B) || !panel_rows_ok(panel_rows)) return 0;
  return posterior_head_bytes(p, m, exceed_panel_bytes(p, m, panel_rows)) + exceedance_moments_workspace_bytes(m, ngroups, nlevels, p->B);
}

int dgp_posterior_exceedance_moments(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* thresh,
                                     int nlevels, const double* w, const int32_t* group, int ngroups, const void* extra_var,
                                     int panel_rows, void* work, size_t work_bytes, double* mean_out, double* cov_out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !mu || !thresh || !w || !group || !mean_out || !cov_out)
    return fail(DGP_E_ARG, "dgp_posterior_exceedance_moments: null argument");
  if (!ex_sizes_ok(m, ngroups, nlevels, p->B))
    return fail(DGP_E_ARG, "dgp_posterior_exceedance_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nlevels <= 64)");
  if (!panel_rows_ok(panel_rows))
    return fail(DGP_E_ARG, "dgp_posterior_exceedance_moments: panel_rows must be a positive multiple of 128");
  return posterior_entry(p, "dgp_posterior_exceedance_moments", work, work_bytes,
                         dgp_posterior_exceedance_moments_workspace_bytes(p, m, ngroups, nlevels, panel_rows), stream,
                         [&](auto t, hipStream_t s) {
                           return post_exceed<decltype(t)>(p, theta, Xs, m, mu, thresh, nlevels, w, group, ngroups, extra_var, panel_rows, work,
                                                           mean_out, cov_out, s);
                         });
}

}  // extern "C"
