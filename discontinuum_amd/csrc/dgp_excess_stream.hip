// dgp_excess_stream.hip -- the moments of dgp_excess_moments straight from the held factorisation, with the posterior covariance
// C = K(Xs, Xs) - V^T V produced R rows at a time and never stored whole (dgp_posterior_excess_moments).
//
// The front end, the panels and their invariants are dgp_stream.h's.  Launches (gridDim.z = sites, one stream, no
// floating-point atomics):
//   init, prep   dgp_excess.hip's, once; the diagonal is the predicted variance (sigma never comes from the panel)
//   per group of up to 8 levels (a function of L alone):
//     zero       Y[l][i][h] = 0 for the levels of the group: the reduce pass finds numbers wherever it reads, whatever the work
//                area held before and however many excluded rows a panel has
//     per panel, in ascending order:
//       gram, cov   the panel of C, ONCE for the group
//       pairs       2 levels per launch (one for an odd last level: the pair function's registers, as in the dense pass), every
//                   launch of the group against the same panel; one workgroup per (64-row block below the panel's end, group h):
//                   Y[l][i][h] += sum_j W_j n_ij over the j of h that xs_pairs_kernel takes for row i and whose pair (i, j) lies
//                   in this panel: for g(i) = h the j < i, when i is a row of the panel (read as C[i][j]); for g(i) < h the j of
//                   h among the panel's rows (read as C[j][i]).  One workgroup owns an entry of Y in a launch and the launches
//                   are ordered: a plain read-modify-write, every sum in a fixed order.
//     reduce     dgp_excess.hip's, on the group's levels of Y
// Repeated calls are bitwise equal and a site's numbers do not depend on its batch; different R regroup the sums over j.
#include "dgp_excess.h"
#include "dgp_stream.h"

namespace dgp {

namespace {

__global__ __launch_bounds__(256) void xss_zero_kernel(double* work, long ws, long M, int P, int L, int GL) {
  const XsWork wk(work, ws, M, P, L, XS_GROUP);
  const long count = (long)GL * M * P;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) wk.Y[i] = 0.0;
}

// levels l0 .. l0 + LV (y0 .. y0 + LV of Y), the pairs of the panel of rows [p0, p1) (row i of C at panel[(i - p0) M]); see the
// file header
template <typename T, int LV>
__global__ __launch_bounds__(256) void xss_pairs_kernel(const T* __restrict__ panel, long pstride, long M, int m, int P, int L, int l0,
                                                        int y0, int p0, int p1, const double* __restrict__ scale2,
                                                        const int* __restrict__ group, double sg, double* __restrict__ work,
                                                        long ws) {
  const int rb = blockIdx.x, h = blockIdx.y, z = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const XsWork wk(work, ws, M, P, L, XS_GROUP);
  const int r0 = rb * EX_ROWS;
  int c0, c1;
  ex_range(wk.se, h, c0, c1);
  const int j0 = c0 > p0 ? c0 : p0, j1 = c1 < p1 ? c1 : p1;  // the j of h among the panel's rows
  const bool lowp = r0 >= p0 && r0 < c1 && r0 + EX_ROWS > c0;  // rows of the panel that may lie in h
  const bool upp = j0 < j1 && r0 < c0;                        // rows of earlier groups, and h has rows in the panel
  if (!lowp && !upp) return;
  ex_tables_init();
  __shared__ double low[LV][EX_ROWS], up[4][LV][EX_ROWS];
  const T* C = panel + (long)z * pstride;
  const int* gz = group + (long)z * m;
  const double s2 = scale2[z];
  __syncthreads();

  // g(i) = h, i a row of the panel: the j < i of the group, C[i][j]; a wave per row, lanes along the row
  for (int ii = wave; ii < EX_ROWS; ii += 4) {
    const int i = r0 + ii;
    double acc[LV];
#pragma unroll
    for (int l = 0; l < LV; ++l) acc[l] = 0.0;
    if (lowp && i < m && gz[i] == h) {
      const T* row = C + (long)(i - p0) * M;
      XsPoint<LV> pi;
      pi.load(wk, M, l0, i);
      for (int j = c0 + lane; j < i; j += 64) {
        XsPoint<LV> pj;
        pj.load(wk, M, l0, j);
        double n[LV];
        xs_pair<LV>(sg, pi, pj, (double)row[j] * s2, n);
        const double Wj = wk.W[j];
#pragma unroll
        for (int l = 0; l < LV; ++l) acc[l] = __builtin_fma(Wj, n[l], acc[l]);
      }
    }
#pragma unroll
    for (int l = 0; l < LV; ++l) {
      const double v = ex_wave_sum(acc[l]);
      if (lane == 0) low[l][ii] = v;
    }
  }

  // 0 <= g(i) < h: the j of the group among the panel's rows (all beyond i), C[j][i]; lanes along i, wave q takes
  // j = j0 + q, j0 + q + 4, ...
  {
    const int i = r0 + lane;
    double acc[LV];
#pragma unroll
    for (int l = 0; l < LV; ++l) acc[l] = 0.0;
    const int gi = i < m ? gz[i] : -1;
    if (upp && gi >= 0 && gi < h) {
      const T* col = C + i;
      XsPoint<LV> pi;
      pi.load(wk, M, l0, i);
      for (int j = j0 + wave; j < j1; j += 4) {
        XsPoint<LV> pj;
        pj.load(wk, M, l0, j);
        double n[LV];
        xs_pair<LV>(sg, pi, pj, (double)col[(long)(j - p0) * M] * s2, n);
        const double Wj = wk.W[j];
#pragma unroll
        for (int l = 0; l < LV; ++l) acc[l] = __builtin_fma(Wj, n[l], acc[l]);
      }
    }
#pragma unroll
    for (int l = 0; l < LV; ++l) up[wave][l][lane] = acc[l];
  }
  __syncthreads();
  if (tid < EX_ROWS)
#pragma unroll
    for (int l = 0; l < LV; ++l)
      wk.Y[((long)(y0 + l) * M + r0 + tid) * P + h] += low[l][tid] + ((up[0][l][tid] + up[1][l][tid]) + (up[2][l][tid] + up[3][l][tid]));
}

// the levels g0 .. g0 + GL (GL <= XS_GROUP) of the call: every panel once, the 2-level and 1-level pair launches against it
template <typename T>
int xss_group(const Posterior<T>& ps, long R, T* panel, long pstride, int P, int L, int g0, int GL, const double* scale2, const int* group,
              double sg, double* work, long ws, double* mean_out, double* cov_out, double* total_out) {
  const long M = ps.M;
  const int B = ps.p->B, m = (int)ps.m;
  hipStream_t s = ps.s;
  const long count = (long)GL * M * P;
  const long zb = (count + 255) / 256;
  xss_zero_kernel<<<dim3((unsigned)(zb < 65536 ? zb : 65536), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P, L, GL);
  const int rc = ps.panels(R, panel, pstride, [&](long p0, long p1) {
    const dim3 grid((unsigned)(p1 / EX_ROWS), (unsigned)P, (unsigned)B);
    for (int y0 = 0; y0 < GL;) {
      if (GL - y0 >= 2) {
        xss_pairs_kernel<T, 2><<<grid, 256, 0, s>>>(panel, pstride, M, m, P, L, g0 + y0, y0, (int)p0, (int)p1, scale2, group, sg, work, ws);
        y0 += 2;
      } else {
        xss_pairs_kernel<T, 1><<<grid, 256, 0, s>>>(panel, pstride, M, m, P, L, g0 + y0, y0, (int)p0, (int)p1, scale2, group, sg, work, ws);
        y0 += 1;
      }
    }
  });
  if (rc) return rc;
  excess_reduce(M, B, P, L, g0, GL, XS_GROUP, work, mean_out, cov_out, total_out, s);
  return (int)hipGetLastError();
}

}  // namespace

// The excess moments with C produced R rows at a time into `panel` (site stride pstride) and never stored whole; every group of
// levels produces all panels once.  `work`: excess_moments_workspace_bytes with XS_GROUP
template <typename T>
static int posterior_excess_moments(const Posterior<T>& ps, const T* mu, const double* scale2, const double* thresh, int L,
                                    const double* w, const int* group, int P, const T* ev, int above, long R, T* panel, long pstride,
                                    double* work, double* mean_out, double* cov_out, double* total_out) {
  const long ws = xs_site_doubles(ps.M, P, L, XS_GROUP);
  const double sg = above ? 1.0 : -1.0;
  excess_prepare<T>(ps.var, ps.wbs, 1, ps.m, ps.p->B, mu, scale2, thresh, L, w, group, P, ev, sg, XS_GROUP, work, ps.s);
  if (int rc = ps.zero_noise()) return rc;
  int rc = 0;
  for (int g0 = 0; g0 < L && !rc; g0 += XS_GROUP)
    rc = xss_group<T>(ps, R, panel, pstride, P, L, g0, L - g0 < XS_GROUP ? L - g0 : XS_GROUP, scale2, group, sg, work, ws, mean_out,
                      cov_out, total_out);
  return rc ? rc : (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

// streamed excess moments: dgp_stream.h's areas with one covariance panel of R x M elements per site, then the moment pass's
// work area
static size_t excess_panel_bytes(const dgp_plan* p, int64_t m, int panel_rows) {
  return panel_bytes(p, m, panel_rows, round_up(m, DGP_TILE_HOST));
}
template <typename T>
static int post_excess(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* scale2,
                       const double* thresh, int L, const double* w, const int32_t* group, int P, const void* ev, int above,
                       int panel_rows, void* work, double* mean_out, double* cov_out, double* total_out, hipStream_t s) {
  const PosteriorAreas<T> A = posterior_areas<T>(p, m, work, excess_panel_bytes(p, m, panel_rows));
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, A.own, s)) return rc;
  return posterior_excess_moments<T>(ps, (const T*)mu, scale2, thresh, L, w, group, P, (const T*)ev, above, panel_rows, A.panel, A.pstride,
                                     (double*)A.own, mean_out, cov_out, total_out);
}

extern "C" {

size_t dgp_posterior_excess_moments_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups, int nlevels, int panel_rows) {
  if (!p || !ex_sizes_ok(m, ngroups, nlevels, p->B) || !panel_rows_ok(panel_rows)) return 0;
  return posterior_head_bytes(p, m, excess_panel_bytes(p, m, panel_rows)) +
         excess_moments_workspace_bytes(m, ngroups, nlevels, p->B, XS_GROUP);
}

int dgp_posterior_excess_moments(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* scale2,
                                 const double* thresh, int nlevels, const double* w, const int32_t* group, int ngroups,
                                 const void* extra_var, int above, int panel_rows, void* work, size_t work_bytes, double* mean_out,
                                 double* cov_out, double* total_out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !mu || !scale2 || !thresh || !w || !group || !mean_out || !cov_out || !total_out)
    return fail(DGP_E_ARG, "dgp_posterior_excess_moments: null argument");
  if (!ex_sizes_ok(m, ngroups, nlevels, p->B))
    return fail(DGP_E_ARG, "dgp_posterior_excess_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nlevels <= 64)");
  if (!panel_rows_ok(panel_rows))
    return fail(DGP_E_ARG, "dgp_posterior_excess_moments: panel_rows must be a positive multiple of 128");
  if (above != 0 && above != 1) return fail(DGP_E_ARG, "dgp_posterior_excess_moments: above must be 0 (deficit) or 1 (excess)");
  return posterior_entry(p, "dgp_posterior_excess_moments", work, work_bytes,
                         dgp_posterior_excess_moments_workspace_bytes(p, m, ngroups, nlevels, panel_rows), stream,
                         [&](auto t, hipStream_t s) {
                           return post_excess<decltype(t)>(p, theta, Xs, m, mu, scale2, thresh, nlevels, w, group, ngroups, extra_var, above,
                                                           panel_rows, work, mean_out, cov_out, total_out, s);
                         });
}

}  // extern "C"
