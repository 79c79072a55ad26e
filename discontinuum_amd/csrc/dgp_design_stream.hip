// dgp_design_stream.hip -- dgp_sample_value's gain map straight from the held factorisation, with the posterior covariance
// C = K(Xs, Xs) - V^T V produced R rows at a time and never stored whole (dgp_posterior_sample_value), and single columns of C
// for the host's conditioning rows (dgp_posterior_cov_columns).
//
// The front end, the panels and their invariants are dgp_stream.h's.  Notation of dgp_design.hip.  The power sums S[p][k][c] = sum_{i in p} A_i b_ic^k
// live in the work area, [P][K][M] doubles per site.  Every ORDERED pair (day i, candidate c) is counted exactly once:
//   i >= c   in the panel that holds row i, read as C[i][c] (row segments, coalesced)
//   i <  c   in the panel that holds row c, read as C[c][i] (transposed on the way into LDS, as sv_sums_kernel does it)
// so a block of 64 candidates takes, from a panel, the panel's rows at or after the block and -- when the block's own rows lie
// in the panel -- also every day before it.  The diagonal entry is the predicted variance, never the panel's.  Launches
// (gridDim.z = sites, one stream, no floating-point atomics):
//   init     S = 0, the groups' day ranges reset: whatever the work area held before does not matter
//   prep     one thread per point: the predicted variance (kept in double), v'_c -> var_out, 1 / sqrt(v'_c), the day ranges
//   per panel, in ascending order:
//     gram, cov   the panel of C
//     sums        one workgroup of four waves per (64 candidates below the panel's end, group p): lanes own candidates, the waves
//                 take the tiles of 16 days in turn, each with dgp_design.hip's staging, on-the-fly subtraction of the
//                 conditioning rows and register-resident power sums; the four waves' sums are added in a fixed order and the
//                 workgroup -- the only owner of its entries of S in the launch -- adds them to S by a plain read-modify-write
//   fold     gain[p][c] = sum_k (s^2)^k / k! S[p][k][c]^2
// Repeated calls are bitwise equal and a site's numbers do not depend on its batch; different R regroup the sums over the days.
#include <climits>

#include "dgp_design.h"
#include "dgp_stream.h"

namespace dgp {

namespace {

constexpr int SVS_WAVES = 4;

// per-site work area, in doubles: 1 / sqrt(v') [M], the predicted variance [M], S [P][K][M], then 2 P ints (group start / end)
__host__ __device__ inline long svs_site_doubles(long M, int P, int K) { return 2 * M + (long)P * K * M + P; }

__global__ __launch_bounds__(256) void svs_init_kernel(double* work, long ws, long M, int P, int K) {
  double* base = work + (long)blockIdx.z * ws;
  double* S = base + 2 * M;
  const long count = (long)P * K * M;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) S[i] = 0.0;
  if (blockIdx.x == 0) {
    int* se = (int*)(base + ws - P);
    for (int g = threadIdx.x; g < P; g += 256) {
      se[2 * g] = INT_MAX;
      se[2 * g + 1] = 0;
    }
  }
}

// var: the predicted variance as the prediction leaves it (site stride vstride elements)
template <typename T>
__global__ __launch_bounds__(256) void svs_prep_kernel(const T* __restrict__ var, long vstride, long M, int m, int P,
                                                       const int* __restrict__ group, const T* __restrict__ ov,
                                                       const double* __restrict__ rows, int nrows, double* work, long ws,
                                                       double* __restrict__ var_out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  double* rs = work + (long)z * ws;
  double* dg = rs + M;
  int* se = (int*)(rs + ws - P);
  double r = 0.0, d = 0.0;
  if (j < m) {
    const long k = (long)z * m + j;
    const int g = group[k];
    if (g >= 0 && g < P) {
      atomicMin(&se[2 * g], (int)j);
      atomicMax(&se[2 * g + 1], (int)j + 1);
    }
    double v = (double)var[(long)z * vstride + j];
    d = v;
    for (int t = 0; t < nrows; ++t) {
      const double b = rows[((long)z * nrows + t) * m + j];
      v -= b * b;
    }
    if (ov) v += (double)ov[k];
    sv_inv_sd(v, r);
    var_out[k] = v;
  }
  rs[j] = r;
  dg[j] = d;
}

// the pairs (day i, candidate c) of the panel of rows [p0, p1) (row i of C at panel[(i - p0) M]); see the file header
template <typename T, int KT>
__global__ __launch_bounds__(64 * SVS_WAVES) void svs_sums_kernel(const T* __restrict__ panel, long pstride, long M, int m, int P, int K,
                                                                  int p0, int p1, const double* __restrict__ a,
                                                                  const int* __restrict__ group, const double* __restrict__ rows,
                                                                  int nrows, double* __restrict__ work, long ws) {
  const int cb = blockIdx.x, p = blockIdx.y, z = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = cb * SV_CAND, c = c0 + lane;
  double* base = work + (long)z * ws;
  const int* se = (const int*)(base + ws - P);
  const int g0 = se[2 * p], g1 = se[2 * p + 1];
  if (g1 <= g0) return;  // empty group (start still INT_MAX)
  const bool own = c0 >= p0;  // the block's own rows lie in the panel (c0 + 63 < p1 by the grid)
  const int dlo = own ? g0 : (g0 > p0 ? g0 : p0);
  const int dhi = g1 < p1 ? g1 : p1;
  if (dlo >= dhi) return;
  const T* C = panel + (long)z * pstride;
  const double* az = a + (long)z * m;
  const int* gz = group + (long)z * m;
  const double* bz = rows + (long)z * nrows * m;  // (never read when nrows == 0)
  extern __shared__ __attribute__((aligned(16))) char svs_smem[];
  double* tiles = (double*)svs_smem;                    // [SVS_WAVES][SV_DAYS][SV_LD]: each wave's C' of (day i0 + u, candidate c0 + lane)
  double* bc = tiles + SVS_WAVES * SV_DAYS * SV_LD;     // [nrows][SV_CAND]: B[t][c0 + lane]
  double* tile = tiles + wave * SV_DAYS * SV_LD;

  const double rs = base[c], dgc = base[M + c];
  for (int t = wave; t < nrows; t += SVS_WAVES) bc[t * SV_CAND + lane] = c < m ? bz[(long)t * m + c] : 0.0;
  double S[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) S[k] = 0.0;

  const int t0 = dlo / SV_DAYS * SV_DAYS;
  const int ntiles = (dhi - t0 + SV_DAYS - 1) / SV_DAYS;
  for (int n = 0; n < ntiles; n += SVS_WAVES) {  // the same trip count for every wave: the barriers below are the workgroup's
    const int i0 = t0 + (n + wave) * SV_DAYS;
    const bool live = i0 < dhi;                                  // wave-uniform
    const bool from_rows = live && i0 + SV_DAYS - 1 >= c0;       // some day i >= some candidate c: C[i][c], i a row of the panel
    const bool from_cols = live && own && i0 < c0 + SV_CAND - 1;  // some day i < some candidate c: C[c][i], c a row of the panel
    // the tile's days: group id and A_i in lanes 0 .. 15 (-2: not a day this workgroup takes from this panel)
    int gl = -2;
    double al = 0.0;
    if (live && lane < SV_DAYS && i0 + lane >= dlo && i0 + lane < dhi) {
      gl = gz[i0 + lane];
      al = az[i0 + lane];
    }
    __syncthreads();  // the previous tile's reads are done (first trip: bc is written)
    if (from_rows) {
      T rv[SV_DAYS];
#pragma unroll
      for (int u = 0; u < SV_DAYS; ++u) {
        rv[u] = T(0);
        if (__builtin_amdgcn_readlane(gl, u) == p && c <= i0 + u) rv[u] = C[(long)(i0 + u - p0) * M + c];
      }
#pragma unroll
      for (int u = 0; u < SV_DAYS; ++u)
        if (c <= i0 + u) tile[u * SV_LD + lane] = c == i0 + u ? dgc : (double)rv[u];  // the diagonal: the predicted variance
    }
    if (from_cols) {
      const int col = lane & (SV_DAYS - 1), r0 = lane / SV_DAYS;
      constexpr int RSTEP = SV_CAND / SV_DAYS, NLOAD = SV_CAND / RSTEP;
      T tv[NLOAD];
#pragma unroll
      for (int j = 0; j < NLOAD; ++j) tv[j] = C[(long)(c0 + r0 + RSTEP * j - p0) * M + i0 + col];
#pragma unroll
      for (int j = 0; j < NLOAD; ++j)
        if (c0 + r0 + RSTEP * j > i0 + col) tile[col * SV_LD + r0 + RSTEP * j] = (double)tv[j];
    }
    __syncthreads();
    if (live) {
      if (nrows > 0) {
        // C' = C - B^T B for the tile, exactly as in sv_sums_kernel
        double x[SV_DAYS];
#pragma unroll
        for (int u = 0; u < SV_DAYS; ++u) x[u] = tile[u * SV_LD + lane];
        const bool whole = i0 + SV_DAYS <= m;
        for (int t = 0; t < nrows; ++t) {
          const double bcv = bc[t * SV_CAND + lane];
          const double* br = bz + (long)t * m + i0;
#pragma unroll
          for (int u = 0; u < SV_DAYS; ++u) x[u] -= (whole || i0 + u < m ? br[u] : 0.0) * bcv;
        }
#pragma unroll
        for (int u = 0; u < SV_DAYS; ++u) tile[u * SV_LD + lane] = x[u];  // (this lane's own column: no barrier)
      }
#pragma unroll 1
      for (int u = 0; u < SV_DAYS; ++u) {
        if (__builtin_amdgcn_readlane(gl, u) != p) continue;  // wave-uniform
        const double b = tile[u * SV_LD + lane] * rs;
        sv_add_day<KT>(S, K, sv_readlane(al, u), b);
      }
    }
  }

  // the four waves' sums in a fixed order, KC terms at a time through the tiles' LDS, then S += them
  constexpr int KC = KT < 16 ? KT : 16;
  static_assert((SVS_WAVES - 1) * KC * SV_CAND <= SVS_WAVES * SV_DAYS * SV_LD, "the fold's staging must fit the tiles");
  double* red = tiles;  // [SVS_WAVES - 1][KC][SV_CAND]
  double* Sg = base + 2 * M + (long)p * K * M + c;
#pragma unroll
  for (int k0 = 0; k0 < KT; k0 += KC) {
    if (k0 < K) {  // workgroup-uniform
      __syncthreads();
      if (wave > 0) {
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) red[((wave - 1) * KC + kk) * SV_CAND + lane] = S[k0 + kk];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
          if (k0 + kk < K) {
            const double v = ((S[k0 + kk] + red[kk * SV_CAND + lane]) + red[(KC + kk) * SV_CAND + lane]) + red[(2 * KC + kk) * SV_CAND + lane];
            Sg[(long)(k0 + kk) * M] += v;
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void svs_fold_kernel(long M, int m, int P, int K, const double* __restrict__ scale2,
                                                       const double* __restrict__ work, long ws, double* __restrict__ gain_out) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y, z = blockIdx.z;
  if (c >= m) return;
  const double* Sg = work + (long)z * ws + 2 * M + (long)p * K * M + c;
  const double s2 = scale2[z];
  double coef = 1.0, gain = 0.0;
  for (int k = 0; k < K; ++k) {
    const double s = Sg[(long)k * M];
    coef *= s2 / (double)(k + 1);
    gain += coef * (s * s);
  }
  gain_out[((long)z * P + p) * m + c] = gain;
}

template <typename T, int KT>
void svs_launch_sums(const T* panel, long pstride, long M, int m, int B, int P, int K, int p0, int p1, const double* a, const int* group,
                     const double* rows, int nrows, double* work, long ws, hipStream_t s) {
  const size_t lds = (SVS_WAVES * SV_DAYS * SV_LD + (size_t)nrows * SV_CAND) * sizeof(double);
  if (lds > 64 * 1024)  // 64 rows: 512 bytes past the default limit; the opt-in belongs to the current device's function object
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&svs_sums_kernel<T, KT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((SVS_WAVES * SV_DAYS * SV_LD + 64 * SV_CAND) * sizeof(double)));
  svs_sums_kernel<T, KT><<<dim3((unsigned)(p1 / SV_CAND), (unsigned)P, (unsigned)B), 64 * SVS_WAVES, lds, s>>>(
      panel, pstride, M, m, P, K, p0, p1, a, group, rows, nrows, work, ws);
}

// the columns idx[t] of the test points, SoA with leading dimension DGP_TILE_HOST: the "training points" of a cross Gram
template <typename T>
__global__ __launch_bounds__(DGP_TILE_HOST) void cc_gather_kernel(const T* __restrict__ Xst, long wbs, long M, int m, int d,
                                                                  const int* __restrict__ idx, int ncols, T* __restrict__ Xc,
                                                                  long xstride) {
  const int t = threadIdx.x, z = blockIdx.z;
  int src = idx[(long)z * ncols + (t < ncols ? t : 0)];
  src = src < 0 ? 0 : (src >= m ? m - 1 : src);
  for (int k = 0; k < d; ++k) Xc[(long)z * xstride + (long)k * DGP_TILE_HOST + t] = Xst[(long)z * wbs + (long)k * M + src];
}

// out[t][i] = k(x_i, x_c) - sum_n V[n][i] V[n][c], c = idx[t]: one thread per point i, the sum in double in ascending n
template <typename T>
__global__ __launch_bounds__(256) void cc_cols_kernel(const T* __restrict__ Kc, const T* __restrict__ V, long N, long M, int m,
                                                      const int* __restrict__ idx, int ncols, long wbs, double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y, z = blockIdx.z;
  if (i >= m) return;
  int c = idx[(long)z * ncols + t];
  c = c < 0 ? 0 : (c >= m ? m - 1 : c);
  const T* Vz = V + (long)z * wbs;
  double acc = 0.0;
  for (long n = 0; n < N; ++n) acc = __builtin_fma((double)Vz[n * M + i], (double)Vz[n * M + c], acc);
  out[((long)z * ncols + t) * m + i] = (double)Kc[(long)z * wbs + (long)t * M + i] - acc;
}

}  // namespace

// The gain map with C produced R rows at a time into `panel` (site stride pstride) and never stored whole.  `work`:
// svs_site_doubles per site
template <typename T>
static int posterior_sample_value(const Posterior<T>& ps, const double* a, const double* scale2, const int* group, int P, const T* ov,
                                  const double* rows, int nrows, int K, long R, T* panel, long pstride, double* work, double* gain_out,
                                  double* var_out) {
  static_assert(SVS_WAVES * SV_DAYS * SV_LD * sizeof(double) % 16 == 0, "the LDS carve offsets must stay 16-byte aligned");
  const long M = ps.M, m = ps.m;
  const long ws = svs_site_doubles(M, P, K);
  const int mi = (int)m, B = ps.p->B;
  hipStream_t s = ps.s;
  const long count = (long)P * K * M, zb = (count + 255) / 256;
  svs_init_kernel<<<dim3((unsigned)(zb < 65536 ? zb : 65536), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P, K);
  svs_prep_kernel<T><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(ps.var, ps.wbs, M, mi, P, group, ov, rows, nrows, work,
                                                                                     ws, var_out);
  if (int rc = ps.zero_noise()) return rc;
  const int rc = ps.panels(R, panel, pstride, [&](long p0, long p1) {
    if (K <= 4)
      svs_launch_sums<T, 4>(panel, pstride, M, mi, B, P, K, (int)p0, (int)p1, a, group, rows, nrows, work, ws, s);
    else if (K <= 16)
      svs_launch_sums<T, 16>(panel, pstride, M, mi, B, P, K, (int)p0, (int)p1, a, group, rows, nrows, work, ws, s);
    else if (K <= 32)
      svs_launch_sums<T, 32>(panel, pstride, M, mi, B, P, K, (int)p0, (int)p1, a, group, rows, nrows, work, ws, s);
    else
      svs_launch_sums<T, 64>(panel, pstride, M, mi, B, P, K, (int)p0, (int)p1, a, group, rows, nrows, work, ws, s);
  });
  if (rc) return rc;
  svs_fold_kernel<<<dim3((unsigned)((m + 255) / 256), (unsigned)P, (unsigned)B), 256, 0, s>>>(M, mi, P, K, scale2, work, ws, gain_out);
  return (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

static bool svs_sizes_ok(const dgp_plan* p, int64_t m, int ngroups, int nrows, int nterms, int panel_rows) {
  return p && m > 0 && m <= (1 << 20) && ngroups > 0 && ngroups <= 65535 && nrows >= 0 && nrows <= 64 && nterms >= 1 && nterms <= 64 &&
         panel_rows_ok(panel_rows);
}

// streamed gain map: dgp_stream.h's areas with one covariance panel of R x M elements per site, then the pass's own area
static size_t svs_panel_bytes(const dgp_plan* p, int64_t m, int panel_rows) {
  return panel_bytes(p, m, panel_rows, round_up(m, DGP_TILE_HOST));
}
template <typename T>
static int post_sample_value(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const double* a, const double* scale2,
                             const int32_t* group, int P, const void* ov, const double* rows, int nrows, int K, int panel_rows, void* work,
                             double* gain_out, double* var_out, hipStream_t s) {
  const PosteriorAreas<T> A = posterior_areas<T>(p, m, work, svs_panel_bytes(p, m, panel_rows));
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, A.own, s)) return rc;
  return posterior_sample_value<T>(ps, a, scale2, group, P, (const T*)ov, rows, nrows, K, panel_rows, A.panel, A.pstride, (double*)A.own,
                                   gain_out, var_out);
}

// columns of C: dgp_stream.h's areas (K(X, Xs)'s place, free once V is formed, takes the columns' cross Gram) with the gathered
// points (d x 128) per site, then the latent mean the prediction also writes
static size_t cc_points_bytes(const dgp_plan* p) { return Carve::up(p->elem * (size_t)DGP_TILE_HOST * (size_t)p->d); }
template <typename T>
static int post_cov_columns(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int32_t* idx, int ncols, void* work,
                            double* out, hipStream_t s) {
  const PosteriorAreas<T> A = posterior_areas<T>(p, m, work, cc_points_bytes(p));
  T* Xc = A.panel;
  T* Kc = (T*)((char*)work + predict_layout(p, m).Ks);
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, A.own, s)) return rc;
  const long M = ps.M, wbs = ps.wbs;
  cc_gather_kernel<T><<<dim3(1, 1, (unsigned)p->B), DGP_TILE_HOST, 0, s>>>(ps.Xst, wbs, M, (int)m, p->d, idx, ncols, Xc, A.pstride);
  Batch bt;
  bt.B = p->B;
  bt.ws = A.pstride;
  if (int rc = gram_cross<T>(p->model, p->d, Xc, DGP_TILE_HOST, ncols, ps.Xst, M, (int)m, theta, Kc, s, bt, wbs, p->pre, nullptr)) return rc;
  cc_cols_kernel<T><<<dim3((unsigned)((m + 255) / 256), (unsigned)ncols, (unsigned)p->B), 256, 0, s>>>(Kc, ps.V, p->N, M, (int)m, idx, ncols, wbs,
                                                                                                    out);
  return (int)hipGetLastError();
}

extern "C" {

size_t dgp_posterior_sample_value_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups, int nrows, int nterms, int panel_rows) {
  if (!svs_sizes_ok(p, m, ngroups, nrows, nterms, panel_rows)) return 0;
  return posterior_head_bytes(p, m, svs_panel_bytes(p, m, panel_rows)) +
         sizeof(double) * (size_t)p->B * (size_t)svs_site_doubles(round_up(m, DGP_TILE_HOST), ngroups, nterms);
}

int dgp_posterior_sample_value(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const double* a, const double* scale2,
                               const int32_t* group, int ngroups, const void* obs_var, const double* rows, int nrows, int nterms,
                               int panel_rows, void* work, size_t work_bytes, double* gain_out, double* var_out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !a || !scale2 || !group || !gain_out || !var_out) return fail(DGP_E_ARG, "dgp_posterior_sample_value: null argument");
  if (!svs_sizes_ok(p, m, ngroups, nrows, nterms, DGP_TILE_HOST))
    return fail(DGP_E_ARG,
                "dgp_posterior_sample_value: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 0 <= nrows <= 64, 1 <= nterms <= 64)");
  if (!panel_rows_ok(panel_rows))
    return fail(DGP_E_ARG, "dgp_posterior_sample_value: panel_rows must be a positive multiple of 128");
  if (nrows > 0 && !rows) return fail(DGP_E_ARG, "dgp_posterior_sample_value: null argument (rows with nrows > 0)");
  return posterior_entry(p, "dgp_posterior_sample_value", work, work_bytes,
                         dgp_posterior_sample_value_workspace_bytes(p, m, ngroups, nrows, nterms, panel_rows), stream,
                         [&](auto t, hipStream_t s) {
                           return post_sample_value<decltype(t)>(p, theta, Xs, m, a, scale2, group, ngroups, obs_var, rows, nrows, nterms,
                                                                 panel_rows, work, gain_out, var_out, s);
                         });
}

size_t dgp_posterior_cov_columns_workspace_bytes(const dgp_plan* p, int64_t m, int ncols) {
  if (!p || m <= 0 || m > (1 << 20) || ncols < 1 || ncols > 64) return 0;
  return posterior_head_bytes(p, m, cc_points_bytes(p)) + Carve::up(p->elem * (size_t)p->B * (size_t)m);
}

int dgp_posterior_cov_columns(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int32_t* idx, int ncols, void* work,
                              size_t work_bytes, double* cols_out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !idx || !cols_out) return fail(DGP_E_ARG, "dgp_posterior_cov_columns: null argument");
  if (m <= 0 || m > (1 << 20) || ncols < 1 || ncols > 64)
    return fail(DGP_E_ARG, "dgp_posterior_cov_columns: bad size (1 <= m <= 2^20, 1 <= ncols <= 64)");
  return posterior_entry(p, "dgp_posterior_cov_columns", work, work_bytes, dgp_posterior_cov_columns_workspace_bytes(p, m, ncols), stream,
                         [&](auto t, hipStream_t s) { return post_cov_columns<decltype(t)>(p, theta, Xs, m, idx, ncols, work, cols_out, s); });
}

}  // extern "C"
