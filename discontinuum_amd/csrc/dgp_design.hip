// dgp_design.hip -- exact value of one more sample for the variance of period sums (dgp_sample_value).
//
// f ~ N(mu, C) over m points (C: the matrix dgp_posterior_cov leaves; only its lower triangle is used), period sums
// L_p = sum_{i in p} w_i c_i of the data-space value c_i = exp(s f_i + t) (or s f_i + t), and a hypothetical observation
// y_c = f_c + eps, Var eps = tau_c^2, on ANY day c.  Conditioning rows B (nrows x m; C' = C - B^T B) stand for the samples
// already decided.  With
//     v'_c = C_cc - sum_t B_tc^2 + tau_c^2,   b_ic = (C_ic - sum_t B_ti B_tc) / sqrt(v'_c),   A_i given (a_dev),
// the expected reduction of Var(L_p) is, by the law of total variance and the exponential series,
//     gain[p][c] = sum_{i,j in p} A_i A_j expm1(s^2 b_ic b_jc) = sum_{k=1..K} (s^2)^k / k! (sum_{i in p} A_i b_ic^k)^2
// (K = 1 is the linear target exactly).  One pass over the covariance, O(m^2 K) multiply-adds on the fp64 vector pipe:
//   prep    one thread per point: v'_c -> var_out, 1 / sqrt(v'_c) (0 where v'_c is not > 0, NaN where it is NaN), and each
//           group's day range [start, end) (integer atomics)
//   sums    one wave per (64 candidates, group p, slab q of p's days): lanes own candidates, the loop over days is
//           wave-uniform.  Days come in tiles of 16, staged in LDS day by day: for days at or below the candidate block,
//           C[i][c .. c + 63] is one coalesced row segment; for days above it, C[c][i] comes from the candidates' rows,
//           read as 128-byte row segments and transposed on the way into LDS (leading dimension 65: conflict-free); the
//           tiles on the diagonal take both, split at c <= i (what they load above the diagonal, and pad rows, is
//           dropped).  Every lower-triangle entry is read twice in all.  The conditioning rows are subtracted tile by
//           tile: 16 accumulators per lane, the candidates' B_tc from LDS, the days' B_ti by wave-uniform loads.  Each
//           lane keeps the K power sums of its candidate in registers; a day outside group p (excluded days too) is
//           skipped.
//   With one slab per group the wave squares and folds its sums itself; otherwise the sums go to the work area and
//   fold    adds the slabs in a fixed order before squaring.  The slab count depends on (M, ngroups) alone, so that one
//           group over a long record still fills the device and a site's numbers do not depend on its batch.
// No floating-point atomics, every sum in a fixed order: bitwise repeatable.  All arithmetic after the loads is double.
#include <climits>

#include "dgp_design.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

constexpr int SV_FILL = 4096;         // workgroups per site the slab count aims for (the tile shape: dgp_design.h)

// slabs per group: a function of (M, P) alone
__host__ __device__ inline int sv_slabs(long M, int P) {
  const long blocks = M / SV_CAND * (long)P;
  long q = (SV_FILL + blocks - 1) / blocks;
  const long most = M / SV_DAYS;
  if (q > most) q = most;
  if (q > 64) q = 64;
  return q < 1 ? 1 : (int)q;
}

// per-site work area, in doubles: 1 / sqrt(v') [M], the slab sums [P][Q][K][M] (only when Q > 1), then 2 P ints (group start / end)
__host__ __device__ inline long sv_site_doubles(long M, int P, int K) {
  const int Q = sv_slabs(M, P);
  return M + (Q > 1 ? (long)P * Q * K * M : 0) + P;
}

__global__ __launch_bounds__(256) void sv_init_kernel(double* work, long ws, int P) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  int* se = (int*)(work + (long)blockIdx.z * ws + ws - P);
  se[2 * g] = INT_MAX;
  se[2 * g + 1] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void sv_prep_kernel(const T* __restrict__ cov, long M, int m, int P,
                                                      const int* __restrict__ group, const T* __restrict__ ov,
                                                      const double* __restrict__ rows, int nrows, double* work, long ws,
                                                      double* __restrict__ var_out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  double* rs = work + (long)z * ws;
  int* se = (int*)(rs + ws - P);
  double r = 0.0;
  if (j < m) {
    const long k = (long)z * m + j;
    const int g = group[k];
    if (g >= 0 && g < P) {
      atomicMin(&se[2 * g], (int)j);
      atomicMax(&se[2 * g + 1], (int)j + 1);
    }
    double v = (double)cov[(long)z * M * M + j * (M + 1)];
    for (int t = 0; t < nrows; ++t) {
      const double b = rows[((long)z * nrows + t) * m + j];
      v -= b * b;
    }
    if (ov) v += (double)ov[k];
    sv_inv_sd(v, r);  // NaN in, NaN out
    var_out[k] = v;
  }
  rs[j] = r;
}

template <typename T, int KT>
__global__ __launch_bounds__(SV_CAND) void sv_sums_kernel(const T* __restrict__ cov, long M, int m, int P, int Q, int K,
                                                           const double* __restrict__ a, const double* __restrict__ scale2,
                                                           const int* __restrict__ group, const double* __restrict__ rows,
                                                           int nrows, double* __restrict__ work, long ws,
                                                           double* __restrict__ gain_out) {
  const int cb = blockIdx.x, p = blockIdx.y / Q, q = blockIdx.y % Q, z = blockIdx.z;
  const int lane = threadIdx.x;
  const int c0 = cb * SV_CAND, c = c0 + lane;
  const T* C = cov + (long)z * M * M;
  const double* base = work + (long)z * ws;
  const double* az = a + (long)z * m;
  const int* gz = group + (long)z * m;
  const double* bz = rows + (long)z * nrows * m;  // (never read when nrows == 0)
  const int* se = (const int*)(base + ws - P);
  extern __shared__ __attribute__((aligned(16))) char sv_smem[];
  double* tile = (double*)sv_smem;        // [SV_DAYS][SV_LD]: C' of (day i0 + u, candidate c0 + lane)
  double* bc = tile + SV_DAYS * SV_LD;    // [nrows][SV_CAND]: B[t][c0 + lane]

  // this slab's days [d0, d1) of group p
  int g0 = se[2 * p], g1 = se[2 * p + 1];
  if (g1 <= g0) g0 = g1 = 0;  // empty group (start still INT_MAX)
  const int per = ((g1 - g0 + Q - 1) / Q + SV_DAYS - 1) / SV_DAYS * SV_DAYS;
  const long d0l = (long)g0 + (long)q * per;
  const int d0 = d0l < g1 ? (int)d0l : g1;
  const int d1 = d0l + per < g1 ? (int)(d0l + per) : g1;

  const double rs = base[c];
  for (int t = 0; t < nrows; ++t) bc[t * SV_CAND + lane] = c < m ? bz[(long)t * m + c] : 0.0;
  double S[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) S[k] = 0.0;

  for (int i0 = d0 / SV_DAYS * SV_DAYS; i0 < d1; i0 += SV_DAYS) {
    const bool from_rows = i0 + SV_DAYS - 1 >= c0;   // some day i >= some candidate c: C[i][c]
    const bool from_cols = i0 < c0 + SV_CAND - 1;    // some day i < some candidate c: C[c][i]
    // the tile's days: group id and A_i in lanes 0 .. 15 (-2: not a day of this slab)
    int gl = -2;
    double al = 0.0;
    if (lane < SV_DAYS && i0 + lane >= d0 && i0 + lane < d1) {
      gl = gz[i0 + lane];
      al = az[i0 + lane];
    }
    __syncthreads();  // the previous tile's reads are done
    if (from_rows) {
      T rv[SV_DAYS];
#pragma unroll
      for (int u = 0; u < SV_DAYS; ++u) {
        rv[u] = T(0);
        if (__builtin_amdgcn_readlane(gl, u) == p && c <= i0 + u) rv[u] = C[(long)(i0 + u) * M + c];
      }
#pragma unroll
      for (int u = 0; u < SV_DAYS; ++u)
        if (c <= i0 + u) tile[u * SV_LD + lane] = (double)rv[u];
    }
    if (from_cols) {
      const int col = lane & (SV_DAYS - 1), r0 = lane / SV_DAYS;
      constexpr int RSTEP = SV_CAND / SV_DAYS, NLOAD = SV_CAND / RSTEP;
      T tv[NLOAD];
#pragma unroll
      for (int j = 0; j < NLOAD; ++j) tv[j] = C[(long)(c0 + r0 + RSTEP * j) * M + i0 + col];
#pragma unroll
      for (int j = 0; j < NLOAD; ++j)
        if (c0 + r0 + RSTEP * j > i0 + col) tile[col * SV_LD + r0 + RSTEP * j] = (double)tv[j];
    }
    __syncthreads();
    if (nrows > 0) {
      // C' = C - B^T B for the tile: 16 independent accumulators per lane; the days' B_ti are wave-uniform loads (whole rows
      // of 16 unless the tile runs past the record), the candidate's B_tc one LDS read per row
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
#pragma unroll 1  // (unrolled, the sums' registers are shuffled between the copies: three moves per multiply-add)
    for (int u = 0; u < SV_DAYS; ++u) {
      if (__builtin_amdgcn_readlane(gl, u) != p) continue;  // wave-uniform
      const double x = tile[u * SV_LD + lane];
      const double b = x * rs;
      double pw = sv_readlane(al, u);
#pragma unroll
      for (int k4 = 0; k4 < KT; k4 += 4) {
        if (k4 < K) {  // wave-uniform; sums past K within the last four are computed and never used
#pragma unroll
          for (int k = k4; k < k4 + 4; ++k) {
            pw *= b;
            S[k] += pw;
          }
        }
      }
    }
  }

  if (Q == 1) {
    const double s2 = scale2[z];
    double coef = 1.0, gain = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < K) {
        coef *= s2 / (double)(k + 1);
        gain += coef * (S[k] * S[k]);
      }
    }
    if (c < m) gain_out[((long)z * P + p) * m + c] = gain;
  } else {
    double* part = work + (long)z * ws + M + ((long)p * Q + q) * K * M;
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) part[(long)k * M + c] = S[k];
  }
}

__global__ __launch_bounds__(256) void sv_fold_kernel(long M, int m, int P, int Q, int K, const double* __restrict__ scale2,
                                                      const double* __restrict__ work, long ws, double* __restrict__ gain_out) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y, z = blockIdx.z;
  if (c >= m) return;
  const double* part = work + (long)z * ws + M + (long)p * Q * K * M + c;
  const double s2 = scale2[z];
  double coef = 1.0, gain = 0.0;
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int qq = 0; qq < Q; ++qq) s += part[((long)qq * K + k) * M];
    coef *= s2 / (double)(k + 1);
    gain += coef * (s * s);
  }
  gain_out[((long)z * P + p) * m + c] = gain;
}

template <typename T, int KT>
void sv_launch_sums(const T* cov, long M, int m, int B, int P, int Q, int K, const double* a, const double* scale2,
                    const int* group, const double* rows, int nrows, double* work, long ws, double* gain_out, hipStream_t s) {
  const size_t lds = (SV_DAYS * SV_LD + (size_t)nrows * SV_CAND) * sizeof(double);
  sv_sums_kernel<T, KT><<<dim3((unsigned)(M / SV_CAND), (unsigned)(P * Q), (unsigned)B), SV_CAND, lds, s>>>(
      cov, M, m, P, Q, K, a, scale2, group, rows, nrows, work, ws, gain_out);
}

}  // namespace

static size_t sample_value_workspace_bytes(long m, int P, int K, int B) {
  return sizeof(double) * (size_t)B * (size_t)sv_site_doubles(round_up(m, DGP_TILE_HOST), P, K);
}

// the expected reduction of Var(L_p) by one more sample on each day c, after `nrows` conditioning rows (rows [B][nrows][m], null
// when nrows == 0; a [B][m] the A_i; ov: the candidates' noise variance or null).  gain_out [B][P][m], var_out [B][m]
template <typename T>
static int sample_value(const T* cov, long m, int B, const double* a, const double* scale2, const int* group, int P, const T* ov,
                        const double* rows, int nrows, int K, double* work, double* gain_out, double* var_out, hipStream_t s) {
  static_assert(SV_DAYS * SV_LD * sizeof(double) % 16 == 0, "the LDS carve offsets must stay 16-byte aligned");
  const long M = round_up(m, DGP_TILE_HOST);
  const int Q = sv_slabs(M, P), mi = (int)m;
  const long ws = sv_site_doubles(M, P, K);
  sv_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work, ws, P);
  sv_prep_kernel<T><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(cov, M, mi, P, group, ov, rows, nrows, work, ws,
                                                                                    var_out);
  if (K <= 4)
    sv_launch_sums<T, 4>(cov, M, mi, B, P, Q, K, a, scale2, group, rows, nrows, work, ws, gain_out, s);
  else if (K <= 16)
    sv_launch_sums<T, 16>(cov, M, mi, B, P, Q, K, a, scale2, group, rows, nrows, work, ws, gain_out, s);
  else if (K <= 32)
    sv_launch_sums<T, 32>(cov, M, mi, B, P, Q, K, a, scale2, group, rows, nrows, work, ws, gain_out, s);
  else
    sv_launch_sums<T, 64>(cov, M, mi, B, P, Q, K, a, scale2, group, rows, nrows, work, ws, gain_out, s);
  if (Q > 1)
    sv_fold_kernel<<<dim3((unsigned)((m + 255) / 256), (unsigned)P, (unsigned)B), 256, 0, s>>>(M, mi, P, Q, K, scale2, work, ws,
                                                                                               gain_out);
  return (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

static bool sv_sizes_ok(int64_t m, int ngroups, int nrows, int nterms, int batch) {
  return m > 0 && m <= (1 << 20) && ngroups > 0 && ngroups <= 65535 && nrows >= 0 && nrows <= 64 && nterms >= 1 && nterms <= 64 &&
         batch > 0 && batch <= DGP_MAX_BATCH_SITES;
}

extern "C" {

size_t dgp_sample_value_workspace_bytes(int64_t m, int ngroups, int nrows, int nterms, int batch) {
  if (!sv_sizes_ok(m, ngroups, nrows, nterms, batch)) return 0;
  return sample_value_workspace_bytes(m, ngroups, nterms, batch);
}

int dgp_sample_value(int dtype, const void* cov, int64_t m, int batch, const double* a, const double* scale2, const int32_t* group,
                     int ngroups, const void* obs_var, const double* rows, int nrows, int nterms, void* work, size_t work_bytes,
                     double* gain_out, double* var_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_sample_value: dtype must be 0 (f64) or 1 (f32)");
  if (!cov || !a || !scale2 || !group || !gain_out || !var_out) return fail(DGP_E_ARG, "dgp_sample_value: null argument");
  if (!sv_sizes_ok(m, ngroups, nrows, nterms, batch))
    return fail(DGP_E_ARG,
                "dgp_sample_value: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 0 <= nrows <= 64, 1 <= nterms <= 64, "
                "1 <= batch <= 1024)");
  if (nrows > 0 && !rows) return fail(DGP_E_ARG, "dgp_sample_value: null argument (rows with nrows > 0)");
  if (!work || work_bytes < sample_value_workspace_bytes(m, ngroups, nterms, batch))
    return fail(DGP_E_WORKSPACE, "dgp_sample_value: workspace missing or too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64 ? sample_value<double>((const double*)cov, m, batch, a, scale2, group, ngroups, (const double*)obs_var,
                                                         rows, nrows, nterms, (double*)work, gain_out, var_out, s)
                                  : sample_value<float>((const float*)cov, m, batch, a, scale2, group, ngroups, (const float*)obs_var,
                                                        rows, nrows, nterms, (double*)work, gain_out, var_out, s);
  return wrap(rc, "dgp_sample_value");
}

}  // extern "C"
