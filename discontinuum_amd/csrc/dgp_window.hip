// dgp_window.hip -- exact moments of ROLLING-WINDOW means of a transformed Gaussian posterior (dgp_window_moments).
//
// f ~ N(mu, C) over m points (C: the matrix dgp_posterior_cov leaves; only its lower triangle is read, an entry above the
// diagonal comes from its mirror), q windows [lo_i, hi_i) over the points (both ends non-decreasing in i), point weights
// a_j >= 0 and W_ij = a_j / sum_{k in window i} a_k.  The rolling statistic W f is exactly Gaussian, N(W mu, W C W^T):
//     mode 0:  b_j = a_j,                             mean_i = sum_j W_ij mu_j,  cov_ik = sum_j sum_l W_ij W_kl C_jl
//     mode 1:  b_j = a_j exp(mu_j + s2 C_jj / 2),     mean_i = sum_j W_ij e_j,   cov_ik = sum_j sum_l W_ij W_kl e_j e_l expm1(s2 C_jl)
// (mu already mapped, as for dgp_period_moments).  With d_i = sum_{k in window i} a_k, four launches, gridDim.z = sites:
//   points   one thread per point: b_j and the mean term
//   windows  one thread per window: the clamped ends (to [0, m]; the pad's windows are empty), 1 / d_i (0 for an empty window
//            or a zero sum) and mean_i, summed in ascending j
//   pass 1   Tt[k][j] = sum_{l in window k} b_l phi(C_sym[j][l])          (Q x M doubles in the work area, phi = id / expm1(s2 .))
//   pass 2   cov_ik   = (sum_{j in window i} b_j Tt[k][j]) / (d_i d_k)    on the lower block triangle; inside a diagonal
//            128-block only k <= i is computed and written to (i, k) and (k, i): those blocks are exactly symmetric.
// Both passes are ONE kernel: a workgroup owns 128 rows r (lanes along r) and 64 windows, walks the windows' column span
// [lo of its first window, hi of its last) in chunks of 32 columns p, stages b_p phi(src[r][p]) as doubles in LDS (phi is
// evaluated once per staged entry, not once per window that holds it) and every thread adds, for each of its 32 windows, the
// staged entries of its row inside the window, p ascending.  src[r][p] is contiguous along p (a row of C at or below the
// diagonal, a row of Tt); a 128 x 32 tile of C ABOVE the diagonal is read from its mirror, contiguous along r.  The LDS rows
// are padded to 33 doubles, so that the reads (lanes along r) and the mirrored stores are free of bank conflicts.  Each sum runs in one
// thread in ascending order: no atomics, bitwise repeatable, and a site's numbers do not depend on its batch.  The output pad
// (rows / columns >= q) is the identity; blocks above the block diagonal are not written, as in dgp_posterior_cov.
#include "dgp_common.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

constexpr int WM_ROWS = 128;              // rows of a workgroup (== DGP_TILE_HOST, the block size of both buffers)
constexpr int WM_WIN = 64;                // windows of a workgroup
constexpr int WM_CHUNK = 32;              // columns staged at a time (divides 128: a chunk lies in one tile of C)
constexpr int WM_PITCH = WM_CHUNK + 1;    // doubles per LDS row
constexpr int WM_THREADS = 256;           // 128 rows x 2 groups of windows
constexpr int WM_ACC = WM_WIN / (WM_THREADS / WM_ROWS);  // windows (accumulators) per thread
static_assert(WM_ROWS % WM_WIN == 0 && WM_ROWS % WM_CHUNK == 0 && WM_THREADS % WM_ROWS == 0 && WM_WIN <= WM_THREADS, "tile shapes");
static_assert(WM_ROWS == 128 && WM_CHUNK == 32, "the staging loop splits its index by >> 7 and >> 5");

// per-site work area, in doubles: Tt[Q x M], b[M], mean term[M], 1 / d[Q], then 2 Q ints (the clamped window ends)
__host__ __device__ inline long wm_site_doubles(long M, long Q) { return M * Q + 2 * M + 2 * Q; }

template <typename T, int MODE>
__global__ __launch_bounds__(256) void wm_points_kernel(const T* __restrict__ cov, long M, int m, long Q, const T* __restrict__ mu,
                                                        const double* __restrict__ scale2, const double* __restrict__ a,
                                                        double* __restrict__ work, long ws) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  double* b = work + (long)z * ws + M * Q;
  double* mt = b + M;
  double bv = 0.0, mv = 0.0;
  if (j < m) {
    const long k = (long)z * m + j;
    const double aj = a ? a[k] : 1.0, muj = (double)mu[k];
    if constexpr (MODE == 1) {
      bv = aj * exp(muj + 0.5 * scale2[z] * (double)cov[(long)z * M * M + j * (M + 1)]);
      mv = bv;
    } else {
      bv = aj;
      mv = aj * muj;
    }
  }
  b[j] = bv;
  mt[j] = mv;
}

__global__ __launch_bounds__(256) void wm_windows_kernel(const double* __restrict__ a, const int* __restrict__ lo,
                                                         const int* __restrict__ hi, long M, int m, long Q, int q,
                                                         double* __restrict__ work, long ws, double* __restrict__ mean_out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (i >= Q) return;
  double* base = work + (long)z * ws + M * Q;
  const double* mt = base + M;
  double* inv = base + 2 * M;
  int* win = (int*)(inv + Q);
  int l0 = 0, l1 = 0;
  double d = 0.0, ms = 0.0;
  if (i < q) {
    l0 = min(max(lo[(long)z * q + i], 0), m);
    l1 = min(max(hi[(long)z * q + i], l0), m);
    const double* az = a ? a + (long)z * m : nullptr;
    for (int j = l0; j < l1; ++j) {
      d += az ? az[j] : 1.0;
      ms += mt[j];
    }
  }
  const double r = d > 0.0 ? 1.0 / d : 0.0;
  inv[i] = r;
  win[2 * i] = l0;
  win[2 * i + 1] = l1;
  if (i < q) mean_out[(long)z * q + i] = ms * r;
}

// PASS 1: rows r = points j of C (T, MODE as given), out Tt[k][j].  PASS 2: rows r = windows k of Tt, out cov_out[i][k].
template <typename T, int MODE, int PASS>
__global__ __launch_bounds__(WM_THREADS) void wm_pass_kernel(const T* __restrict__ cov, const double* __restrict__ scale2, long M, long Q,
                                                      int m, int q, double* __restrict__ work, long ws,
                                                      double* __restrict__ cov_out) {
  const int wt = blockIdx.x, rb = blockIdx.y, z = blockIdx.z;
  if constexpr (PASS == 2) {
    if (rb > wt / (WM_ROWS / WM_WIN)) return;  // a block above the block diagonal
  }
  const int t = threadIdx.x;
  double* base = work + (long)z * ws;
  double* Tt = base;
  const double* b = base + M * Q;
  const double* inv = b + 2 * M;
  const int* win = (const int*)(inv + Q);
  __shared__ double tile[WM_ROWS * WM_PITCH];
  __shared__ int slo[WM_WIN], shi[WM_WIN];
  const int k0 = wt * WM_WIN, r0 = rb * WM_ROWS;
  if (t < WM_WIN) {
    slo[t] = win[2 * (k0 + t)];
    shi[t] = win[2 * (k0 + t) + 1];
  }
  // the column span of this workgroup's windows (those of the pad are empty and take no part)
  const int klast = min(k0 + WM_WIN, q) - 1;
  int l0 = 0, l1 = 0;
  if (klast >= k0) {
    l0 = win[2 * k0];
    l1 = min(win[2 * klast + 1], m);
  }
  const int rr = t & (WM_ROWS - 1), kg = t / WM_ROWS;
  const int rlim = PASS == 1 ? m : q;  // rows past it hold zeros
  double s2 = 0.0;
  if constexpr (PASS == 1 && MODE == 1) s2 = scale2[z];
  const T* C = PASS == 1 ? cov + (long)z * M * M : nullptr;
  double acc[WM_ACC];
#pragma unroll
  for (int u = 0; u < WM_ACC; ++u) acc[u] = 0.0;

  for (int pc = l0 / WM_CHUNK * WM_CHUNK; pc < l1; pc += WM_CHUNK) {
    __syncthreads();  // the previous chunk is consumed (the first time: slo / shi are there)
    const bool mirrored = PASS == 1 && pc / WM_ROWS > rb;  // a tile of C above the diagonal: lanes along r
    for (int e = t; e < WM_ROWS * WM_CHUNK; e += WM_THREADS) {
      int jj, ll;
      if (mirrored) {
        jj = e & (WM_ROWS - 1);
        ll = e >> 7;
      } else {
        ll = e & (WM_CHUNK - 1);
        jj = e >> 5;
      }
      const int r = r0 + jj, p = pc + ll;
      double v = 0.0;
      if (r < rlim && p < m) {
        if constexpr (PASS == 1) {
          const double x = (double)(r >= p ? C[(long)r * M + p] : C[(long)p * M + r]);
          if constexpr (MODE == 1)
            v = b[p] * expm1(s2 * x);
          else
            v = b[p] * x;
        } else {
          v = b[p] * Tt[(long)r * M + p];
        }
      }
      tile[jj * WM_PITCH + ll] = v;
    }
    __syncthreads();
    const double* row = tile + rr * WM_PITCH;
#pragma unroll
    for (int u = 0; u < WM_ACC; ++u) {
      const int kk = kg * WM_ACC + u;  // the same for all lanes of a wave
      const int a0 = max(__builtin_amdgcn_readfirstlane(slo[kk]), pc) - pc;
      const int a1 = min(__builtin_amdgcn_readfirstlane(shi[kk]), pc + WM_CHUNK) - pc;
      for (int l = a0; l < a1; ++l) acc[u] += row[l];
    }
  }

  const int r = r0 + rr;
  if constexpr (PASS == 1) {
#pragma unroll
    for (int u = 0; u < WM_ACC; ++u) Tt[(long)(k0 + kg * WM_ACC + u) * M + r] = acc[u];
  } else {
    double* out = cov_out + (long)z * Q * Q;
    const bool diag = rb == wt / (WM_ROWS / WM_WIN);
    const double invr = r < q ? inv[r] : 0.0;
#pragma unroll
    for (int u = 0; u < WM_ACC; ++u) {
      const int i = k0 + kg * WM_ACC + u;
      const double v = (i < q && r < q) ? (acc[u] * inv[i]) * invr : (i == r ? 1.0 : 0.0);
      if (!diag) {
        out[(long)i * Q + r] = v;
      } else if (r <= i) {
        out[(long)i * Q + r] = v;
        out[(long)r * Q + i] = v;
      }
    }
  }
}

template <typename T, int MODE>
int window_moments_mode(const T* cov, long M, int m, int B, const T* mu, const double* scale2, const double* a, const int* lo,
                        const int* hi, long Q, int q, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  const long ws = wm_site_doubles(M, Q);
  wm_points_kernel<T, MODE><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(cov, M, m, Q, mu, scale2, a, work, ws);
  wm_windows_kernel<<<dim3((unsigned)((Q + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(a, lo, hi, M, m, Q, q, work, ws, mean_out);
  wm_pass_kernel<T, MODE, 1><<<dim3((unsigned)(Q / WM_WIN), (unsigned)(M / WM_ROWS), (unsigned)B), WM_THREADS, 0, s>>>(cov, scale2, M, Q, m, q,
                                                                                                             work, ws, cov_out);
  wm_pass_kernel<double, 0, 2><<<dim3((unsigned)(Q / WM_WIN), (unsigned)(Q / WM_ROWS), (unsigned)B), WM_THREADS, 0, s>>>(nullptr, nullptr, M, Q, m,
                                                                                                               q, work, ws, cov_out);
  return (int)hipGetLastError();
}

}  // namespace

static size_t window_moments_workspace_bytes(long m, long q, int B) {
  return sizeof(double) * (size_t)B * (size_t)wm_site_doubles(round_up(m, DGP_TILE_HOST), round_up(q, DGP_TILE_HOST));
}

// exact mean / covariance of rolling-window means W f (mode 0) or W exp(f) (mode 1), f ~ N(mu, C); windows [lo_i, hi_i) per site
// ([B][q], non-decreasing), weights a [B][m] or null; mean_out [B][q], cov_out [B][Q][Q] in the layout of posterior_cov
// (Q = round_up(q, 128)); `work`: window_moments_workspace_bytes
template <typename T>
static int window_moments(int mode, const T* cov, long m, int B, const T* mu, const double* scale2, const double* a, const int* lo,
                          const int* hi, long q, double* work, double* mean_out, double* cov_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST), Q = round_up(q, DGP_TILE_HOST);
  return mode == 1 ? window_moments_mode<T, 1>(cov, M, (int)m, B, mu, scale2, a, lo, hi, Q, (int)q, work, mean_out, cov_out, s)
                   : window_moments_mode<T, 0>(cov, M, (int)m, B, mu, scale2, a, lo, hi, Q, (int)q, work, mean_out, cov_out, s);
}

}  // namespace dgp

using namespace dgp;

static bool wm_sizes_ok(int64_t m, int64_t q, int batch) {
  return m > 0 && m <= (1 << 20) && q > 0 && q <= (1 << 20) && batch > 0 && batch <= DGP_MAX_BATCH_SITES;
}

extern "C" {

size_t dgp_window_moments_workspace_bytes(int64_t m, int64_t q, int batch) {
  if (!wm_sizes_ok(m, q, batch)) return 0;
  return window_moments_workspace_bytes(m, q, batch);
}

int dgp_window_moments(int dtype, int mode, const void* cov, int64_t m, int batch, const void* mu, const double* scale2,
                       const double* a, const int32_t* lo, const int32_t* hi, int64_t q, void* work, size_t work_bytes,
                       double* mean_out, double* cov_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_window_moments: dtype must be 0 (f64) or 1 (f32)");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_window_moments: mode must be 0 (linear) or 1 (log)");
  if (!cov || !mu || !lo || !hi || !mean_out || !cov_out || (mode == 1 && !scale2))
    return fail(DGP_E_ARG, "dgp_window_moments: null argument");
  if (!wm_sizes_ok(m, q, batch))
    return fail(DGP_E_ARG, "dgp_window_moments: bad size (1 <= m <= 2^20, 1 <= q <= 2^20, 1 <= batch <= 1024)");
  if (!work || work_bytes < window_moments_workspace_bytes(m, q, batch))
    return fail(DGP_E_WORKSPACE, "dgp_window_moments: workspace missing or too small");
  if (((uintptr_t)work & 7) != 0) return fail(DGP_E_ARG, "dgp_window_moments: the work area must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64 ? window_moments<double>(mode, (const double*)cov, m, batch, (const double*)mu, scale2, a, lo, hi, q,
                                                           (double*)work, mean_out, cov_out, s)
                                  : window_moments<float>(mode, (const float*)cov, m, batch, (const float*)mu, scale2, a, lo, hi, q,
                                                          (double*)work, mean_out, cov_out, s);
  return wrap(rc, "dgp_window_moments");
}

}  // extern "C"
