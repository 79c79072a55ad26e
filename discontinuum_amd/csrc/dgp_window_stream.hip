// dgp_window_stream.hip -- the VARIANCES of rolling-window means (the diagonal of dgp_window_moments' W C W^T) from a BAND of the
// posterior covariance that is produced R rows at a time and never stored whole (dgp_posterior_window_variances), the same
// contraction on a dense matrix (dgp_window_variances), and a block of the covariance itself (dgp_posterior_cov_block).
//
// Notation, modes, weights and window rules are dgp_window.hip's: f ~ N(mu, C) over m points, q windows [lo_i, hi_i), b_j = a_j
// (mode 0) or a_j exp(mu_j + s2 C_jj / 2) (mode 1), d_i = sum_{k in window i} a_k, phi = id / expm1(s2 .), and
//     var_i = d_i^-2 sum_{j in win_i} b_j ( b_j phi(C_jj) + 2 sum_{l in [lo_i, j)} b_l phi(C_jl) ).
// Every unordered pair (j >= l) lies in exactly one row panel, j's, so var_i d_i^2 is a sum of per-panel partials and needs no
// halo, only one accumulator per window.  Two points share a window only if |j - l| < reach = max_i (hi_i - lo_i): the panel of
// rows [p0, p1) needs the columns [c0, p1), c0 = 128 floor(max(0, p0 - reach + 1) / 128), and the band buffer holds exactly
// those (first element C[p0][c0]).  The front end, the band loop and their invariants are dgp_stream.h's: on the streamed path
// C_jj is the PREDICTED variance, never a panel's diagonal.
// Launches (gridDim.z = sites, one stream, no floating-point atomics):
//   points    one thread per point: b_j, the mean term, C_jj as a double; the site's reach flag is reset
//   windows   one thread per window: the clamped ends, 1 / d_i, mean_i (ascending j), acc_i = 0, and the site's flag when a
//             window holds more than `reach` points
//   per panel, in ascending order:  [band Gram, band update,]  contraction
//   finish    var_i = (acc_i / d_i) / d_i
// The contraction: a workgroup OWNS 64 windows and walks the 128-row blocks of the panel that their span [lo of the first, hi of
// the last) meets.  Per block it stages b_p phi(C[r][p]) for p < r (0 otherwise) in chunks of 32 columns in LDS -- phi once per
// staged entry, rows padded to 33 doubles, lanes along r, as wm_pass_kernel does --, every thread adds for each of its 32
// windows the staged entries of its row inside the window (p ascending), forms b_r (b_r phi(C_rr) + 2 sum) where r lies in the
// window, and the 128 rows are summed by a fixed shuffle tree and a fixed join of the two waves.  The window's owner thread adds
// the blocks in ascending order and finishes with a plain read-modify-write of acc_i: launches are ordered, so every sum runs in
// one owner in a fixed order, repeated calls are bitwise equal and a site's numbers do not depend on its batch.
// Every column index is clamped to [c0, p1) before it becomes an address: a window longer than `reach` reads a wrong entry of
// the band, never one outside it, and the call then reports the flag.
#include <vector>

#include "dgp_common.h"
#include "dgp_stream.h"

namespace dgp {

namespace {

constexpr int WS_ROWS = 128;            // rows of a staged block (== DGP_TILE_HOST)
constexpr int WS_WIN = 64;              // windows of a workgroup
constexpr int WS_CHUNK = 32;            // columns staged at a time
constexpr int WS_PITCH = WS_CHUNK + 1;  // doubles per LDS row (wm_pass_kernel's padded pitch)
constexpr int WS_THREADS = 256;         // 128 rows x 2 groups of windows
constexpr int WS_ACC = WS_WIN / (WS_THREADS / WS_ROWS);  // windows (accumulators) per thread
static_assert(WS_ROWS == 128 && WS_CHUNK == 32 && WS_ACC == 32 && WS_THREADS == 256, "the index splits below");

// per-site work area, in doubles: b[M], mean term[M], C_jj[M], 1 / d[Q], acc[Q], then 2 Q ints (the clamped window ends)
__host__ __device__ inline long ws_site_doubles(long M, long Q) { return 3 * M + 3 * Q; }

struct WsWork {
  double *b, *mt, *dg, *inv, *acc;
  int* win;
  __host__ __device__ WsWork(double* work, long ws, long M, long Q, int z) {
    b = work + (long)z * ws;
    mt = b + M;
    dg = mt + M;
    inv = dg + M;
    acc = inv + Q;
    win = (int*)(acc + Q);
  }
};

__device__ __forceinline__ double ws_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// diag: C_jj of point j of site z at diag[z dsite + j dstep] (a dense matrix: dstep = M + 1; the predicted variance: dstep = 1)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void ws_points_kernel(const T* __restrict__ diag, long dsite, long dstep, long M, int m, long Q,
                                                        const T* __restrict__ mu, const double* __restrict__ scale2,
                                                        const double* __restrict__ a, double* __restrict__ work, long ws,
                                                        int* __restrict__ flags) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j == 0) flags[z] = 0;
  if (j >= M) return;
  const WsWork wk(work, ws, M, Q, z);
  double bv = 0.0, mv = 0.0, dv = 0.0;
  if (j < m) {
    const long k = (long)z * m + j;
    const double aj = a ? a[k] : 1.0, muj = (double)mu[k];
    dv = (double)diag[(long)z * dsite + j * dstep];
    if constexpr (MODE == 1) {
      bv = aj * exp(muj + 0.5 * scale2[z] * dv);
      mv = bv;
    } else {
      bv = aj;
      mv = aj * muj;
    }
  }
  wk.b[j] = bv;
  wk.mt[j] = mv;
  wk.dg[j] = dv;
}

__global__ __launch_bounds__(256) void ws_windows_kernel(const double* __restrict__ a, const int* __restrict__ lo,
                                                         const int* __restrict__ hi, long M, int m, long Q, int q, long reach,
                                                         double* __restrict__ work, long ws, double* __restrict__ mean_out,
                                                         int* __restrict__ flags) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (i >= Q) return;
  const WsWork wk(work, ws, M, Q, z);
  int l0 = 0, l1 = 0;
  double d = 0.0, ms = 0.0;
  if (i < q) {
    l0 = min(max(lo[(long)z * q + i], 0), m);
    l1 = min(max(hi[(long)z * q + i], l0), m);
    const double* az = a ? a + (long)z * m : nullptr;
    for (int j = l0; j < l1; ++j) {
      d += az ? az[j] : 1.0;
      ms += wk.mt[j];
    }
    if ((long)(l1 - l0) > reach) flags[z] = 1;  // (every writer stores the same value)
  }
  const double r = d > 0.0 ? 1.0 / d : 0.0;
  wk.inv[i] = r;
  wk.acc[i] = 0.0;
  wk.win[2 * i] = l0;
  wk.win[2 * i + 1] = l1;
  if (i < q) mean_out[(long)z * q + i] = ms * r;
}

// The panel of rows [p0, p1) (multiples of 128) of C, columns [c0, p1): src[(r - p0) ld + (p - c0)], site stride sstride.
template <typename T, int MODE>
__global__ __launch_bounds__(WS_THREADS) void ws_contract_kernel(const T* __restrict__ src, long sstride, long ld, int p0, int p1, int c0,
                                                                 const double* __restrict__ scale2, long M, long Q, int m, int q,
                                                                 double* __restrict__ work, long ws) {
  const int wt = blockIdx.x, z = blockIdx.z, t = threadIdx.x;
  const WsWork wk(work, ws, M, Q, z);
  const int k0 = wt * WS_WIN;
  const int klast = min(k0 + WS_WIN, q) - 1;
  if (klast < k0) return;
  // the column span of this workgroup's windows, and its rows inside the panel (uniform over the workgroup)
  const int l0 = wk.win[2 * k0], l1 = wk.win[2 * klast + 1];
  const int ra = max(l0, p0), rz = min(l1, p1);
  if (ra >= rz) return;
  __shared__ double tile[WS_ROWS * WS_PITCH];
  __shared__ double part[WS_THREADS / 64][WS_ACC];
  __shared__ int slo[WS_WIN], shi[WS_WIN];
  if (t < WS_WIN) {
    slo[t] = wk.win[2 * (k0 + t)];
    shi[t] = wk.win[2 * (k0 + t) + 1];
  }
  const int rr = t & (WS_ROWS - 1), kg = t / WS_ROWS, lane = t & 63, wave = t >> 6;
  double s2 = 0.0;
  if constexpr (MODE == 1) s2 = scale2[z];
  const T* C = src + (long)z * sstride;
  double total = 0.0;  // thread t < 64: window k0 + t, the blocks in ascending order

  for (int r0 = ra / WS_ROWS * WS_ROWS; r0 < rz; r0 += WS_ROWS) {  // p0 <= r0 and r0 + 128 <= p1: both are multiples of 128
    double acc[WS_ACC];
#pragma unroll
    for (int u = 0; u < WS_ACC; ++u) acc[u] = 0.0;
    const int pend = min(l1, r0 + WS_ROWS);  // columns p >= r are staged as zeros: nothing beyond the block's last row
    for (int pc = l0 / WS_CHUNK * WS_CHUNK; pc < pend; pc += WS_CHUNK) {
      __syncthreads();  // the previous chunk is consumed (the first time: slo / shi are there)
      for (int e = t; e < WS_ROWS * WS_CHUNK; e += WS_THREADS) {
        const int ll = e & (WS_CHUNK - 1), jj = e >> 5;
        const int r = r0 + jj, p = pc + ll;
        double v = 0.0;
        if (p < r && r < m) {
          const int pa = min(max(p, c0), p1 - 1) - c0;  // never an address outside the band
          const double x = (double)C[(long)(r - p0) * ld + pa];
          if constexpr (MODE == 1)
            v = wk.b[p] * expm1(s2 * x);
          else
            v = wk.b[p] * x;
        }
        tile[jj * WS_PITCH + ll] = v;
      }
      __syncthreads();
      const double* row = tile + rr * WS_PITCH;
#pragma unroll
      for (int u = 0; u < WS_ACC; ++u) {
        const int kk = kg * WS_ACC + u;  // the same for all lanes of a wave
        const int a0 = max(__builtin_amdgcn_readfirstlane(slo[kk]), pc) - pc;
        const int a1 = min(__builtin_amdgcn_readfirstlane(shi[kk]), pc + WS_CHUNK) - pc;
        for (int l = a0; l < a1; ++l) acc[u] += row[l];
      }
    }
    // row r's share of every window that holds it, then the 128 rows: a shuffle tree per wave, the two waves joined below
    const int r = r0 + rr;
    const double br = wk.b[r];
    double dterm;
    if constexpr (MODE == 1)
      dterm = br * expm1(s2 * wk.dg[r]);
    else
      dterm = br * wk.dg[r];
#pragma unroll
    for (int u = 0; u < WS_ACC; ++u) {
      const int kk = kg * WS_ACC + u;
      const bool inside = r >= slo[kk] && r < shi[kk];
      const double v = ws_wave_sum(inside ? br * (dterm + 2.0 * acc[u]) : 0.0);
      if (lane == 0) part[wave][u] = v;
    }
    __syncthreads();
    if (t < WS_WIN) total += part[2 * (t / WS_ACC)][t % WS_ACC] + part[2 * (t / WS_ACC) + 1][t % WS_ACC];
    __syncthreads();
  }
  if (t < WS_WIN && k0 + t < q) wk.acc[k0 + t] += total;  // this workgroup alone owns the window in this launch
}

__global__ __launch_bounds__(256) void ws_finish_kernel(long M, long Q, int q, const double* __restrict__ work, long ws,
                                                        double* __restrict__ var_out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (i >= q) return;
  const WsWork wk(const_cast<double*>(work), ws, M, Q, z);
  var_out[(long)z * q + i] = (wk.acc[i] * wk.inv[i]) * wk.inv[i];
}

struct WsArea {
  double* work;
  int* flags;
  long ws;
};
inline size_t ws_area_bytes(long M, long Q, int B) {
  return Carve::up(sizeof(double) * (size_t)B * (size_t)ws_site_doubles(M, Q)) + Carve::up(sizeof(int) * (size_t)B);
}
inline WsArea ws_area(void* base, long M, long Q, int B) {
  WsArea A;
  A.work = (double*)base;
  A.ws = ws_site_doubles(M, Q);
  A.flags = (int*)((char*)base + Carve::up(sizeof(double) * (size_t)B * (size_t)A.ws));
  return A;
}

template <typename T, int MODE>
void ws_begin(const T* diag, long dsite, long dstep, long M, int m, int B, const T* mu, const double* scale2, const double* a,
              const int* lo, const int* hi, long Q, int q, long reach, const WsArea& A, double* mean_out, hipStream_t s) {
  ws_points_kernel<T, MODE><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(diag, dsite, dstep, M, m, Q, mu, scale2, a,
                                                                                            A.work, A.ws, A.flags);
  ws_windows_kernel<<<dim3((unsigned)((Q + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(a, lo, hi, M, m, Q, q, reach, A.work, A.ws, mean_out,
                                                                                    A.flags);
}
template <typename T, int MODE>
void ws_contract(const T* src, long sstride, long ld, long p0, long p1, long c0, const double* scale2, long M, int m, int B, long Q,
                 int q, const WsArea& A, hipStream_t s) {
  ws_contract_kernel<T, MODE><<<dim3((unsigned)(Q / WS_WIN), 1, (unsigned)B), WS_THREADS, 0, s>>>(src, sstride, ld, (int)p0, (int)p1, (int)c0,
                                                                                               scale2, M, Q, m, q, A.work, A.ws);
}
inline void ws_finish(long M, int B, long Q, int q, const WsArea& A, double* var_out, hipStream_t s) {
  ws_finish_kernel<<<dim3((unsigned)((q + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(M, Q, q, A.work, A.ws, var_out);
}

// the dense matrix as ONE panel with c0 = 0; its diagonal is read from it
template <typename T, int MODE>
int window_variances_mode(const T* cov, long m, int B, const T* mu, const double* scale2, const double* a, const int* lo,
                          const int* hi, long q, void* work, double* mean_out, double* var_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST), Q = round_up(q, DGP_TILE_HOST);
  const WsArea A = ws_area(work, M, Q, B);
  ws_begin<T, MODE>(cov, M * M, M + 1, M, (int)m, B, mu, scale2, a, lo, hi, Q, (int)q, M, A, mean_out, s);
  ws_contract<T, MODE>(cov, M * M, M, 0, M, 0, scale2, M, (int)m, B, Q, (int)q, A, s);
  ws_finish(M, B, Q, (int)q, A, var_out, s);
  return (int)hipGetLastError();
}

}  // namespace

static long window_band_ld(long m, long R, long reach) { return panel_rows(m, R) + round_up(reach, DGP_TILE_HOST); }

// The streamed pass.  `band`: R x ld elements per site at site stride bstride; flags_host: B ints, valid after the stream has
// been synchronised by the caller
template <typename T, int MODE>
static int posterior_window_variances(const Posterior<T>& ps, const T* mu, const double* scale2, const double* a, const int* lo,
                                      const int* hi, long q, long reach, long R, T* band, long bstride, void* area, double* mean_out,
                                      double* var_out, int* flags_host) {
  const long M = ps.M, Q = round_up(q, DGP_TILE_HOST);
  const long ld = window_band_ld(ps.m, R, reach);
  const int m = (int)ps.m, B = ps.p->B;
  hipStream_t s = ps.s;
  const WsArea A = ws_area(area, M, Q, B);
  ws_begin<T, MODE>(ps.var, ps.wbs, 1, M, m, B, mu, scale2, a, lo, hi, Q, (int)q, reach, A, mean_out, s);
  if (int rc = ps.zero_noise()) return rc;
  const int rc = ps.bands(R, reach, ld, band, bstride, [&](long p0, long p1, long c0) {
    ws_contract<T, MODE>(band, bstride, ld, p0, p1, c0, scale2, M, m, B, Q, (int)q, A, s);
  });
  if (rc) return rc;
  ws_finish(M, B, Q, (int)q, A, var_out, s);
  const hipError_t he = hipMemcpyAsync(flags_host, A.flags, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s);
  if (he != hipSuccess) return (int)he;
  return (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

static bool wv_sizes_ok(int64_t m, int64_t q, int batch) {
  return m > 0 && m <= (1 << 20) && q > 0 && q <= (1 << 20) && batch > 0 && batch <= DGP_MAX_BATCH_SITES;
}
static bool wv_panel_ok(int64_t reach, int panel_rows) {
  return reach >= 1 && reach <= (1 << 20) && panel_rows_ok(panel_rows);
}
static size_t wv_band_bytes(const dgp_plan* p, int64_t m, int64_t reach, int panel_rows) {
  return panel_bytes(p, m, panel_rows, window_band_ld((long)m, panel_rows, (long)reach));
}

template <typename T>
static int post_window(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* scale2, const double* a,
                       const int32_t* lo, const int32_t* hi, int64_t q, int mode, int64_t reach, int panel_rows, void* work,
                       double* mean_out, double* var_out, hipStream_t s, int* flags_host) {
  const PosteriorAreas<T> A = posterior_areas<T>(p, m, work, wv_band_bytes(p, m, reach, panel_rows));
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, A.own, s)) return rc;
  return mode == 1 ? posterior_window_variances<T, 1>(ps, (const T*)mu, scale2, a, lo, hi, (long)q, (long)reach, panel_rows, A.panel, A.pstride,
                                                      A.own, mean_out, var_out, flags_host)
                   : posterior_window_variances<T, 0>(ps, (const T*)mu, scale2, a, lo, hi, (long)q, (long)reach, panel_rows, A.panel, A.pstride,
                                                      A.own, mean_out, var_out, flags_host);
}

// a block of the covariance: the front end, then one band straight into `out`; the latent mean goes behind the prediction's area
static bool block_ok(int64_t m, int64_t row0, int64_t row1, int64_t col0) {
  if (m <= 0 || m > (1 << 20)) return false;
  const int64_t M = round_up(m, DGP_TILE_HOST);
  return row0 >= 0 && col0 >= 0 && col0 <= row0 && row0 < row1 && row1 <= M && row0 % DGP_TILE_HOST == 0 &&
         row1 % DGP_TILE_HOST == 0 && col0 % DGP_TILE_HOST == 0;
}
template <typename T>
static int post_block(dgp_plan* p, const double* theta, const void* Xs, int64_t m, long row0, long row1, long col0, void* work, void* out,
                      hipStream_t s) {
  const long ld = row1 - col0;
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, posterior_areas<T>(p, m, work, 0).own, s)) return rc;
  if (int rc = ps.zero_noise()) return rc;
  return ps.band((T*)out, row0, row1, col0, ld, (row1 - row0) * ld);
}

extern "C" {

size_t dgp_posterior_cov_block_workspace_bytes(const dgp_plan* p, int64_t m, int64_t row0, int64_t row1, int64_t col0) {
  if (!p || !block_ok(m, row0, row1, col0)) return 0;
  return posterior_head_bytes(p, m, Carve::up(p->elem * (size_t)m));
}

int dgp_posterior_cov_block(dgp_plan* p, const double* theta, const void* Xs, int64_t m, int64_t row0, int64_t row1, int64_t col0,
                            void* work, size_t work_bytes, void* out, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !out) return fail(DGP_E_ARG, "dgp_posterior_cov_block: null argument");
  if (!block_ok(m, row0, row1, col0))
    return fail(DGP_E_ARG, "dgp_posterior_cov_block: bad block (1 <= m <= 2^20; row0, row1, col0 multiples of 128 with "
                           "0 <= col0 <= row0 < row1 <= padded m)");
  return posterior_entry(p, "dgp_posterior_cov_block", work, work_bytes, dgp_posterior_cov_block_workspace_bytes(p, m, row0, row1, col0), stream,
                         [&](auto t, hipStream_t s) {
                           return post_block<decltype(t)>(p, theta, Xs, m, (long)row0, (long)row1, (long)col0, work, out, s);
                         });
}

size_t dgp_window_variances_workspace_bytes(int64_t m, int64_t q, int batch) {
  if (!wv_sizes_ok(m, q, batch)) return 0;
  return ws_area_bytes(round_up(m, DGP_TILE_HOST), round_up(q, DGP_TILE_HOST), batch);
}

int dgp_window_variances(int dtype, int mode, const void* cov, int64_t m, int batch, const void* mu, const double* scale2,
                         const double* a, const int32_t* lo, const int32_t* hi, int64_t q, void* work, size_t work_bytes,
                         double* mean_out, double* var_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_window_variances: dtype must be 0 (f64) or 1 (f32)");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_window_variances: mode must be 0 (linear) or 1 (log)");
  if (!cov || !mu || !lo || !hi || !mean_out || !var_out || (mode == 1 && !scale2))
    return fail(DGP_E_ARG, "dgp_window_variances: null argument");
  if (!wv_sizes_ok(m, q, batch))
    return fail(DGP_E_ARG, "dgp_window_variances: bad size (1 <= m <= 2^20, 1 <= q <= 2^20, 1 <= batch <= 1024)");
  if (!work || work_bytes < dgp_window_variances_workspace_bytes(m, q, batch))
    return fail(DGP_E_WORKSPACE, "dgp_window_variances: workspace missing or too small");
  if (((uintptr_t)work & 7) != 0) return fail(DGP_E_ARG, "dgp_window_variances: the work area must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (dtype == DGP_F64)
    rc = mode == 1 ? window_variances_mode<double, 1>((const double*)cov, m, batch, (const double*)mu, scale2, a, lo, hi, q, work, mean_out, var_out, s)
                   : window_variances_mode<double, 0>((const double*)cov, m, batch, (const double*)mu, scale2, a, lo, hi, q, work, mean_out, var_out, s);
  else
    rc = mode == 1 ? window_variances_mode<float, 1>((const float*)cov, m, batch, (const float*)mu, scale2, a, lo, hi, q, work, mean_out, var_out, s)
                   : window_variances_mode<float, 0>((const float*)cov, m, batch, (const float*)mu, scale2, a, lo, hi, q, work, mean_out, var_out, s);
  return wrap(rc, "dgp_window_variances");
}

size_t dgp_posterior_window_variances_workspace_bytes(const dgp_plan* p, int64_t m, int64_t q, int64_t reach, int panel_rows) {
  if (!p || !wv_sizes_ok(m, q, p->B) || !wv_panel_ok(reach, panel_rows)) return 0;
  return posterior_head_bytes(p, m, wv_band_bytes(p, m, reach, panel_rows)) +
         ws_area_bytes(round_up(m, DGP_TILE_HOST), round_up(q, DGP_TILE_HOST), p->B);
}

int dgp_posterior_window_variances(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* mu, const double* scale2,
                                   const double* a, const int32_t* lo, const int32_t* hi, int64_t q, int mode, int64_t reach,
                                   int panel_rows, void* work, size_t work_bytes, double* mean_out, double* var_out, void* stream) {
  const char* where = "dgp_posterior_window_variances";
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_posterior_window_variances: mode must be 0 (linear) or 1 (log)");
  if (!theta || !Xs || !mu || !lo || !hi || !mean_out || !var_out || (mode == 1 && !scale2))
    return fail(DGP_E_ARG, "dgp_posterior_window_variances: null argument");
  if (!wv_sizes_ok(m, q, p->B))
    return fail(DGP_E_ARG, "dgp_posterior_window_variances: bad size (1 <= m <= 2^20, 1 <= q <= 2^20)");
  if (reach < 1 || reach > (1 << 20)) return fail(DGP_E_ARG, "dgp_posterior_window_variances: reach must be in 1 .. 2^20");
  if (!panel_rows_ok(panel_rows))
    return fail(DGP_E_ARG, "dgp_posterior_window_variances: panel_rows must be a positive multiple of 128");
  if (int rc = need_factor(p, where, "call dgp_factorize or dgp_fit_step")) return rc;
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  int rc = need_work(work, work_bytes, dgp_posterior_window_variances_workspace_bytes(p, m, q, reach, panel_rows), where);
  if (rc || (rc = factor_ok(p, s, where))) return rc;
  std::vector<int> flags((size_t)p->B, 0);
  rc = DGP_BY_DTYPE(p, post_window<double>(p, theta, Xs, m, mu, scale2, a, lo, hi, q, mode, reach, panel_rows, work, mean_out, var_out, s, flags.data()),
                    post_window<float>(p, theta, Xs, m, mu, scale2, a, lo, hi, q, mode, reach, panel_rows, work, mean_out, var_out, s, flags.data()));
  // the flags travel behind the pass (the host vector must outlive the copy: the stream is synchronised either way)
  const hipError_t he = hipStreamSynchronize(s);
  if (rc) return wrap(rc, where);
  if (he != hipSuccess) return hipfail(he, where);
  for (int f : flags)
    if (f) return fail(DGP_E_ARG, "dgp_posterior_window_variances: a window holds more than reach points");
  return 0;
}

}  // extern "C"
