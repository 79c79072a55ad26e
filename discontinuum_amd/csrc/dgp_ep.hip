// dgp_ep.hip -- censored observations by EXPECTATION PROPAGATION: Gaussian sites (y~_i, n~_i) on the censored rows, found by
// parallel sweeps of moment matching.  fp64, one site.
//
// An EP state is, like the Laplace mode, a GP regression on pseudo-data: a sweep is ONE factorisation of K + diag n~ with the
// residual r~ = y~ - m (dgp_factorize's launches, untouched), and everything else is O(n) except the diagonal of the inverse:
//     k_i   = [(K + diag n~)^-1]_ii = sum_{j >= i} T_ji^2,  T = L^-1 as the plan holds it
//     v_c   = 1 / k - n~,   mu_c = y~ - alpha / k                       the cavity = the leave-one-out predictive
//     log Z^, g, W  at  s = sqrt(v + v_c)  by the pointwise functions of the Laplace fit (dgp_censored_fn.h): one-sided rows
//           z = side (mu_c - l) / s, brackets za = (y - mu_c) / s, zb = (upper - mu_c) / s;  g = (.) / s,  W = (.) / s^2
//     tau'  = W / (1 - W v_c),  y' = mu_c + g / W                       (n' = 1 / tau' = 1 / W - v_c >= v)
//     cap   tau' v < CEN_CAP: tau' = CEN_CAP / v (y' kept);   guard  v_c <= 0 or 1 - W v_c <= 0: the row keeps its site this sweep
//     test  max_i |mu_i - mu_i^prev| <= tol (mu = y~ - n~ o alpha; first sweep: max v |nu' - nu~| over the censored rows, there is no
//           previous mean)  and  max v |tau' - tau~| <= tol.   Sigma_ii = n~ - n~^2 k is NOT tested: pure cancellation for flat sites.
//
//   ep_init_kernel      the sites before the first sweep: cold = the Laplace terms at f = m (cen_terms' r~, n~), warm = the caller's;
//                       rows of side 0 always (y, v)
//   ep_diag_kernel      k: column sums of squares of the row-major lower triangle T.  Workgroup = 64 columns x a chunk of 256 rows,
//                       4 row lanes: a wave reads 64 CONSECUTIVE COLUMNS of one row (512 contiguous bytes) per load, a column's rows
//                       are added in a fixed order (lane rows ascending, lanes 0..3, chunks ascending in ep_diag_sum_kernel).  n^2 / 2
//                       doubles of traffic, nothing else: memory-bound
//   ep_sites_kernel     one row per thread: cavity, moments, proposal, cap / guard, damping; PROPOSALS go to a second buffer;
//                       block partials of the two maxima and the three counts
//   ep_finish_kernel    one workgroup: reduces them in a fixed order, decides, writes the status block, and ONLY WHEN THE SWEEP HAS
//                       NOT CONVERGED (and is not the last) copies the proposals over the sites and refreshes r~.  The sites that
//                       were factorised therefore stay in place on convergence and at maxit: the factorisation, the cavities and
//                       log Z^ of the result belong to one state
//   ep_result_kernel    NLL_EP - NLL_engine = -sum_censored [log Z^_i + 1/2 log 2 pi - 1/2 log k_i + alpha_i^2 / (2 k_i)] as block
//                       partials (added to out[DGP_OUT_NLL] in a fixed order by ep_result_finish_kernel) and the optional cavity outputs
// No floating-point atomics; every result repeats bitwise.
#include "dgp_censored_fn.h"
#include "dgp_internal.h"

namespace dgp {

#define EP_DIAG_ROWS 256  // rows per partial sum of ep_diag_kernel
#define EP_LOG2PI 1.83787706640934548356

// block partials: columns [0, NMAX) are maxima, the rest sums; lane order then wave order
template <int K, int NMAX>
__device__ __forceinline__ void ep_block_reduce(double (&v)[K], double* __restrict__ part) {
  __shared__ double red[4][K];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    double x = v[q];
    if (q < NMAX) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
    } else {
      x = wave_sum(x);
    }
    if (lane == 0) red[wv][q] = x;
  }
  __syncthreads();
  if (t < K)
    part[(long)blockIdx.x * EP_PART + t] = t < NMAX ? fmax(fmax(red[0][t], red[1][t]), fmax(red[2][t], red[3][t]))
                                                    : red[0][t] + red[1][t] + red[2][t] + red[3][t];
}
// second stage, one workgroup: column q of nblk rows of partials -> tot[q]
template <int K, int NMAX>
__device__ __forceinline__ void ep_total(const double* __restrict__ part, int nblk, double* tot /* LDS [EP_PART] */) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  for (int q = 0; q < K; ++q) {
    double v = 0.0;
    for (int b = t; b < nblk; b += 256) v = q < NMAX ? fmax(v, part[(long)b * EP_PART + q]) : v + part[(long)b * EP_PART + q];
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] = q < NMAX ? fmax(red[t], red[t + s]) : red[t] + red[t + s];
      __syncthreads();
    }
    if (t == 0) tot[q] = red[0];
    __syncthreads();
  }
}

// rt_cold / nn_cold: cen_terms' pass at f = m; rt (the same buffer as rt_cold: each thread reads its entry before it writes it)
// receives r~ = y~ - m.  A warm row whose site is not a finite y~ with a positive finite n~ starts cold.
__global__ __launch_bounds__(256) void ep_init_kernel(const double* __restrict__ y, const int* __restrict__ side,
                                                      const double* __restrict__ v, const double* __restrict__ m, const double* rt_cold,
                                                      const double* __restrict__ nn_cold, double* __restrict__ yt, double* __restrict__ nt,
                                                      double* rt, int n, int cold) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double rc = rt_cold[i];
  if (side[i] == 0) {
    yt[i] = y[i];
    nt[i] = v[i];
    rt[i] = rc;  // y - m as the plain step's caller would form it
    return;
  }
  double ys = yt[i], ns = nt[i];
  const double inf = __builtin_inf();
  if (cold || !(ns > 0.0 && ns < inf && fabs(ys) < inf)) {
    ys = m[i] + rc;
    ns = nn_cold[i];
    yt[i] = ys;
    nt[i] = ns;
  }
  rt[i] = ys - m[i];
}

// kpart[chunk][j] = sum over the chunk's rows i >= j, i < n of T[i][j]^2.  Only entries of the lower triangle are read (T is not
// initialised everywhere above its diagonal blocks); a tile above the diagonal leaves without writing, and the sum below skips it.
__global__ __launch_bounds__(256) void ep_diag_kernel(const double* __restrict__ T, long ld, int n, double* __restrict__ kpart) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long j = (long)blockIdx.x * 64 + tx;
  const long r0 = (long)blockIdx.y * EP_DIAG_ROWS;
  const long r1 = min(r0 + (long)EP_DIAG_ROWS, (long)n);
  if (r1 <= (long)blockIdx.x * 64) return;  // (workgroup-uniform)
  __shared__ double red[4][64];
  const long rs = max(r0, (long)blockIdx.x * 64);
  double acc = 0.0;
  if (j < n) {
    long i = rs + ty;
    for (; i + 12 < r1; i += 16) {  // four rows in flight per thread
      const double a = i >= j ? T[i * ld + j] : 0.0, b = i + 4 >= j ? T[(i + 4) * ld + j] : 0.0;
      const double c = i + 8 >= j ? T[(i + 8) * ld + j] : 0.0, d = i + 12 >= j ? T[(i + 12) * ld + j] : 0.0;
      acc += a * a;
      acc += b * b;
      acc += c * c;
      acc += d * d;
    }
    for (; i < r1; i += 4) {
      const double a = i >= j ? T[i * ld + j] : 0.0;
      acc += a * a;
    }
  }
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0) kpart[(long)blockIdx.y * ld + j] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}
__global__ __launch_bounds__(256) void ep_diag_sum_kernel(const double* __restrict__ kpart, long ld, int n, double* __restrict__ k) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int nchunk = (int)((n + EP_DIAG_ROWS - 1) / EP_DIAG_ROWS);
  double acc = 0.0;
  for (int c = (int)(j / EP_DIAG_ROWS); c < nchunk; ++c) acc += kpart[(long)c * ld + j];
  k[j] = acc;
}

struct EpTilt {
  double logz, g, W;
};
// the tilted distribution N(f | mu_c, v_c) p(y | f) of a censored row: s = sqrt(v + v_c)
__device__ __forceinline__ EpTilt ep_tilt(int s, double yi, double ui, double vi, double muc, double vc) {
  EpTilt o;
  const double sd = sqrt(vi + vc);
  if (s == 2) {
    const IntFn f = iv_fn((yi - muc) / sd, (ui - muc) / sd, (ui - yi) / sd);
    o.logz = f.logp;
    o.g = f.mu / sd;
    o.W = f.wv / (sd * sd);
  } else {
    const double sg = (double)s;
    const CenFn f = cen_fn(sg * (muc - yi) / sd);
    o.logz = f.logphi;
    o.g = sg * f.h / sd;
    o.W = f.q / (sd * sd);
  }
  return o;
}

// partial columns: max d_mu, max d_tau | capped, held, censored
__global__ __launch_bounds__(256) void ep_sites_kernel(const double* __restrict__ y, const int* __restrict__ side,
                                                       const double* __restrict__ v, const double* __restrict__ upper,
                                                       const double* __restrict__ yt, const double* __restrict__ nt,
                                                       const double* __restrict__ alpha, const double* __restrict__ kdiag,
                                                       double* __restrict__ muprev, double* __restrict__ yprop, double* __restrict__ nprop,
                                                       int n, int sweep, double damping, double cap, double* __restrict__ part) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const double inf = __builtin_inf();
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const int s = side[i];
    const double ys = yt[i], ns = nt[i], a = alpha[i], k = kdiag[i], vi = v[i];
    const double mu = ys - ns * a;
    if (sweep > 1) {
      const double d = fabs(mu - muprev[i]);
      acc[0] = d == d ? d : inf;
    }
    muprev[i] = mu;
    double yp = ys, np = ns;
    if (s != 0) {
      acc[4] = 1.0;
      const double vc = 1.0 / k - ns, muc = ys - a / k;
      bool ok = vc > 0.0 && vc < inf;
      if (ok) {
        const EpTilt o = ep_tilt(s, y[i], s == 2 ? upper[i] : 0.0, vi, muc, vc);
        const double om = 1.0 - o.W * vc;
        ok = om > 0.0 && fabs(o.g) < inf && o.W == o.W;
        if (ok) {
          double taup = o.W / om;
          const bool capped = !(taup * vi >= cap);
          if (capped) taup = cap / vi;
          const double ypp = muc + (o.W > 0.0 ? o.g / o.W : 0.0);
          const double tau = 1.0 / ns, nu = ys / ns, nup = ypp * taup;
          const double dt = vi * fabs(taup - tau);
          acc[1] = dt == dt ? dt : inf;
          if (sweep == 1) {
            const double dn = vi * fabs(nup - nu);
            acc[0] = dn == dn ? dn : inf;
          }
          acc[2] = capped ? 1.0 : 0.0;
          if (damping == 1.0) {
            np = 1.0 / taup;
            yp = ypp;
          } else {
            const double tn = (1.0 - damping) * tau + damping * taup, nn = (1.0 - damping) * nu + damping * nup;
            np = 1.0 / tn;
            yp = nn / tn;
          }
        }
      }
      if (!ok) acc[3] = 1.0;
    }
    yprop[i] = yp;
    nprop[i] = np;
  }
  ep_block_reduce<5, 2>(acc, part);
}

// outblk: the result row of the sweep's factorisation (DGP_OUT_INFO != 0: not positive definite -- the search ends, nothing moves)
__global__ __launch_bounds__(256) void ep_finish_kernel(const double* __restrict__ part, int nblk, int sweep, int last, double tol,
                                                        const double* __restrict__ outblk, double* __restrict__ status,
                                                        const double* __restrict__ m, const double* __restrict__ yprop,
                                                        const double* __restrict__ nprop, double* __restrict__ yt,
                                                        double* __restrict__ nt, double* __restrict__ rt, int n) {
  __shared__ double tot[EP_PART];
  ep_total<5, 2>(part, nblk, tot);
  const double info = outblk[3];
  const bool conv = info == 0.0 && tot[0] <= tol && tot[1] <= tol;
  const bool done = conv || info != 0.0;
  if (threadIdx.x == 0) {
    status[EP_ST_DMU] = info == 0.0 ? tot[0] : __builtin_inf();
    status[EP_ST_DTAU] = info == 0.0 ? tot[1] : __builtin_inf();
    status[EP_ST_CAPPED] = tot[2];
    status[EP_ST_HELD] = tot[3];
    status[EP_ST_NCENS] = tot[4];
    status[EP_ST_DONE] = done ? (double)sweep : 0.0;
    status[EP_ST_INFO] = info;
    status[EP_ST_CONV] = conv ? 1.0 : 0.0;
  }
  if (done || last) return;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double ys = yprop[i];
    yt[i] = ys;
    nt[i] = nprop[i];
    rt[i] = ys - m[i];
  }
}

// the correction and the optional outputs at the final state.  Rows of side 0: their cavity too, and log Z^ = log N(y | mu_c, v + v_c)
__global__ __launch_bounds__(256) void ep_result_kernel(const double* __restrict__ y, const int* __restrict__ side,
                                                        const double* __restrict__ v, const double* __restrict__ upper,
                                                        const double* __restrict__ yt, const double* __restrict__ nt,
                                                        const double* __restrict__ alpha, const double* __restrict__ kdiag, int n,
                                                        double* __restrict__ cav_mean, double* __restrict__ cav_var,
                                                        double* __restrict__ logz, double* __restrict__ part) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double acc[1] = {0.0};
  if (i < n) {
    const int s = side[i];
    const double a = alpha[i], k = kdiag[i], vi = v[i], yi = y[i];
    const double vc = 1.0 / k - nt[i], muc = yt[i] - a / k;
    double lz;
    if (s != 0) {
      lz = ep_tilt(s, yi, s == 2 ? upper[i] : 0.0, vi, muc, vc).logz;
      acc[0] = -(lz + 0.5 * EP_LOG2PI - 0.5 * log(k) + a * a / (2.0 * k));
    } else {
      const double e = yi - muc, s2 = vi + vc;
      lz = -0.5 * e * e / s2 - 0.5 * log(6.28318530717958647692 * s2);
    }
    if (cav_mean) cav_mean[i] = muc;
    if (cav_var) cav_var[i] = vc;
    if (logz) logz[i] = lz;
  }
  ep_block_reduce<1, 0>(acc, part);
}
__global__ __launch_bounds__(256) void ep_result_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out,
                                                               double* __restrict__ status) {
  __shared__ double tot[EP_PART];
  ep_total<1, 0>(part, nblk, tot);
  if (threadIdx.x != 0) return;
  if (out) out[0] += tot[0];  // DGP_OUT_NLL
  status[EP_ST_CORR] = tot[0];
}

EpLayout ep_layout(long N, long n) {
  EpLayout L;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  L.cen = censored_layout(N, n, 1);
  const size_t vec = al(sizeof(double) * (size_t)n);
  size_t o = L.cen.total;
  L.yprop = o; o += vec;
  L.nprop = o; o += vec;
  L.muprev = o; o += vec;
  L.kdiag = o; o += vec;
  L.nchunk = (int)((n + EP_DIAG_ROWS - 1) / EP_DIAG_ROWS);
  L.kpart = o; o += al(sizeof(double) * (size_t)L.nchunk * (size_t)N);
  L.nblk = (int)((n + 255) / 256);
  L.part = o; o += al(sizeof(double) * (size_t)L.nblk * EP_PART);
  L.status = o; o += al(sizeof(double) * EP_ST_LEN);
  L.total = o;
  return L;
}

int ep_init(const double* y, const int* side, const double* v, const double* m, double* yt, double* nt, int n, int cold, char* work,
            const EpLayout& L, hipStream_t s) {
  double* rt = (double*)(work + L.cen.rt);
  ep_init_kernel<<<dim3((unsigned)L.nblk), 256, 0, s>>>(y, side, v, m, rt, (const double*)(work + L.cen.nn), yt, nt, rt, n, cold);
  return (int)hipGetLastError();
}

int ep_diag(const double* Tm, long N, int n, double* k, char* work, const EpLayout& L, hipStream_t s) {
  double* kpart = (double*)(work + L.kpart);
  ep_diag_kernel<<<dim3((unsigned)((n + 63) / 64), (unsigned)L.nchunk), 256, 0, s>>>(Tm, N, n, kpart);
  ep_diag_sum_kernel<<<dim3((unsigned)L.nblk), 256, 0, s>>>(kpart, N, n, k);
  return (int)hipGetLastError();
}

int ep_sweep(const double* Tm, long N, const double* alpha, const double* y, const int* side, const double* v, const double* m,
             const double* upper, double* yt, double* nt, int n, int sweep, int last, double tol, double damping, char* work,
             const EpLayout& L, hipStream_t s) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  int rc;
  if ((rc = ep_diag(Tm, N, n, D(L.kdiag), work, L, s))) return rc;
  ep_sites_kernel<<<dim3((unsigned)L.nblk), 256, 0, s>>>(y, side, v, upper, yt, nt, alpha, D(L.kdiag), D(L.muprev), D(L.yprop), D(L.nprop),
                                                         n, sweep, damping, CEN_CAP, D(L.part));
  ep_finish_kernel<<<dim3(1), 256, 0, s>>>(D(L.part), L.nblk, sweep, last, tol, D(L.cen.out), D(L.status), m, D(L.yprop), D(L.nprop), yt,
                                           nt, D(L.cen.rt), n);
  return (int)hipGetLastError();
}

int ep_result(const double* alpha, const double* y, const int* side, const double* v, const double* upper, const double* yt,
              const double* nt, int n, double* out, double* cav_mean, double* cav_var, double* logz, char* work, const EpLayout& L,
              hipStream_t s) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  ep_result_kernel<<<dim3((unsigned)L.nblk), 256, 0, s>>>(y, side, v, upper, yt, nt, alpha, D(L.kdiag), n, cav_mean, cav_var, logz,
                                                          D(L.part));
  ep_result_finish_kernel<<<dim3(1), 256, 0, s>>>(D(L.part), L.nblk, out, D(L.status));
  return (int)hipGetLastError();
}

}  // namespace dgp
