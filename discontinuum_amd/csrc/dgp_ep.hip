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
#include "dgp_plan.h"

namespace dgp {

// The work area is an EpLayout: a CensoredLayout first (the terms pass at f = m validates the rows and gives the cold start; its
// rt holds r~, its `out` the result row of the sweep's factorisation), then the proposals, the previous means, k and the partials.
#define EP_PART 8  // doubles per workgroup of the block partials
enum {
  EP_ST_DMU = 0,  // max |mu - mu_prev| of the sweep (first sweep: max v |nu' - nu~|); inf when the factorisation failed
  EP_ST_DTAU,     // max v |tau' - tau~|
  EP_ST_CAPPED,   // proposals at the cap
  EP_ST_HELD,     // rows held back by the guard (v_c <= 0 or 1 - W v_c <= 0)
  EP_ST_NCENS,
  EP_ST_DONE,     // 0: the sweeps go on; k > 0: ended in sweep k (converged, or not positive definite)
  EP_ST_INFO,     // DGP_OUT_INFO of the sweep's factorisation
  EP_ST_CONV,     // 1: both tests passed
  EP_ST_CORR,     // NLL_EP - NLL_engine (ep_result)
  EP_ST_LEN = 16
};
struct EpLayout {
  CensoredLayout cen;
  size_t yprop, nprop, muprev, kdiag, kpart, part, status, total;  // byte offsets
  int nchunk, nblk;
};

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

static EpLayout ep_layout(long N, long n) {
  EpLayout L;
  L.cen = censored_layout(N, n, 1);
  const size_t vec = sizeof(double) * (size_t)n;
  Carve c;
  c.o = L.cen.total;
  L.yprop = c.take(vec);
  L.nprop = c.take(vec);
  L.muprev = c.take(vec);
  L.kdiag = c.take(vec);
  L.nchunk = (int)((n + EP_DIAG_ROWS - 1) / EP_DIAG_ROWS);
  L.kpart = c.take(sizeof(double) * (size_t)L.nchunk * (size_t)N);
  L.nblk = (int)((n + 255) / 256);
  L.part = c.take(sizeof(double) * (size_t)L.nblk * EP_PART);
  L.status = c.take(sizeof(double) * EP_ST_LEN);
  L.total = c.o;
  return L;
}

// the sites before the first sweep, after censored_terms(f = m, init) has filled L.cen: cold != 0: every censored row from the
// Laplace terms at m; else the caller's (a row without a usable site starts cold).  Rows of side 0: (y, v).  Writes r~ to L.cen.rt.
static int ep_init(const double* y, const int* side, const double* v, const double* m, double* yt, double* nt, int n, int cold, char* work,
            const EpLayout& L, hipStream_t s) {
  double* rt = (double*)(work + L.cen.rt);
  ep_init_kernel<<<dim3((unsigned)L.nblk), 256, 0, s>>>(y, side, v, m, rt, (const double*)(work + L.cen.nn), yt, nt, rt, n, cold);
  return (int)hipGetLastError();
}

// k_i = sum_{j >= i} T_ji^2, i < n, from the row-major lower triangle T = L^-1 (leading dimension N)
static int ep_diag(const double* Tm, long N, int n, double* k, char* work, const EpLayout& L, hipStream_t s) {
  double* kpart = (double*)(work + L.kpart);
  ep_diag_kernel<<<dim3((unsigned)((n + 63) / 64), (unsigned)L.nchunk), 256, 0, s>>>(Tm, N, n, kpart);
  ep_diag_sum_kernel<<<dim3((unsigned)L.nblk), 256, 0, s>>>(kpart, N, n, k);
  return (int)hipGetLastError();
}

// after the factorisation at (r~, n~) left T and alpha in the plan and its result row in L.cen.out: k, proposals, test, status; the
// proposals replace the sites (and r~) only when the sweep neither converged nor is the last
static int ep_sweep(const double* Tm, long N, const double* alpha, const double* y, const int* side, const double* v, const double* m,
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

// out[DGP_OUT_NLL] += NLL_EP - NLL_engine (out null: not wanted) from alpha and L.kdiag; cavities and log Z^ (n doubles each, nullable)
static int ep_result(const double* alpha, const double* y, const int* side, const double* v, const double* upper, const double* yt,
                     const double* nt, int n, double* out, double* cav_mean, double* cav_var, double* logz, char* work, const EpLayout& L,
                     hipStream_t s) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  ep_result_kernel<<<dim3((unsigned)L.nblk), 256, 0, s>>>(y, side, v, upper, yt, nt, alpha, D(L.kdiag), n, cav_mean, cav_var, logz,
                                                          D(L.part));
  ep_result_finish_kernel<<<dim3(1), 256, 0, s>>>(D(L.part), L.nblk, out, D(L.status));
  return (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

// ---- the entries: parallel sweeps on the factorise path, then (fit step) one step at the final sites, whose explicit gradient IS
// the gradient at the fixed point.  The host reads one status block per sweep.  The sites that were factorised last are the result
// (a converged or last sweep's proposal is not applied), so the plan's factorisation, k, the cavities and log Z^ belong to one
// state.  stat: [6].
static int ep(dgp_plan* p, const double* theta, const double* y, const double* mean, const double* noise, const int* side,
              const double* upper, double* yt, double* nt, int cold, int maxit, double tol, double damping, char* work, double* out,
              double* dr, double* stat, double* cav_mean, double* cav_var, double* logz, int with_grad, const char* where, hipStream_t s) {
  const EpLayout L = ep_layout(p->N, p->n);
  const Batch bt = batch_of<double>(p);
  auto D = [&](size_t off) { return (double*)(work + off); };
  const int n = (int)p->n;
  const double* alpha = (const double*)p->alpha;
  const double* Tm = (const double*)p->Tm;
  double st[CEN_ST_LEN > EP_ST_LEN ? CEN_ST_LEN : EP_ST_LEN];
  auto read_status = [&](size_t off, int len) -> int {
    hipError_t e = hipMemcpyAsync(st, D(off), sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
  };
  int rc;
  for (int k = 0; k < 6; ++k) stat[k] = 0.0;
  // the Laplace terms at f = m: the rows are checked as the Laplace entries check them, and a cold start is their pseudo-data
  if ((rc = censored_terms(mean, y, side, noise, mean, n, 1, 0, work, L.cen, s, bt, upper)) || (rc = read_status(L.cen.status, CEN_ST_LEN)))
    return rc;
  if (st[CEN_ST_BAD] != 0.0)
    return failf(DGP_E_ARG,
                 upper ? "%s: side values must be -1, 0, +1 or 2" : "%s: a row of side 2 needs upper_dev; other side values must be -1, 0 or +1",
                 where);
  if (st[CEN_ST_BADBRK] != 0.0)
    return failf(DGP_E_ARG, "%s: %d bad bracket(s): a row of side 2 needs a finite upper above its y", where, (int)st[CEN_ST_BADBRK]);
  const double ncens = st[CEN_ST_NCENS];
  stat[5] = ncens;
  const bool aux = cav_mean || cav_var || logz;
  if (ncens == 0.0) {  // nothing censored: the plain step on (y - m, v), bit for bit; the sites are (y, v)
    if ((rc = fit_step<double>(p, theta, D(L.cen.rt), D(L.cen.nn), out, with_grad ? dr : nullptr, with_grad ? D(L.cen.dnoise) : nullptr,
                               with_grad, s)) ||
        (rc = ep_init(y, side, noise, mean, yt, nt, n, 1, work, L, s)))
      return rc;
    if (aux && ((rc = ep_diag(Tm, p->N, n, D(L.kdiag), work, L, s)) ||
                (rc = ep_result(alpha, y, side, noise, upper, yt, nt, n, nullptr, cav_mean, cav_var, logz, work, L, s))))
      return rc;
    return 0;
  }
  if ((rc = ep_init(y, side, noise, mean, yt, nt, n, cold, work, L, s))) return rc;
  int it = 0;
  bool conv = false;
  for (;;) {
    if ((rc = fit_step<double>(p, theta, D(L.cen.rt), nt, D(L.cen.out), nullptr, nullptr, 0, s))) return rc;
    ++it;
    if ((rc = ep_sweep(Tm, p->N, alpha, y, side, noise, mean, upper, yt, nt, n, it, it >= maxit, tol, damping, work, L, s)) ||
        (rc = read_status(L.status, EP_ST_LEN)))
      return rc;
    stat[0] = (double)it;
    stat[1] = st[EP_ST_DMU];
    stat[2] = st[EP_ST_DTAU];
    stat[3] = st[EP_ST_CAPPED];
    stat[4] = st[EP_ST_HELD];
    conv = st[EP_ST_DONE] != 0.0;  // converged, or not positive definite: the result row reports that through DGP_OUT_INFO
    if (conv || it >= maxit) break;
  }
  if (with_grad) {
    // the same system once more with K^^-1 and the gradient contraction: the same T and alpha, so k stays valid
    if ((rc = fit_step<double>(p, theta, D(L.cen.rt), nt, out, dr, D(L.cen.dnoise), 1, s))) return rc;
  } else if ((rc = (int)hipMemcpyAsync(out, D(L.cen.out), sizeof(double) * DGP_OUT_LEN, hipMemcpyDeviceToDevice, s))) {
    return rc;
  }
  if ((rc = ep_result(alpha, y, side, noise, upper, yt, nt, n, out, cav_mean, cav_var, logz, work, L, s)) || (rc = (int)hipStreamSynchronize(s)))
    return rc;
  if (!conv)
    return failf(DGP_E_NOCONV, "%s: expectation propagation did not converge in %d sweeps (max |dmu| = %.3g, max v |dtau| = %.3g)", where, it,
                 stat[1], stat[2]);
  return 0;
}
static int ep_entry(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                    const void* upper, void* yt, void* nt, int cold, int maxit, double tol, double damping, void* work, size_t work_bytes,
                    void* out, void* dr, double* stat, void* cav_mean, void* cav_var, void* logz, int with_grad, const char* where,
                    void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64 || p->B != 1)
    return failf(DGP_E_ARG, "%s: expectation propagation needs a float64 single-site plan (fp32 and batched plans are not supported)", where);
  if (!theta || !y || !mean || !noise || !side || !yt || !nt || !out || !stat || maxit < 1 || !(tol >= 0.0))
    return failf(DGP_E_ARG, "%s: null argument (ytilde_dev / ntilde_dev included), maxit < 1 or a negative tol", where);
  if (!(damping > 0.0 && damping <= 1.0)) return failf(DGP_E_ARG, "%s: damping must lie in (0, 1]", where);
  DGP_CHECK_PLAN(p);
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_ep_*: call dgp_set_inputs first");
  if (!work || work_bytes < dgp_ep_workspace_bytes(p)) return failf(DGP_E_WORKSPACE, "%s: workspace missing or too small", where);
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_ep_*: the work area must be 256-byte aligned");
  const int rc = ep(p, theta, (const double*)y, (const double*)mean, (const double*)noise, (const int*)side, (const double*)upper,
                    (double*)yt, (double*)nt, cold, maxit, tol, damping, (char*)work, (double*)out, (double*)dr, stat, (double*)cav_mean,
                    (double*)cav_var, (double*)logz, with_grad, where, (hipStream_t)stream);
  if (rc == DGP_E_ARG || rc == DGP_E_NOCONV) return rc;  // text set where it arose
  return wrap(rc, where);
}

extern "C" {

size_t dgp_ep_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64 || p->B != 1) return 0;
  return ep_layout(p->N, p->n).total;
}

int dgp_ep_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                    const void* upper, void* ytilde, void* ntilde, int cold_start, int maxit, double tol, double damping, void* work,
                    size_t work_bytes, void* out, void* dr, double* stat, void* cav_mean, void* cav_var, void* logz, void* stream) {
  return ep_entry(p, theta, y, mean, noise, side, upper, ytilde, ntilde, cold_start, maxit, tol, damping, work, work_bytes, out, dr, stat,
                  cav_mean, cav_var, logz, 1, "dgp_ep_fit_step", stream);
}

int dgp_ep_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                     const void* upper, void* ytilde, void* ntilde, int cold_start, int maxit, double tol, double damping, void* work,
                     size_t work_bytes, void* out, double* stat, void* cav_mean, void* cav_var, void* logz, void* stream) {
  return ep_entry(p, theta, y, mean, noise, side, upper, ytilde, ntilde, cold_start, maxit, tol, damping, work, work_bytes, out, nullptr,
                  stat, cav_mean, cav_var, logz, 0, "dgp_ep_factorize", stream);
}

int dgp_ep_diag(dgp_plan* p, void* k, void* work, size_t work_bytes, void* stream) {
  if (!p || p->dtype != DGP_F64 || p->B != 1) return fail(DGP_E_ARG, "dgp_ep_diag: needs a float64 single-site plan");
  if (!k) return fail(DGP_E_ARG, "dgp_ep_diag: null argument");
  DGP_CHECK_PLAN(p);
  int rc = need_factor(p, "dgp_ep_diag", nullptr);
  if (rc || (rc = need_work(work, work_bytes, dgp_ep_workspace_bytes(p), "dgp_ep_diag"))) return rc;
  return wrap(ep_diag((const double*)p->Tm, p->N, (int)p->n, (double*)k, (char*)work, ep_layout(p->N, p->n), (hipStream_t)stream),
              "dgp_ep_diag");
}

}  // extern "C"
