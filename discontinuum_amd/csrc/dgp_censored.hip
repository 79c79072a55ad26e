// dgp_censored.hip -- censored observations (non-detects): the Laplace approximation of a GP with a Tobit likelihood.
//
// Row i of a site of an fp64 plan (single-site or batched: blockIdx.z = site, ragged sizes through site_n) is either observed (side 0: Gaussian, variance v_i) or censored at the limit l_i
// (side s_i = -1: the truth lies below it, +1: above):  log p_i = log Phi(z_i),  z_i = s_i (f_i - l_i) / sigma_i.
// With h = phi(z) / Phi(z),
//     g_i  =  d log p_i / d f_i     =  s_i h / sigma_i
//     W_i  = -d^2 log p_i / d f_i^2 =  h (z + h) / v_i               in (0, 1 / v_i)
//     d3_i =  d^3 log p_i / d f_i^3 = -(s_i / sigma_i^3) h [1 - (z + h)(z + 2 h)]
// A fourth kind, side 2, is INTERVAL-censored: the truth lies in [y_i, upper_i], log p_i = log[Phi(zb) - Phi(za)] (iv_fn below:
// the same three derivatives, the same Newton / pseudo-data / correction / sweep machinery; `upper` is an optional pointer of the
// terms and search kernels, and without it 2 is a bad side value and every bit is what it was).
// At the mode the posterior of f is the exact GP posterior for the pseudo-targets y~_i = f_i + g_i / W_i with the
// pseudo-noise n~_i = 1 / W_i (observed rows: y~ = y, n~ = v).  A Newton step is therefore ONE factorisation with the
// residual r~ = y~ - m and the noise n~:  a = (K + diag n~)^-1 r~,  f_new = m + K a = y~ - n~ o a  (no product with K).
//
//   cen_terms_kernel    one elementwise pass: r~, n~, g, W, d3 and the per-row part of the NLL correction; block partials
//   cen_search_kernel   the proposal f_new, max |f_new - f| and Psi(t) = sum log p_i(f(t)) - 1/2 a(t)^T (f(t) - m) on
//                       t in {0, 1, 1/2, .., 1/64} in one pass (f and a are linear in t); block partials
//   cen_*_finish        one workgroup per site, fixed order: no floating-point atomics anywhere, every result repeats bitwise
//   gram_bilinear       sum_ij u_i dK_ij/dtheta_p a_j for all p in one sweep over the lower triangle (sibling of
//                       dgp_gram.hip::gram_grad_kernel: same tiling, staging and two-stage reduction; weights
//                       u_i a_j + u_j a_i, the diagonal once) -- dK/dtheta is never stored
// The non-destructive solve u = T^T (T w) is dgp_chol.hip::solve_work: z, u and the partials in the caller's work area.
// A batch runs Newton's iterations in lockstep (each factorises all sites); a site that has finished is frozen (CEN_ST_DONE).
// Roofline: the elementwise passes are O(n) and latency-bound; the sweep is VALU-bound like gram_grad (one derivative pair
// evaluation per entry of the triangle, nothing streamed from HBM but the two vectors).
#include <vector>

#include "dgp_censored_fn.h"
#include "dgp_gram_shared.h"
#include "dgp_plan.h"
#include "dgp_models.h"

namespace dgp {

// The pointwise functions of z (cen_fn, cen_logphi) and of a bracket (iv_fn, iv_logp) live in dgp_censored_fn.h.

__global__ __launch_bounds__(256) void cen_debug_kernel(const double* __restrict__ z, long count, double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const CenFn o = cen_fn(z[i]);
  out[i] = o.logphi;
  out[count + i] = o.h;
  out[2 * count + i] = o.q;
  out[3 * count + i] = o.c3;
}

static int debug_censored_terms(const double* z, long count, double* out, hipStream_t s) {
  cen_debug_kernel<<<dim3((unsigned)((count + 255) / 256)), 256, 0, s>>>(z, count, out);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void iv_debug_kernel(const double* __restrict__ za, const double* __restrict__ delta, long count,
                                                       double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const IntFn o = iv_fn(za[i], za[i] + delta[i], delta[i]);
  out[i] = o.logp;
  out[count + i] = o.mu;
  out[2 * count + i] = o.wv;
  out[3 * count + i] = o.d3;
}

static int debug_interval_terms(const double* za, const double* delta, long count, double* out, hipStream_t s) {
  iv_debug_kernel<<<dim3((unsigned)((count + 255) / 256)), 256, 0, s>>>(za, delta, count, out);
  return (int)hipGetLastError();
}

// block sums of K <= CEN_PART values per thread (column `maxcol`, if any, is a maximum), lane order then wave order
template <int K>
__device__ __forceinline__ void cen_block_reduce(double (&v)[K], int maxcol, double* __restrict__ part) {
  __shared__ double red[4][K];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    double x = v[q];
    if (q == maxcol) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
    } else {
      x = wave_sum(x);
    }
    if (lane == 0) red[wv][q] = x;
  }
  __syncthreads();
  if (t < K)
    part[(long)blockIdx.x * CEN_PART + t] = t == maxcol ? fmax(fmax(red[0][t], red[1][t]), fmax(red[2][t], red[3][t]))
                                                        : red[0][t] + red[1][t] + red[2][t] + red[3][t];
}
// the second stage: one workgroup, column q of nblk rows of partials -> tot[q], fixed strided order + fixed tree
__device__ __forceinline__ void cen_total(const double* __restrict__ part, int nblk, int K, int maxcol, double* tot /* LDS [CEN_PART] */) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  for (int q = 0; q < K; ++q) {
    double v = 0.0;
    for (int b = t; b < nblk; b += 256) v = q == maxcol ? fmax(v, part[(long)b * CEN_PART + q]) : v + part[(long)b * CEN_PART + q];
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] = q == maxcol ? fmax(red[t], red[t + s]) : red[t] + red[t + s];
      __syncthreads();
    }
    if (t == 0) tot[q] = red[0];
    __syncthreads();
  }
}

// ---- per-site control.  status: the site's CEN_ST_* block.  A site that finished in an earlier iteration than `it` (or has no
// censored row) is frozen; the one that finishes in `it` still takes its step and has its terms evaluated at the mode.
__device__ __forceinline__ bool cen_frozen(const double* __restrict__ status, int it) {
  const double d = status[CEN_ST_DONE];
  return d != 0.0 && d != (double)it;
}

// ---- terms at the current f.  y holds the observation (side 0), the limit (side +-1) or a bracket's lower end (side 2, with
// `upper`: its upper end; a bracket whose upper end is NaN, infinite or not above y is counted in the fifth sum).  Capped rows (W v < cap: the limit
// says nothing) get n~ = v / cap and d3 = 0.  corr: the row's part of the NLL correction that does not involve alpha.
// Every elementwise vector is [site][nfull]; `part` [site][nblk][CEN_PART]; status [site][CEN_ST_LEN].
__global__ __launch_bounds__(256) void cen_terms_kernel(const double* __restrict__ f, const double* __restrict__ y,
                                                        const int* __restrict__ side, const double* __restrict__ v,
                                                        const double* __restrict__ m, int n, const int* __restrict__ ns, double cap,
                                                        double* __restrict__ rt, double* __restrict__ nn, double* __restrict__ g,
                                                        double* __restrict__ W, double* __restrict__ d3, double* __restrict__ corr,
                                                        double* __restrict__ logp, double* __restrict__ part,
                                                        const double* __restrict__ status, int init, int it,
                                                        const double* __restrict__ upper) {
  status = site(status, (long)CEN_ST_LEN);
  if (!init && (cen_frozen(status, it) || status[CEN_ST_INFO] != 0.0)) return;
  const long nfull = n;
  n = site_n(ns, n);
  f = site(f, nfull); y = site(y, nfull); side = site(side, nfull); v = site(v, nfull); m = site(m, nfull);
  rt = site(rt, nfull); nn = site(nn, nfull); g = site(g, nfull); W = site(W, nfull); d3 = site(d3, nfull);
  corr = site(corr, nfull); logp = site(logp, nfull);
  if (upper) upper = site(upper, nfull);
  part = site(part, (long)gridDim.x * CEN_PART);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // correction, capped rows, bad side values, censored rows, bad brackets
  if (i < n) {
    const int s = side[i];
    const double vi = v[i], mi = m[i], yi = y[i], fi = f[i];
    const bool brk = s == 2 && upper != nullptr;  // (without `upper`, 2 is a bad side value)
    const double ui = brk ? upper[i] : 0.0;
    if (brk && ui > yi && ui < __builtin_inf()) {
      const double sg = sqrt(vi);
      const IntFn o = iv_fn((yi - fi) / sg, (ui - fi) / sg, (ui - yi) / sg);
      const bool capped = !(o.wv >= cap);
      const double ni = capped ? vi / cap : vi / o.wv, wi = 1.0 / ni, gi = o.mu / sg;
      rt[i] = (fi + gi * ni) - mi;
      nn[i] = ni;
      g[i] = gi;
      W[i] = wi;
      d3[i] = capped ? 0.0 : o.d3 / (sg * vi);
      const double c = -o.logp + 0.5 * log(wi) - 0.5 * 1.83787706640934548356;
      corr[i] = c;
      logp[i] = o.logp;
      acc[0] = c;
      acc[1] = capped ? 1.0 : 0.0;
      acc[3] = 1.0;
    } else if (s == 0 || (s != 1 && s != -1)) {
      const double e = yi - fi;
      rt[i] = yi - mi;
      nn[i] = vi;
      g[i] = e / vi;
      W[i] = 1.0 / vi;
      d3[i] = 0.0;
      corr[i] = 0.0;
      logp[i] = -0.5 * e * e / vi - 0.5 * log(6.28318530717958647692 * vi);
      acc[2] = (s == 0 || brk) ? 0.0 : 1.0;
      acc[4] = brk ? 1.0 : 0.0;  // NaN, infinite or not above y
    } else {
      const double sg = sqrt(vi), sd = (double)s;
      const CenFn o = cen_fn(sd * (fi - yi) / sg);
      const bool capped = !(o.q >= cap);
      const double ni = capped ? vi / cap : vi / o.q, wi = 1.0 / ni, gi = sd * o.h / sg;
      rt[i] = (fi + gi * ni) - mi;
      nn[i] = ni;
      g[i] = gi;
      W[i] = wi;
      d3[i] = capped ? 0.0 : -(sd / (sg * vi)) * o.c3;
      const double c = -o.logphi + 0.5 * log(wi) - 0.5 * 1.83787706640934548356;
      corr[i] = c;
      logp[i] = o.logphi;
      acc[0] = c;
      acc[1] = capped ? 1.0 : 0.0;
      acc[3] = 1.0;
    }
  }
  cen_block_reduce<5>(acc, -1, part);
}
__global__ __launch_bounds__(256) void cen_terms_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ status,
                                                               int init, int it) {
  status = site(status, (long)CEN_ST_LEN);
  if (!init && (cen_frozen(status, it) || status[CEN_ST_INFO] != 0.0)) return;
  part = site(part, (long)nblk * CEN_PART);
  __shared__ double tot[CEN_PART];
  cen_total(part, nblk, 5, -1, tot);
  if (threadIdx.x < 4) status[CEN_ST_CORR + threadIdx.x] = tot[threadIdx.x];
  if (init && threadIdx.x >= 4 && threadIdx.x < CEN_ST_LEN)
    status[threadIdx.x] = (threadIdx.x == CEN_ST_DONE && tot[3] == 0.0) ? -1.0 : (threadIdx.x == CEN_ST_BADBRK ? tot[4] : 0.0);
}

// ---- proposal and line search.  anew: the plan's alpha of the factorisation at (r~, n~); acur: the a of the current f (f - m =
// K acur), which the first step from a caller's f does not know.
__global__ __launch_bounds__(256) void cen_search_kernel(const double* __restrict__ f, const double* __restrict__ y,
                                                         const int* __restrict__ side, const double* __restrict__ v,
                                                         const double* __restrict__ m, const double* __restrict__ rt,
                                                         const double* __restrict__ nn, const double* __restrict__ anew, long as,
                                                         const double* __restrict__ acur, int n, const int* __restrict__ ns,
                                                         double* __restrict__ delta, double* __restrict__ part,
                                                         const double* __restrict__ status, const double* __restrict__ upper) {
  if (site(status, (long)CEN_ST_LEN)[CEN_ST_DONE] != 0.0) return;
  const long nfull = n;
  n = site_n(ns, n);
  f = site(f, nfull); y = site(y, nfull); side = site(side, nfull); v = site(v, nfull); m = site(m, nfull);
  rt = site(rt, nfull); nn = site(nn, nfull); acur = site(acur, nfull); delta = site(delta, nfull);
  anew = site(anew, as);
  if (upper) upper = site(upper, nfull);
  part = site(part, (long)gridDim.x * CEN_PART);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double acc[CEN_NT + 1];
#pragma unroll
  for (int j = 0; j <= CEN_NT; ++j) acc[j] = 0.0;
  if (i < n) {
    const int s = side[i];
    const double vi = v[i], mi = m[i], yi = y[i], fi = f[i], an = anew[i], ac = acur[i];
    const double dlt = (mi + rt[i] - nn[i] * an) - fi, da = an - ac, sg = sqrt(vi);
    const bool brk = s == 2 && upper != nullptr;  // (a bad bracket has ended the call after the first pass)
    const double ui = brk ? upper[i] : 0.0, dz = (ui - yi) / sg;
    delta[i] = dlt;
    acc[CEN_NT] = fabs(dlt);
    double t = 0.0;
#pragma unroll  // (acc[j] stays in registers)
    for (int j = 0; j < CEN_NT; ++j) {
      const double ft = fi + t * dlt, at = ac + t * da;
      double lp;
      if (s == 0) {
        const double e = yi - ft;
        lp = -0.5 * e * e / vi - 0.5 * log(6.28318530717958647692 * vi);
      } else if (brk) {
        lp = iv_logp((yi - ft) / sg, (ui - ft) / sg, dz);
      } else {
        lp = cen_logphi((double)s * (ft - yi) / sg);
      }
      acc[j] = lp - 0.5 * at * (ft - mi);
      t = j == 0 ? 1.0 : 0.5 * t;
    }
  }
  cen_block_reduce<CEN_NT + 1>(acc, CEN_NT, part);
}
// chooses the step: the whole step in the first iteration or when it is below tol, else the largest t of the set that does not
// lower Psi (slack: rounding of the sums).  status: max |delta|, t, halvings, the factorisation's info, Psi(0), Psi(t); the site is
// done (CEN_ST_DONE = it) when the proposal is within tol or the factorisation failed.
__global__ __launch_bounds__(256) void cen_search_finish_kernel(const double* __restrict__ part, int nblk, int it, double tol,
                                                                const double* __restrict__ outblk, double* __restrict__ status) {
  status = site(status, (long)CEN_ST_LEN);
  if (status[CEN_ST_DONE] != 0.0) return;
  part = site(part, (long)nblk * CEN_PART);
  outblk = site(outblk, 32L);
  __shared__ double tot[CEN_PART];
  cen_total(part, nblk, CEN_NT + 1, CEN_NT, tot);
  if (threadIdx.x != 0) return;
  const double dmax = tot[CEN_NT], info = outblk[3];
  int j = 1;
  if (it != 1 && !(dmax <= tol)) {
    const double floor_ = tot[0] - 1e-9 * (1.0 + fabs(tot[0]));
    while (j < CEN_NT - 1 && !(tot[j] >= floor_)) ++j;
  }
  double t = 1.0;
  for (int k = 1; k < j; ++k) t *= 0.5;
  const double dm = (info == 0.0 && dmax == dmax) ? dmax : __builtin_inf();
  status[CEN_ST_DMAX] = dm;
  status[CEN_ST_T] = t;
  status[CEN_ST_HALVINGS] = (double)(j - 1);
  status[CEN_ST_INFO] = info;
  status[CEN_ST_PSI0] = tot[0];
  status[CEN_ST_PSI] = tot[j];
  if (info != 0.0 || dm <= tol) status[CEN_ST_DONE] = (double)it;
}
// f <- f + t delta, acur <- acur + t (anew - acur); nothing moves when the factorisation failed or the site is frozen
__global__ __launch_bounds__(256) void cen_update_kernel(double* __restrict__ f, const double* __restrict__ delta,
                                                         double* __restrict__ acur, const double* __restrict__ anew, long as,
                                                         const double* __restrict__ status, int n, const int* __restrict__ ns, int it) {
  status = site(status, (long)CEN_ST_LEN);
  const long nfull = n;
  n = site_n(ns, n);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || status[CEN_ST_INFO] != 0.0 || cen_frozen(status, it)) return;
  f = site(f, nfull); delta = site(delta, nfull); acur = site(acur, nfull);
  anew = site(anew, as);
  const double t = status[CEN_ST_T];
  f[i] = t == 1.0 ? f[i] + delta[i] : f[i] + t * delta[i];
  acur[i] = t == 1.0 ? anew[i] : acur[i] + t * (anew[i] - acur[i]);
}
// the mode of the system just solved, for the sites without a censored row: f = m + r~ - n~ o alpha (the exact posterior mean at
// the samples)
__global__ __launch_bounds__(256) void cen_mode_kernel(double* __restrict__ f, const double* __restrict__ m,
                                                       const double* __restrict__ rt, const double* __restrict__ nn,
                                                       const double* __restrict__ alpha, long as, int n, const int* __restrict__ ns,
                                                       const double* __restrict__ status) {
  if (site(status, (long)CEN_ST_LEN)[CEN_ST_DONE] != -1.0) return;
  const long nfull = n;
  n = site_n(ns, n);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  f = site(f, nfull); m = site(m, nfull); rt = site(rt, nfull); nn = site(nn, nfull);
  alpha = site(alpha, as);
  f[i] = m[i] + rt[i] - nn[i] * alpha[i];
}

// ---- gradient.  (K^^-1)_ii = 2 dnoise_i + alpha_i^2;  Sigma_ii = n~_i - n~_i^2 (K^^-1)_ii;  t_i = -1/2 Sigma_ii d3_i;  w = n~ o t
__global__ __launch_bounds__(256) void cen_weight_kernel(const double* __restrict__ nn, const double* __restrict__ d3,
                                                         const double* __restrict__ dnoise, const double* __restrict__ alpha, long as,
                                                         int n, const int* __restrict__ ns, long N, double* __restrict__ w, long ws) {
  const long nfull = n;
  n = site_n(ns, n);
  nn = site(nn, nfull); d3 = site(d3, nfull); dnoise = site(dnoise, nfull);
  alpha = site(alpha, as);
  w = site(w, ws);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double wi = 0.0;
  if (i < n && d3[i] != 0.0) {
    const double a = alpha[i], kii = 2.0 * dnoise[i] + a * a, ni = nn[i];
    wi = ni * (-0.5 * (ni - ni * ni * kii) * d3[i]);
  }
  w[i] = wi;
}
// dr = alpha - u (u null: alpha) and the sums of the result row that depend on it; the NLL correction with its alpha part
__global__ __launch_bounds__(256) void cen_result_kernel(const double* __restrict__ alpha, long as, const double* __restrict__ u, long us,
                                                         const double* __restrict__ nn, const double* __restrict__ corr,
                                                         const int* __restrict__ side, const double* __restrict__ wts, int n,
                                                         const int* __restrict__ ns, double* __restrict__ dr, double* __restrict__ part) {
  const long nfull = n;
  n = site_n(ns, n);
  alpha = site(alpha, as);
  if (u) u = site(u, us);
  nn = site(nn, nfull); corr = site(corr, nfull); side = site(side, nfull);
  if (wts) wts = site(wts, 2 * nfull);  // [site][2][n]
  if (dr) dr = site(dr, nfull);
  part = site(part, (long)gridDim.x * CEN_PART);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // correction, sum dr, sum dr w0, sum dr w1
  if (i < n) {
    const double a = alpha[i], d = u ? a - u[i] : a;
    if (dr) dr[i] = d;
    if (side[i] != 0) acc[0] = corr[i] - 0.5 * nn[i] * a * a;
    acc[1] = d;
    if (wts) {
      acc[2] = d * wts[i];
      acc[3] = d * wts[nfull + i];
    }
  } else if (i < nfull && dr) {
    dr[i] = 0.0;  // the unused rows of a ragged site
  }
  cen_block_reduce<4>(acc, -1, part);
}
__global__ __launch_bounds__(256) void cen_result_finish_kernel(const double* __restrict__ part, int nblk, int with_grad,
                                                                double* __restrict__ out, double* __restrict__ status) {
  part = site(part, (long)nblk * CEN_PART);
  out = site(out, 32L);
  status = site(status, (long)CEN_ST_LEN);
  __shared__ double tot[CEN_PART];
  cen_total(part, nblk, 4, -1, tot);
  if (threadIdx.x != 0) return;
  out[0] += tot[0];  // DGP_OUT_NLL
  status[CEN_ST_NLL_CORR] = tot[0];
  if (with_grad) {
    out[28] = tot[1];  // DGP_OUT_SUM_DR, DGP_OUT_DR_W0, + 1
    out[29] = tot[2];
    out[30] = tot[3];
  }
}

CensoredLayout censored_layout(long N, long n, int B) {
  CensoredLayout L;
  const size_t vec = sizeof(double) * (size_t)B * (size_t)n;
  Carve c;
  L.rt = c.take(vec);
  L.nn = c.take(vec);
  L.dnoise = c.take(vec);
  L.g = c.take(vec);
  L.W = c.take(vec);
  L.d3 = c.take(vec);
  L.corr = c.take(vec);
  L.logp = c.take(vec);
  L.delta = c.take(vec);
  L.acur = c.take(vec);
  L.nblk = (int)((n + 255) / 256);
  L.part = c.take(sizeof(double) * (size_t)B * (size_t)L.nblk * CEN_PART);
  L.status = c.take(sizeof(double) * (size_t)B * CEN_ST_LEN);
  L.out = c.take(sizeof(double) * (size_t)B * 32);
  L.slices = c.o;
  const size_t nvec = sizeof(double) * (size_t)N;
  Carve q;  // inside a site's slice
  L.w = q.take(nvec);
  L.u = q.take(nvec);
  L.z = q.take(nvec);
  L.spart = q.take(sizeof(double) * (size_t)solve_partials(N));
  L.gpart = q.take(sizeof(double) * (size_t)gram_grad_partials(N));
  L.quad = q.take(sizeof(double) * 8);
  L.slice = q.o;
  L.total = c.o + q.o * (size_t)B;
  L.B = B;
  L.n = n;
  return L;
}

int censored_terms(const double* f, const double* y, const int* side, const double* v, const double* m, int n, int init, int it,
                   char* work, const CensoredLayout& L, hipStream_t s, Batch bt, const double* upper) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  const unsigned Bz = (unsigned)bt.B;
  cen_terms_kernel<<<dim3((unsigned)L.nblk, 1, Bz), 256, 0, s>>>(f, y, side, v, m, n, bt.ns, CEN_CAP, D(L.rt), D(L.nn), D(L.g), D(L.W),
                                                                 D(L.d3), D(L.corr), D(L.logp), D(L.part), D(L.status), init, it, upper);
  cen_terms_finish_kernel<<<dim3(1, 1, Bz), 256, 0, s>>>(D(L.part), L.nblk, D(L.status), init, it);
  return (int)hipGetLastError();
}

static int censored_newton_update(double* f, const double* y, const int* side, const double* v, const double* m, const double* anew, int n,
                           int it, double tol, char* work, const CensoredLayout& L, hipStream_t s, Batch bt, const double* upper) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  const unsigned Bz = (unsigned)bt.B;
  cen_search_kernel<<<dim3((unsigned)L.nblk, 1, Bz), 256, 0, s>>>(f, y, side, v, m, D(L.rt), D(L.nn), anew, bt.ws, D(L.acur), n, bt.ns,
                                                                  D(L.delta), D(L.part), D(L.status), upper);
  cen_search_finish_kernel<<<dim3(1, 1, Bz), 256, 0, s>>>(D(L.part), L.nblk, it, tol, D(L.out), D(L.status));
  cen_update_kernel<<<dim3((unsigned)L.nblk, 1, Bz), 256, 0, s>>>(f, D(L.delta), D(L.acur), anew, bt.ws, D(L.status), n, bt.ns, it);
  return (int)hipGetLastError();
}

static int censored_mode(double* f, const double* m, const double* alpha, int n, char* work, const CensoredLayout& L, hipStream_t s, Batch bt) {
  cen_mode_kernel<<<dim3((unsigned)L.nblk, 1, (unsigned)bt.B), 256, 0, s>>>(f, m, (const double*)(work + L.rt),
                                                                            (const double*)(work + L.nn), alpha, bt.ws, n, bt.ns,
                                                                            (const double*)(work + L.status));
  return (int)hipGetLastError();
}

static int censored_weights(const double* alpha, int n, long N, char* work, const CensoredLayout& L, hipStream_t s, Batch bt) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  cen_weight_kernel<<<dim3((unsigned)((N + 255) / 256), 1, (unsigned)bt.B), 256, 0, s>>>(
      D(L.nn), D(L.d3), D(L.dnoise), alpha, bt.ws, n, bt.ns, N, D(L.slices + L.w), (long)(L.slice / sizeof(double)));
  return (int)hipGetLastError();
}

static int censored_result(const double* alpha, const int* side, const double* wts, int n, int with_grad, double* out, double* dr, char* work,
                    const CensoredLayout& L, hipStream_t s, Batch bt) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  const unsigned Bz = (unsigned)bt.B;
  cen_result_kernel<<<dim3((unsigned)L.nblk, 1, Bz), 256, 0, s>>>(alpha, bt.ws, with_grad ? D(L.slices + L.u) : nullptr,
                                                                  (long)(L.slice / sizeof(double)), D(L.nn), D(L.corr), side,
                                                                  with_grad ? wts : nullptr, n, bt.ns, with_grad ? dr : nullptr, D(L.part));
  cen_result_finish_kernel<<<dim3(1, 1, Bz), 256, 0, s>>>(D(L.part), L.nblk, with_grad, out, D(L.status));
  return (int)hipGetLastError();
}

// ---- the bilinear derivative sweep: partials[tile][p] = sum over the tile's entries (i >= j) of
// (u_i a_j + u_j a_i) dK_ij/dtheta_p, the diagonal at half weight; summed by grad_reduce_kernel in fixed order.  Batched like
// dgp_gram.hip::gram_grad_kernel: blockIdx.z = site, its hyperparameters from the PreBatch, u / alpha / partials at their strides.
template <typename T, typename M>
__global__ __launch_bounds__(256) void gram_bilinear_kernel(const T* __restrict__ Xt, long N, int n, const PreBatch<M> pb,
                                                            const T* __restrict__ u, const T* __restrict__ alpha,
                                                            T* __restrict__ partials, long bs, const int* __restrict__ ns, long us,
                                                            long as, long ps) {
  n = site_n(ns, n);
  const typename M::Pre& pre = pb.get();
  Xt = site(Xt, bs);
  u = site(u, us);
  alpha = site(alpha, as);
  partials = site(partials, ps);
  __shared__ T sfi[M::NF][64], sfj[M::NF][64], sai[64], saj[64], sui[64], suj[64];
  __shared__ T red[4][M::NTHETA];
  int bi, bj;
  tri_decode(blockIdx.x, bi, bj);
  const int t = threadIdx.x;
  exp_table_init<T>();
  if (t < 64) {
    stage_strip<T, M>(Xt, N, (long)bi * 64, pre, sfi, t);
    sai[t] = alpha[(long)bi * 64 + t];
    sui[t] = u[(long)bi * 64 + t];
  } else if (t < 128) {
    stage_strip<T, M>(Xt, N, (long)bj * 64, pre, sfj, t - 64);
    saj[t - 64] = alpha[(long)bj * 64 + t - 64];
    suj[t - 64] = u[(long)bj * 64 + t - 64];
  }
  __syncthreads();
  const int ty = t >> 4, tx = t & 15;
  T acc[M::NTHETA];
#pragma unroll
  for (int p = 0; p < M::NTHETA; ++p) acc[p] = T(0);
  // one entry at a time, the column point's features from LDS per entry (see gram_grad_kernel)
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {
    const long gi = (long)bi * 64 + ty * 4 + a;
    T fi[M::NF];
#pragma unroll
    for (int c = 0; c < M::NF; ++c) fi[c] = sfi[c][ty * 4 + a];
    const T ai = sai[ty * 4 + a], ui = sui[ty * 4 + a];
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
      const int cj = tx * 4 + b;
      const long gj = (long)bj * 64 + cj;
      T fj[M::NF];
#pragma unroll
      for (int c = 0; c < M::NF; ++c) fj[c] = sfj[c][cj];
      T w = ui * saj[cj] + suj[cj] * ai;
      w = (gj > gi || gi >= n) ? T(0) : (gj == gi ? T(0.5) * w : w);
      (void)M::template pair<true>(fi, fj, pre, w, acc);
    }
  }
  M::finalize(acc, pre);
  const int lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int p = 0; p < M::NTHETA; ++p) {
    T v = wave_sum(acc[p]);
    if (lane == 0) red[wv][p] = v;
  }
  __syncthreads();
  if (t < M::NTHETA) partials[(long)blockIdx.x * DGP_MAX_THETA + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

template <typename T>
int gram_bilinear(int model, int d, const T* Xt, long N, int n, const double* theta, const T* u, const T* alpha, T* partials,
                  T* dtheta, int accumulate, hipStream_t s, Batch bt, long us, long as, long ps, long dstride, void* pre_scratch,
                  bool upload, void* pre_staging) {
  const int nt = model_ntheta(model, d);
  if (nt < 0) return -2;
  const long nb = N / 64;
  const long nblk = nb * (nb + 1) / 2;
  const unsigned Bz = (unsigned)bt.B;
  DGP_DISPATCH_MODEL(model, d,
                     (gram_bilinear_kernel<T, M><<<dim3((unsigned)nblk, 1, Bz), dim3(256), 0, s>>>(
                         Xt, N, n, prepare_batch<M>(theta, nt, bt.B, pre_scratch, upload, s, pre_staging), u, alpha, partials, bt.ws,
                         bt.ns, us, as, ps)));
  grad_reduce_kernel<T><<<dim3((unsigned)nt, 1, Bz), dim3(256), 0, s>>>(partials, nblk, nt, dtheta, accumulate, ps, dstride);
  return (int)hipGetLastError();
}
template int gram_bilinear<double>(int, int, const double*, long, int, const double*, const double*, const double*, double*, double*,
                                   int, hipStream_t, Batch, long, long, long, long, void*, bool, void*);

}  // namespace dgp

using namespace dgp;

// ---- the entries: Newton's mode search on the factorise path, then one step at the mode.
// One code path for a single-site plan and for a batch: every Newton iteration factorises ALL sites in lockstep; a site is done when
// it has no censored row, its proposal is within tol or its factorisation failed, and a done site is frozen on the device
// (CEN_ST_DONE), so that it rides through the remaining factorisations on unchanged pseudo-data.  The host reads the B status
// blocks in one copy per iteration.  stat: [B][4].  `batched`: the entry's texts name the site.
// Returns 0, a HIP error (> 0), or DGP_E_ARG / DGP_E_NOCONV with the error text already set.
static int laplace(dgp_plan* p, const double* theta, const double* y, const double* mean, const double* noise, const int* side,
                   double* f, int maxit, double tol, char* work, double* out, double* dr, double* stat, int with_grad, int batched,
                   const char* where, hipStream_t s, const double* upper = nullptr, int interval = 0) {
  const int B = p->B;
  const CensoredLayout L = censored_layout(p->N, p->n, B);
  const Batch bt = batch_of<double>(p);
  auto D = [&](size_t off) { return (double*)(work + off); };
  const int n = (int)p->n;
  const long wss = (long)(L.slice / sizeof(double));
  const double* alpha = (const double*)p->alpha;
  std::vector<double> st((size_t)B * CEN_ST_LEN);
  auto S = [&](int b, int k) -> double { return st[(size_t)b * CEN_ST_LEN + k]; };
  auto read_status = [&]() -> int {
    hipError_t e = hipMemcpyAsync(st.data(), D(L.status), sizeof(double) * st.size(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
  };
  int rc;
  for (int k = 0; k < 4 * B; ++k) stat[k] = 0.0;
  if ((rc = censored_terms(f, y, side, noise, mean, n, 1, 0, work, L, s, bt, upper)) || (rc = read_status())) return rc;
  bool any = false, any_plain = false;
  for (int b = 0; b < B; ++b) {
    if (interval && S(b, CEN_ST_BAD) != 0.0)
      return failf(DGP_E_ARG,
                   upper ? "%s: side values must be -1, 0, +1 or 2 (site %d)"
                         : "%s: a row of side 2 needs upper_dev; other side values must be -1, 0 or +1 (site %d)",
                   where, b);
    if (S(b, CEN_ST_BADBRK) != 0.0)
      return failf(DGP_E_ARG, "%s: %d bad bracket(s) in site %d: a row of side 2 needs a finite upper above its y", where,
                   (int)S(b, CEN_ST_BADBRK), b);
    if (S(b, CEN_ST_BAD) != 0.0)
      return batched ? failf(DGP_E_ARG, "%s: side values must be -1, 0 or +1 (site %d)", where, b)
                     : failf(DGP_E_ARG, "%s: side values must be -1, 0 or +1", where);
    (S(b, CEN_ST_NCENS) != 0.0 ? any : any_plain) = true;
  }
  if (!any) {  // nothing censored: the plain step on (y - m, v), bit for bit
    if ((rc = fit_step<double>(p, theta, D(L.rt), D(L.nn), out, with_grad ? dr : nullptr, with_grad ? D(L.dnoise) : nullptr, with_grad, s)))
      return rc;
    return censored_mode(f, mean, alpha, n, work, L, s, bt);
  }
  if ((rc = (int)hipMemsetAsync(D(L.acur), 0, sizeof(double) * (size_t)B * (size_t)n, s))) return rc;
  std::vector<char> active((size_t)B);
  for (int b = 0; b < B; ++b) active[b] = S(b, CEN_ST_DONE) == 0.0;
  int it = 0;
  for (;;) {
    if ((rc = fit_step<double>(p, theta, D(L.rt), D(L.nn), D(L.out), nullptr, nullptr, 0, s))) return rc;
    ++it;
    // proposal, line search, update; then the next system (or the one at the mode) of every site that moved
    if ((rc = censored_newton_update(f, y, side, noise, mean, alpha, n, it, tol, work, L, s, bt, upper)) ||
        (rc = censored_terms(f, y, side, noise, mean, n, 0, it, work, L, s, bt, upper)) || (rc = read_status()))
      return rc;
    bool all_done = true;
    for (int b = 0; b < B; ++b) {
      if (!active[b]) continue;
      stat[4 * b] = (double)it;
      stat[4 * b + 1] = S(b, CEN_ST_DMAX);
      stat[4 * b + 2] += S(b, CEN_ST_HALVINGS);
      if (S(b, CEN_ST_DONE) != 0.0)
        active[b] = 0;  // converged, or not positive definite: f did not move; the step below reports it through DGP_OUT_INFO
      else
        all_done = false;
    }
    if (all_done || it >= maxit) break;
  }
  if ((rc = fit_step<double>(p, theta, D(L.rt), D(L.nn), out, nullptr, with_grad ? D(L.dnoise) : nullptr, with_grad, s))) return rc;
  if (with_grad) {
    if ((rc = censored_weights(alpha, n, p->N, work, L, s, bt))) return rc;
    // u = T^T (T w) in the work area: the plan's z, alpha and result rows stay as the step left them
    if ((rc = solve_work<double>((const double*)p->Tm, p->N, D(L.slices + L.w), n, D(L.slices + L.z), D(L.slices + L.u),
                                 D(L.slices + L.spart), D(L.slices + L.quad), wss, s, bt)))
      return rc;
    // (the step's Gram build left this theta in the plan's hyperparameter scratch)
    if ((rc = gram_bilinear<double>(p->model, p->d, (const double*)p->Xt, p->N, n, theta, D(L.slices + L.u), alpha,
                                    D(L.slices + L.gpart), out + DGP_OUT_DTHETA, 1, s, bt, wss, bt.ws, wss, DGP_OUT_LEN, p->pre, false,
                                    nullptr)))
      return rc;
  }
  if (any_plain && (rc = censored_mode(f, mean, alpha, n, work, L, s, bt))) return rc;  // the batch-mates without a censored row
  if ((rc = censored_result(alpha, side, (const double*)p->dr_w, n, with_grad, out, dr, work, L, s, bt)) || (rc = read_status())) return rc;
  int open_site = -1;
  for (int b = 0; b < B; ++b) {
    stat[4 * b + 3] = S(b, CEN_ST_CAPPED);
    if (active[b] && open_site < 0) open_site = b;
  }
  if (open_site >= 0)
    return batched ? failf(DGP_E_NOCONV, "%s: the mode search of site %d did not converge in %d Newton iterations (max |df| = %.3g)", where,
                           open_site, it, stat[4 * open_site + 1])
                   : failf(DGP_E_NOCONV, "%s: the mode search did not converge in %d Newton iterations (max |df| = %.3g)", where, it, stat[1]);
  return 0;
}
static int laplace_entry(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                         void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, void* dr, double* stat,
                         int with_grad, int batched, const char* where, void* stream, const void* upper = nullptr, int interval = 0) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (batched ? p->dtype != DGP_F64 : (p->dtype != DGP_F64 || p->B != 1))
    return batched ? failf(DGP_E_ARG, "%s: censored fits need a float64 plan (fp32 plans are not supported)", where)
                   : failf(DGP_E_ARG, "%s: censored fits need a float64 single-site plan (fp32 and batched plans are not supported)", where);
  if (!theta || !y || !mean || !noise || !side || !f || !out || !stat || maxit < 1 || !(tol >= 0.0))
    return failf(DGP_E_ARG, "%s: null argument (f_dev included), maxit < 1 or a negative tol", where);
  DGP_CHECK_PLAN(p);
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_laplace_*: call dgp_set_inputs first");
  if (!work || work_bytes < (batched ? dgp_laplace_batched_workspace_bytes(p) : dgp_laplace_workspace_bytes(p)))
    return failf(DGP_E_WORKSPACE, "%s: workspace missing or too small", where);
  if (((uintptr_t)work & 255) != 0) return fail(DGP_E_ARG, "dgp_laplace_*: the work area must be 256-byte aligned");
  const int rc = laplace(p, theta, (const double*)y, (const double*)mean, (const double*)noise, (const int*)side, (double*)f, maxit, tol,
                         (char*)work, (double*)out, (double*)dr, stat, with_grad, batched, where, (hipStream_t)stream,
                         (const double*)upper, interval);
  if (rc == DGP_E_ARG || rc == DGP_E_NOCONV) return rc;  // text set where it arose
  return wrap(rc, where);
}

// u_dev / alpha_dev [B][n] -> dtheta_dev [B][ntheta]; B = 1: the single-site sweep
static int debug_bilinear(dgp_plan* p, const double* theta, const void* u, const void* alpha, void* work, size_t work_bytes, double* dtheta,
                          int batched, const char* where, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64 || (!batched && p->B != 1))
    return failf(DGP_E_ARG, batched ? "%s: needs a float64 plan" : "%s: needs a float64 single-site plan", where);
  if (!theta || !u || !alpha || !dtheta) return failf(DGP_E_ARG, "%s: null argument", where);
  DGP_CHECK_PLAN(p);
  if (!p->have_inputs) return failf(DGP_E_STATE, "%s: call dgp_set_inputs first", where);
  if (int rc = need_work(work, work_bytes, batched ? dgp_laplace_batched_workspace_bytes(p) : dgp_laplace_workspace_bytes(p), where))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = p->B;
  const CensoredLayout L = censored_layout(p->N, p->n, B);
  char* slices = (char*)work + L.slices;
  double *up = (double*)(slices + L.u), *ap = (double*)(slices + L.w);
  const size_t nb = sizeof(double) * (size_t)p->n;
  hipError_t e = hipMemsetAsync(slices, 0, L.slice * (size_t)B, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(up, L.slice, u, nb, nb, (size_t)B, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(ap, L.slice, alpha, nb, nb, (size_t)B, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return hipfail(e, where);
  const long wss = (long)(L.slice / sizeof(double));
  void* staging = p->pre ? p->ring.acquire(pre_scratch_bytes(B)) : nullptr;
  const int rc = gram_bilinear<double>(p->model, p->d, (const double*)p->Xt, p->N, (int)p->n, theta, up, ap, (double*)(slices + L.gpart),
                                       dtheta, 0, s, batch_of<double>(p), wss, wss, wss, p->ntheta, p->pre, true, staging);
  if (staging) p->ring.commit(s);
  p->pre_ready = 0;
  return wrap(rc, where);
}

extern "C" {

size_t dgp_laplace_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64 || p->B != 1) return 0;
  return censored_layout(p->N, p->n, 1).total;
}
size_t dgp_laplace_batched_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64) return 0;
  return censored_layout(p->N, p->n, p->B).total;
}

int dgp_laplace_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                         void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, void* dr, double* stat,
                         void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, dr, stat, 1, 0, "dgp_laplace_fit_step",
                       stream);
}

int dgp_laplace_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                          void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, nullptr, stat, 0, 0, "dgp_laplace_factorize",
                       stream);
}

int dgp_laplace_batched_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                 const int32_t* side, void* f, int maxit, double tol, void* work, size_t work_bytes, void* out, void* dr,
                                 double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, dr, stat, 1, 1,
                       "dgp_laplace_batched_fit_step", stream);
}

int dgp_laplace_batched_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                  const int32_t* side, void* f, int maxit, double tol, void* work, size_t work_bytes, void* out,
                                  double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, nullptr, stat, 0, 1,
                       "dgp_laplace_batched_factorize", stream);
}

int dgp_laplace_interval_fit_step(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                  const int32_t* side, const void* upper, void* f, int maxit, double tol, void* work, size_t work_bytes,
                                  void* out, void* dr, double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, dr, stat, 1, 1,
                       "dgp_laplace_interval_fit_step", stream, upper, 1);
}

int dgp_laplace_interval_factorize(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise,
                                   const int32_t* side, const void* upper, void* f, int maxit, double tol, void* work,
                                   size_t work_bytes, void* out, double* stat, void* stream) {
  return laplace_entry(p, theta, y, mean, noise, side, f, maxit, tol, work, work_bytes, out, nullptr, stat, 0, 1,
                       "dgp_laplace_interval_factorize", stream, upper, 1);
}

int dgp_debug_interval_terms(const double* za, const double* delta, int64_t count, double* out, void* stream) {
  if (!za || !delta || !out || count <= 0 || count > (1ll << 29))
    return fail(DGP_E_ARG, "dgp_debug_interval_terms: null argument / bad count");
  return wrap(debug_interval_terms(za, delta, count, out, (hipStream_t)stream), "dgp_debug_interval_terms");
}

int dgp_debug_censored_terms(const double* z, int64_t count, double* out, void* stream) {
  if (!z || !out || count <= 0 || count > (1ll << 29)) return fail(DGP_E_ARG, "dgp_debug_censored_terms: null argument / bad count");
  return wrap(debug_censored_terms(z, count, out, (hipStream_t)stream), "dgp_debug_censored_terms");
}

int dgp_debug_bilinear(dgp_plan* p, const double* theta, const void* u, const void* alpha, void* work, size_t work_bytes, double* dtheta,
                       void* stream) {
  return debug_bilinear(p, theta, u, alpha, work, work_bytes, dtheta, 0, "dgp_debug_bilinear", stream);
}

int dgp_debug_bilinear_batched(dgp_plan* p, const double* theta, const void* u, const void* alpha, void* work, size_t work_bytes,
                               double* dtheta, void* stream) {
  return debug_bilinear(p, theta, u, alpha, work, work_bytes, dtheta, 1, "dgp_debug_bilinear_batched", stream);
}

}  // extern "C"
