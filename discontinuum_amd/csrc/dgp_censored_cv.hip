// dgp_censored_cv.hip -- cross-validation of a censored (Laplace) fit from the factorisation a plan holds: cavity folds.
//
// At the Laplace mode f the posterior of the latent is the GP posterior of the pseudo-data (y~, n~ = 1 / W).  Taking the Gaussian
// sites of a fold F out of it gives the fold's CAVITY distribution (the LA-LOO of Vehtari et al. 2016, in block form); the
// pseudo-data of the rows that stay are held at the full-data mode -- an approximation on top of Laplace's, no fold is refitted.
// With T = L^-1 of the pseudo-data system,
//     G_F = (K^^-1)_FF = T[:, F]^T T[:, F],      Sigma_FF = K_FF - V_F^T V_F,  V = T K(X, X)   (the latent posterior covariance),
//     W_F = 1 / n~_F,                            g_F = d log p / d f at the mode,
// the latent cavity is, exactly (N~_F G_F = I - Sigma_FF W_F),
//     V_c = G_F^-1 diag(W_F) Sigma_FF  (only its diagonal is used),       mu_c = f_F - V_c g_F.
// Nothing of the size of n~ is subtracted anywhere: the obvious form C_ii - n~_i loses everything on a row whose limit is
// uninformative (n~ up to 1e12 v).  G_F is badly scaled by rows and columns only, which its Cholesky factor does not mind.
//   terms       W, g (and the cap) at f by the fit's own terms pass (dgp_censored.hip::censored_terms): same guards, same bits
//   LOO         1 / G_ii from cross_validate's leave-one-out pass over T; Sigma_ii from the prediction's variance pass at
//               Xs = X (the n x n covariance is never stored);  v_c = Sigma_ii W_i / G_ii
//   folds > 1   Sigma = K - V^T V as lower 128-tiles in the work area (posterior_cov's kernel); per chunk of folds, behind
//               cross_validate's block route (G_F from T's columns, the library's batched potrf / trtri: M^-1 with G_F = M M^T):
//               C_F = G_F^-1 = M^-T M^-1 on the double tile core (k-tiles last to first), h = W_F o (Sigma_FF g_F), then one wave
//               per row:  v_c,i = sum_j C_ij W_j Sigma_ji,  mu_c,i = f_i - sum_j C_ij h_j
//   epilogue    per held-out row the predictive of the OBSERVATION, s_p^2 = v_c + v_i, and the seven planes of the result (below)
// Everything is double; no floating-point atomics, every sum has a fixed order: bitwise repeatable.  Indices read from order /
// start are clamped (cv_bounds / cv_index).  The plan's L, T, alpha are only read.  Roofline: V = T K and Sigma are two N^3-flop
// products on the MFMA tile core and dominate; the fold algebra is sum_F M^3.
#include "dgp_censored_fn.h"
#include "dgp_gemm.h"
#include "dgp_gemm_dma.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

// out [LCV_PLANES][n] (== DGP_LCV_* of dgp_hip.h)
enum { LCV_MU = 0, LCV_VAR, LCV_LPD, LCV_PLO, LCV_PHI, LCV_DLP, LCV_TILT, LCV_PLANES };
// what the terms pass found, before any other launch: a bad side value (without / with `upper`), a bad bracket
enum { LCV_E_SIDE_NO_UPPER = -100, LCV_E_SIDE = -101, LCV_E_BRACKET = -102 };

// folds of 2 .. CV_SMALL_GROUP run on cross_validate's block route too (blocks of order 128): only that route calls the tap
constexpr int LCV_MIN_BLOCK_GROUP = CV_SMALL_GROUP + 1;

__device__ __forceinline__ double lcv_Phi(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

// the seven planes of row i from its latent cavity (mu, vc); out [LCV_PLANES][n]
__device__ __forceinline__ void lcv_epilogue(int i, long n, double mu, double vc, bool bad, const double* __restrict__ y,
                                             const double* __restrict__ v, const int* __restrict__ side,
                                             const double* __restrict__ upper, double shift, double* __restrict__ out) {
  double r[LCV_PLANES];
  if (bad) {
#pragma unroll
    for (int q = 0; q < LCV_PLANES; ++q) r[q] = __longlong_as_double(0x7ff8000000000000LL);
  } else {
    const int s = side[i];
    const double yi = y[i], sp2 = vc + v[i], sp = sqrt(sp2), za = (yi - mu) / sp, tz = shift * sp;
    r[LCV_MU] = mu;
    r[LCV_VAR] = sp2;
    if (s == 2 && upper != nullptr) {
      const double ui = upper[i], dz = (ui - yi) / sp, zb = (ui - mu) / sp;
      const IntFn o = iv_fn(za, zb, dz);
      r[LCV_LPD] = o.logp;
      r[LCV_PLO] = lcv_Phi(za);
      r[LCV_PHI] = lcv_Phi(zb);
      r[LCV_DLP] = o.mu / sp;
      r[LCV_TILT] = shift == 0.0 ? 0.0 : iv_logp(za - tz, zb - tz, dz) - o.logp;
    } else if (s == -1) {
      const CenFn o = cen_fn(za);
      r[LCV_LPD] = o.logphi;
      r[LCV_PLO] = 0.0;
      r[LCV_PHI] = lcv_Phi(za);
      r[LCV_DLP] = -o.h / sp;
      r[LCV_TILT] = shift == 0.0 ? 0.0 : cen_logphi(za - tz) - o.logphi;
    } else if (s == 1) {
      const CenFn o = cen_fn(-za);
      r[LCV_LPD] = o.logphi;
      r[LCV_PLO] = lcv_Phi(za);
      r[LCV_PHI] = 1.0;
      r[LCV_DLP] = o.h / sp;
      r[LCV_TILT] = shift == 0.0 ? 0.0 : cen_logphi(tz - za) - o.logphi;
    } else {
      r[LCV_LPD] = -0.5 * za * za - 0.5 * log(6.28318530717958647692 * sp2);
      r[LCV_PLO] = r[LCV_PHI] = lcv_Phi(za);
      r[LCV_DLP] = (yi - mu) / sp2;
      r[LCV_TILT] = 0.0;
    }
  }
#pragma unroll
  for (int q = 0; q < LCV_PLANES; ++q) out[(long)q * n + i] = r[q];
}

struct LcvRows {  // the per-row inputs of the epilogue and of the cavity
  const double *f, *y, *v, *upper, *W, *g;
  const int* side;
  double shift;
};

// ---- leave-one-out: pvar = 1 / G_ii (cross_validate's pass), svar = Sigma_ii (the prediction's variance at Xs = X)
__global__ __launch_bounds__(256) void lcv_loo_kernel(LcvRows R, const double* __restrict__ pvar, const double* __restrict__ svar, int n,
                                                      const int* __restrict__ order, const int* __restrict__ start, int ngroups,
                                                      const int* __restrict__ info, double* __restrict__ out) {
  const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= ngroups) return;
  int s0, b;
  cv_bounds(start, g, n, 1, s0, b);
  if (b == 0) return;
  const int i = cv_index(order, s0, n);
  const double vc = svar[i] * R.W[i] * pvar[i];
  lcv_epilogue(i, n, R.f[i] - vc * R.g[i], vc, info[g] != 0, R.y, R.v, R.side, R.upper, R.shift, out);
}

// ---- larger folds.  Slot c of a chunk = fold g0 + c; its M^-1 (M x M row-major, lower, identity pad) at minv + c stride.
struct LcvChunk {
  int g0, C, ngroups, n;
  long N, M;
};
__device__ __forceinline__ bool lcv_fold(const LcvChunk& ck, const int* __restrict__ start, int& g, int& s0, int& b) {
  g = ck.g0 + (int)blockIdx.z;
  s0 = b = 0;
  if (g >= ck.ngroups) return false;
  cv_bounds(start, g, ck.n, (int)ck.M, s0, b);
  return b > 0;
}

// C_F = M^-T M^-1, lower 128-tiles (diagonal tiles complete); rows of M^-1 above the tile row's first column are zero
__global__ __launch_bounds__(256, (TileCore<double, false, false, 128, 128, 1, true>::OCC)) void lcv_ginv_kernel(
    const double* __restrict__ minv, long stride, long M, double* __restrict__ ginv) {
  using K = TileCore<double, false, false, 128, 128, 1, true>;
  using G = typename K::G;
  __shared__ double smem[K::SMEM_ELEMS];
  int bm, bn;
  tri_decode((int)blockIdx.x, bm, bn);
  const double* P = minv + (long)blockIdx.z * stride + (long)bm * 128 * M;  // k starts at the diagonal block of column block bm
  typename G::acc_t acc[G::MI][G::NI];
  G::zero(acc);
  double* out = ginv + (long)blockIdx.z * M * M + (long)bm * 128 * M + (long)bn * 128;
  auto store = [&]() { K::foreach (acc, [&](int r, int c, double& v) { out[(long)r * M + c] = v; }); };
  K::template run_tri<true, TRI_NONE>(P + (long)bm * 128, M, P + (long)bn * 128, M, (int)((M - (long)bm * 128) / 16), smem, acc, store);
}

// h_j = W_j sum_k Sigma[F_j][F_k] g_k: one wave per row of the fold (lanes over k, then the wave's fixed tree); Sigma: lower tiles
__global__ __launch_bounds__(256) void lcv_h_kernel(LcvChunk ck, LcvRows R, const double* __restrict__ Sig, const int* __restrict__ order,
                                                    const int* __restrict__ start, double* __restrict__ h) {
  int g, s0, b;
  const bool live = lcv_fold(ck, start, g, s0, b);
  const int lane = (int)threadIdx.x & 63, j = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (j >= ck.M) return;
  double acc = 0.0;
  if (live && j < b) {
    const int oj = cv_index(order, s0 + j, ck.n);
    for (int k = lane; k < b; k += 64) {
      const int ok = cv_index(order, s0 + k, ck.n);
      acc += Sig[(long)max(oj, ok) * ck.N + min(oj, ok)] * R.g[ok];
    }
    acc = wave_sum(acc) * R.W[oj];
  }
  if (lane == 0) h[(long)blockIdx.z * ck.M + j] = acc;
}

// v_c,i = sum_j C_ij W_j Sigma[F_j][F_i], mu_c,i = f_i - sum_j C_ij h_j, then the row's planes: one wave per row of the fold
__global__ __launch_bounds__(256) void lcv_rows_kernel(LcvChunk ck, LcvRows R, const double* __restrict__ Sig,
                                                       const double* __restrict__ ginv, const double* __restrict__ h,
                                                       const int* __restrict__ order, const int* __restrict__ start,
                                                       const int* __restrict__ info, double* __restrict__ out) {
  int g, s0, b;
  if (!lcv_fold(ck, start, g, s0, b)) return;
  const int lane = (int)threadIdx.x & 63, i = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (i >= b) return;
  const double* Cm = ginv + (long)blockIdx.z * ck.M * ck.M;
  const double* hz = h + (long)blockIdx.z * ck.M;
  const int oi = cv_index(order, s0 + i, ck.n);
  double av = 0.0, aw = 0.0;
  for (int j = lane; j < b; j += 64) {
    const int oj = cv_index(order, s0 + j, ck.n);
    const double c = Cm[(long)max(i, j) * ck.M + min(i, j)];
    av += c * (R.W[oj] * Sig[(long)max(oi, oj) * ck.N + min(oi, oj)]);
    aw += c * hz[j];
  }
  av = wave_sum(av);
  aw = wave_sum(aw);
  if (lane == 0) lcv_epilogue(oi, ck.n, R.f[oi] - aw, av, info[g] != 0, R.y, R.v, R.side, R.upper, R.shift, out);
}

struct LcvCtx {
  LcvRows R;
  const double* Sig;
  double *ginv, *h, *out;
  const int *order, *start, *info;
  int ngroups, n;
  long N;
  hipStream_t s;
};
int lcv_chunk(void* ctx_, const CvBlocks& cb) {
  const LcvCtx& c = *(const LcvCtx*)ctx_;
  const LcvChunk ck{cb.g0, cb.C, c.ngroups, c.n, c.N, cb.M};
  const unsigned Z = (unsigned)cb.C, nt = (unsigned)(cb.M / DGP_TILE_HOST);
  lcv_ginv_kernel<<<dim3(nt * (nt + 1) / 2, 1, Z), 256, 0, c.s>>>(cb.minv, cb.stride, cb.M, c.ginv);
  lcv_h_kernel<<<dim3((unsigned)(cb.M / 4), 1, Z), 256, 0, c.s>>>(ck, c.R, c.Sig, c.order, c.start, c.h);
  lcv_rows_kernel<<<dim3((unsigned)(cb.M / 4), 1, Z), 256, 0, c.s>>>(ck, c.R, c.Sig, c.ginv, c.h, c.order, c.start, c.info, c.out);
  return (int)hipGetLastError();
}

struct LaplaceCvLayout {
  size_t cen, resid, var, lpd, Ks, V, kss, mean, svar, part, cvw, ginv, h, total;  // byte offsets into the work area
  long route_group, M;  // the bound handed to cross_validate (1: leave-one-out; else >= 65: its block route) and the block order
  int C;                // folds per chunk of the block route
};
LaplaceCvLayout laplace_cv_layout(long N, long n, int ngroups, long max_group) {
  LaplaceCvLayout L;
  const size_t d = sizeof(double), vecN = d * (size_t)N;
  L.route_group = max_group <= 1 ? 1 : (max_group < LCV_MIN_BLOCK_GROUP ? LCV_MIN_BLOCK_GROUP : max_group);
  L.M = max_group <= 1 ? 0 : round_up(L.route_group, DGP_TILE_HOST);
  L.C = max_group <= 1 ? 0 : cross_validate_chunk_groups(N, 1, ngroups, L.route_group);
  Carve c;
  L.cen = c.take(censored_layout(N, n, 1).total);
  L.resid = c.take(d * (size_t)n);
  L.var = c.take(d * (size_t)n);
  L.lpd = c.take(d * (size_t)ngroups);
  L.Ks = c.take(d * (size_t)N * (size_t)N);
  L.V = c.take(d * (size_t)N * (size_t)N);
  L.kss = c.take(vecN);
  L.mean = c.take(vecN);
  L.svar = c.take(vecN);
  L.part = c.take(d * 2 * PREDICT_SPLIT * (size_t)N);
  L.cvw = c.take(cross_validate_workspace_bytes(N, 1, ngroups, L.route_group));
  L.ginv = c.take(d * (size_t)L.C * (size_t)L.M * (size_t)L.M);
  L.h = c.take(d * (size_t)L.C * (size_t)L.M);
  L.total = c.o;
  return L;
}

// W, g and the cap at the mode, by the fit's own pass, into the work area; its sums (read back: synchronises the stream) tell a bad
// side value or bracket before anything else runs: 0, a HIP error or LCV_E_*
int laplace_cv_terms(long N, int n, const double* y, const double* mean, const double* noise, const int* side, const double* upper,
                     const double* f, char* work, const LaplaceCvLayout& L, hipStream_t s) {
  int rc;
  hipError_t e;
  const CensoredLayout CL = censored_layout(N, n, 1);
  char* cw = work + L.cen;
  if ((rc = censored_terms(f, y, side, noise, mean, n, 1, 0, cw, CL, s, Batch(), upper))) return rc;
  double st[CEN_ST_LEN];
  if ((e = hipMemcpyAsync(st, cw + CL.status, sizeof(st), hipMemcpyDeviceToHost, s)) != hipSuccess) return (int)e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return (int)e;
  if (st[CEN_ST_BAD] != 0.0) return upper ? LCV_E_SIDE : LCV_E_SIDE_NO_UPPER;
  if (st[CEN_ST_BADBRK] != 0.0) return LCV_E_BRACKET;
  return 0;
}

// everything behind laplace_cv_terms (which left W and g in the work area): asynchronous on `s`
int laplace_cross_validate(int model, int d, const double* Xt, const double* Tm, const double* alpha, long N, int n, const double* theta,
                           const double* y, const double* noise, const int* side, const double* upper,
                           const double* f, const int* order, const int* start, int ngroups, double shift, char* work,
                           const LaplaceCvLayout& L, double* out, int* info, hipStream_t s, Batch bt, void* pre_scratch,
                           void* pre_staging) {
  auto D = [&](size_t off) { return (double*)(work + off); };
  int rc;
  hipError_t e;
  // only cross_validate's block route (groups above CV_SMALL_GROUP) calls the tap: any other route would leave `out` at its zeros
  if (L.route_group > 1 && (L.C < 1 || L.route_group <= CV_SMALL_GROUP)) return -1;
  const CensoredLayout CL = censored_layout(N, n, 1);
  const char* cw = work + L.cen;
  const LcvRows R{f, y, noise, upper, (const double*)(cw + CL.W), (const double*)(cw + CL.g), side, shift};
  // rows that no fold holds keep zeros
  if ((e = hipMemsetAsync(out, 0, sizeof(double) * LCV_PLANES * (size_t)n, s)) != hipSuccess) return (int)e;
  // ---- K(X, X) (zero pad) and V = T K: what the prediction at Xs = X starts with
  if ((rc = gram_cross<double>(model, d, Xt, N, n, Xt, N, n, theta, D(L.Ks), s, bt, 0, pre_scratch, pre_staging))) return rc;
  if (L.route_group == 1) {
    Batch one;
    if ((rc = gram_diag<double>(model, d, Xt, N, n, theta, D(L.kss), s, one, 0, pre_scratch))) return rc;
    if ((rc = predict_var<double>(Tm, N, D(L.Ks), N, D(L.V), alpha, D(L.kss), D(L.part), D(L.mean), D(L.svar), s, bt, 0))) return rc;
    // cross_validate is called for var = 1 / G_ii and info alone; its resid and lpd (of the pseudo-data, meaningless here) land in
    // scratch planes of the work area that nobody reads -- O(n) beside the pass over T
    if ((rc = cross_validate<double>(Tm, nullptr, alpha, N, n, order, start, ngroups, 1, work + L.cvw, D(L.resid), D(L.var), D(L.lpd), info,
                                     s, bt)))
      return rc;
    lcv_loo_kernel<<<dim3((unsigned)((ngroups + 255) / 256)), 256, 0, s>>>(R, D(L.var), D(L.svar), n, order, start, ngroups, info, out);
    return (int)hipGetLastError();
  }
  // ---- Sigma = K - V^T V in place of K: lower 128-tiles, diagonal tiles complete
  if ((rc = predict_v<double>(Tm, N, D(L.Ks), N, D(L.V), s, bt, 0))) return rc;
  if ((rc = posterior_cov<double>(D(L.V), N, N, D(L.Ks), s, 1, 0))) return rc;
  LcvCtx ctx{R, D(L.Ks), D(L.ginv), D(L.h), out, order, start, info, ngroups, n, N, s};
  CvTap tap;
  tap.chunk = lcv_chunk;
  tap.ctx = &ctx;
  // G_F from T's columns in every plan state (S = null), its factor and M^-1 by the block route; the tap runs behind each chunk.
  // Only M^-1 and info are used: the route's own resid / var / lpd of the pseudo-data (its e_B, trmv, column and lpd kernels per
  // chunk, O(M^2) beside the O(M^3) factorisation) go to scratch planes of the work area that nobody reads.
  return cross_validate<double>(Tm, nullptr, alpha, N, n, order, start, ngroups, L.route_group, work + L.cvw, D(L.resid), D(L.var),
                                D(L.lpd), info, s, bt, &tap);
}

bool lcv_plan_ok(const dgp_plan* p) { return p && p->dtype == DGP_F64 && p->B == 1; }

}  // namespace

}  // namespace dgp

using namespace dgp;

extern "C" {

size_t dgp_laplace_cross_validate_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group) {
  if (!lcv_plan_ok(p) || !cv_sizes_ok(p, ngroups, max_group)) return 0;
  return laplace_cv_layout(p->N, p->n, ngroups, max_group).total;
}

int dgp_laplace_cross_validate(dgp_plan* p, const double* theta, const void* y, const void* mean, const void* noise, const int32_t* side,
                               const void* upper, const void* f, const int32_t* order, const int32_t* start, int ngroups,
                               int64_t max_group, double shift, void* work, size_t work_bytes, double* out, int32_t* info, void* stream) {
  const char* where = "dgp_laplace_cross_validate";
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!lcv_plan_ok(p))
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: needs a float64 single-site plan (fp32 and batched plans are not supported)");
  if (!theta || !y || !mean || !noise || !side || !f || !order || !start || !out || !info || !(shift == shift))
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: null argument (f_dev included) or a NaN shift");
  if (!cv_sizes_ok(p, ngroups, max_group))
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: bad size (1 <= ngroups <= n, 1 <= max_group <= n)");
  DGP_CHECK_PLAN(p);
  int rc = need_factor(p, where, "call dgp_laplace_factorize or dgp_laplace_fit_step");
  if (rc || (rc = need_work(work, work_bytes, dgp_laplace_cross_validate_workspace_bytes(p, ngroups, max_group), where))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const LaplaceCvLayout L = laplace_cv_layout(p->N, p->n, ngroups, max_group);
  // the terms pass and its read-back first: the staging slot below is not held across the synchronisation
  rc = laplace_cv_terms(p->N, (int)p->n, (const double*)y, (const double*)mean, (const double*)noise, side, (const double*)upper,
                        (const double*)f, (char*)work, L, s);
  if (rc == 0) {
    PreSlot slot(p, s);
    rc = laplace_cross_validate(p->model, p->d, (const double*)p->Xt, (const double*)p->Tm, (const double*)p->alpha, p->N, (int)p->n, theta,
                                (const double*)y, (const double*)noise, side, (const double*)upper, (const double*)f, order, start,
                                ngroups, shift, (char*)work, L, out, info, s, batch_of<double>(p), p->pre, slot.staging);
  }
  if (rc == LCV_E_SIDE_NO_UPPER)
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: a row of side 2 needs upper_dev; other side values must be -1, 0 or +1");
  if (rc == LCV_E_SIDE) return fail(DGP_E_ARG, "dgp_laplace_cross_validate: side values must be -1, 0, +1 or 2");
  if (rc == LCV_E_BRACKET)
    return fail(DGP_E_ARG, "dgp_laplace_cross_validate: bad bracket(s): a row of side 2 needs a finite upper above its y");
  return wrap(rc, where);
}

}  // extern "C"
