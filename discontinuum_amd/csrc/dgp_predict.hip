// dgp_predict.hip -- inference on the factorisation a plan holds: mean and variance, the posterior covariance, the mean alone and
// its vector-Jacobian product, the covariance's additive parts (dgp_terms.hip) and the input derivatives (dgp_slopes.hip), draws.
// Batched plans run every launch once for all sites (gridDim.z = sites, like the fit step): the caller's work area holds one
// slice per site (site stride = the single-site size).
#include "dgp_common.h"
#include "dgp_stream.h"

using namespace dgp;

template <typename T>
__global__ void copy_rows_kernel(const T* src, long n, T* dst, long src_stride) {  // dst [site][n] <- src at src_stride
  src = site(src, src_stride);
  dst = site(dst, n);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

template <typename T>
int dgp::predict_common(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, T** V_out, T** Xst_out,
                        T** vpad_out, long* wbs_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const PredictLayout L = predict_layout(p, m);
  const long wbs = p->B > 1 ? (long)(L.total / sizeof(T)) : 0;
  char* w = (char*)work;
  T* Xst = (T*)(w + L.Xst);
  T* Ks = (T*)(w + L.Ks);
  T* V = (T*)(w + L.V);
  T* kss = (T*)(w + L.kss);
  T* mpad = (T*)(w + L.mean);
  T* vpad = (T*)(w + L.var);
  T* part = (T*)(w + L.part);
  const unsigned Bz = (unsigned)p->B;
  int rc = cross<T>(p, theta, Xs, m, Xst, Ks, s, wbs);
  if (rc) return rc;
  Batch wb;
  wb.B = p->B;
  if ((rc = gram_diag<T>(p->model, p->d, Xst, M, (int)m, theta, kss, s, wb, wbs, p->pre))) return rc;
  if ((rc = predict_var<T>((const T*)p->Tm, p->N, Ks, M, V, (const T*)p->alpha, kss, part, mpad, vpad, s, batch_of<T>(p), wbs))) return rc;
  copy_rows_kernel<T><<<dim3((unsigned)((m + 255) / 256), 1, Bz), 256, 0, s>>>(mpad, m, (T*)mean, wbs);
  *V_out = V;
  *Xst_out = Xst;
  *vpad_out = vpad;
  *wbs_out = wbs;
  return (int)hipGetLastError();
}
template int dgp::predict_common<double>(dgp_plan*, const double*, const void*, int64_t, void*, void*, double**, double**, double**, long*,
                                         hipStream_t);
template int dgp::predict_common<float>(dgp_plan*, const double*, const void*, int64_t, void*, void*, float**, float**, float**, long*,
                                        hipStream_t);

template <typename T>
static int predict(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, void* var,
                   hipStream_t s) {
  T *V, *Xst, *vpad;
  long wbs;
  int rc = predict_common<T>(p, theta, Xs, m, work, mean, &V, &Xst, &vpad, &wbs, s);
  if (rc) return rc;
  copy_rows_kernel<T><<<dim3((unsigned)((m + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>(vpad, m, (T*)var, wbs);
  return (int)hipGetLastError();
}

template <typename T>
static int post_cov(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, void* cov,
                    hipStream_t s) {
  Posterior<T> ps;
  if (int rc = ps.fill(p, theta, Xs, m, work, mean, s)) return rc;
  if (int rc = ps.zero_noise()) return rc;
  const long M = ps.M;
  if (int rc = gram_sym<T>(p->model, p->d, ps.Xst, M, (int)m, theta, ps.var, (T*)cov, s, ps.batch(), p->pre, nullptr, M * M, ps.wbs, true)) return rc;
  return posterior_cov<T>(ps.V, p->N, M, (T*)cov, s, p->B, ps.wbs);
}

struct VjpLayout {
  size_t Xst, Ks, g, beta, part, spart, total;
};
static VjpLayout vjp_layout(const dgp_plan* p, int64_t m) {
  const size_t M = (size_t)round_up(m, DGP_TILE_HOST), e = p->elem, N = (size_t)p->N;
  const size_t nb = N / 64, blocks_sym = nb * (nb + 1) / 2, blocks_cross = (M / 64) * nb;
  VjpLayout L;
  Carve c;
  L.Xst = c.take(e * M * p->d);
  L.Ks = c.take(e * N * M);
  L.g = c.take(e * (N > M ? N : M));
  L.beta = c.take(e * N);
  L.part = c.take(e * 24 * (blocks_sym > blocks_cross ? blocks_sym : blocks_cross));
  L.spart = c.take(e * (size_t)solve_partials(p->N));
  L.total = c.o;
  return L;
}

template <typename T>
__global__ void matvec_cols_kernel(const T* Ks, long N, long Mp, int n, const T* alpha, T* out, long bs, long wbs, const int* ns) {
  // out[j] = sum_i Ks[i][j] alpha_i : one thread per column, coalesced across columns
  Ks = site(Ks, wbs);
  out = site(out, wbs);
  alpha = site(alpha, bs);
  n = site_n(ns, n);
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  T acc = T(0);
  for (long i = 0; i < n; ++i) acc += Ks[i * Mp + j] * alpha[i];
  out[j] = acc;
}

template <typename T>
static int predict_mean(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean,
                        hipStream_t s) {
  const VjpLayout L = vjp_layout(p, m);
  const long M = round_up(m, DGP_TILE_HOST);
  const long wbs = p->B > 1 ? (long)(L.total / sizeof(T)) : 0;
  const Batch bt = batch_of<T>(p);
  char* w = (char*)work;
  int rc = cross<T>(p, theta, Xs, m, w + L.Xst, w + L.Ks, s, wbs);
  if (rc) return rc;
  matvec_cols_kernel<T><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>((const T*)(w + L.Ks), p->N, M, (int)p->n,
                                                                                           (const T*)p->alpha, (T*)(w + L.g), bt.ws, wbs, bt.ns);
  copy_rows_kernel<T><<<dim3((unsigned)((m + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>((const T*)(w + L.g), m, (T*)mean, wbs);
  return (int)hipGetLastError();
}

template <typename T>
static int mean_vjp(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* wts, void* work,
                    void* dtheta, void* dr, void* dnoise, hipStream_t s) {
  const VjpLayout L = vjp_layout(p, m);
  const long M = round_up(m, DGP_TILE_HOST);
  const long wbs = p->B > 1 ? (long)(L.total / sizeof(T)) : 0;
  const Batch bt = batch_of<T>(p);
  char* w = (char*)work;
  T* Xst = (T*)(w + L.Xst);
  T* Ks = (T*)(w + L.Ks);
  T* g = (T*)(w + L.g);
  T* beta = (T*)(w + L.beta);
  int rc = cross<T>(p, theta, Xs, m, Xst, Ks, s, wbs);
  if (rc) return rc;
  if ((rc = gemv_rows<T>(Ks, p->N, M, (int)m, (const T*)wts, g, s, p->B, wbs))) return rc;   // g = K(X, X*) w
  if ((rc = symv_lower<T>((const T*)p->S, p->N, g, (int)p->n, (const T*)p->alpha, beta, (T*)(w + L.spart),
                          (T*)dnoise, s, bt, wbs)))                                         // beta = K^^-1 g
    return rc;
  if (dr) copy_rows_kernel<T><<<dim3((unsigned)((p->n + 255) / 256), 1, (unsigned)p->B), 256, 0, s>>>(beta, p->n, (T*)dr, wbs);
  PreSlot slot(p, s);
  return mean_vjp_grad<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, Xst, M, (int)m, theta, (const T*)p->alpha,
                          beta, (const T*)wts, (T*)(w + L.part), (T*)dtheta, s, bt, wbs, p->B > 1 ? p->ntheta : 0, p->pre, slot.staging);
}

// ---- posterior products of `planes` side-by-side cross Grams per test point: the covariance's additive parts (dgp_terms.hip,
// planes = C) and the value with its input derivatives (dgp_slopes.hip, planes = P = 1 + ncols).  Work area per site: the test
// points' SoA copy, the cross Grams side by side (N x planes M), V = T Ks of the same shape, `prior_rows` rows of M prior
// (co)variances -- the parts' C variances, or the derivatives' packed P (P + 1) / 2 block -- and the slab partials.
struct PlanesLayout {
  size_t Xst, Ks, V, prior, part, total;
};
static PlanesLayout planes_layout(const dgp_plan* p, int64_t m, int planes, int prior_rows) {
  const size_t M = (size_t)round_up(m, DGP_TILE_HOST), e = p->elem, N = (size_t)p->N;
  PlanesLayout L;
  Carve c;
  L.Xst = c.take(e * M * p->d);
  L.Ks = c.take(e * N * (size_t)planes * M);
  L.V = c.take(e * N * (size_t)planes * M);
  L.prior = c.take(e * (size_t)prior_rows * M);
  L.part = c.take(e * (size_t)terms_partials(planes, (long)M));
  L.total = c.o;
  return L;
}

// The driver: pack the test points, fill the cross planes, the prior rows, V = T Ks at width planes x M, reduce.  The three
// launchers that differ between the products are callables:
//   cross(Xst, M, Ks, bt, wbs, staging)      prior(Xst, M, prior, wb, wbs)      reduce(V, Ks, M, prior, part, bt, wbs)
template <typename T, typename Cross, typename Prior, typename Reduce>
static int predict_planes(dgp_plan* p, const void* Xs, int64_t m, const PlanesLayout& L, int planes, void* work, hipStream_t s,
                          Cross cross, Prior prior, Reduce reduce) {
  const long M = round_up(m, DGP_TILE_HOST);
  const long wbs = p->B > 1 ? (long)(L.total / sizeof(T)) : 0;
  const Batch bt = batch_of<T>(p);
  char* w = (char*)work;
  T* Xst = (T*)(w + L.Xst);
  T* Ks = (T*)(w + L.Ks);
  T* V = (T*)(w + L.V);
  T* pr = (T*)(w + L.prior);
  Batch wb;  // the test points: [B][m][d] -> SoA in the work area
  wb.B = p->B;
  wb.ws = wbs;
  int rc = pack_x<T>((const T*)Xs, (int)m, p->d, M, Xst, s, wb);
  if (rc) return rc;
  {
    PreSlot slot(p, s);
    if ((rc = cross(Xst, M, Ks, bt, wbs, slot.staging))) return rc;
  }
  wb.ws = 0;
  if ((rc = prior(Xst, M, pr, wb, wbs))) return rc;
  if ((rc = predict_v<T>((const T*)p->Tm, p->N, Ks, (long)planes * M, V, s, bt, wbs))) return rc;
  return reduce(V, Ks, M, pr, (T*)(w + L.part), bt, wbs);
}

template <typename T>
static int predict_terms(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, void* cov,
                         hipStream_t s) {
  const int C = model_nterms(p->model, p->d);
  return predict_planes<T>(
      p, Xs, m, planes_layout(p, m, C, C), C, work, s,
      [&](const T* Xst, long M, T* Ks, const Batch& bt, long wbs, void* staging) {
        return gram_cross_terms<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, Xst, M, (int)m, theta, Ks, s, bt, wbs, p->pre, staging);
      },
      [&](const T* Xst, long M, T* kss, const Batch& wb, long wbs) {
        return gram_diag_terms<T>(p->model, p->d, Xst, M, (int)m, theta, kss, s, wb, wbs, p->pre);
      },
      [&](const T* V, const T* Ks, long M, const T* kss, T* part, const Batch& bt, long wbs) {
        return terms_reduce<T>(C, V, Ks, p->N, M, (int)m, (const T*)p->alpha, kss, part, (T*)mean, (T*)cov, s, bt, wbs);
      });
}

template <typename T>
static int predict_slopes(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int* cols, int ncols, void* work,
                          void* mean, void* cov, hipStream_t s) {
  const int P = 1 + ncols;
  return predict_planes<T>(
      p, Xs, m, planes_layout(p, m, P, P * (P + 1) / 2), P, work, s,
      [&](const T* Xst, long M, T* Ks, const Batch& bt, long wbs, void* staging) {
        return gram_cross_slopes<T>(p->model, p->d, (const T*)p->Xt, p->N, (int)p->n, Xst, M, (int)m, theta, cols, ncols, Ks, s, bt, wbs,
                                    p->pre, staging);
      },
      [&](const T* Xst, long M, T* prior, const Batch& wb, long wbs) {
        return gram_prior_slopes<T>(p->model, p->d, Xst, M, (int)m, theta, cols, ncols, prior, s, wb, wbs, p->pre);
      },
      [&](const T* V, const T* Ks, long M, const T* prior, T* part, const Batch& bt, long wbs) {
        return slopes_reduce<T>(P, V, Ks, p->N, M, (int)m, (const T*)p->alpha, prior, part, (T*)mean, (T*)cov, s, bt, wbs);
      });
}

extern "C" {

size_t dgp_predict_workspace_bytes(const dgp_plan* p, int64_t m) {
  if (!p || m <= 0) return 0;
  return predict_layout(p, m).total * (size_t)p->B;
}

int dgp_predict(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes,
                void* mean, void* var, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !work || !mean || !var || m <= 0) return fail(DGP_E_ARG, "dgp_predict: null argument");
  if (int rc = need_factor(p, "dgp_predict", "call dgp_factorize")) return rc;
  if (work_bytes < dgp_predict_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_predict: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict<double>(p, theta, Xs, m, work, mean, var, s), predict<float>(p, theta, Xs, m, work, mean, var, s));
  return wrap(rc, "dgp_predict");
}

int dgp_posterior_cov(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes,
                      void* mean, void* cov, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !work || !mean || !cov || m <= 0) return fail(DGP_E_ARG, "dgp_posterior_cov: null argument");
  if (int rc = need_factor(p, "dgp_posterior_cov", "call dgp_factorize")) return rc;
  if (work_bytes < dgp_predict_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_posterior_cov: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int rc = DGP_BY_DTYPE(p, post_cov<double>(p, theta, Xs, m, work, mean, cov, s),
                        post_cov<float>(p, theta, Xs, m, work, mean, cov, s));
  return wrap(rc, "dgp_posterior_cov");
}

int dgp_model_nterms(int model, int d) { return model_nterms(model, d); }

size_t dgp_predict_terms_workspace_bytes(const dgp_plan* p, int64_t m) {
  if (!p || m <= 0) return 0;
  const int C = model_nterms(p->model, p->d);
  return planes_layout(p, m, C, C).total * (size_t)p->B;
}

int dgp_predict_terms(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes, void* mean,
                      void* cov, void* stream) {
  if (!p) return fail(DGP_E_ARG, "dgp_predict_terms: null plan");
  if (!theta || !Xs || !work || !mean || m <= 0) return fail(DGP_E_ARG, "dgp_predict_terms: null argument or m <= 0");
  if (!p->ws) return fail(DGP_E_WORKSPACE, "plan has no workspace: call dgp_plan_set_workspace");
  if (int rc = need_factor(p, "dgp_predict_terms", "call dgp_factorize")) return rc;
  if (work_bytes < dgp_predict_terms_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_predict_terms: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict_terms<double>(p, theta, Xs, m, work, mean, cov, s),
                              predict_terms<float>(p, theta, Xs, m, work, mean, cov, s));
  return wrap(rc, "dgp_predict_terms");
}

int dgp_model_input_differentiable(int model, int d, int col) { return model_input_differentiable(model, d, col); }

size_t dgp_predict_slopes_workspace_bytes(const dgp_plan* p, int64_t m, int ncols) {
  if (!p || m <= 0 || ncols < 1 || ncols > p->d) return 0;
  const int P = 1 + ncols;
  return planes_layout(p, m, P, P * (P + 1) / 2).total * (size_t)p->B;
}

int dgp_predict_slopes(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int* cols, int ncols, void* work,
                       size_t work_bytes, void* mean, void* cov, void* stream) {
  if (!p) return fail(DGP_E_ARG, "dgp_predict_slopes: null plan");
  if (!theta || !Xs || !cols || !work || !mean || m <= 0) return fail(DGP_E_ARG, "dgp_predict_slopes: null argument or m <= 0");
  if (ncols < 1 || ncols > p->d) return fail(DGP_E_ARG, "dgp_predict_slopes: ncols must be in 1 .. d");
  for (int q = 0; q < ncols; ++q) {
    if (cols[q] < 0 || cols[q] >= p->d) return fail(DGP_E_ARG, "dgp_predict_slopes: column outside 0 .. d - 1");
    for (int r = 0; r < q; ++r)
      if (cols[r] == cols[q]) return fail(DGP_E_ARG, "dgp_predict_slopes: repeated column");
  }
  for (int q = 0; q < ncols; ++q)
    if (model_input_differentiable(p->model, p->d, cols[q]) != 1)
      return fail(DGP_E_MODEL, "dgp_predict_slopes: the covariance is not differentiable in a requested column (Matern-1/2 factor)");
  if (!p->ws) return fail(DGP_E_WORKSPACE, "plan has no workspace: call dgp_plan_set_workspace");
  if (int rc = need_factor(p, "dgp_predict_slopes", "call dgp_factorize")) return rc;
  if (work_bytes < dgp_predict_slopes_workspace_bytes(p, m, ncols))
    return fail(DGP_E_WORKSPACE, "dgp_predict_slopes: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict_slopes<double>(p, theta, Xs, m, cols, ncols, work, mean, cov, s),
                              predict_slopes<float>(p, theta, Xs, m, cols, ncols, work, mean, cov, s));
  return wrap(rc, "dgp_predict_slopes");
}

size_t dgp_mean_vjp_workspace_bytes(const dgp_plan* p, int64_t m) { return (p && m > 0) ? vjp_layout(p, m).total * (size_t)p->B : 0; }

int dgp_predict_mean(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, size_t work_bytes,
                     void* mean, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !work || !mean || m <= 0) return fail(DGP_E_ARG, "dgp_predict_mean: null argument");
  if (int rc = need_factor(p, "dgp_predict_mean", nullptr)) return rc;
  if (work_bytes < dgp_mean_vjp_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_predict_mean: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = DGP_BY_DTYPE(p, predict_mean<double>(p, theta, Xs, m, work, mean, s), predict_mean<float>(p, theta, Xs, m, work, mean, s));
  return wrap(rc, "dgp_predict_mean");
}

int dgp_mean_vjp(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* wts, void* work,
                 size_t work_bytes, void* dtheta, void* dr, void* dnoise, void* stream) {
  DGP_CHECK_PLAN(p);
  if (!theta || !Xs || !wts || !work || !dtheta || m <= 0) return fail(DGP_E_ARG, "dgp_mean_vjp: null argument");
  if (!p->have_factor || !p->have_inverse)
    return fail(DGP_E_STATE, "dgp_mean_vjp: needs K^^-1 and alpha from dgp_fit_step at the same theta");
  if (work_bytes < dgp_mean_vjp_workspace_bytes(p, m)) return fail(DGP_E_WORKSPACE, "dgp_mean_vjp: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  return wrap(DGP_BY_DTYPE(p, mean_vjp<double>(p, theta, Xs, m, wts, work, dtheta, dr, dnoise, s),
                           mean_vjp<float>(p, theta, Xs, m, wts, work, dtheta, dr, dnoise, s)), "dgp_mean_vjp");
}

int dgp_sample_draws(int dtype, const void* L, int64_t m, const void* Z, int64_t ndraw, const void* mean, void* out,
                     void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_sample_draws: dtype must be 0 (f64) or 1 (f32)");
  if (!L || !Z || !out || m <= 0 || ndraw <= 0 || m > (1 << 20) || ndraw > (1 << 24))
    return fail(DGP_E_ARG, "dgp_sample_draws: null argument / bad size");
  const long M = round_up(m, DGP_TILE_HOST), Q = round_up(ndraw, DGP_TILE_HOST);
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64
                     ? sample_draws<double>((const double*)L, M, (const double*)Z, Q, (const double*)mean, (int)m, (int)ndraw, (double*)out, s)
                     : sample_draws<float>((const float*)L, M, (const float*)Z, Q, (const float*)mean, (int)m, (int)ndraw, (float*)out, s);
  return wrap(rc, "dgp_sample_draws");
}

}  // extern "C"
