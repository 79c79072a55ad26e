// dgp_stream.h -- the posterior front end: what every entry that works from the held factorisation does before and around its own
// launches.  The prediction's first stages leave V = L^-1 K(X, Xs) (N x M), the test points' SoA coordinates (d x M) and the
// predicted variance (M) in the head of the caller's work area; the posterior covariance C = K(Xs, Xs) - V^T V then comes whole
// (dgp_posterior_cov), as one block (dgp_posterior_cov_block), or R rows at a time into a panel that the streamed passes consume
// and overwrite (dgp_exceed_stream.hip, dgp_excess_stream.hip, dgp_design_stream.hip, dgp_window_stream.hip).  Panel q holds the
// rows [q R, (q + 1) R) of C and the columns 0 .. (q + 1) R - 1 in a buffer of R x M elements: gram_sym's tiles of K(Xs, Xs)
// followed by posterior_cov's trailing update, both on the tile rows of the panel only -- the launches, the k order and hence
// (fp64) the bits of dgp_posterior_cov.  Every unordered pair (i < j) lies in exactly one panel, j's.  A band is the same with the
// columns before c0 = window_band_col0(p0, reach) left out.  What this header holds for all of them:
//   - the diagonal of C is the predicted variance: a pass reads `var` (its prepare launch), never a panel's diagonal;
//   - `var` is consumed BEFORE zero_noise() turns its place into the zero "noise" of K(Xs, Xs);
//   - the hyperparameter scratch of a large batch is already filled by `cross` in the same call when a panel's Gram runs
//     (the Gram launchers' prepare_batch(..., false)): fill() comes first, always;
//   - R is clamped to M before any size is computed: panel_bytes() and the loops clamp, nobody else does.
// Private to csrc, host code only.
#pragma once
#include "dgp_plan.h"

namespace dgp {

// ---- panel sizing, for all streamed passes
inline long panel_rows(long m, long R) {
  const long M = round_up(m, DGP_TILE_HOST);
  return R < M ? R : M;
}
inline bool panel_rows_ok(int panel_rows) { return panel_rows > 0 && panel_rows % DGP_TILE_HOST == 0; }
// one site's panel: panel_rows(m, rows) x cols elements
inline size_t panel_bytes(const dgp_plan* p, int64_t m, long rows, long cols) {
  return Carve::up(p->elem * (size_t)panel_rows((long)m, rows) * (size_t)cols);
}
// first column of the band of rows [p0, ..) when two points share a window only if they are less than `reach` apart
inline long window_band_col0(long p0, long reach) {
  const long c = p0 - reach + 1;
  return c > 0 ? c / DGP_TILE_HOST * DGP_TILE_HOST : 0;
}

// ---- the work area: the prediction's area x B, then `pb` bytes per site (a panel, or whatever else the entry keeps per site),
// then the entry's own area
template <typename T>
struct PosteriorAreas {
  T* panel;
  void* own;
  long pstride;  // elements between the sites' panels
};
inline size_t posterior_head_bytes(const dgp_plan* p, int64_t m, size_t pb) { return (predict_layout(p, m).total + pb) * (size_t)p->B; }
template <typename T>
inline PosteriorAreas<T> posterior_areas(const dgp_plan* p, int64_t m, void* work, size_t pb) {
  PosteriorAreas<T> A;
  A.panel = (T*)((char*)work + posterior_head_bytes(p, m, 0));
  A.own = (char*)work + posterior_head_bytes(p, m, pb);
  A.pstride = (long)(pb / sizeof(T));
  return A;
}

// ---- the prediction's state and the loops over it
template <typename T>
struct Posterior {
  dgp_plan* p;
  const double* theta;
  hipStream_t s;
  long m, M, wbs;
  T *V, *Xst, *var;

  // The prediction's first stages into the head of `work`.  The latent mean it also writes (B x m elements) goes to `mean`:
  // the caller's output, or the head of the entry's own area, which the entry's first launch resets.
  int fill(dgp_plan* plan, const double* th, const void* Xs, int64_t points, void* work, void* mean, hipStream_t stream) {
    p = plan, theta = th, s = stream, m = (long)points, M = round_up(points, DGP_TILE_HOST);
    return predict_common<T>(p, theta, Xs, points, work, mean, &V, &Xst, &var, &wbs, s);
  }
  // `var` becomes the zero "noise" of K(Xs, Xs) (a batched plan's sites keep theirs at the work area's site stride): whatever
  // reads the predicted variance must have been enqueued before
  int zero_noise() const {
    return (int)hipMemset2DAsync(var, sizeof(T) * (size_t)(wbs > 0 ? wbs : M), 0, sizeof(T) * M, (size_t)p->B, s);
  }
  Batch batch() const {  // the work area as a batch
    Batch wb;
    wb.B = p->B;
    wb.ws = wbs;
    return wb;
  }
  // rows [p0, p1) x columns [c0, p1) of C into `band` (first element C[p0][c0], leading dimension ld, site stride bstride)
  int band(T* band, long p0, long p1, long c0, long ld, long bstride) const {
    if (int rc = gram_sym_band<T>(p->model, p->d, Xst, M, (int)m, theta, var, band, p0, p1, c0, ld, s, batch(), p->pre, bstride, wbs)) return rc;
    return posterior_cov_band<T>(V, p->N, M, band, p0, p1, c0, ld, bstride, s, p->B, wbs);
  }
  // Every panel of panel_rows(m, R) rows in ascending order: the panel of C, then body(p0, p1) -- the caller's launches on it.
  // Stops at the first launcher that fails.
  template <typename Body>
  int panels(long R, T* panel, long pstride, Body body) const {
    R = panel_rows(m, R);
    const Batch wb = batch();
    for (long p0 = 0; p0 < M; p0 += R) {
      const long p1 = p0 + R < M ? p0 + R : M;
      int rc = gram_sym_panel<T>(p->model, p->d, Xst, M, (int)m, theta, var, panel, p0, p1, s, wb, p->pre, pstride, wbs);
      if (rc) return rc;
      if ((rc = posterior_cov_panel<T>(V, p->N, M, panel, p0, p1, pstride, s, p->B, wbs))) return rc;
      body(p0, p1);
    }
    return 0;
  }
  // the same with bands: body(p0, p1, c0)
  template <typename Body>
  int bands(long R, long reach, long ld, T* buf, long bstride, Body body) const {
    R = panel_rows(m, R);
    for (long p0 = 0; p0 < M; p0 += R) {
      const long p1 = p0 + R < M ? p0 + R : M, c0 = window_band_col0(p0, reach);
      if (int rc = band(buf, p0, p1, c0, ld, bstride)) return rc;
      body(p0, p1, c0);
    }
    return 0;
  }
};

// ---- the entry prologue of the posterior entries whose checks, order and texts are exactly these (the rule above need_work):
// need_factor with the hint "call dgp_factorize or dgp_fit_step", DGP_CHECK_PLAN, need_work against `need`, factor_ok, then
// run(T(), stream) for the plan's T, wrapped
template <typename Run>
inline int posterior_entry(dgp_plan* p, const char* where, const void* work, size_t work_bytes, size_t need, void* stream, Run run) {
  if (int rc = need_factor(p, where, "call dgp_factorize or dgp_fit_step")) return rc;
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  int rc = need_work(work, work_bytes, need, where);
  if (rc || (rc = factor_ok(p, s, where))) return rc;
  return wrap(DGP_BY_DTYPE(p, run(double(), s), run(float(), s)), where);
}

}  // namespace dgp
