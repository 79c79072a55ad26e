// dgp_plan.h -- the plan as the entry points see it: its fields, its workspace layout, the error channel and the checks every
// entry repeats.  Private to csrc: neither include/ nor the Python package knows it.  dgp_api.hip owns the plan and the fit step;
// every other entry point lives in the unit that holds the launchers it drives and reaches the plan through this header.
#pragma once
#include <stdarg.h>

#include <type_traits>

#include "../../include/dgp_hip.h"
#include "dgp_internal.h"

// Small host -> device uploads (site sizes, the hyperparameters of large batches) go through PINNED staging slots that
// the plan owns: an asynchronous copy from pageable memory is only safe while the runtime happens to stage it before
// returning.  A slot is reused after the event recorded behind its last copy has completed.
struct PinnedRing {
  static constexpr int SLOTS = 4;
  void* buf[SLOTS];
  size_t cap[SLOTS];
  hipEvent_t ev[SLOTS];
  int busy[SLOTS], have_ev[SLOTS], next;
  void* acquire(size_t bytes) {
    const int i = next;
    if (busy[i]) {
      (void)hipEventSynchronize(ev[i]);
      busy[i] = 0;
    }
    if (cap[i] < bytes) {
      if (buf[i]) (void)hipHostFree(buf[i]);
      buf[i] = nullptr;
      cap[i] = 0;
      if (hipHostMalloc(&buf[i], bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
      cap[i] = bytes;
    }
    return buf[i];
  }
  void commit(hipStream_t s) {  // after the copy out of the slot handed out last has been enqueued on s
    const int i = next;
    if (!have_ev[i]) have_ev[i] = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    if (have_ev[i] && hipEventRecord(ev[i], s) == hipSuccess) busy[i] = 1;
    else (void)hipStreamSynchronize(s);
    next = (next + 1) % SLOTS;
  }
  void destroy() {
    for (int i = 0; i < SLOTS; ++i) {
      if (busy[i]) (void)hipEventSynchronize(ev[i]);
      if (have_ev[i]) (void)hipEventDestroy(ev[i]);
      if (buf[i]) (void)hipHostFree(buf[i]);
    }
  }
};

struct dgp_plan {
  int model, dtype, d, ntheta;
  PinnedRing ring;
  int* nsite_host;        // host copy of the sites' sizes (B > 1): the inference entry points walk the sites on the host
  int B;                  // sites carried in lockstep (1 = plain plan); site b's buffers sit b * site_bytes further on
  size_t site_bytes;
  void* pre;              // device scratch for the batch's hyperparameters (B > 8), after the last site
  void* pre2;             // a second one for the fp64 evaluator of the refinement (fp32 plans), so that `pre` stays valid
  int pre_ready;          // the Gram build of the current step has uploaded them
  dgp::Tuning tune;       // tile-shape selectors (dgp_plan_set_option)
  int refine;             // fp32 plans: one step of iterative refinement with an fp64 residual after the solves
  int* nsite;             // device: the sites' own sizes (B > 1), after the hyperparameter scratch
  const void* dr_w;       // caller's [2][n] weight vectors for the out[DGP_OUT_DR_W0..] reductions, or null
  int64_t n, N;
  size_t elem;
  char* ws;
  size_t ws_bytes;
  // carved workspace
  void *Xt, *A, *Tm, *S, *z, *alpha, *gpart, *spart, *scal, *snap;
  int* info;
  hipStream_t sc;         // rest of the split panel chain (dgp_chol.hip::potrf_split)
  int lookahead, early;   // potrf schedule; issue the inverse's level recursion behind the factorisation's checkpoints
  int have_inputs, have_factor, have_inverse;
  hipStream_t s2, s3;     // bulk trailing updates; early inverse work
  hipEvent_t xev[8];      // checkpoints of the factorisation and fork/join events for s3
  int have_xev;
  hipEvent_t* ev;
  int nev;
  // optional HIP-event timing of the fit-step stages
  int timing, n_syrk, timed_valid;
  double syrk_flop;
  hipEvent_t* tev;   // 2 per stage (start, stop)
  hipEvent_t* sev;   // 2 per bulk syrk launch
  int nsev;
};

namespace dgp {

// ---- the error channel: ONE thread_local text, defined in dgp_api.hip and read by dgp_last_error().  Each sets the text and
// returns the code it was given, so that an entry can `return fail(...)`.
int fail(int code, const char* msg);
int hipfail(hipError_t e, const char* where);  // "<where>: <the runtime's text>", returns (int)e
int failf(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int wrap(int rc, const char* where) {  // a launcher's result: a HIP error (> 0), a DGP_E_* (< 0) or 0
  if (rc > 0) return hipfail((hipError_t)rc, where);
  if (rc < 0) return fail(rc, where);
  return 0;
}

#define DGP_BY_DTYPE(p, CALL64, CALL32) ((p)->dtype == DGP_F64 ? (CALL64) : (CALL32))
#define DGP_CHECK_PLAN(p)                                                        \
  if (!(p)) return fail(DGP_E_ARG, "null plan");                                 \
  if (!(p)->ws) return fail(DGP_E_WORKSPACE, "plan has no workspace: call dgp_plan_set_workspace")
#define DGP_SINGLE_SITE(p) \
  if ((p)->B != 1)         \
  return fail(DGP_E_STATE, "batched plans support dgp_set_inputs / dgp_fit_step / dgp_factorize / dgp_predict / dgp_predict_mean / dgp_mean_vjp only")

// The three checks that used to be pasted.  Each returns 0 or the refusal's code with its text set; an entry uses one only where
// its own text and ORDER of checks are exactly these -- entries that differ keep their own line.
//   "<where>: workspace missing or too small" (DGP_E_WORKSPACE), then "<where>: the work area must be 256-byte aligned" (DGP_E_ARG)
inline int need_work(const void* work, size_t bytes, size_t need, const char* where) {
  if (!work || bytes < need) return failf(DGP_E_WORKSPACE, "%s: workspace missing or too small", where);
  if (((uintptr_t)work & 255) != 0) return failf(DGP_E_ARG, "%s: the work area must be 256-byte aligned", where);
  return 0;
}
//   "<where>: no factorisation in the plan (<hint>)", without the parenthesis when hint is null
inline int need_factor(const dgp_plan* p, const char* where, const char* hint) {
  if (p->have_factor) return 0;
  return hint ? failf(DGP_E_STATE, "%s: no factorisation in the plan (%s)", where, hint)
              : failf(DGP_E_STATE, "%s: no factorisation in the plan", where);
}
// A failed factorisation leaves no T to read: every site's pivot word, read back on `s` (synchronises it) before any launch.
//   "<where>: the factorisation the plan holds failed (matrix not positive definite)" (DGP_E_STATE)
int factor_ok(dgp_plan* p, hipStream_t s, const char* where);

// ---- the plan's workspace: B sites of `total` bytes, then the hyperparameter scratch of a batch of more than 8 (twice: `pre`
// and the refinement's `pre2`), then the sites' sizes (B > 1)
struct Layout {
  size_t Xt, A, Tm, S, z, alpha, gpart, spart, scal, info, snap, total;  // inside a site
  size_t pre, pre2, nsite, ws_total;                                     // behind the last site; the whole workspace
};
inline Layout layout(const dgp_plan* p) {
  Layout L;
  const size_t e = p->elem, N = (size_t)p->N;
  Carve c;
  L.Xt = c.take(e * N * p->d);
  L.A = c.take(e * N * N);
  L.Tm = c.take(e * N * N);
  L.S = c.take(e * N * N);
  L.z = c.take(e * N);
  L.alpha = c.take(e * N);
  L.gpart = c.take(e * (size_t)gram_grad_partials(p->N));
  L.spart = c.take(e * (size_t)solve_partials(p->N));
  L.scal = c.take(e * 16);
  L.info = c.take(sizeof(int) * POTRF_INFO_INTS);
  L.snap = c.take(e * 2 * DGP_TILE_HOST * DGP_TILE_HOST);  // the split chain's two snapshot blocks
  L.total = c.o;
  c.o *= (size_t)p->B;
  L.pre = c.take(pre_scratch_bytes(p->B));
  L.pre2 = c.take(pre_scratch_bytes(p->B));
  L.nsite = c.take(p->B > 1 ? sizeof(int) * (size_t)p->B : 0);
  L.ws_total = c.o;
  return L;
}

template <typename T>
inline Batch batch_of(const dgp_plan* p) {
  Batch bt;
  bt.B = p->B;
  bt.ws = (long)(p->site_bytes / sizeof(T));  // layout offsets are multiples of 256 bytes
  bt.ns = p->nsite;
  bt.tune = &p->tune;
  bt.W = p->S;  // scratch of the factorisation's group inverse (S is free until trtri / lauum use it)
  return bt;
}

// hyperparameters of a batch of more than 8 sites travel through the plan's device scratch + a pinned staging slot
struct PreSlot {
  dgp_plan* p;
  void* staging;
  hipStream_t s;
  PreSlot(dgp_plan* plan, hipStream_t st) : p(plan), staging(plan->pre ? plan->ring.acquire(pre_scratch_bytes(plan->B)) : nullptr), s(st) {
    plan->pre_ready = 0;  // the fit step's copy of the hyperparameters is overwritten
  }
  ~PreSlot() {
    if (staging) p->ring.commit(s);
  }
};

// ---- the prediction's work area, per site (a batched plan: one slice per site at the single-site size): the test points' SoA
// copy, K(X, X*) and V = T K(X, X*) (N x M each), the prior variances, the padded mean and variance, the slab partials.
// dgp_predict.hip fills it; the posterior entries put their own areas behind it (dgp_stream.h).
struct PredictLayout {
  size_t Xst, Ks, V, kss, mean, var, part, total;
};
inline PredictLayout predict_layout(const dgp_plan* p, int64_t m) {
  const size_t M = (size_t)round_up(m, DGP_TILE_HOST), e = p->elem, N = (size_t)p->N;
  PredictLayout L;
  Carve c;
  L.Xst = c.take(e * M * p->d);
  L.Ks = c.take(e * N * M);
  L.V = c.take(e * N * M);
  L.kss = c.take(e * M);
  L.mean = c.take(e * M);
  L.var = c.take(e * M);
  L.part = c.take(e * 2 * PREDICT_SPLIT * M);
  L.total = c.o;
  return L;
}

// folds of the cross-validation entries (dgp_crossval.hip, dgp_censored_cv.hip)
inline bool cv_sizes_ok(const dgp_plan* p, int ngroups, int64_t max_group) {
  return p && ngroups >= 1 && ngroups <= p->n && max_group >= 1 && max_group <= p->n;
}

// sizes of the exceedance entries (dgp_exceed.hip, dgp_exceed_stream.hip)
inline bool ex_sizes_ok(int64_t m, int ngroups, int nlevels, int batch) {
  return m > 0 && m <= (1 << 20) && ngroups > 0 && ngroups <= 65535 && nlevels >= 1 && nlevels <= 64 && batch > 0 &&
         batch <= DGP_MAX_BATCH_SITES;
}
// their L levels in chunks of 8, then 4, 2, 1 -- a function of L alone --: rc = f(l0, width), the width a compile-time constant
// (std::integral_constant); stops at the first non-zero rc and returns it
template <typename F>
inline int level_chunks(int L, F f) {
  int rc = 0, l0 = 0;
  auto chunk = [&](auto width) {
    rc = f(l0, width);
    l0 += width;
  };
  while (l0 < L && !rc) {
    const int left = L - l0;
    if (left >= 8) chunk(std::integral_constant<int, 8>());
    else if (left >= 4) chunk(std::integral_constant<int, 4>());
    else if (left >= 2) chunk(std::integral_constant<int, 2>());
    else chunk(std::integral_constant<int, 1>());
  }
  return rc;
}

// ---- what crosses units (explicitly instantiated for double and float where it is defined)
// dgp_api.hip: one fit step (with_grad) or the factorise path (without), and K(X, X*) into the caller's work area
template <typename T>
int fit_step(dgp_plan* p, const double* theta, const void* r, const void* noise, void* out, void* dr, void* dnoise, int with_grad,
             hipStream_t s);
template <typename T>
int cross(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* Ks, hipStream_t s, long wbs = 0);
// dgp_predict.hip: the prediction's first stages into a PredictLayout; the latent mean (B x m) to `mean`
template <typename T>
int predict_common(dgp_plan* p, const double* theta, const void* Xs, int64_t m, void* work, void* mean, T** V_out, T** Xst_out,
                   T** vpad_out, long* wbs_out, hipStream_t s);
extern template int fit_step<double>(dgp_plan*, const double*, const void*, const void*, void*, void*, void*, int, hipStream_t);
extern template int fit_step<float>(dgp_plan*, const double*, const void*, const void*, void*, void*, void*, int, hipStream_t);
extern template int cross<double>(dgp_plan*, const double*, const void*, int64_t, void*, void*, hipStream_t, long);
extern template int cross<float>(dgp_plan*, const double*, const void*, int64_t, void*, void*, hipStream_t, long);
extern template int predict_common<double>(dgp_plan*, const double*, const void*, int64_t, void*, void*, double**, double**, double**,
                                           long*, hipStream_t);
extern template int predict_common<float>(dgp_plan*, const double*, const void*, int64_t, void*, void*, float**, float**, float**, long*,
                                          hipStream_t);

}  // namespace dgp
