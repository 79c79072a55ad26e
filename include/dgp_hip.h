/* dgp_hip.h -- C ABI of libdgp_hip.so, the MI355X (gfx950) exact-GP marginal-likelihood engine.
 *
 * The reference (thodson-usgs/discontinuum) has NO FFI for this path: its boundary is the Python
 * class contract of `MarginalGPyTorch` (src/discontinuum/engines/gpytorch.py:36-626) and the hot-path
 * arithmetic is delegated to gpytorch.  Each entry point below therefore cites the reference call site
 * whose work it replaces.  Plain pointers and sizes only: device pointers are owned by the caller
 * (e.g. torch tensors), `stream` is a hipStream_t passed as void*, host pointers are read before
 * the call returns.  All functions are asynchronous on `stream` and return 0 on success, a negative
 * DGP_E* code for bad arguments, or a positive hipError_t.  No exceptions cross the ABI; a
 * non-positive-definite matrix is reported through the `info` slot of the output vector
 * (index of the first failing pivot, 1-based; the NLL is then NaN) so that the caller's NaN/exception
 * guard (engines/gpytorch.py:352-382) keeps working.
 *
 * dtype: 0 = float64, 1 = float32 (sizeof element = 8 / 4; every device array below has that type).
 * model: 0 = loadest-gp composite kernel, d columns (time first), 2d+5 constrained hyperparameters
 *            (src/loadest_gp/models/gpytorch.py:61-128)
 *        1 = rating-gp composite kernel, d = 2 (time, stage), 16 constrained hyperparameters
 *            (src/rating_gp/models/gpytorch.py:205-372, src/rating_gp/models/kernels.py:242-382)
 *        >= 16: a generic composite model registered with dgp_composite_define (below)
 *        parameter order: DESIGN.md section "Hyperparameter vectors".
 */
#ifndef DGP_HIP_H
#define DGP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGP_F64 0
#define DGP_F32 1
#define DGP_MODEL_LOADEST 0
#define DGP_MODEL_RATING 1

#define DGP_E_ARG (-1)       /* null pointer / bad size / bad dtype */
#define DGP_E_MODEL (-2)     /* unsupported (model, d) */
#define DGP_E_WORKSPACE (-3) /* workspace missing or too small */
#define DGP_E_STATE (-4)     /* call order violated (e.g. predict before factorize) */
#define DGP_E_FULL (-5)      /* dgp_composite_define: all 64 slots of the process hold other structures */
#define DGP_E_NOCONV (-6)    /* dgp_laplace_*: the mode search did not converge within maxit Newton iterations */

/* output vector of dgp_fit_step / dgp_factorize, in elements of the plan dtype */
#define DGP_OUT_NLL 0    /* 1/2 r^T K^^-1 r + 1/2 log|K^| + n/2 log 2 pi */
#define DGP_OUT_QUAD 1   /* r^T K^^-1 r */
#define DGP_OUT_LOGDET 2 /* log|K^| */
#define DGP_OUT_INFO 3   /* 0, or 1-based index of the first non-positive pivot; -7: an internal wait of the factorisation's
                            split panel chain timed out (the NLL is NaN; see dgp_chol.hip::chain_wait) */
#define DGP_OUT_DTHETA 4 /* d NLL / d theta_p, p = 0 .. ntheta-1 */
#define DGP_OUT_SUM_DR 28 /* sum_i d NLL / d r_i (gradient of a constant prior mean is its negative); fit step only */
#define DGP_OUT_DR_W0 29  /* sum_i d NLL / d r_i * w0[i], and w1 in the next slot: see dgp_plan_set_dr_weights */
#define DGP_OUT_SUM_DNOISE 31 /* sum_i d NLL / d noise_i (gradient of a homoskedastic noise term); fit step only */
#define DGP_OUT_LEN 32

/* buffers exposed by dgp_plan_buffer (tests and profiling) */
#define DGP_BUF_XT 0    /* coordinates, SoA d x N */
#define DGP_BUF_A 1     /* K^ then its Cholesky factor L (lower), N x N row-major */
#define DGP_BUF_T 2     /* L^-1 (lower) */
#define DGP_BUF_S 3     /* K^^-1 (lower) */
#define DGP_BUF_Z 4     /* L^-1 r */
#define DGP_BUF_ALPHA 5 /* K^^-1 r */
#define DGP_BUF_INFO 6  /* int32: info of the last factorisation */
#define DGP_BUF_SCAL 7  /* scalars: [0] log|K^| accumulated by the diagonal-block kernels, [1] r^T K^^-1 r; float32 plans also keep
                           both UNROUNDED as doubles at elements [2..3] and [4..5] (the NLL's three terms are added in double) */

typedef struct dgp_plan dgp_plan;

int dgp_version(void);
const char* dgp_last_error(void);
/* number of constrained kernel hyperparameters of (model, d); <0 if unsupported */
int dgp_model_ntheta(int model, int d);
/* A GENERIC model: any sum of (optionally scaled) products of stationary factors -- RBF, Matern(nu = 1/2, 3/2, 5/2),
 * Periodic -- on subsets of the d <= 6 input columns, e.g. the reference's covariance with its unused trend term
 * (src/loadest_gp/models/gpytorch.py:78-88) switched on.  `spec` (host ints) describes the tree:
 *     d, nterms, then per term:  scaled (0/1), nfactors (<= 3), then per factor:
 *         type (0 RBF, 1 Matern, 2 Periodic), 2 nu (Matern: 1, 3, 5; else 0), ard (0/1), ndims, the ndims column indices
 * (<= 6 terms, Periodic factors on one column).  The constrained hyperparameters follow the same order: per term
 * [outputscale if scaled], per factor [lengthscale: one, or one per column if ard], [period if Periodic]; at most 24.
 * *model_out (>= 16) is then accepted wherever a model id is (dgp_plan_create, dgp_dist_create, dgp_model_ntheta).  An
 * interpreted evaluator: slower per matrix entry than the two fused models, same kernels otherwise.
 * Returns 0, DGP_E_MODEL for a malformed or unsupported description, DGP_E_FULL when the process already holds 64 distinct
 * structures (an identical description reuses its id and never needs a slot); *model_out is written on success only. */
int dgp_composite_define(const int* spec_host, int nspec, int* model_out);
/* padded order N = round_up(n, 128) used by every N x N buffer */
int64_t dgp_padded_n(int64_t n);

/* A plan fixes (model, dtype, n, d) and owns host-side resources only (up to two internal HIP streams
 * and events).  Device memory is the caller's: query the size, allocate, hand it over. */
int dgp_plan_create(int model, int dtype, int64_t n, int d, dgp_plan** out);
int dgp_plan_destroy(dgp_plan* plan);
size_t dgp_plan_workspace_bytes(const dgp_plan* plan);
/* Optional, before dgp_plan_set_workspace: carry `batch` (1..1024) independent sites of the same (model, dtype, n, d)
 * in lockstep -- every kernel of a fit step is launched once for all of them (gridDim.z = batch), which amortises
 * the sequential panel chain and the launch rate over the batch (the reference analogue is its map over sites,
 * examples/nwqn-loadest-example/nwqn-loadest-example.py:156-159).  The workspace grows by the same factor and the
 * arrays of dgp_set_inputs / dgp_fit_step / dgp_factorize become batch-major: X[batch][n][d], theta[batch][ntheta],
 * r / noise / dr / dnoise [batch][n], out[batch][DGP_OUT_LEN].  dgp_predict, dgp_posterior_cov, dgp_predict_mean and
 * dgp_mean_vjp also accept batched plans: every site works at its own m points -- Xs[batch][m][d], theta[batch][ntheta]
 * -> mean / var [batch][m], cov [batch][M][M]; dgp_mean_vjp: w[batch][m] -> dtheta[batch][ntheta], dr / dnoise [batch][n]
 * -- with ONE launch sequence for all sites (gridDim.z = batch, like the fit step); their work areas are batch times the
 * single-site size (the *_workspace_bytes queries account for it).  The stage-level entries dgp_stage_grad and
 * dgp_cross_gram need batch == 1. */
int dgp_plan_set_batch(dgp_plan* plan, int batch);
int dgp_plan_batch(const dgp_plan* plan);
/* Ragged batches (after dgp_plan_set_workspace, before dgp_set_inputs): site b has sizes[b] <= n observations; it
 * uses the first sizes[b] rows of its [n]-sized slots in X / r / noise (the rest is ignored), its padding is handled
 * like the plan's own (identity), its NLL carries sizes[b]/2 log(2 pi), and dr / dnoise are zero beyond sizes[b]. */
int dgp_plan_set_site_sizes(dgp_plan* plan, const int64_t* sizes_host, void* stream);
int dgp_plan_set_workspace(dgp_plan* plan, void* dev_ptr, size_t bytes);
/* Reductions for a parametric prior mean mu(x; phi) that lives on the host side (rating-gp's power law,
 * src/rating_gp/models/gpytorch.py:28-40): with w_dev = two device vectors [2][n] (e.g. d mu_i / d phi_k), every
 * following dgp_fit_step also writes sum_i dNLL/dr_i w_k[i] to out[DGP_OUT_DR_W0 + k], next to out[DGP_OUT_SUM_DR]
 * and out[DGP_OUT_SUM_DNOISE] -- the host gets its mean / noise gradients from the one result row instead of reducing
 * dr and dnoise itself.  The vectors are read when the step runs; NULL clears.  Batched plans: [batch][2][n]. */
int dgp_plan_set_dr_weights(dgp_plan* plan, const void* w_dev);
/* Concurrency inside one fit step.  0: everything in order on the caller's stream.  1: the bulk trailing
 * updates of the factorisation run on a second (lowest-priority) stream beside the panel chain, and -- single-site
 * plans -- the chain itself is split: the next diagonal block's own rows and tile on the caller's stream, the rest of
 * the chain on a third (highest-priority) stream.  2 (default): additionally the inverse's level recursion is issued
 * on another stream behind checkpoints of the factorisation, filling the CUs its sequential tail leaves idle -- best
 * for ONE plan per GPU; callers that keep several plans in flight on one GPU should select 1 (the other plans already
 * fill the idle CUs).  The internal streams belong to the CALLER's stream: every plan driven from one stream shares
 * one set (a process has few hardware queues), plans driven from different streams get a set each; they live as long
 * as the process.  Results are ordered on the caller's stream whatever the level. */
int dgp_plan_set_lookahead(dgp_plan* plan, int level);
/* Plan-level options (any time; they take effect at the next call).  The first three select the TILE SHAPE of the three
 * O(n^3) stages, which the library otherwise derives from the problem size -- the parity tests use them to run the
 * kernels of the benchmark shapes (128 x 128 tiles of the direct-to-LDS core) at sizes the dense CPU oracle reaches;
 * results must not depend on them beyond rounding.  Nothing in the reference corresponds (gpytorch picks its own
 * LAPACK / CG paths, engines/gpytorch.py:350-353).
 *   DGP_OPT_LAUUM64_MAX_TILES  K^^-1 = L^-T L^-1 runs in 64 x 64 tiles while (128-tiles x batch) <= value (default 1000;
 *                              0: always the 128 x 128 kernel)
 *   DGP_OPT_SYRK_SLOTS         workgroup slots of one round of the bulk trailing update: whole rounds run as 128 x 128
 *                              tiles, the remainder is cut into 64-wide pieces (default 512)
 *   DGP_OPT_TRTRI_SMALL        a level of the inverse with fewer than `value` 128-tiles (x batch) runs in 64 x 64 tiles
 *                              (default 1024; 0: always 128 x 128)
 *   DGP_OPT_REFINE             float32 plans only (default 1): after the triangular solves, ONE step of iterative
 *                              refinement -- residual r - K^ alpha in float64 with K^ re-evaluated on the fly, correction
 *                              through the float32 factor -- so that alpha, the quadratic form and everything computed
 *                              from alpha (gradients, dnoise, predictive mean) carry ~cond(K^) eps32 SQUARED instead of
 *                              cond(K^) eps32; the reference trains in float32 (engines/gpytorch.py:221-222). */
#define DGP_OPT_LAUUM64_MAX_TILES 0
#define DGP_OPT_SYRK_SLOTS 1
#define DGP_OPT_TRTRI_SMALL 2
#define DGP_OPT_REFINE 3
/* tile ORDER of the bulk update / of K^^-1 = L^-T L^-1 (measurement knobs, default 0 = rows of the triangle): S > 0 runs
 * S x S supertiles per XCD -- S times fewer distinct operand panels in flight per L2.  Same tiles, same sums: results are
 * bitwise those of the default order. */
#define DGP_OPT_SYRK_ORDER 4
#define DGP_OPT_LAUUM_ORDER 5
/* single-site plans (default 1): while the diagonal-block kernel of the panel chain runs, the waves of the concurrent bulk
 * update that share ITS compute unit sleep (a word in the plan's status block names the CU; bounded at ~0.2 ms) -- the
 * block kernel is one workgroup of dependent latencies on the critical path and runs 3-5 times slower beside them.  A
 * scheduling hint: results are bitwise the same with 0. */
#define DGP_OPT_CHAIN_YIELD 6
/* default 0 (a measured alternative, not faster: csrc/dgp_fused.hip): 1 = when K^^-1 = L^-T L^-1 runs in 128 x 128 tiles (see
 * DGP_OPT_LAUUM64_MAX_TILES) and the model is one of the two fused covariance functions, every tile contracts itself with
 * dK/dtheta right after it is stored (one launch instead of lauum + gram_grad; K^^-1 is never re-read from HBM).  Same sums in
 * a different order: the gradients agree to rounding (1e-11 relative in fp64), everything else is bitwise the same.  The
 * backward pass of engines/gpytorch.py:384. */
#define DGP_OPT_FUSED_GRAD 7
/* batched plans of 4 or more sites (default 0: measured neutral; 1 =): the factorisation's panel GROUPS (4 panels) solve their rows below the group's
 * diagonal block with ONE GEMM against that block's inverse -- L[i, group] = A[i, group] T_D^T -- instead of panel-by-panel trsm
 * and column-update launches over the full height; 0 = the panel-by-panel chain (the form until round 4).  A different
 * association of the same sums: results agree to rounding (fp64 ~1e-13).  Replaces part of what gpytorch's Cholesky does
 * at engines/gpytorch.py:350-353. */
#define DGP_OPT_GROUP_GEMM 8
/* batched plans of 4 or more sites, the SCHEDULE of the factorisation: 0 = group-ahead (right-looking: every trailing tile is
 * read, updated and stored once per group of 4 panels, K = 512), 1 = left-looking at group level (each group of columns is
 * updated once, just before it is factored, with everything to its left: long K, each tile stored once; csrc/dgp_schedule.h).
 * Every tile receives its k-blocks in ascending gap-free order either way: with DGP_OPT_POTRF_SOLVE = 0 the float64 results
 * are bitwise the same.  DGP_OPT_POTRF_SWEEP: panels per super-group (right-looking sweeps between super-groups, left-looking
 * inside; 0 = none).  DGP_OPT_POTRF_SOLVE = 1: the rows below a group's diagonal block by one GEMM (as DGP_OPT_GROUP_GEMM;
 * agrees to rounding).  DGP_OPT_POTRF_OVERLAP = 1 (with SOLVE): that part of the group's update runs beside the block's panels.
 * The Cholesky inside the reference's mll(output, y), engines/gpytorch.py:350-353. */
#define DGP_OPT_POTRF_SCHEDULE 9
#define DGP_OPT_POTRF_SWEEP 10
#define DGP_OPT_POTRF_SOLVE 11
#define DGP_OPT_POTRF_OVERLAP 12
#define DGP_OPT_POTRF_SLOTS 13 /* workgroup slots of a round of the strip updates, whole batch (768); tests force small rounds */
#define DGP_OPT_POTRF_TAIL 14       /* the last this-many block columns are a super-group of their own (0 = none) */
#define DGP_OPT_POTRF_TAIL_SWEEP 15 /* panels per super-group inside that tail (0 = the whole tail) */
int dgp_plan_set_option(dgp_plan* plan, int key, int64_t value);
int dgp_plan_get_option(const dgp_plan* plan, int key, int64_t* value_out);
int dgp_plan_buffer(const dgp_plan* plan, int which, void** dev_ptr, int64_t* ld);
/* batched plans: site b's copy of every dgp_plan_buffer buffer starts this many bytes after site b - 1's (tests) */
size_t dgp_plan_site_stride_bytes(const dgp_plan* plan);

/* Training inputs X (n x d row-major, device) -> internal SoA copy.  Replaces the train_x tensor
 * handed to ExactGP at engines/gpytorch.py:221-235. */
int dgp_set_inputs(dgp_plan* plan, const void* X_dev, void* stream);

/* One fit step = one evaluation of the data term of the objective and ALL its gradients, the work of
 * `output = model(train_x); nll = -mll(output, train_y); objective.backward()` at
 * engines/gpytorch.py:350-384 (minus the O(P) prior / constraint algebra, which stays in torch):
 *   theta_host  ntheta constrained kernel hyperparameters (host, double)
 *   r_dev       residual y - mean(X) (n)          noise_dev  diagonal of Sigma (n)
 *   out_dev     DGP_OUT_LEN elements, layout DGP_OUT_*
 *   dr_dev      d NLL / d r = alpha = K^^-1 r (n)
 *   dnoise_dev  d NLL / d noise_i = 1/2 (K^^-1_ii - alpha_i^2) (n)
 * Leaves L, L^-1, K^^-1, alpha in the plan buffers. */
int dgp_fit_step(dgp_plan* plan, const double* theta_host, const void* r_dev, const void* noise_dev,
                 void* out_dev, void* dr_dev, void* dnoise_dev, void* stream);

/* Value only (no K^^-1, no gradient): Gram, Cholesky, L^-1, alpha.  out_dev as above with dtheta = 0.
 * This is the eval-mode cache build of ExactGP (engines/gpytorch.py:618-622). */
int dgp_factorize(dgp_plan* plan, const double* theta_host, const void* r_dev, const void* noise_dev,
                  void* out_dev, void* stream);

/* CENSORED OBSERVATIONS (non-detects) by the Laplace approximation of a GP with a Tobit likelihood.  Row i is observed
 * (side 0: y_i, Gaussian with variance v_i = noise_i) or censored at the limit l_i = y_i (side -1: the truth is below it,
 * +1: above): log p_i = log Phi(z_i), z_i = s_i (f_i - l_i) / sigma_i.  With h = phi(z) / Phi(z):
 *   g_i = s_i h / sigma_i,   W_i = h (z + h) / v_i,   d3_i = -(s_i / sigma_i^3) h [1 - (z + h)(z + 2 h)]
 * (observed rows: W = 1 / v, d3 = 0).  At the mode the posterior of the latent f is the exact GP posterior for the
 * pseudo-targets y~_i = f_i + g_i / W_i with the diagonal pseudo-noise n~_i = 1 / W_i, so
 *   a Newton step   = one dgp_factorize pass with r~ = y~ - m and n~:  a = (K + diag n~)^-1 r~,  f_new = y~ - n~ o a
 *                     (no product with K).  The first step from the caller's f is taken whole (the a with f - m = K a is
 *                     not known for it); later steps are halved, t in {1, 1/2, .. 1/64}, until the objective
 *                     Psi(t) = sum_i log p_i(f(t)) - 1/2 a(t)^T (f(t) - m) does not fall (f and a are linear in t: O(n)).
 *   at the mode     NLL_L = NLL_engine + sum_{censored} [-log Phi(z_i) - 1/2 n~_i alpha_i^2 + 1/2 log W_i - 1/2 log 2 pi],
 *                   Sigma_ii = n~_i - n~_i^2 (K^^-1)_ii,  t_i = -1/2 Sigma_ii d3_i,  u = K^^-1 (n~ o t) = T^T (T (n~ o t)),
 *                   dNLL_L/dtheta_p = dtheta_engine[p] + u^T dK/dtheta_p alpha  (one pair sweep over the lower triangle for
 *                   all p, dK/dtheta never stored),   dNLL_L/dr = alpha - u.
 * Guards: the functions of z go through erfcx for z < 0 and erfc / log1p for z >= 0; a censored row with W_i v_i < 1e-12 (an
 * uninformative limit, about z > 7.5) is CAPPED: n~_i = 1e12 v_i, d3_i = 0.
 *   y_dev / mean_dev / noise_dev   n doubles: observation or limit, prior mean m, noise variance v (model space)
 *   side_dev    n int32: -1 / 0 / +1
 *   f_dev       n doubles, in: the start of the mode search (m for a cold start), out: the mode
 *   out_dev     DGP_OUT_* layout: NLL = NLL_L, DTHETA the total gradient, SUM_DR / DR_W0.. from dr = alpha - u; QUAD, LOGDET
 *               and INFO are those of the pseudo-data system (a non-positive pivot is reported through INFO as by dgp_fit_step)
 *   dr_dev      alpha - u (n doubles, or null)
 *   stat_host   4 doubles: Newton iterations (factorise passes of the search), final max |f_new - f|, halvings, capped rows
 * Passes: terms (elementwise) -> status read; per Newton iteration: dgp_factorize's launches, proposal + line search +
 * update (elementwise, two-stage fixed-order sums), terms; then dgp_fit_step's launches at the mode, two triangular products
 * for u, the pair sweep, one result pass.  The host reads one small status block per Newton iteration: ONE STREAM
 * SYNCHRONISATION PER ITERATION, and one more before returning.  No floating-point atomics: bitwise repeatable.
 * With no censored row both entries launch exactly what dgp_fit_step / dgp_factorize launch on (y - m, v) -- the same bits
 * in out_dev, dr_dev and the plan -- report 0 iterations and set f = m + K alpha.
 * float64 single-site plans only.  Before any launch: DGP_E_ARG (null plan / argument, f_dev included; an fp32 or batched
 * plan; maxit < 1; tol < 0; misaligned work area), DGP_E_WORKSPACE (work area missing or smaller than
 * dgp_laplace_workspace_bytes), DGP_E_STATE (no inputs).  After the first pass: DGP_E_ARG for a side value outside -1 / 0 / +1.
 * DGP_E_NOCONV when max |f_new - f| > tol after maxit iterations: the step at the last iterate has still run, the results
 * and stat_host are filled and the plan holds that system.  dgp_laplace_fit_step leaves L, L^-1, K^^-1 and alpha of the
 * pseudo-data system in the plan; dgp_laplace_factorize (value only, dtheta = 0: the prediction-time cache build) L, L^-1
 * and alpha -- every product that reads the held factorisation then sees the Laplace posterior. */
size_t dgp_laplace_workspace_bytes(const dgp_plan* plan);
int dgp_laplace_fit_step(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev, const void* noise_dev,
                         const int32_t* side_dev, void* f_dev, int maxit, double tol, void* work_dev, size_t work_bytes,
                         void* out_dev, void* dr_dev, double* stat_host, void* stream);
int dgp_laplace_factorize(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev, const void* noise_dev,
                          const int32_t* side_dev, void* f_dev, int maxit, double tol, void* work_dev, size_t work_bytes,
                          void* out_dev, double* stat_host, void* stream);
/* The same for EVERY plan of float64, batched and ragged ones included (gridDim.z = sites).  Arrays are batch-major: theta_host
 * [B][ntheta], y / mean / noise / f / dr [B][n], side int32 [B][n], out [B][DGP_OUT_LEN], stat_host [B][4] = per site (its Newton
 * iterations, its final max |f_new - f|, its halvings, its capped rows).  Rows >= sizes[b] of a ragged site are ignored in every
 * input (side values there may be anything) and its f tail is left untouched.
 * Newton's iterations run in LOCKSTEP: each one factorises all B sites.  A site is done when it has no censored row (before the
 * first iteration), when its proposal satisfied max |f_new - f| <= tol, or when its factorisation failed; a done site is FROZEN on
 * the device -- its f, its a, its pseudo-data (r~, n~) and its status are left untouched -- so it rides through the remaining
 * factorisations on unchanged pseudo-data and its mode, iteration count and halvings are its own, whatever its batch-mates need.
 * The host reads all B status blocks in one copy per iteration and stops when every site is done or at maxit.  Then ONE
 * dgp_fit_step pass at the modes, u = T^T (T w) per site in the work area (the plan's z / alpha untouched), the pair sweep
 * (hyperparameters by value up to 8 sites, through the plan's scratch above) and the result pass.  No floating-point atomics.
 * Return: 0; DGP_E_ARG for a side value outside -1 / 0 / +1 (the text names the first such site); DGP_E_NOCONV when a censored
 * site is not done after maxit (all results filled, stat_host says which sites, the text names the first); DGP_E_WORKSPACE /
 * DGP_E_STATE / DGP_E_ARG before any launch as above (fp32 plans are refused).  A site whose matrix is not positive definite
 * reports that in its own out[DGP_OUT_INFO]: the return code stays 0 and the other sites are unaffected.
 * On a plan of one site these entries return bitwise what dgp_laplace_* return; with no censored row in any site they launch
 * exactly what dgp_fit_step / dgp_factorize launch on (y - m, v) and set every f = m + r - v o alpha. */
size_t dgp_laplace_batched_workspace_bytes(const dgp_plan* plan); /* 0 for null / fp32 */
int dgp_laplace_batched_fit_step(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev,
                                 const void* noise_dev, const int32_t* side_dev, void* f_dev, int maxit, double tol, void* work_dev,
                                 size_t work_bytes, void* out_dev, void* dr_dev, double* stat_host, void* stream);
int dgp_laplace_batched_factorize(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev,
                                  const void* noise_dev, const int32_t* side_dev, void* f_dev, int maxit, double tol, void* work_dev,
                                  size_t work_bytes, void* out_dev, double* stat_host, void* stream);
/* INTERVAL-CENSORED OBSERVATIONS: a fourth row kind, side 2 -- the truth of row i lies in [y_i, upper_i] (model space,
 * upper_i > y_i; EGRET's ConcLow / ConcHigh).  With za = (y_i - f_i) / sigma_i, zb = (upper_i - f_i) / sigma_i, Delta = zb - za,
 * P = Phi(zb) - Phi(za), ra = phi(za) / P, rb = phi(zb) / P:
 *   log p_i = log P,   g_i = (ra - rb) / sigma_i,   W_i v_i = zb rb - za ra + (ra - rb)^2   in (0, 1],
 *   d3_i = { ra (za^2 - 1) - rb (zb^2 - 1) - (ra - rb)(za ra - zb rb) + 2 (ra - rb) W_i v_i } / sigma_i^3
 * i.e. sigma g, 1 - W v and sigma^3 d3 are the mean, the variance and the third central moment of a standard normal truncated
 * to [za, zb].  log P is concave in f, so Newton's search, the pseudo-data identity, the NLL correction (with log P in place of
 * log Phi) and the implicit gradient sweep are those of the one-sided rows above, unchanged.
 * Regimes (none of the formulas can be evaluated as written: P underflows and cancels in a tail, and for Delta << 1 W v is a sum
 * of O(1 / Delta^2) terms).  A bracket whose centre c = (za + zb) / 2 lies right of 0 is reflected; then, with h = Delta / 2,
 *   narrow    h <= 1 and |c| h <= 2: P = h phi(c) I with I = int_-1^1 exp(-c h t - h^2 t^2 / 2) dt and the moments of that tilted
 *             density by a fixed 12-point Gauss-Legendre rule, central moments about the computed mean (no cancellation as
 *             Delta -> 0: W v -> 1 - Delta^2 / 12)
 *   tail      zb <= 0: P = phi(zb) [M(zb) - rho M(za)], M = Phi / phi through erfcx, rho = exp(Delta c) <= e^-2 through expm1
 *   straddle  za < 0 < zb: P = [erf(zb / sqrt 2) + erf(-za / sqrt 2)] / 2, a sum of positive terms
 * Guards: W v is clamped to <= 1; the capping rule is that of the one-sided rows (W v < 1e-12: n~ = 1e12 v, d3 = 0).
 * Measured against a 600-digit fixture on za in [-40, 38], Delta in [1e-6, 30], relative to max(1, |value|): see DESIGN.md.
 * The two entries serve EVERY float64 plan (single-site, batched, ragged); their arguments, workspace query
 * (dgp_laplace_batched_workspace_bytes), stat_host layout, passes and error rules are dgp_laplace_batched_*'s, plus
 *   upper_dev   [B][n] doubles, read only on the rows of side 2 (anything elsewhere, NaN included); may be null when no row has
 *               side 2.
 * DGP_E_ARG in addition: a row of side 2 with a null upper_dev, or a BAD BRACKET (upper NaN, infinite or not above y) -- both
 * reported after the first pass, as bad side values are, the text naming the first such site.  With no row of side 2 they launch
 * exactly what dgp_laplace_batched_* launch and give the same bits in every output and plan buffer.  The entries above are
 * unchanged: for them 2 stays a bad side value. */
int dgp_laplace_interval_fit_step(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev,
                                  const void* noise_dev, const int32_t* side_dev, const void* upper_dev, void* f_dev, int maxit,
                                  double tol, void* work_dev, size_t work_bytes, void* out_dev, void* dr_dev, double* stat_host,
                                  void* stream);
int dgp_laplace_interval_factorize(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev,
                                   const void* noise_dev, const int32_t* side_dev, const void* upper_dev, void* f_dev, int maxit,
                                   double tol, void* work_dev, size_t work_bytes, void* out_dev, double* stat_host, void* stream);
/* CENSORED OBSERVATIONS BY EXPECTATION PROPAGATION.  The Laplace approximation above centres the Gaussian on the MODE of the
 * posterior; with most rows censored far below their limits that posterior is one-sided and its mean lies well away from the
 * mode.  EP keeps a Gaussian SITE (pseudo-target y~_i, pseudo-noise n~_i; tau~ = 1 / n~, nu~ = y~ / n~) on every censored row
 * (side -1 / +1 / 2 as above) and matches moments; rows of side 0 keep their exact site (y, v).  An EP state is a GP regression on
 * (y~, n~), so the plan holds the result exactly as it holds a Laplace mode, and every product reads it unchanged.
 *   a sweep         = one dgp_factorize pass with r~ = y~ - m and n~: alpha, T = L^-1, k_i = [(K + diag n~)^-1]_ii = sum_{j >= i} T_ji^2;
 *                     the cavity  v_c = 1 / k - n~,  mu_c = y~ - alpha / k  (the leave-one-out predictive of that regression);
 *                     log Z^, g = d log Z^ / d mu_c, W = -d2 log Z^ / d mu_c^2 by the pointwise functions above at the standard
 *                     deviation s = sqrt(v + v_c) (one-sided: z = side (mu_c - l) / s; bracket: za = (y - mu_c) / s, zb = (upper -
 *                     mu_c) / s; g and W scale by 1 / s and 1 / s^2);  tau' = W / (1 - W v_c),  y' = mu_c + g / W;  damped in the
 *                     natural parameters: tau~ <- (1 - damping) tau~ + damping tau', nu~ likewise.  All censored rows at once.
 *   guards          CAP: tau' v < 1e-12 -> tau' = 1e-12 / v, y' kept, the row is counted.  HOLD: v_c <= 0 or 1 - W v_c <= 0 (or not
 *                   a number) -> the row keeps its site for this sweep and is counted.
 *   convergence     max_i |mu_i - mu_i^prev| <= tol over all rows, mu = y~ - n~ o alpha the posterior mean at the samples (in the
 *                   first sweep, which has no previous mean: max v |nu' - nu~| over the censored rows), AND max v |tau' - tau~| <= tol.
 *                   (Sigma_ii = n~ - n~^2 k is not tested: pure cancellation for nearly uninformative rows.)
 *   final state     the proposal of the sweep that converged -- or of the last sweep -- is NOT applied: the sites returned are the
 *                   ones that were factorised, so the plan's factorisation, the cavities and log Z^ belong to one state.
 *   value           NLL_EP = NLL_engine(r~, n~) - sum_censored [log Z^_i + 1/2 log 2 pi - 1/2 log k_i + alpha_i^2 / (2 k_i)]
 *   gradient        at the fixed point dNLL_EP / dtheta is the engine's explicit gradient at the sites and dNLL_EP / dr = alpha:
 *                   dgp_ep_fit_step ends with one dgp_fit_step pass at the final sites and returns its DTHETA, SUM_DR, DR_W0.. and
 *                   dr as they are.  No implicit term, no pair sweep.
 *   y_dev / mean_dev / noise_dev / side_dev / upper_dev   as for dgp_laplace_interval_* (upper_dev may be null without a row of side 2)
 *   ytilde_dev, ntilde_dev   n doubles each, in: the sites of a warm start (read on the censored rows; a row without a finite y~ and
 *               a positive finite n~ starts cold), out: the final sites of every row
 *   cold_start  != 0: ignore their contents and start every censored row from the Laplace terms at f = m (n~ = 1 / W(m),
 *               y~ = m + g / W, with the Laplace cap)
 *   maxit, tol, damping   sweeps at most (>= 1), the tolerance of both tests (>= 0), damping in (0, 1]
 *   out_dev     DGP_OUT_* layout: NLL = NLL_EP; QUAD, LOGDET, INFO and (fit step) DTHETA, SUM_DR, DR_W0.., SUM_DNOISE those of the
 *               pseudo-data system; dgp_ep_factorize: the row of the last sweep's factorisation, dtheta = 0
 *   dr_dev      alpha (n doubles, or null)
 *   stat_host   6 doubles: sweeps, final max |dmu|, final max v |dtau|, capped rows, rows held back, censored rows (the counts are
 *               those of the last sweep)
 *   cav_mean_dev, cav_var_dev, logz_dev   n doubles each or null: mu_c, v_c and log Z^ of the final state (rows of side 0: their
 *               leave-one-out predictive and log N(y | mu_c, v + v_c))
 * Passes: the Laplace terms at m (row checks, cold start) -> status read; per sweep: dgp_factorize's launches, k (n^2 / 2 doubles read
 * once, coalesced along the columns of the row-major T), sites, finish -> status read: ONE STREAM SYNCHRONISATION PER SWEEP; then
 * (fit step) dgp_fit_step's launches, the result pass and one more synchronisation.  No floating-point atomics: bitwise repeatable.
 * With no censored row both entries launch exactly what dgp_fit_step / dgp_factorize launch on (y - m, v) -- the same bits in
 * out_dev, dr_dev and the plan -- report 0 sweeps and return the sites (y, v).
 * float64 single-site plans only.  Before any launch: DGP_E_ARG (null plan / argument; an fp32 or batched plan -- the text says
 * so; maxit < 1; tol < 0; damping outside (0, 1]; misaligned work area), DGP_E_WORKSPACE, DGP_E_STATE (no inputs).  After the first
 * pass: DGP_E_ARG for a bad side value or a bad bracket, as for dgp_laplace_interval_*.  DGP_E_NOCONV when the tests still fail
 * after maxit sweeps: everything is filled, the sites are those of the last factorisation.  A matrix that is not positive definite
 * ends the sweeps and is reported through out[DGP_OUT_INFO], return code 0. */
size_t dgp_ep_workspace_bytes(const dgp_plan* plan); /* 0 for null / fp32 / batched */
int dgp_ep_fit_step(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev, const void* noise_dev,
                    const int32_t* side_dev, const void* upper_dev, void* ytilde_dev, void* ntilde_dev, int cold_start, int maxit,
                    double tol, double damping, void* work_dev, size_t work_bytes, void* out_dev, void* dr_dev, double* stat_host,
                    void* cav_mean_dev, void* cav_var_dev, void* logz_dev, void* stream);
int dgp_ep_factorize(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev, const void* noise_dev,
                     const int32_t* side_dev, const void* upper_dev, void* ytilde_dev, void* ntilde_dev, int cold_start, int maxit,
                     double tol, double damping, void* work_dev, size_t work_bytes, void* out_dev, double* stat_host,
                     void* cav_mean_dev, void* cav_var_dev, void* logz_dev, void* stream);
/* k_dev[i] = [(K^)^-1]_ii = sum_{j >= i} T_ji^2, i < n, from the factorisation the plan holds (any of the entries above): the
 * diagonal pass of an EP sweep alone, for tests and timing.  work_dev: dgp_ep_workspace_bytes.  DGP_E_STATE without a factorisation. */
int dgp_ep_diag(dgp_plan* plan, void* k_dev, void* work_dev, size_t work_bytes, void* stream);

/* ---- The exact leave-one-out predictive likelihood as a training objective.
 * With S = (K^)^-1, alpha = S r and k_i = S_ii the leave-one-out predictive of row i is N(y_i - alpha_i / k_i, 1 / k_i) and
 *     L_LOO = sum_i [ 1/2 log 2 pi - 1/2 log k_i + alpha_i^2 / (2 k_i) ]        (minus the elpd of dgp_cross_validate's folds of one)
 * dgp_loo_fit_step has the arguments, shapes and batching of dgp_fit_step plus a work area (dgp_loo_workspace_bytes: three N x N
 * matrices per site and change).  It runs dgp_fit_step's launches unchanged into a result row of its own, then
 *     w = (1 + alpha^2 / k) / (2 k),  c = alpha / k,  M = S diag(w) S (one symmetric N^3 product on the MFMA tile cores, lower tiles,
 *     k ascending; 64 x 64 tiles while a launch has too few: DGP_OPT_LAUUM64_MAX_TILES),  b = S c
 *     dL/dtheta_p = 1/2 tr((2 M - b alpha^T - alpha b^T) dK/dtheta_p),  dL/dr = b,  dL/dnoise_i = M_ii - b_i alpha_i
 * out_dev: DGP_OUT_* layout with NLL = L_LOO and DTHETA, SUM_DR, DR_W0.., SUM_DNOISE its gradients; QUAD, LOGDET and INFO are those of
 * the factorisation.  A site one of whose k_i is not a positive finite number reports the 1-based index of the first such row in its
 * INFO (when the factorisation's own status is 0) and NaN as its value: the return code stays 0 and the other sites are unaffected.
 * The plan holds afterwards exactly what dgp_fit_step with the same arguments leaves (factor, inverse, z, alpha): every inference
 * entry point works on it unchanged.  No floating-point atomics: bitwise repeatable, a site's result does not depend on its batch.
 * dgp_loo_value: out2_dev [batch][2] doubles = (L_LOO, info) from the factorisation the plan holds, when the last step left S in it
 * (dgp_fit_step / dgp_loo_fit_step; DGP_E_STATE otherwise); work area: dgp_loo_value_workspace_bytes.
 * float64 plans, single-site or batched.  Before any launch: DGP_E_ARG (null plan / argument; a float32 plan -- the text says so;
 * misaligned work area), DGP_E_WORKSPACE (work area missing or too small), DGP_E_STATE (no inputs / no inverse). */
size_t dgp_loo_workspace_bytes(const dgp_plan* plan);
size_t dgp_loo_value_workspace_bytes(const dgp_plan* plan);
int dgp_loo_fit_step(dgp_plan* plan, const double* theta_host, const void* r_dev, const void* noise_dev, void* work_dev,
                     size_t work_bytes, void* out_dev, void* dr_dev, void* dnoise_dev, void* stream);
int dgp_loo_value(dgp_plan* plan, void* work_dev, size_t work_bytes, void* out2_dev, void* stream);
/* out [4][count] = log P, sigma g, W v, sigma^3 d3 of the brackets [za, za + Delta]: the pointwise functions of the two entries
 * above, for tests.  za_dev, delta_dev: count doubles on the device (Delta > 0). */
int dgp_debug_interval_terms(const double* za_dev, const double* delta_dev, int64_t count, double* out_dev, void* stream);
/* out [4][count] = log Phi(z), h = phi(z) / Phi(z), h (z + h), h [1 - (z + h)(z + 2 h)]: the pointwise functions of the
 * entries above, for tests.  z_dev: count doubles on the device. */
int dgp_debug_censored_terms(const double* z_dev, int64_t count, double* out_dev, void* stream);
/* dtheta_dev[p] = sum_ij u_i dK_ij/dtheta_p alpha_j, p < ntheta: the pair sweep of dgp_laplace_fit_step alone, for tests (u_dev,
 * alpha_dev: n doubles; work area as for dgp_laplace_fit_step).  Reads the plan's inputs only. */
int dgp_debug_bilinear(dgp_plan* plan, const double* theta_host, const void* u_dev, const void* alpha_dev, void* work_dev,
                       size_t work_bytes, double* dtheta_dev, void* stream);

/* The same sweep for every site of a batched float64 plan: u_dev / alpha_dev [B][n], dtheta_dev [B][ntheta], theta_host
 * [B][ntheta]; work area as for dgp_laplace_batched_fit_step. */
int dgp_debug_bilinear_batched(dgp_plan* plan, const double* theta_host, const void* u_dev, const void* alpha_dev, void* work_dev,
                               size_t work_bytes, double* dtheta_dev, void* stream);

/* Workspace for dgp_predict on m test points. */
size_t dgp_predict_workspace_bytes(const dgp_plan* plan, int64_t m);
/* Posterior at Xs (m x d row-major, device) from the factorisation currently held by the plan:
 *   mean_dev[j] = K(x*_j, X) alpha            (add the mean function on the host)
 *   var_dev[j]  = k(x*_j, x*_j) - || L^-1 K(X, x*_j) ||^2   (latent f; add likelihood noise on the host)
 * Replaces `self.likelihood(self.model(x))` .mean/.variance at engines/gpytorch.py:621-624. */
int dgp_predict(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, void* work_dev,
                size_t work_bytes, void* mean_dev, void* var_dev, void* stream);

/* Full latent posterior covariance for sample() (engines/gpytorch.py:575-580):
 *   cov_dev (M x M row-major, M = dgp_padded_n(m), lower triangle valid, identity pad)
 *     = K(Xs, Xs) - V^T V,  V = L^-1 K(X, Xs);   mean_dev[j] = K(x*_j, X) alpha  (m entries).
 * work_dev as for dgp_predict (dgp_predict_workspace_bytes). */
int dgp_posterior_cov(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, void* work_dev,
                      size_t work_bytes, void* mean_dev, void* cov_dev, void* stream);

/* Draws from N(mean, L L^T) -- what `f_preds.sample(torch.Size([n]))` does at engines/gpytorch.py:575-580:
 *     out_dev[q][j] = mean_dev[j] + sum_{k <= j} L[j][k] Z[k][q]        (ndraw x m row-major, q = draw)
 * L_dev   M x M row-major, M = dgp_padded_n(m): a lower-triangular factor with zeros above the diagonal inside its
 *         diagonal 128-blocks and the identity in the pad -- e.g. DGP_BUF_A of an order-m plan after dgp_stage_potrf
 *         of the matrix dgp_posterior_cov wrote there (blocks above the block diagonal are never read);
 * Z_dev   M x Q row-major standard normals, Q = dgp_padded_n(ndraw) (the pad only feeds entries that are not stored);
 * mean_dev m entries or NULL.  One MFMA launch (the same tile core as the factorisation); needs no plan. */
int dgp_sample_draws(int dtype, const void* L_dev, int64_t m, const void* Z_dev, int64_t ndraw, const void* mean_dev,
                     void* out_dev, void* stream);

/* Exact mean and covariance of PERIOD SUMS of a transformed posterior -- annual / monthly loads with their uncertainty,
 * which the reference estimates by Monte Carlo: sample() (engines/gpytorch.py:551-593) -> concentration_to_flux
 * (src/loadest_gp/utils.py:14-56) -> flux.resample(time="YE").sum() (utils.py:59-103).  With f ~ N(mu, C) per site,
 * s2 = s^2, the mean mu_dev ALREADY mapped (mu_i <- s mu_i + t) and c_i the data-space value:
 *   mode 1 (log,    c_i = exp(s f_i + t)):  a_i = w_i exp(mu_i + s2 C_ii / 2)
 *            mean[g] = sum_{i in g} a_i          cov[g][h] = sum_{i in g, j in h} a_i a_j expm1(s2 C_ij)
 *   mode 0 (linear, c_i = s f_i + t):       mean[g] = sum_{i in g} w_i mu_i   cov[g][h] = s2 sum_{i in g, j in h} w_i w_j C_ij
 * cov_dev    `dtype` elements, per site M x M (M = dgp_padded_n(m)) at stride M M: exactly what dgp_posterior_cov writes; only
 *            the lower triangle (j <= i) is read; accumulation is in double;
 * mu_dev     batch x m, `dtype`;  scale2_dev: batch doubles (s^2);  w_dev: batch x m doubles;
 * group_dev  batch x m int32 group ids in 0 .. ngroups-1, NON-DECREASING along the points except for -1 (excluded) anywhere
 *            (a violation gives wrong numbers, never an access out of bounds);
 * extra_var_dev  NULL or batch x m `dtype`, added to C_ii (predictive noise);
 * mean_out_dev   batch x ngroups doubles;  cov_out_dev  batch x ngroups x ngroups doubles (exactly symmetric).
 * work_dev: dgp_period_moments_workspace_bytes(m, ngroups, batch) bytes (m P + 2 m doubles per site; 0 for bad sizes).
 * Four launches (gridDim.z = batch); no floating-point atomics: bitwise repeatable, and a site's result does not depend on
 * the batch it is in.  Needs no plan. */
size_t dgp_period_moments_workspace_bytes(int64_t m, int ngroups, int batch);
int dgp_period_moments(int dtype, int mode, const void* cov_dev, int64_t m, int batch, const void* mu_dev,
                       const double* scale2_dev, const double* w_dev, const int32_t* group_dev, int ngroups,
                       const void* extra_var_dev, void* work_dev, size_t work_bytes, double* mean_out_dev,
                       double* cov_out_dev, void* stream);

/* The same period moments straight from the factorisation the plan holds: C = K(Xs, Xs) - V^T V, V = L^-1 K(X, Xs), is
 * folded into the ngroups x ngroups moments tile by tile and never stored -- for records whose m x m covariance does not fit
 * the device (30 years of daily points: m ~ 330 000, 870 GB in fp64), and for flow-normalized loads (EGRET's FN flux, which
 * the reference's WRTDS lineage points to: README.md, src/discontinuum/utils.py:36-67), whose point sets grow with the
 * square of the record length.
 *   Xs_dev     m x d row-major (batch x m x d for batched plans), as for dgp_posterior_cov; mode, mu_dev (mapped), scale2_dev,
 *              w_dev, group_dev, ngroups, extra_var_dev, mean_out_dev, cov_out_dev: as for dgp_period_moments.
 * work_dev: dgp_posterior_period_moments_workspace_bytes(plan, m, ngroups) bytes -- per site the prediction's work area
 * (2 N M + O(M) plan-dtype elements) and M ngroups + O(M) doubles; no buffer grows with M^2.  0 for bad sizes.
 * One MFMA pass over about m^2 / 2 (1 + 1/ngroups) entries (2 N flop each) with the covariance function evaluated per entry,
 * no floating-point atomics: bitwise repeatable, a site's result does not depend on its batch.  DGP_E_STATE without a
 * factorisation.  Every (model, d) of dgp_posterior_cov, batched plans included (gridDim.z = sites). */
size_t dgp_posterior_period_moments_workspace_bytes(const dgp_plan* plan, int64_t m, int ngroups);
int dgp_posterior_period_moments(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, int mode,
                                 const void* mu_dev, const double* scale2_dev, const double* w_dev,
                                 const int32_t* group_dev, int ngroups, const void* extra_var_dev,
                                 void* work_dev, size_t work_bytes, double* mean_out_dev, double* cov_out_dev,
                                 void* stream);

/* Exact mean and covariance of ROLLING-WINDOW MEANS of a posterior -- the 30-day geometric mean, the 4-day average, the 7-day
 * mean flow that water-quality criteria are written on -- which the reference can only estimate by Monte Carlo: sample()
 * (engines/gpytorch.py:551-593), roll every draw, average.  With f ~ N(mu, C) per site, window i the points lo[i] <= j < hi[i]
 * and W_ij = a_j / sum_{k in window i} a_k, the statistic W f is exactly Gaussian:
 *   mode 0 (linear):  mean[i] = sum_j W_ij mu_j        cov[i][k] = sum_j sum_l W_ij W_kl C_jl   (scale2_dev ignored, may be NULL)
 *   mode 1 (log, the ARITHMETIC mean of exp(s f + t); mu_dev ALREADY mapped, as for dgp_period_moments):
 *           e_j = exp(mu_j + s2 C_jj / 2),  mean[i] = sum_j W_ij e_j,  cov[i][k] = sum_j sum_l W_ij W_kl e_j e_l expm1(s2 C_jl)
 * cov_dev, mu_dev, batch and the padding: as for dgp_period_moments (per site M x M, M = dgp_padded_n(m); only the lower
 *            triangle is read, an entry above the diagonal is taken from its mirror);
 * a_dev      batch x m non-negative doubles, or NULL for 1;
 * lo_dev, hi_dev  batch x q int32, both NON-DECREASING in i, 0 <= lo <= hi <= m; the device clamps them to [0, m] (a violation
 *            gives wrong numbers, never an access out of bounds);
 * mean_out_dev  batch x q doubles;  cov_out_dev  batch x Q x Q doubles, Q = dgp_padded_n(q), in the layout dgp_posterior_cov
 *            writes -- lower triangle and diagonal 128-blocks valid, those blocks exactly symmetric, identity pad, blocks above
 *            the block diagonal not written -- so that it goes into dgp_exceedance_moments, dgp_period_moments and
 *            dgp_sample_value as an fp64 covariance.  An empty window or a zero weight sum gives mean 0 and a zero row and column.
 * work_dev: dgp_window_moments_workspace_bytes(m, q, batch) bytes, 8-byte aligned (M Q + 2 M + 2 Q doubles per site; 0 for bad
 * sizes).  Four launches (gridDim.z = batch): T = C_sym W^T, then S = W T on the lower block triangle; all arithmetic after the
 * loads is double, every sum runs in one thread in ascending order: no floating-point atomics, bitwise repeatable, and a
 * site's result does not depend on the batch it is in.  DGP_E_ARG: a null argument, a bad dtype / mode / size (1 <= m, q <=
 * 2^20, 1 <= batch <= 1024), a misaligned work area; DGP_E_WORKSPACE: a work area too small.  Needs no plan. */
size_t dgp_window_moments_workspace_bytes(int64_t m, int64_t q, int batch);
int dgp_window_moments(int dtype, int mode, const void* cov_dev, int64_t m, int batch, const void* mu_dev,
                       const double* scale2_dev, const double* a_dev, const int32_t* lo_dev, const int32_t* hi_dev,
                       int64_t q, void* work_dev, size_t work_bytes, double* mean_out_dev, double* cov_out_dev,
                       void* stream);

/* Exact mean and covariance of THRESHOLD-EXCEEDANCE COUNTS of a posterior -- days per year above a criterion, the fraction
 * of a record above a level (duration curves) -- which the reference can only estimate by Monte Carlo: sample()
 * (engines/gpytorch.py:551-593), compare every draw with the threshold, count per period.  With f ~ N(mu, C) per site, per
 * level l a threshold u_il in MODEL space, sigma_i^2 = C_ii (+ extra_var_i), z_il = (mu_i - u_il) / sigma_i,
 * rho_ij = C_ij / (sigma_i sigma_j) and N_g = sum_{i in g} w_i 1[f_i > u_il]:
 *   mean[l][g] = sum_{i in g} w_i Phi(z_il)
 *   cov[l][g][h] = sum_{i in g, j in h} w_i w_j (Phi2(z_il, z_jl; rho_ij) - Phi(z_il) Phi(z_jl)),  Phi (1 - Phi) for i = j
 * Phi2 the standard bivariate normal distribution function (Genz 2004: a Gauss-Legendre rule in asin(rho) below
 * |rho| = 0.925, the expansion about |rho| = 1 above; absolute error of the order of 1e-15 per pair).  Levels do not interact: the
 * covariance between counts at different levels is not computed.
 * cov_dev, mu_dev, w_dev, group_dev, extra_var_dev, batch and the padding: as for dgp_period_moments (only the lower triangle
 *            of cov_dev is read; group -1 = excluded; extra_var_dev enters sigma only, never rho's numerator);
 * thresh_dev batch x nlevels x m doubles, 1 <= nlevels <= 64; +-inf allowed (never / always exceeded);
 * mean_out_dev  batch x nlevels x ngroups doubles;  cov_out_dev  batch x nlevels x ngroups x ngroups doubles (exactly
 *            symmetric).  All arithmetic after the loads of C and mu is double, for float32 covariances too.
 * A point with sigma_i^2 <= 0 or an infinite threshold is decided (Phi = 0 or 1, a tie mu = u counting as not exceeded, no
 * covariance with any point); NaN inputs come out as NaN.
 * work_dev: dgp_exceedance_moments_workspace_bytes(m, ngroups, nlevels, batch) bytes -- per site M ngroups min(nlevels, 8)
 * + 2 M (nlevels + 1) doubles, nothing of order M^2; 0 for bad sizes.
 * Two launches, then two per chunk of 8 / 4 / 2 / 1 levels (gridDim.z = batch); every unordered pair is evaluated once, about
 * m^2 / 2 bivariate probabilities per level on the fp64 vector pipe; no floating-point atomics: bitwise repeatable, and a
 * site's result does not depend on the batch it is in.  Needs no plan. */
size_t dgp_exceedance_moments_workspace_bytes(int64_t m, int ngroups, int nlevels, int batch);
int dgp_exceedance_moments(int dtype, const void* cov_dev, int64_t m, int batch, const void* mu_dev,
                           const double* thresh_dev, int nlevels, const double* w_dev, const int32_t* group_dev,
                           int ngroups, const void* extra_var_dev, void* work_dev, size_t work_bytes,
                           double* mean_out_dev, double* cov_out_dev, void* stream);
/* The same exceedance moments straight from the factorisation the plan holds, for records whose m x m covariance does not fit
 * the device (a multi-year 15-minute stage record: m ~ 140 000, 157 GB in fp64).  C = K(Xs, Xs) - V^T V is produced panel_rows
 * rows at a time -- the tiles, the k order and (fp64) the bits of dgp_posterior_cov -- into one panel buffer; every unordered
 * pair (i < j) lies in exactly one panel, j's, and is evaluated there; the panels run in order on the stream.
 *   Xs_dev     m x d row-major (batch x m x d for batched plans), as for dgp_posterior_cov;
 *   mu_dev, thresh_dev, nlevels, w_dev, group_dev, ngroups, extra_var_dev, mean_out_dev, cov_out_dev: as for
 *              dgp_exceedance_moments; sigma_i^2 is the predicted variance (+ extra_var_i), never read from a panel;
 *   panel_rows a positive multiple of 128; the pass uses min(panel_rows, M).
 * work_dev: dgp_posterior_exceedance_moments_workspace_bytes(plan, m, ngroups, nlevels, panel_rows) bytes, 256-byte aligned --
 * per site the prediction's work area (2 N M + O(M) plan-dtype elements), the panel (min(panel_rows, M) M plan-dtype elements)
 * and dgp_exceedance_moments' doubles; no buffer grows with M^2.  0 for bad sizes.
 * Per chunk of 8 / 4 / 2 / 1 levels every panel is produced again (N m^2 matrix-core flop, small beside the m^2 / 2 bivariate
 * probabilities per level).  No floating-point atomics: bitwise repeatable, a site's result does not depend on its batch;
 * different panel_rows group the sums differently (equal to rounding).  DGP_E_ARG: a null argument, a bad size, panel_rows not
 * a positive multiple of 128, a misaligned work area; DGP_E_WORKSPACE: a work area too small; DGP_E_STATE: no factorisation
 * or a failed one.  Every (model, d) of dgp_posterior_cov, batched plans included (gridDim.z = sites).  The plan's
 * factorisation and every later product are left bitwise intact. */
size_t dgp_posterior_exceedance_moments_workspace_bytes(const dgp_plan* plan, int64_t m, int ngroups, int nlevels,
                                                        int panel_rows);
int dgp_posterior_exceedance_moments(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m,
                                     const void* mu_dev, const double* thresh_dev, int nlevels, const double* w_dev,
                                     const int32_t* group_dev, int ngroups, const void* extra_var_dev, int panel_rows,
                                     void* work_dev, size_t work_bytes, double* mean_out_dev, double* cov_out_dev,
                                     void* stream);
/* out[i] = Phi2(h_i, k_i; rho_i) - Phi(h_i) Phi(k_i), the pair function of dgp_exceedance_moments pointwise (rho clamped to
 * [-1, 1]; |h| or |k| above 38 gives 0): for tests.  All arrays `count` doubles on the device. */
int dgp_debug_bvn_excess(const double* h_dev, const double* k_dev, const double* rho_dev, int64_t count, double* out_dev,
                         void* stream);

/* Exact VALUE OF ONE MORE SAMPLE for the variance of period sums -- monitoring design -- which the reference could only
 * estimate by refitting on simulated data.  Setting of dgp_period_moments: f ~ N(mu, C) per site, c_i = exp(s f_i + t) (or
 * s f_i + t), L_p = sum_{i in p} w_i c_i.  A hypothetical observation y_c = f_c + eps, Var eps = tau_c^2, on day c moves the
 * covariance deterministically and the mean randomly; with conditioning rows B (nrows x m, C' = C - B^T B: the samples
 * already decided),
 *   v'_c = C_cc - sum_t B_tc^2 + tau_c^2,   b_ic = (C_ic - sum_t B_ti B_tc) / sqrt(v'_c),
 *   gain[p][c] = Var(E[L_p | y_c]) = sum_{i,j in p} A_i A_j expm1(s^2 b_ic b_jc)
 *              = sum_{k=1..nterms} (s^2)^k / k! (sum_{i in p} A_i b_ic^k)^2           (the exponential series; every term >= 0)
 * with A_i = w_i exp(s mu_i + t + s^2 C_ii / 2) for a log target; A_i = w_i and nterms = 1 is the linear target exactly.  By
 * the law of total variance Var(L_p) - gain[p][c] = E[Var(L_p | y_c)].  Since b_ic^2 <= C_ii, the tail after K terms is at
 * most (sum_{i in p} |A_i|)^2 sum_{k>K} beta^k / k!, beta = s^2 max_i C_ii: the caller picks nterms.
 * cov_dev, group_dev, batch and the padding: as for dgp_period_moments (each site M x M, M = dgp_padded_n(m); only the lower
 *            triangle is used; group -1 = excluded, ids non-decreasing otherwise -- a violation gives wrong numbers, never an
 *            access out of bounds).  The covariance is never modified and never copied: C' is formed on the fly.
 * a_dev      batch x m doubles, the A_i (computed by the host);  scale2_dev: batch doubles (s^2);
 * obs_var_dev  NULL or batch x m `dtype` (tau_c^2);
 * rows_dev   NULL or batch x nrows x m doubles, 0 <= nrows <= 64;  nterms: 1 <= K <= 64;
 * gain_out_dev  batch x ngroups x m doubles;  var_out_dev  batch x m doubles (v'_c: what the next row is divided by).
 * EVERY day is a candidate, excluded days included: a sample outside the periods of interest still informs them.  A candidate
 * whose v'_c is not > 0 gets gain 0 in every period and var 0, never NaN; NaN inputs come out as NaN.  All arithmetic after
 * the loads is double, for float32 buffers too.
 * work_dev: dgp_sample_value_workspace_bytes(m, ngroups, nrows, nterms, batch) bytes -- per site M + ngroups doubles, plus
 * ngroups Q nterms M doubles of partial sums when a group's days are cut into Q > 1 slabs (few groups: the launch fills the
 * device whatever ngroups is; Q depends on M and ngroups alone); 0 for bad sizes.
 * One pass of O(m^2 nterms) multiply-adds over about M^2 elements read (every lower-triangle entry twice); no floating-point
 * atomics: bitwise repeatable, and a site's result does not depend on the batch it is in.  Needs no plan. */
size_t dgp_sample_value_workspace_bytes(int64_t m, int ngroups, int nrows, int nterms, int batch);
int dgp_sample_value(int dtype, const void* cov_dev, int64_t m, int batch, const double* a_dev, const double* scale2_dev,
                     const int32_t* group_dev, int ngroups, const void* obs_var_dev, const double* rows_dev, int nrows,
                     int nterms, void* work_dev, size_t work_bytes, double* gain_out_dev, double* var_out_dev, void* stream);

/* Exact leave-one-out / leave-group-out cross-validation at FIXED hyperparameters from the factorisation the plan holds (after
 * dgp_factorize or dgp_fit_step; DGP_E_STATE without one) -- no fold is refitted.  The reference has no counterpart: with
 * gpytorch every fold is a new factorisation behind the `predict` call site (src/discontinuum/engines/gpytorch.py:599-626).
 * With T = L^-1, alpha = K^^-1 r and a held-out index set B of b observations (Rasmussen & Williams 5.4.2, block form):
 *     G_B = (K^^-1)_BB = T[:, B]^T T[:, B]       e_B = y_B - E[y_B | y_-B] = G_B^-1 alpha_B       C_B = Cov[y_B | y_-B] = G_B^-1
 *     lpd_B = log p(y_B | y_-B) = -1/2 alpha_B^T e_B + 1/2 log|G_B| - b/2 log 2 pi
 * (C_B is the covariance of the held-out OBSERVATIONS: their own noise is in K^).
 *   order_dev  [batch][n] int32: observation indices sorted by group, held-out ones first (the rest of a row is ignored)
 *   start_dev  [batch][ngroups + 1] int32: group g = order[start[g] .. start[g + 1]); empty groups are allowed (lpd 0)
 *   max_group  an upper bound of every group's size (1 .. n); it selects the route and sizes the work area:
 *              1: one pass over the lower triangle of T (column sums of squares, K^^-1 never formed);  <= 64: one workgroup
 *              per (group, site) with G_B, its factor and the solves in LDS;  larger: blocks of order round_up(max_group, 128)
 *              in the work area -- T[k0:, B] packed, G_B on the MFMA tile core (k-tiles last to first), the library's batched
 *              potrf / trtri -- in chunks of at most 1024 groups.  When the last step was a dgp_fit_step, G_B is a gather of the
 *              plan's K^^-1 instead; after a bare dgp_factorize that buffer is dead and is not touched.
 *   resid_dev / var_dev [batch][n] doubles: e_i and diag C_B at the observations' own positions, 0 for observations no group
 *              holds;  lpd_dev [batch][ngroups] doubles;  info_dev [batch][ngroups] int32: 0, or the 1-based failing pivot of G_B
 *              (the group's results are then NaN).
 * The indices are the caller's to validate (discontinuum_amd.backend.GPPlan.cross_validate does): the kernels clamp what they
 * read from order / start, so bad content gives wrong numbers or a set info, never an access out of bounds.  The plan's L, T,
 * alpha and (valid) K^^-1 are only read: dgp_predict, dgp_mean_vjp, dgp_stage_grad answer bitwise the same before and after.
 * All results are double whatever the plan's dtype (float32 plans: only the operands T, alpha are float32).  Batched plans:
 * gridDim.z = sites, dgp_plan_set_site_sizes respected, a site's result does not depend on its batch.  No floating-point
 * atomics: bitwise repeatable.  DGP_E_ARG for bad sizes (1 <= ngroups <= n, 1 <= max_group <= n; the query then returns 0). */
size_t dgp_cross_validate_workspace_bytes(const dgp_plan* plan, int ngroups, int64_t max_group);
int dgp_cross_validate(dgp_plan* plan, const int32_t* order_dev, const int32_t* start_dev, int ngroups, int64_t max_group,
                       void* work_dev, size_t work_bytes, double* resid_dev, double* var_dev, double* lpd_dev, int32_t* info_dev,
                       void* stream);

/* CROSS-VALIDATION OF A CENSORED FIT by Laplace CAVITY folds (the LA-LOO of Vehtari et al. 2016, in block form), from the
 * factorisation of the pseudo-data system that dgp_laplace_*factorize / *_fit_step left in the plan; no fold is refitted.
 * dgp_cross_validate on that plan would read the pseudo-data (y~, n~ = 1 / W) as if they were samples.  With f the mode, W and
 * g = d log p / d f the terms of the fit at f, G_F = (K^^-1)_FF and Sigma_FF = K_FF - V_F^T V_F (V = T K(X, X): the latent
 * posterior covariance at the fold's own rows), the latent distribution of a fold F with its own sites removed is exactly
 *     V_c = G_F^-1 diag(W_F) Sigma_FF  (its diagonal is used),      mu_c = f_F - V_c g_F
 * -- nothing of the size of n~ is subtracted, so rows whose limit is uninformative (n~ capped at 1e12 v) keep full accuracy.
 * What is approximate: the pseudo-data of the rows that STAY are held at the full-data mode (a refit would move them).
 *   y / mean / noise / side / upper: what the fit was given (upper_dev: the upper ends of the rows of side 2, or NULL -- 2 is
 *   then a bad side value);  f_dev: the mode the held factorisation was built at;  order / start / ngroups / max_group: as for
 *   dgp_cross_validate (max_group == 1: leave-one-out, G_ii from one pass over T and Sigma_ii from the prediction's variance
 *   pass at Xs = X; larger: blocks of order round_up(max(max_group, 65), 128) -- G_F from T's columns in every plan state, the
 *   batched potrf / trtri, Sigma as lower 128-tiles in the work area).
 *   out_dev [7][n] doubles, row i of plane q at out[q n + i]; with s_p^2 = v_c + noise_i (the held-out predictive of the
 *   OBSERVATION, as dgp_cross_validate's y - resid / var), za = (y - mu_c) / s_p, zb = (upper - mu_c) / s_p:
 *     DGP_LCV_MU    mu_c                       DGP_LCV_VAR   s_p^2
 *     DGP_LCV_LPD   log N(y; mu_c, s_p^2) | log Phi(za) (side -1) | log Phi(-za) (+1) | log [Phi(zb) - Phi(za)] (2)
 *     DGP_LCV_PLO / DGP_LCV_PHI   the observation's PIT, an interval for censored rows: Phi(za), Phi(za) | 0, Phi(za) |
 *                   Phi(za), 1 | Phi(za), Phi(zb)
 *     DGP_LCV_DLP   d LPD / d mu_c             DGP_LCV_TILT  log P(both ends shifted by -shift s_p) - log P (0 on observed
 *                   rows and when shift == 0): E[exp(shift c) | the row's bracket] = exp(shift mu_c + shift^2 s_p^2 / 2 + TILT)
 *   Rows that no fold holds are 0 in every plane.  info_dev [ngroups] int32: 0, or the failing pivot of G_F (the fold's rows NaN).
 * The log probabilities go through the fit's own erfcx / three-regime functions, never through a difference of cdfs.  The
 * plan's L, T, alpha are only read; no floating-point atomics, fixed orders: bitwise repeatable; indices read from order / start
 * are clamped.  work_dev: dgp_laplace_cross_validate_workspace_bytes bytes, 256-byte aligned (2 N^2 doubles for K(X, X) and V,
 * the fit's terms area, dgp_cross_validate's own area and chunk x order^2 for the folds' G_F^-1); 0 for a null, float32 or
 * batched plan or bad sizes.
 * DGP_E_ARG (float32 or batched plan, null argument, bad sizes, misaligned work area), DGP_E_STATE (no factorisation),
 * DGP_E_WORKSPACE -- all before any launch; DGP_E_ARG after the terms pass alone (its sums are read back, which synchronises the
 * stream) for a bad side value, a row of side 2 without upper_dev or a bad bracket. */
#define DGP_LCV_MU 0
#define DGP_LCV_VAR 1
#define DGP_LCV_LPD 2
#define DGP_LCV_PLO 3
#define DGP_LCV_PHI 4
#define DGP_LCV_DLP 5
#define DGP_LCV_TILT 6
#define DGP_LCV_PLANES 7
size_t dgp_laplace_cross_validate_workspace_bytes(const dgp_plan* plan, int ngroups, int64_t max_group);
int dgp_laplace_cross_validate(dgp_plan* plan, const double* theta_host, const void* y_dev, const void* mean_dev, const void* noise_dev,
                               const int32_t* side_dev, const void* upper_dev, const void* f_dev, const int32_t* order_dev,
                               const int32_t* start_dev, int ngroups, int64_t max_group, double shift, void* work_dev,
                               size_t work_bytes, double* out_dev, int32_t* info_dev, void* stream);

/* Exact FISHER INFORMATION of the hyperparameters from the factorisation the plan holds (after dgp_factorize or dgp_fit_step):
 * how well the data determine them.  The reference has no counterpart.  For the Gaussian marginal likelihood the expected
 * information of the covariance parameters is (Mardia & Marshall 1984)
 *     F_ab = 1/2 tr(K^^-1 D_a K^^-1 D_b) = 1/2 <G_a, G_b>_F,      G_a = T D_a T^T,  T = L^-1,
 * over P + E DIRECTIONS D_a (symmetric derivative matrices of K^): first the P = dgp_model_ntheta kernel directions
 * dK/dtheta_p at theta_host (constrained values, as for dgp_fit_step), then E = ndiag diagonal directions diag(d_e) --
 * derivatives of learned noise terms -- with d_e = diag_dev[site][e][0 .. n) in the plan's dtype (entries beyond a ragged
 * site's own size are ignored).  0 <= ndiag <= 8; diag_dev may be NULL when ndiag = 0.  Only first derivatives of the
 * kernel are needed and F is positive semi-definite by construction -- the observed Hessian is neither.
 *   fisher_dev  [batch][P + E][P + E] doubles whatever the plan's dtype, bitwise symmetric, in un-normalised
 *               log-likelihood units (the fit step's NLL is not divided by n either).
 * Passes: all P derivative matrices in one sweep of pair evaluations; per direction V = T D (the prediction's GEMM at width
 * N; a column scaling of T for a diagonal direction) and the lower triangle of G = V T^T on the MFMA tile cores (128 x 128
 * direct-to-LDS tiles, 64 x 64 ones while a launch has too few: DGP_OPT_LAUUM64_MAX_TILES; k-tiles last to first); then
 * the pairwise contraction in double, two stages, fixed order.  (P + E) (4/3) N^3 flop.  No floating-point atomics: bitwise
 * repeatable; batched plans: gridDim.z = sites, dgp_plan_set_site_sizes respected.  The plan is only read -- no refactoring;
 * A, T, K^^-1, alpha and every later dgp_predict / dgp_stage_grad answer are bitwise what they were.
 * work_dev: dgp_fisher_workspace_bytes(plan, ndiag) bytes, 256-byte aligned: per site (P + E + 1) N^2 plan-dtype elements
 * (the directions' matrices -- D_a lives in G_a's slot until its own product overwrites it -- and V) plus
 * (N/64)(N/64 + 1)/2 (P + E)^2 doubles of tile partials; 0 for a null plan or a bad ndiag.
 * DGP_E_ARG (null plan / result, ndiag outside 0 .. 8, ndiag > 0 without diag_dev, misaligned work area), DGP_E_WORKSPACE
 * (work area missing or too small), DGP_E_STATE (no factorisation in the plan, or the factorisation it holds failed: the
 * status word of every site is read back, which synchronises the stream) -- all before any launch. */
size_t dgp_fisher_workspace_bytes(const dgp_plan* plan, int ndiag);
int dgp_fisher(dgp_plan* plan, const double* theta_host, const void* diag_dev, int ndiag, void* work_dev, size_t work_bytes,
               double* fisher_dev, void* stream);

/* Exact JACOBIANS of the posterior mean and variance with respect to the hyperparameter directions, at all m test points, from
 * the factorisation the plan holds: what a first-order (delta-method) propagation of the hyperparameters' uncertainty into
 * predictions and loads needs beside dgp_fisher's covariance.  The Jacobians are exact; any propagation built on them is
 * first order in that covariance.  The reference has no counterpart (it could only refit).  With T = L^-1, alpha = K^^-1 r,
 * K* = K(X, X*) and beta = T^T T K* = K^^-1 K*, over dgp_fisher's P kernel and E = ndiag diagonal directions plus C = nrhs
 * RIGHT-HAND-SIDE columns g_c = rhs_dev[site][c][0 .. n) (derivatives of the prior mean at the training rows, plan dtype):
 *     dmean[p][j]         = sum_i dK*_ij/dtheta_p alpha_i - sum_i beta_ij (D_p alpha)_i
 *     dvar [p][j]         = dk(x*_j, x*_j)/dtheta_p - 2 sum_i beta_ij dK*_ij/dtheta_p + beta_j^T D_p beta_j
 *     dmean[P + e][j]     = -sum_i beta_ij d_e,i alpha_i,        dvar[P + e][j] = sum_i beta_ij^2 d_e,i
 *     dmean[P + E + c][j] = -sum_i beta_ij g_c,i   (the caller adds dm(x*_j)/draw_c; the variance does not depend on it)
 *   dmean_dev [batch][P + E + C][m], dvar_dev [batch][P + E][m]: doubles whatever the plan's dtype.  dvar_dev may be NULL
 *   (means only): the quadratic-form pass is then skipped.  0 <= ndiag, nrhs <= 8; diag_dev / rhs_dev may be NULL when their
 *   count is 0; entries beyond a ragged site's own size are ignored.
 * Passes: dgp_fisher's sweep for all D_p; K* and V = T K* (the prediction's launches); beta = T^T V on the MFMA tile cores (T
 * as the k-major operand, triangular k-range, last k-tile first; 128 x 128 direct-to-LDS tiles, 64 x 64 ones while a launch
 * has too few: DGP_OPT_LAUUM64_MAX_TILES); G = [D_p alpha | d_e o alpha | g_c] by an HBM-bound multi-slot matvec; a cross sweep
 * with ONE derivative pair evaluation per (i, j) accumulated in double against alpha_i and beta_ij; -beta^T G and beta^2 d;
 * the quadratic forms as the products D_p beta on the tile cores, contracted with beta in the tile epilogue (the dominant
 * cost: 2 P N^2 M flop); all column sums in double, two stages, fixed order.  No floating-point atomics: bitwise repeatable;
 * batched plans: gridDim.z = sites, dgp_plan_set_site_sizes respected.  The plan is only read: A, T, K^^-1, alpha and every
 * later answer are bitwise what they were.
 * work_dev: dgp_predict_sensitivity_workspace_bytes(plan, m, ndiag, nrhs) bytes, 256-byte aligned: per site P N^2 + 3 N M
 * plan-dtype elements (the D_p, K*, V, beta; M = m rounded up to 128) plus doubles: (P + E + C) N of G,
 * 32 (3 P + 2 E + C) M of slab partials and P (N/64) M of row-tile partials; 0 for a null plan or bad sizes.
 * DGP_E_ARG (null plan / theta / Xs / dmean_dev, m <= 0, ndiag or nrhs outside 0 .. 8, a positive count without its array,
 * misaligned work area), DGP_E_WORKSPACE (work area missing or too small), DGP_E_STATE (no factorisation in the plan, or the
 * one it holds failed: the status word of every site is read back, which synchronises the stream) -- all before any launch. */
size_t dgp_predict_sensitivity_workspace_bytes(const dgp_plan* plan, int64_t m, int ndiag, int nrhs);
int dgp_predict_sensitivity(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, const void* diag_dev, int ndiag,
                            const void* rhs_dev, int nrhs, void* work_dev, size_t work_bytes, double* dmean_dev, double* dvar_dev,
                            void* stream);

/* Exact INFLUENCE of the samples a fit already has: the change of every period sum when a fold of training observations is
 * DELETED, for all folds at once, at the hyperparameters of the factorisation the plan holds -- the case-deletion diagnostic of
 * regression and the delete-a-group jackknife of WRTDS practice, which the reference can only answer by one refit per deletion.
 * With S = K^^-1 = T^T T, alpha = S r, beta = S K* and, for a fold F of f rows, G_F = S_FF = M M^T, u = M^-1 alpha_F,
 * z_j = M^-1 beta_{F,j} (an f-vector per test point), the posterior without F is exactly
 *     mu'_j = mu_j - z_j^T u,      C'_jl = C_jl + z_j^T z_l      (sigma'^2_j = sigma^2_j + |z_j|^2)
 * and for the period sums of dgp_period_moments / dgp_sample_value over the m test points:
 *     mode 1 (log target),    a_j = w_j exp(s mu_j + t + s^2 C_jj / 2):  dload[F][g] = sum_{j in g} a_j expm1(s dmu_Fj + s^2 dsigma^2_Fj / 2)
 *     mode 0 (linear target), a_j = s w_j:                               dload[F][g] = sum_{j in g} a_j dmu_Fj
 *                                                                        dvar [F][g] = |sum_{j in g} a_j z_j|^2    (always >= 0)
 * Sign: the sum WITHOUT the fold minus the sum with it.  Hyperparameters, prior mean and transforms are held fixed.
 *   theta_host, Xs_dev [batch][m][d]: as for dgp_predict_sensitivity.  order_dev [batch][n], start_dev [batch][nfolds + 1], nfolds,
 *   max_fold: dgp_cross_validate's fold description (fold g of a site = order[start[g] .. start[g + 1]); empty folds and
 *   observations in no fold are allowed; max_fold >= the largest fold selects the route).  a_dev [batch][m] doubles, scale_dev
 *   [batch] doubles (s; read in mode 1), group_dev [batch][m] int32 in 0 .. ngroups - 1, non-decreasing, -1 = excluded (a violation
 *   gives wrong numbers, never an access out of bounds), inv_sd_dev NULL or [batch][m] doubles (1 / sigma_j).
 *   dload_dev [batch][nfolds][ngroups]; dvar_dev NULL or [batch][nfolds][ngroups] (mode 0 only); shift_dev NULL or [batch][nfolds]:
 *   max_j |dmu_Fj| inv_sd_j over all m points (a DFFITS-style screen; needs inv_sd_dev); info_dev [batch][nfolds] int32: 0, or the
 *   1-based failing pivot of G_F -- that fold's results are then NaN.  All results are doubles whatever the plan's dtype.
 * Passes: K*, V = T K*, beta = T^T V (the launchers of dgp_predict_sensitivity, DGP_OPT_LAUUM64_MAX_TILES included); the fold
 * algebra by dgp_cross_validate's three routes (max_fold == 1: column sums of squares of T, K^^-1 is never formed; <= 64: G_F, M,
 * M^-1 in LDS; larger: blocks of order round_up(max_fold, 128) with the batched potrf / trtri, then Z = M^-1 beta_F as one product
 * per fold on the double tile core); one sweep over (fold, test point) -- a wave per (fold, slab of points), beta read along j,
 * expm1, a segmented sum into the periods by shuffles -- and a finish kernel that adds the slabs in order.  No floating-point
 * atomics, fixed orders: bitwise repeatable; a site's result depends on its batch only through nfolds (it sets the slab cut of
 * the test points), max_fold (the route) and the tile selector of beta: bitwise under the same three, to rounding otherwise;
 * gridDim.z = sites, dgp_plan_set_site_sizes respected.  The plan is only read.
 * work_dev: dgp_deletion_influence_workspace_bytes(plan, m, nfolds, max_fold, ngroups) bytes, 256-byte aligned: per site 3 N M
 * plan-dtype elements (K*, V, beta; M = m rounded up to 128) plus doubles: the slab partials, n ngroups row sums,
 * dgp_cross_validate's own area, nfolds max_fold^2 (LDS route) or 2 chunk order M (block route: panel and Z); 0 for a null plan or
 * bad sizes (1 <= m <= 2^20, 1 <= nfolds, max_fold <= n, 1 <= ngroups <= 65535).
 * DGP_E_ARG (null plan / argument, bad sizes, mode outside 0 / 1, dvar_dev in mode 1, shift_dev without inv_sd_dev, misaligned
 * work area), DGP_E_WORKSPACE (work area missing or too small), DGP_E_STATE (no factorisation in the plan, or the one it holds
 * failed: the status word of every site is read back, which synchronises the stream) -- all before any launch. */
size_t dgp_deletion_influence_workspace_bytes(const dgp_plan* plan, int64_t m, int nfolds, int64_t max_fold, int ngroups);
int dgp_deletion_influence(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, const int32_t* order_dev,
                           const int32_t* start_dev, int nfolds, int64_t max_fold, int mode, const double* a_dev, const double* scale_dev,
                           const int32_t* group_dev, int ngroups, const double* inv_sd_dev, void* work_dev, size_t work_bytes,
                           double* dload_dev, double* dvar_dev, double* shift_dev, int32_t* info_dev, void* stream);

/* The posterior of the covariance's ADDITIVE PARTS.  Both fused covariances and every generic one are sums of named terms,
 *   loadest: seasonal + covariates + residual;  rating: shift_1 + shift_2 + bend + base + periodic (the shifts and the bend
 *   carry their gates);  composite: its terms in descriptor order (an unscaled term counts outputscale 1),
 * C = dgp_model_nterms(model, d) of them (3 / 5 / the descriptor's count; < 0 for an unsupported (model, d); needs no device).
 * With T = L^-1, alpha = K^^-1 r from the held factorisation, K_c the Gram of part c and V_c = T K_c(X, X*):
 *     mean_dev[site][c][j]            = K_c(x*_j, X) alpha                                   E[f_c(x*_j) | y]
 *     cov_dev[site][c(c+1)/2 + c'][j] = delta_cc' k_c(x*_j, x*_j) - V_c[:, j]^T V_c'[:, j]   Cov[f_c, f_c' | y](x*_j), c' <= c
 * in the plan's dtype.  The C means sum to dgp_predict's latent mean and the full C x C covariance at a point (off-diagonal
 * entries twice) to its variance; the cross-covariances give the variance of any merged part.  One pair evaluation per matrix
 * entry for all parts, the prediction's GEMM at width C M, one pass over V and Ks; fixed summation orders (bitwise repeatable).
 * Preconditions and arguments as dgp_predict (single-site, batched and ragged plans; Xs[batch][m][d], theta[batch][ntheta]);
 * cov_dev may be NULL (means only).  work_dev: dgp_predict_terms_workspace_bytes(plan, m) bytes, about
 * batch x 2 C N M elements.  DGP_E_ARG / DGP_E_WORKSPACE / DGP_E_STATE before any launch for a null plan or argument, m <= 0,
 * a plan without workspace or factorisation, a work area that is too small. */
int dgp_model_nterms(int model, int d);
size_t dgp_predict_terms_workspace_bytes(const dgp_plan* plan, int64_t m);
int dgp_predict_terms(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, void* work_dev,
                      size_t work_bytes, void* mean_dev, void* cov_dev, void* stream);

/* The posterior of the fit's INPUT DERIVATIVES (slopes).  The derivative of a GP is a GP: with D_0 = id, D_q = d / d x*_{c_q}
 * acting on the test point (c_q = cols_host[q - 1], raw input columns as in Xs; P = 1 + ncols), T = L^-1, alpha = K^^-1 r and
 * V_a = T (D_a K)(X, X*):
 *     mean_dev[site][a][j]           = (D_a K)(x*_j, X) alpha                                         E[D_a f(x*_j) | y]
 *     cov_dev[site][a(a+1)/2 + b][j] = D_a D'_b k(x, x')|x=x'=x*_j - V_a[:, j]^T V_b[:, j],  b <= a    Cov[D_a f, D_b f | y](x*_j)
 * in the plan's dtype; plane 0 is dgp_predict's latent mean and variance, the rest the slopes in the model's input units and
 * their covariances with each other and with the value.  This is what a user of the reference can only approximate by
 * differencing two calls of its predict (src/discontinuum/engines/gpytorch.py:599-626), without a standard error, and the
 * a-posteriori reading of the monotonicity that rating-gp only penalises while it trains
 * (src/rating_gp/models/gpytorch.py:130-187): P(d ln Q / d stage > 0) at any stage and time.
 * Every shipped covariance is mean-square differentiable in every column except through a Matern-1/2 factor of a composite:
 * dgp_model_input_differentiable(model, d, col) -> 1 / 0, < 0 for an unsupported (model, d) or a column outside 0 .. d - 1
 * (needs no device).  The prior block is not diagonal for rating (the gates correlate value and stage slope).
 * One pair evaluation per matrix entry for all planes, the prediction's GEMM at width P M, one pass over V and Ks; fixed
 * summation orders (bitwise repeatable); the plan is only read.  Preconditions and arguments as dgp_predict_terms
 * (single-site, batched and ragged plans); cols: distinct, in 0 .. d - 1, 1 <= ncols <= d; cov_dev may be NULL.  work_dev:
 * dgp_predict_slopes_workspace_bytes(plan, m, ncols) bytes (0 for bad arguments), about batch x 2 P N M elements.
 * DGP_E_ARG / DGP_E_WORKSPACE / DGP_E_STATE before any launch as for dgp_predict_terms, DGP_E_ARG for bad cols,
 * DGP_E_MODEL for a column that is not differentiable. */
int dgp_model_input_differentiable(int model, int d, int col);
size_t dgp_predict_slopes_workspace_bytes(const dgp_plan* plan, int64_t m, int ncols);
int dgp_predict_slopes(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, const int* cols_host, int ncols,
                       void* work_dev, size_t work_bytes, void* mean_dev, void* cov_dev, void* stream);

/* Predictive mean only, and its vector-Jacobian product -- what the rating-gp monotonicity penalty
 * differentiates (src/rating_gp/models/gpytorch.py:130-187: mean of likelihood(model(x_grid)) with grad).
 *   dgp_predict_mean : mean_dev[j] = K(x*_j, X) alpha                                  (m entries)
 *   dgp_mean_vjp     : given w_dev[j] = dLoss/dmean[j], with g = K(X, X*) w and beta = K^^-1 g:
 *        dtheta_dev[p] = sum_ij alpha_i w_j dK*_ij/dtheta_p - beta^T (dK/dtheta_p) alpha   (ntheta entries)
 *        dr_dev        = beta                       (dLoss/dr,     n entries)
 *        dnoise_dev    = -beta * alpha              (dLoss/dnoise, n entries)
 * Both use the factorisation (alpha, K^^-1) left in the plan by dgp_fit_step at the SAME theta. */
size_t dgp_mean_vjp_workspace_bytes(const dgp_plan* plan, int64_t m);
int dgp_predict_mean(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, void* work_dev,
                     size_t work_bytes, void* mean_dev, void* stream);
int dgp_mean_vjp(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, const void* w_dev,
                 void* work_dev, size_t work_bytes, void* dtheta_dev, void* dr_dev, void* dnoise_dev, void* stream);

/* In-library HIP-event timing of the stages of dgp_fit_step (events are recorded on the stream each
 * kernel is launched on, including the internal lookahead stream).  dgp_plan_get_timing synchronises
 * on the events of the most recent fit step and fills ms_out[DGP_TIME_COUNT]. */
#define DGP_TIME_GRAM 0      /* gram_sym kernel */
#define DGP_TIME_POTRF 1     /* whole factorisation, wall time on the caller's stream */
#define DGP_TIME_SYRK_SUM 2  /* sum of the bulk trailing-update (syrk) launches */
#define DGP_TIME_SYRK_N 3    /* number of those launches */
#define DGP_TIME_TRTRI 4     /* all trtri level launches */
#define DGP_TIME_LAUUM 5     /* lauum kernel */
#define DGP_TIME_SOLVE 6     /* triangular solves */
#define DGP_TIME_GRAD 7      /* gram_grad + reduction */
#define DGP_TIME_SYRK_FLOP 8 /* algorithmic flops of those bulk launches (not a time) */
#define DGP_TIME_COUNT 9
int dgp_plan_set_timing(dgp_plan* plan, int enabled);
int dgp_plan_get_timing(dgp_plan* plan, double* ms_out);

/* ---- ONE matrix distributed over `world` GPUs (BASELINE config 5; nothing in the reference corresponds) ----------
 * 1-D block-cyclic by column groups of `group_panels` 128-wide panels, group g on rank g % world.  A rank holds ONLY its
 * own groups -- three column slabs (K^ -> L, L^-1, K^^-1) of N x (its groups x 128 group_panels) elements, N =
 * dgp_dist_padded_n() -- plus whatever panel buffers the caller allocates for the payloads in flight
 * (dgp_dist_panel_elems(group) elements).  The caller moves the payloads (torch.distributed broadcast = RCCL over xGMI;
 * discontinuum_amd/dist_chol.py) and sums the O(n) vectors; all O(n^2) / O(n^3) work is in these entry points.
 *
 *   dgp_dist_gram                         every rank: its columns of K^ (the inputs are replicated)
 *   for g = 0 .. groups-1:   dgp_dist_factor(g, panel)        owner: panel chain, diagonal-block inverse, pack
 *                            <broadcast panel from rank g % world>
 *                            dgp_dist_update(g, panel, cb, ce) every rank: its block columns in [cb, ce) right of g
 *                                                              (ce <= 0: to the end; the owner of g + 1 brings that group
 *                                                              up to date first and factors it while the rest runs)
 *                            dgp_dist_invert(g, panel)         every rank: its columns of L^-1 advance by group g
 *   dgp_dist_status -> (local log-determinant, local info)     sum / max over the ranks
 *   dgp_dist_solve_partial(r) -> z_part (N)                    sum over the ranks: z = L^-1 r ;  r^T K^^-1 r = z^T z
 *   dgp_dist_alpha_partial(z) -> alpha_part (N)                sum over the ranks: alpha = K^^-1 r
 *   fp32 handles, one refinement step (the single plan's DGP_OPT_REFINE):
 *     dgp_dist_residual(alpha) -> rho64, rho32 (N)             every rank, no exchange: rho = r - K^ alpha, K^ re-evaluated
 *                                                              in double; then delta = K^^-1 rho32 by the two calls above,
 *                                                              alpha += delta, r^T K^^-1 r = r^T alpha0 + rho^T (alpha0 + delta)
 *   for g = 0 .. groups-1:   dgp_dist_pack_inverse(g, panel)  owner: its columns of L^-1 from the diagonal down
 *                            <broadcast>
 *                            dgp_dist_product(g, panel)        every rank: K^^-1 [group g rows, its columns >= g]
 *   dgp_dist_grad_partial(theta, alpha) -> dtheta_part (DGP_OUT_LEN, first ntheta valid), dnoise_part (N, zeros outside
 *                            the rank's columns)               sum over the ranks: dNLL/dtheta, 1/2 (diag K^^-1 - alpha^2)
 * Together: the NLL and ALL gradients of one fit step (engines/gpytorch.py:350-384) with N^3 / world flops per rank. */
typedef struct dgp_dist dgp_dist;
const char* dgp_dist_last_error(void);
int dgp_dist_create(int model, int dtype, int64_t n, int d, int rank, int world, int group_panels, dgp_dist** out);
int dgp_dist_destroy(dgp_dist* h);
int64_t dgp_dist_padded_n(const dgp_dist* h);     /* round_up(n, 128 group_panels) */
int dgp_dist_groups(const dgp_dist* h);
int64_t dgp_dist_slab_columns(const dgp_dist* h); /* columns of each of the rank's three slabs */
size_t dgp_dist_workspace_bytes(const dgp_dist* h);
size_t dgp_dist_panel_elems(const dgp_dist* h, int group);
int dgp_dist_set_workspace(dgp_dist* h, void* dev_ptr, size_t bytes);
int dgp_dist_set_inputs(dgp_dist* h, const void* X_dev, void* stream);
int dgp_dist_gram(dgp_dist* h, const double* theta_host, const void* noise_dev, void* stream);
int dgp_dist_factor(dgp_dist* h, int group, void* panel_dev, void* stream);
int dgp_dist_update(dgp_dist* h, int group, const void* panel_dev, int col_begin, int col_end, void* stream);
int dgp_dist_invert(dgp_dist* h, int group, const void* panel_dev, void* stream);
int dgp_dist_status(dgp_dist* h, void* stat_dev /* 2 elements */, void* stream);
int dgp_dist_solve_partial(dgp_dist* h, const void* r_dev, void* z_part_dev, void* stream);
int dgp_dist_alpha_partial(dgp_dist* h, const void* z_dev, void* alpha_part_dev, void* stream);
/* fp32 only; between the factorisation and dgp_dist_pack_inverse (the K^^-1 slab is its scratch: N^2 / 8 bytes, i.e. at
 * most 32 ranks).  rho64: N doubles; rho32: N floats (the same vector rounded, the right-hand side of the solves). */
int dgp_dist_residual(dgp_dist* h, const double* theta_host, const void* noise_dev, const void* r_dev, const void* alpha_dev,
                      double* rho64_dev, void* rho32_dev, void* stream);
int dgp_dist_pack_inverse(dgp_dist* h, int group, void* panel_dev, void* stream);
int dgp_dist_product(dgp_dist* h, int group, const void* panel_dev, void* stream);
int dgp_dist_grad_partial(dgp_dist* h, const double* theta_host, const void* alpha_dev, void* dtheta_part_dev,
                          void* dnoise_part_dev, void* stream);
/* the rank's slab `which` = DGP_BUF_A / DGP_BUF_T / DGP_BUF_S (tests) */
int dgp_dist_slab(const dgp_dist* h, int which, void** dev_ptr);

/* ---- single stages on the plan buffers, for parity tests and per-kernel profiling ---- */
int dgp_stage_gram(dgp_plan* plan, const double* theta_host, const void* noise_dev, void* stream);
int dgp_stage_potrf(dgp_plan* plan, void* stream);  /* A: K^ -> L ; T diag blocks <- L_kk^-1 */
int dgp_stage_trtri(dgp_plan* plan, void* stream);  /* T <- L^-1 */
int dgp_stage_lauum(dgp_plan* plan, void* stream);  /* S <- T^T T */
int dgp_stage_solve(dgp_plan* plan, const void* r_dev, void* stream); /* z, alpha, quad */
int dgp_stage_grad(dgp_plan* plan, const double* theta_host, void* dtheta_dev, void* stream);
/* rectangular K(X, Xs) into caller memory (N x M row-major, M = dgp_padded_n(m)); Xs as in dgp_predict;
 * work_dev holds the SoA copy of Xs (d * M elements) */
int dgp_cross_gram(dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, void* work_dev,
                   void* Ks_dev, void* stream);

/* ---- diagnostics ----
 * One grid of 128 x 128 output tiles through either tile-GEMM core of the O(n^3) stages (core 0: register-staged
 * dgp_gemm.h::TileGemm; 1: direct-to-LDS dgp_gemm_dma.h::DmaGemm), for the test that they are BITWISE equal:
 *     C[128 bm + i][128 bn + j] = sum_{kk < k} opA(128 bm + i, kk) opB(128 bn + j, kk),   bm < tiles_m, bn < tiles_n
 *     x_kc != 0: op(i, kk) = p[i ld + kk] (k-contiguous);  x_kc == 0: op(i, kk) = p[kk ld + i]
 * k a multiple of 16; A, B 16-byte aligned with ld a multiple of 16 bytes; all device pointers of `dtype`.
 * reverse != 0: the k-tiles of 16 are summed from the last to the first (ascending inside a tile) -- the order of
 * K^^-1 = L^-T L^-1, whose terms decay along k (small-to-large summation; csrc/dgp_gemm.h).
 * variant (core 1 only): 0 = the plain accumulator map; 1 = 16-row / 16-column groups dealt alternately to the wave rows /
 * columns; 2..5 = that map + zero-work skipping in the block of 128 k's visited LAST (k a multiple of 128): 2 operand A is
 * op(i, kk) = 0 for i > kk there, 3 op(i, kk) = 0 for kk > i, 4 operand B is op(j, kk) = 0 for j > kk, 5 the output is a
 * diagonal tile of a symmetric product (only the 16 x 16 sub-tiles with row group >= column group are specified).  With
 * operands that have that structure the specified results are bitwise those of variant 0. */
int dgp_debug_tile_gemm(int dtype, int core, int a_kc, int b_kc, const void* A_dev, int64_t lda, const void* B_dev,
                        int64_t ldb, int64_t k, void* C_dev, int64_t ldc, int tiles_m, int tiles_n, int reverse, int variant,
                        void* stream);

/* Shader-clock probe: `nwg` one-wave workgroups (8 or more reach every XCD) stay resident for `seconds` (<= 5) on one of
 * the library's INTERNAL streams of the caller's `stream` (no new stream: a process has few hardware queues) and write
 * (d s_memtime, d s_memrealtime) -- shader cycles and ticks of the 100 MHz wall clock -- to out_dev[2 i], out_dev[2 i + 1]
 * (uint64).  Enqueue the load to be clocked on `stream` meanwhile and synchronise the DEVICE before reading: the clock the
 * chip held is d s_memtime / d s_memrealtime x 100 MHz (MI355X lowers it under MFMA-dense load).  bench.py uses it for
 * `roofline.clock_mhz`; no product kernel carries a stamp. */
int dgp_debug_clock_probe(void* out_dev, int nwg, double seconds, void* stream);

/* The fit step's two triangular solves on caller-supplied device arrays (dtype DGP_F64 / DGP_F32): with T = Tm_dev (N x N
 * row-major, N % 128 == 0, 128 <= N <= 65536, 16-byte aligned; read up to the end of each row's diagonal 128-block only),
 *   z = T r (r_j = 0 for j >= n),  alpha = T^T z,  quad[0] = z^T z   (quad holds 8 elements, 8-byte aligned; fp32: the value
 * rounded to float at quad[1] and, summed in double and unrounded, as ONE double in quad[4..5] -- a plan's scalar block).
 * `partials_dev`: scratch of dgp_debug_solve_partials(N) elements, 16-byte aligned.  `capacity` 0 runs the kernels exactly as a
 * plan does; 1 shrinks the row kernel's register capacity to one 16-byte group per thread, so that the path for rows longer
 * than the registers hold (fp64: N > 8192 in a plan) runs at small N.  DGP_E_ARG on a bad argument, before any launch. */
int dgp_debug_solve(int dtype, int capacity, const void* Tm_dev, int64_t N, const void* r_dev, int64_t n, void* z_dev,
                    void* alpha_dev, void* partials_dev, void* quad_dev, void* stream);
int64_t dgp_debug_solve_partials(int64_t N);

/* The exact THIRD CENTRAL MOMENT of the same period sums (log targets: dgp_period_moments' mode 1 and its notation) -- the
 * skewness of an annual load, which a two-moment lognormal (Fenton-Wilkinson) only guesses and the reference can only sample.
 * With e_ij = expm1(s2 C_ij) (C_ii + extra_var_i on the diagonal) and S_g = sum_{i in g} w_i exp(s f_i + t):
 *   k3[g] = E[(S_g - E S_g)^3] = sum_{i,j in g} a_i a_j e_ij G_ij + 3 sum_{i in g} a_i y_i^2,
 *   G = e_gg diag(a_g) e_gg^T,   y_i = sum_{j in g} a_j e_ij      (no moment is subtracted from another)
 * and skewness = k3[g] / cov[g][g]^1.5 with dgp_period_moments' variance.  A linear target is Gaussian: k3 = 0, no call.
 * dtype, cov_dev, m, batch, mu_dev (mapped), scale2_dev, w_dev, group_dev, ngroups, extra_var_dev and the padding: as for
 *            dgp_period_moments (only the lower triangle of cov_dev is read; everything after the loads of C and mu is
 *            double; a violated group order gives wrong numbers, never an access out of bounds);
 * tile       0: the 64 x 64 register-staged tile core while the launch has few 128-tiles, the 128 x 128 direct-to-LDS core
 *            otherwise (the rule of K^^-1 = L^-T L^-1); 64 / 128 force one (tests).  The cores agree to rounding, not bitwise;
 * k3_out_dev batch x ngroups doubles.
 * work_dev: dgp_period_third_moments_workspace_bytes(m, ngroups, batch) bytes, 256-byte aligned -- per site 2 M^2 doubles (e
 * masked to the periods' block diagonal, and the same times diag(a)), M^2 / 128 + M / 2 doubles of per-(tile, row) partials and
 * O(M + ngroups) of vectors; 0 for bad sizes.  One symmetric product of at most M^3 multiply-adds per site on the MFMA pipe
 * (k clipped to the periods a tile pair shares, pairs that share none skipped), never stored: its epilogue contracts it.
 * Seven launches (gridDim.z = batch), no floating-point atomics: bitwise repeatable, and a site's result does not depend on
 * the batch it is in.  Needs no plan.  DGP_E_ARG: null arguments, bad sizes, tile not 0 / 64 / 128, a misaligned work area;
 * DGP_E_WORKSPACE: work area missing or too small -- all before any launch. */
size_t dgp_period_third_moments_workspace_bytes(int64_t m, int ngroups, int batch);
int dgp_period_third_moments(int dtype, const void* cov_dev, int64_t m, int batch, const void* mu_dev,
                             const double* scale2_dev, const double* w_dev, const int32_t* group_dev, int ngroups,
                             const void* extra_var_dev, int tile, void* work_dev, size_t work_bytes,
                             double* k3_out_dev /* batch x ngroups */, void* stream);

#include "dgp_hip_ext.h"
#include "dgp_hip_ext2.h"

#ifdef __cplusplus
}
#endif
#endif /* DGP_HIP_H */
