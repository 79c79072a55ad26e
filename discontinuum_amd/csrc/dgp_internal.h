// dgp_internal.h -- host-side launcher declarations shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DGP_TILE_HOST 128  // == DGP_TILE in dgp_common.h

namespace dgp {

inline long round_up(long n, long q) { return (n + q - 1) / q * q; }
// The one workspace carver: every *_layout() takes its areas in order, each rounded up to 256 bytes; `o` is the running total.
struct Carve {
  size_t o = 0;
  static size_t up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  size_t take(size_t bytes) {
    const size_t at = o;
    o += up(bytes);
    return at;
  }
};

// A batched plan carries B <= DGP_MAX_BATCH_SITES sites in lockstep: every fit-step kernel is launched once with
// gridDim.z = B and finds its site's buffers at blockIdx.z * stride (workspace buffers: `ws` elements of the plan's
// dtype; caller arrays: n or DGP_OUT_LEN).  B = 1 is the plain single-site plan.
#define DGP_MAX_BATCH_HOST 8     // == DGP_MAX_BATCH in dgp_common.h: hyperparameters by value up to here
#define DGP_MAX_BATCH_SITES 1024  // largest batch of a plan
// Tile-shape selectors of the O(n^3) stages.  Plan-level (dgp_plan_set_option) so that a test can force the kernels the
// benchmark shapes run -- lauum_kernel, the 128-tile rounds of the bulk update, the 128-tile inverse levels -- at sizes
// the dense oracle reaches; the defaults are the measured optima (environment overrides read once: DGP_LAUUM64,
// DGP_SYRK_SLOTS, DGP_TRTRI_SMALL).
struct Tuning {
  int lauum64_max_tiles;  // K^^-1 = L^-T L^-1 in 64 x 64 tiles while (128-tiles x batch) <= this (1000)
  int syrk_slots;         // workgroup slots of a bulk-update round: whole rounds in 128 x 128 tiles, the rest cut (512)
  long trtri_small;       // an inverse level with fewer 128-tiles (x batch) than this runs in 64 x 64 tiles (1024)
  int syrk_super;         // tile order of the bulk update: 0 = rows of the trailing matrix, S > 0 = S x S supertiles (experiment)
  int lauum_super;        // tile order of K^^-1 = L^-T L^-1: 0 = rows, S > 0 = S x S supertiles dealt round-robin over the XCDs
  int chain_yield;        // single-site plans: bulk-update waves leave their CU to the diagonal-block kernel while it runs there (1)
  int fused_grad;         // the gradient contraction runs in the epilogue of K^^-1's 128 x 128 tiles (dgp_fused.hip) when it applies (1)
  int group_gemm;         // batched plans: a panel group's rows below its diagonal block are solved by ONE GEMM against the inverted
                          // G x G-block diagonal block instead of G trsm + G - 1 column-update launches (dgp_chol.hip::potrf)
  int potrf_schedule;     // batched plans: -1 = by shape (potrf_schedule_auto), 0 = the group-ahead schedule (right-looking, K = 128 G passes), 1 = the left-looking family of
                          // dgp_schedule.h (each column group updated once, K = everything to its left); the three below are its cut points
  int potrf_sweep;        // panels per super-group (right-looking sweeps between them), 0 = none: pure left-looking
  int potrf_tail;         // the last potrf_tail block columns form a super-group of their own (0 = none): few, long tiles otherwise
  int potrf_tail_sweep;   // panels per super-group inside that tail (0 = the whole tail)
  int potrf_solve;        // the rows below a group's diagonal block by ONE GEMM (trsm_group_kernel) -- not bitwise the panel chain
  int potrf_slots;        // workgroup slots of a round of that schedule's strip UPDATEs, over the whole batch (768: three per CU)
  int potrf_overlap;      // with potrf_solve: the part of a group's update below its diagonal block runs on the bulk stream beside the block's panels
};
const Tuning& default_tuning();
int potrf_schedule_auto(int B, long nbk, int elem);  // the schedule a batched plan of B sites of nbk block columns (elem bytes per element) runs when Tuning::potrf_schedule < 0
struct Batch {
  int B = 1;
  long ws = 0;
  const int* ns = nullptr;  // device array of the sites' own sizes n_b <= n (ragged batch), or null: all n
  const Tuning* tune = nullptr;  // null: default_tuning()
  void* W = nullptr;             // N x N scratch per site (the plan's S buffer: free during the factorisation), or null: the
                                 // group schedule's panel solve as ONE GEMM against the inverted diagonal group block needs it
  const Tuning& tuning() const { return tune ? *tune : default_tuning(); }
};
int model_ntheta(int model, int d);  // number of constrained kernel hyperparameters, -1 if unsupported
int model_nterms(int model, int d);  // number of additive parts of the covariance (Model::terms), -1 if unsupported
int composite_define(const int* spec, int nspec);  // register a generic composite model (dgp_models.h), -> model id or < 0
bool composite_select(int model, int d);  // make `model` the composite the next Composite<T, d>::prepare reads; false if it is none

// ---- dgp_gram.hip ---------------------------------------------------------------------------
template <typename T>
int pack_x(const T* X, int n, int d, long N, T* Xt, hipStream_t s, Batch bt = Batch());
template <typename T>
int gram_sym(int model, int d, const T* Xt, long N, int n, const double* theta, const T* noise, T* K, hipStream_t s,
             Batch bt = Batch(), void* pre_scratch = nullptr /* pre_scratch_bytes(B) of device memory, B > 8 */,
             void* pre_staging = nullptr /* pinned host memory of the same size that outlives the copy, or null: blocking copy */,
             long k_stride = -1 /* site stride of K (default bt.ws) */, long noise_stride = -1 /* of noise (default n) */,
             bool pre_ready = false /* pre_scratch already holds this theta (gram_cross of the same call) */);
// The tile rows [row0, row1) (multiples of 64) of the same lower triangle, columns 0 .. row1 - 1, into a panel buffer whose first
// row is row `row0` of K (leading dimension N, site stride k_stride): gram_sym's kernel and values on a row range.  The
// hyperparameters of a batch of more than 8 must already be in pre_scratch.
template <typename T>
int gram_sym_panel(int model, int d, const T* Xt, long N, int n, const double* theta, const T* noise, T* K, long row0, long row1,
                   hipStream_t s, Batch bt, void* pre_scratch, long k_stride, long noise_stride);
// The rectangular block rows [row0, row1) x columns [col0, row1) (multiples of 64, col0 <= row0) of the same lower triangle
// into a band buffer whose first element is K[row0][col0] (leading dimension ld, site stride k_stride): gram_sym's evaluation
// and values; tiles above the diagonal are not written.  The hyperparameters as for gram_sym_panel.
template <typename T>
int gram_sym_band(int model, int d, const T* Xt, long N, int n, const double* theta, const T* noise, T* K, long row0, long row1,
                  long col0, long ld, hipStream_t s, Batch bt, void* pre_scratch, long k_stride, long noise_stride);
// The inference launchers take a Batch like the fit-step ones (gridDim.z = sites): training-side arrays at the plan's
// site stride bt.ws, everything in the caller's work area (test coordinates, cross Gram, partials ...) at `wbs` elements.
template <typename T>
int gram_cross(int model, int d, const T* Xt, long N, int n, const T* Xst, long M, int m, const double* theta,
               T* Ks, hipStream_t s, Batch bt = Batch(), long wbs = 0, void* pre_scratch = nullptr, void* pre_staging = nullptr);
template <typename T>
int gram_diag(int model, int d, const T* Xst, long M, int m, const double* theta, T* kss, hipStream_t s, Batch bt = Batch(),
              long wbs = 0, void* pre_scratch = nullptr);
template <typename T>
int gram_grad(int model, int d, const T* Xt, long N, int n, const double* theta, const T* S, const T* alpha,
              T* partials, T* dtheta, hipStream_t s, Batch bt = Batch(), long dtheta_stride = 0,
              void* pre_scratch = nullptr, bool pre_ready = false /* gram_sym of this step filled pre_scratch */,
              void* pre_staging = nullptr);
size_t pre_scratch_bytes(int B);  // device scratch for the hyperparameters of a batch of B (0 up to 8)
// rho = r - (K(X, X; theta) + diag(noise)) alpha in DOUBLE, the covariance re-evaluated pair by pair from the stored
// (TS = float) coordinates -- K^ itself was overwritten by its factor.  Lower 64 x 64 tiles only (each tile feeds its
// row block and, transposed, its column block); `part` = (N/64)^2 x 64 doubles of scratch per site (site stride ps
// doubles), rho64 / rho32 N elements per site at strides ps / rs.  Deterministic (fixed summation order).
template <typename TS>
int gram_residual(int model, int d, const TS* Xt, long N, int n, const double* theta, const TS* noise, const TS* r,
                  const TS* alpha, double* part, double* rho64, TS* rho32, hipStream_t s, Batch bt, long ps, long rs,
                  void* pre_scratch, void* pre_staging);
size_t gram_residual_scratch_bytes(long N);  // part + rho64 + rho32 + delta, per site
long gram_grad_partials(long N);
// ---- dgp_fused.hip: K^^-1 = L^-T L^-1 with the gradient contraction in the epilogue of every 128 x 128 tile
bool lauum_grad_applies(int model, long N, const Batch& bt);
template <typename T>
int lauum_grad(int model, int d, const T* Tm, long N, T* S, const T* Xt, int n, const double* theta, const T* alpha, T* partials,
               T* dtheta, hipStream_t s, Batch bt, long dtheta_stride, void* pre_scratch, bool pre_ready, void* pre_staging);
template <typename T>
int mean_vjp_grad(int model, int d, const T* Xt, long N, int n, const T* Xst, long Mp, int m, const double* theta,
                  const T* alpha, const T* beta, const T* wts, T* partials, T* dtheta, hipStream_t s, Batch bt = Batch(),
                  long wbs = 0, long dstride = 0, void* pre_scratch = nullptr, void* pre_staging = nullptr);
template <typename T>
int gemv_rows(const T* Ks, long N, long Mp, int m, const T* w, T* out, hipStream_t s, int B = 1, long wbs = 0);

// ---- dgp_chol.hip ---------------------------------------------------------------------------
// What watches a factorisation from outside: the timing of its bulk launches (dgp_plan_get_timing) and the checkpoints behind which
// the caller enqueues dependent work (fit_step's early inverse).  One per factorisation: a schedule that hands over to another
// (potrf with q_stop -> potrf_split) passes it on, counters and next checkpoint included.
struct PotrfObservers {
  hipEvent_t* syrk_ev = nullptr;  // 2 per timed bulk launch, or null: launches are counted but not timed
  int syrk_pool = 0;              // bulk launches the event pool can time
  int n_syrk = 0;                 // bulk launches so far, and their flops
  double syrk_flop = 0.0;
  int nck = 0;                    // checkpoint c is due once the first ck_blocks[c] (ascending) block columns of L are final
  const int* ck_blocks = nullptr;
  hipEvent_t* ck_ev = nullptr;
  void (*on_ck)(void* ctx, int idx) = nullptr;  // called right after checkpoint idx is recorded
  void* ck_ctx = nullptr;
  int ck_next = 0;

  bool bulk_begin(hipStream_t s) {  // -> whether this launch is timed
    const bool timed = syrk_ev != nullptr && n_syrk < syrk_pool;
    if (timed) hipEventRecord(syrk_ev[2 * n_syrk], s);
    return timed;
  }
  void bulk_end(hipStream_t s, double flop) {
    if (syrk_ev != nullptr && n_syrk < syrk_pool) hipEventRecord(syrk_ev[2 * n_syrk + 1], s);
    syrk_flop += flop;
    ++n_syrk;
  }
  // every checkpoint due at cols_final, on `s` (every schedule records every checkpoint, at the latest when the factorisation is complete)
  void checkpoint(int cols_final, hipStream_t s) {
    while (ck_next < nck && ck_blocks[ck_next] <= cols_final) {
      hipEventRecord(ck_ev[ck_next], s);
      if (on_ck) on_ck(ck_ctx, ck_next);  // the caller enqueues its dependent work NOW, not after the whole schedule
      ++ck_next;
    }
  }
};
template <typename T>
int potrf(T* A, long N, T* Dinv, T* logdet, int* info, int lookahead, hipStream_t s, hipStream_t s2, hipEvent_t* ev,
          PotrfObservers* obs = nullptr /* null: none */, Batch bt = Batch(), int q_stop = -1 /* stop after chain(q_stop - 1): potrf_split */);
// the split panel chain (one site, fewer than 96 block columns): critical tile on `s`, rest of the chain on `c2`,
// bulk updates on `s2`; ev holds 3 N/128 events; snap = 2 x 128 x 128 elements of workspace
template <typename T>
int potrf_split(T* A, long N, T* Dinv, T* logdet, int* info, T* snap, hipStream_t s, hipStream_t c2, hipStream_t s2,
                hipEvent_t* ev, PotrfObservers* obs = nullptr, int k_start = 0 /* block columns before it by the single-stream group schedule */,
                int G_old = 2 /* panels per group of that schedule */, const Tuning* tune = nullptr);
// progress of the level recursion of trtri when it is issued piecewise (trtri_advance)
struct TrtriProgress {
  static constexpr int MAXLVL = 16;
  int wdone[MAXLVL] = {0}, gdone[MAXLVL] = {0};  // per level: groups whose W-step / both steps are launched
  int pairs_used = 0;                            // counter pairs consumed by queue-driven launches
};
template <typename T>
int trtri_advance(const T* L, long N, T* Tm, T* W, int ready_blocks, TrtriProgress* st, hipStream_t s, int wg_cap,
                  int* ctr /* info + EARLY_CTR0, or null */, int nctr_pairs, int reserve_cus, Batch bt = Batch(),
                  long ld = 0 /* leading dimension of L, Tm, W if not N */);
// info[0] = potrf status; info[EARLY_CTR0 + 2i ..] = (tile queue, worker count) of the i-th early inverse launch
#define CHAIN_FLAG0 2  /* info[2], info[3]: the split chain's progress counters (rest steps / bulk launches finished) */
#define EARLY_CTR0 4
#define EARLY_CTR_PAIRS 125
#define POTRF_INFO_INTS (EARLY_CTR0 + 2 * EARLY_CTR_PAIRS + 4)
#define CHAIN_ABORT (POTRF_INFO_INTS - 4)      /* != 0: a bounded wait of the split chain ran out -- every later waiter leaves at once */
#define CHAIN_YIELD (POTRF_INFO_INTS - 3)      /* cu_code() of the running diagonal-block kernel, else 0 (dgp_common.h: yield_if_asked) */
#define CHAIN_DIAG_DONE (POTRF_INFO_INTS - 2)  /* diagonal blocks finished (split chain: the rest stream's trsm waits on it) */
#define CHAIN_TICKET (POTRF_INFO_INTS - 1)     /* workgroup ticket of the rest stream's column-update kernel */
// per-device table of compute units kept free of early-inverse workgroups (null if unavailable)
const unsigned char* reserved_cu_table(int nreserve, int* n_cu);
template <typename T>
int trtri(const T* L, const T* Dinv, long N, T* Tm, T* W, hipStream_t s, Batch bt = Batch(), long ld = 0);
template <typename T>
int lauum(const T* Tm, long N, T* S, hipStream_t s, Batch bt = Batch());
template <typename T>
int solve(const T* Tm, long N, const T* r, int n, T* z, T* alpha, T* partials, T* quad, hipStream_t s,
          Batch bt = Batch(), int kt = 0 /* diagnostic: register capacity of the row kernel, dgp_chol.hip::solve_pair */);
// fp32 plans, after solve(): one step of iterative refinement with an fp64 residual (dgp_gram.hip::gram_residual).
//   delta = T^T (T rho32)  (the fp32 factor),  alpha <- alpha + delta,  quad = r^T alpha0 + rho^T (alpha0 + delta) in double
// (second-order accurate in the error of delta).  z and `partials` are solve()'s scratch; rho32 / delta: N elements each.
template <typename T>
int refine_solve(const T* Tm, long N, const T* r, int n, const double* rho64, const T* rho32, T* z, T* delta, T* alpha,
                 T* partials, T* quad, hipStream_t s, Batch bt, long scratch_stride /* site stride of rho64 (in doubles) */,
                 long rho32_stride /* site stride of rho32 / delta, in elements */);
// row slabs of the prediction's column reductions (part: 2 x PREDICT_SPLIT x M elements of workspace)
#define PREDICT_SPLIT 32
template <typename T>
int predict_var(const T* Tm, long N, const T* Ks, long M, T* V, const T* alpha, const T* kss, T* part, T* mean, T* var,
                hipStream_t s, Batch bt = Batch(), long wbs = 0);
// V = T Ks alone (Ks, V: N x M row-major in the caller's work area, M % 128 == 0): predict_var's first launch
template <typename T>
int predict_v(const T* Tm, long N, const T* Ks, long M, T* V, hipStream_t s, Batch bt = Batch(), long wbs = 0);
// solve() with r, z, the result, the partials and quad in the caller's work area at one site stride wss: the plan's z / alpha untouched
template <typename T>
int solve_work(const T* Tm, long N, const T* r, int n, T* z, T* out, T* partials, T* quad, long wss, hipStream_t s, Batch bt = Batch());
long solve_partials(long N);
// ---- one matrix over several GPUs (dgp_dist.hip): the panel chain of W block columns on a slab-addressed matrix
template <typename T>
int potrf_group(T* A, long ld, int nbk, T* Tinv, T* logdet, int* info, int k0, int W, hipStream_t s);
// Block-cyclic column ownership: groups of W 128-wide panels, group g on rank g % world; a rank keeps its groups side
// by side in a slab of Cl columns (local column block lb <-> global block column gblock(lb)).
struct SlabMap {
  int W, world, rank;
  __host__ __device__ int gblock(int lb) const { return ((lb / W) * world + rank) * W + lb % W; }
};
template <typename T>
int gram_slab(int model, int d, const T* Xt, long N, int n, const double* theta, const T* noise, T* Aslab, long Cl,
              SlabMap sm, hipStream_t s);
// partial gradient over the tiles of K^^-1 this rank holds (rows <= columns of its own block columns) and
// 1/2 (diag K^^-1 - alpha^2) for its own columns (dnoise_part: N entries, others untouched)
template <typename T>
int gram_grad_slab(int model, int d, const T* Xt, long N, int n, const double* theta, const T* Sslab, long Cl, SlabMap sm,
                   const T* alpha, T* partials, T* dtheta, T* dnoise_part, hipStream_t s);
long gram_grad_slab_partials(long N, long Cl);
template <typename T>
int symv_lower(const T* S, long N, const T* g, int n, const T* alpha, T* beta, T* partials, T* dnoise, hipStream_t s,
               Batch bt = Batch(), long wbs = 0);
// cov (M x M) = Kss - V^T V, lower tiles; Kss already holds K(Xs, Xs) (identity pad)
template <typename T>
int posterior_cov(const T* V, long N, long M, T* cov, hipStream_t s, int B = 1, long wbs = 0);
// the tile rows [row0, row1) (multiples of 128) of the same update, into a panel buffer whose first row is row `row0` of the
// matrix (leading dimension M, site stride panel_stride elements): the same kernel, tiles, k order and values on a row range
template <typename T>
int posterior_cov_panel(const T* V, long N, long M, T* panel, long row0, long row1, long panel_stride, hipStream_t s, int B = 1,
                        long wbs = 0);
// the block rows [row0, row1) x columns [col0, row1) (multiples of 128, col0 <= row0) of the same update, into a band buffer
// whose first element is C[row0][col0] (leading dimension ld, site stride band_stride elements): the same tile core, k order
// and values; tiles above the diagonal are not touched
template <typename T>
int posterior_cov_band(const T* V, long N, long M, T* band, long row0, long row1, long col0, long ld, long band_stride,
                       hipStream_t s, int B = 1, long wbs = 0);

// out (ndraw x m) = mean + (L Z)^T : L is M x M lower (identity pad), Z is M x Q standard normals, Q % 128 == 0
template <typename T>
int sample_draws(const T* L, long M, const T* Z, long Q, const T* mean, int m, int ndraw, T* out, hipStream_t s);

// ---- dgp_exceed.hip: exact mean / covariance of the counts sum_{i in g} w_i 1[f_i > u_il], f ~ N(mu, C), per level l.  thresh
// [B][L][m] in model space; mean_out [B][L][P], cov_out [B][L][P][P]; `work`: exceedance_moments_workspace_bytes
size_t exceedance_moments_workspace_bytes(long m, int P, int L, int B);
// the passes before and after the pairs pass, for dgp_exceed_stream.hip: init + prep (C_jj of site z at diag[z dsite + j dstep]),
// and the reduce pass of the levels l0 .. l0 + LC
template <typename T>
void exceedance_prepare(const T* diag, long dsite, long dstep, long m, int B, const T* mu, const double* thresh, int L, const double* w,
                        const int* group, int P, const T* ev, double* work, hipStream_t s);
void exceedance_reduce(long M, int B, int P, int L, int l0, int LC, double* work, double* mean_out, double* cov_out, hipStream_t s);

// ---- dgp_excess.hip: exact mean / covariance of the period sums of the excess (deficit) of a log-transformed posterior over a
// threshold; the work area's layout, with Y holding min(L, YL) levels, is dgp_excess.h's (YL = XS_CHUNK dense, XS_GROUP streamed)
size_t excess_moments_workspace_bytes(long m, int P, int L, int B, int YL);
// the passes before and after the pairs pass, for dgp_excess_stream.hip: init + prep (C_jj of site z at diag[z dsite + j dstep];
// sg = +1 excess, -1 deficit), and the reduce pass of the levels l0 .. l0 + LV, which reads Y's levels 0 .. LV
template <typename T>
void excess_prepare(const T* diag, long dsite, long dstep, long m, int B, const T* mu, const double* scale2, const double* thresh, int L,
                    const double* w, const int* group, int P, const T* ev, double sg, int YL, double* work, hipStream_t s);
void excess_reduce(long M, int B, int P, int L, int l0, int LV, int YL, double* work, double* mean_out, double* cov_out,
                   double* total_out, hipStream_t s);

// ---- dgp_terms.hip: the posterior of the covariance's additive parts (C = model_nterms).  Ks / V: N x (C Mp) row-major, term c
// of test point j in column c Mp + j; kss: C Mp; part: terms_partials(C, Mp) elements; mean [B][C][m], cov [B][C (C + 1) / 2][m]
// (entry (c, c'), c' <= c, at c (c + 1) / 2 + c'; null: not wanted) in the caller's arrays.
template <typename T>
int gram_cross_terms(int model, int d, const T* Xt, long N, int n, const T* Xst, long Mp, int m, const double* theta, T* Ks,
                     hipStream_t s, Batch bt = Batch(), long wbs = 0, void* pre_scratch = nullptr, void* pre_staging = nullptr);
template <typename T>
int gram_diag_terms(int model, int d, const T* Xst, long Mp, int m, const double* theta, T* kss, hipStream_t s, Batch bt = Batch(),
                    long wbs = 0, void* pre_scratch = nullptr);
long terms_partials(int C, long Mp);
template <typename T>
int terms_reduce(int C, const T* V, const T* Ks, long N, long Mp, int m, const T* alpha, const T* kss, T* part, T* mean, T* cov,
                 hipStream_t s, Batch bt = Batch(), long wbs = 0);

// ---- dgp_slopes.hip: the posterior of the fit's derivatives w.r.t. the raw input columns cols[0 .. ncols) of the test point
// (distinct, in 0 .. d - 1).  P = 1 + ncols planes, plane 0 the value: Ks / V N x (P Mp) row-major, plane a of test point j in
// column a Mp + j; prior: the packed P (P + 1) / 2 block D_a D'_b k(x*, x*) per point, entry (a, b <= a) at
// (a (a + 1) / 2 + b) Mp + j; part: terms_partials(P, Mp); mean [B][P][m], cov [B][P (P + 1) / 2][m] (null: not wanted).
struct SlopeCols {        // kernel argument
  int ncols;
  signed char plane[7];   // of (value, column 0 .. 5): the plane it is written to, -1 = not requested
  unsigned char col[6];   // of plane q + 1: its column
};
int model_input_differentiable(int model, int d, int col);  // 1 / 0, -1 for an unsupported (model, d) or a column outside 0 .. d - 1
template <typename T>
int gram_cross_slopes(int model, int d, const T* Xt, long N, int n, const T* Xst, long Mp, int m, const double* theta,
                      const int* cols, int ncols, T* Ks, hipStream_t s, Batch bt = Batch(), long wbs = 0,
                      void* pre_scratch = nullptr, void* pre_staging = nullptr);
template <typename T>
int gram_prior_slopes(int model, int d, const T* Xst, long Mp, int m, const double* theta, const int* cols, int ncols, T* prior,
                      hipStream_t s, Batch bt = Batch(), long wbs = 0, void* pre_scratch = nullptr);
template <typename T>
int slopes_reduce(int P, const T* V, const T* Ks, long N, long Mp, int m, const T* alpha, const T* prior, T* part, T* mean, T* cov,
                  hipStream_t s, Batch bt = Batch(), long wbs = 0);  // dgp_terms.hip: shares its reduction kernels

// ---- dgp_crossval.hip: exact leave-one-out / leave-group-out cross-validation from T = L^-1, alpha and -- when it is valid --
// S = K^^-1 (null otherwise).  order [B][n] / start [B][ngroups + 1]: group g of a site = order[start[g] .. start[g + 1]); every
// group has at most max_group members.  resid / var [B][n], lpd / info [B][ngroups], all double / int whatever T is; `work`:
// cross_validate_workspace_bytes.  Reads T, S, alpha only.
#define CV_SMALL_GROUP 64  // largest group of cross_validate's fused LDS route; larger groups take the block route (and its tap)
size_t cross_validate_workspace_bytes(long N, int B, int ngroups, long max_group);
// A TAP on the fold algebra for passes that need more of a fold than cross_validate's own results (dgp_influence.hip): the factor
// M of G_B = M M^T, inverted.  Groups of up to 64 (the LDS route): M^-1 of fold g of a site is written lower, row-major, to
// minv[(site ngroups + g) ld ld ...] (ld >= max_group; a failed fold writes nothing).  Larger groups (the block route): `chunk`
// is called once per chunk of C folds g0 .. g0 + C - 1, after the chunk's launches are on the stream and before the next chunk
// reuses the blocks; it enqueues its own work on the same stream and returns 0 or an error.  Neither changes what
// cross_validate computes.  For dgp_lgo.hip the LDS route also writes, when `wblk` is set, the fold's FULL weight block
// W_g = G_B^-1 + e_B e_B^T (b x b, symmetric, leading dimension wld, cv_wblock_shift columns in) at wblk + site wsite + start[g] wld -- the folds of a site are
// disjoint, so its blocks stack into at most n rows -- and the block route lends `scratch`, M x M per slot that nothing reads
// any more, to the chunk's callback.
struct CvBlocks {
  const double* minv;  // slot z = site C + c: M^-1 (M x M row-major, lower, identity pad) at minv + z stride
  const double* e;     // e_B = G_B^-1 alpha_B in the fold's own order (M entries) at e + z stride
  long stride, M;
  int g0, C;
  double* scratch;     // M x M at scratch + z stride (the inverse's work block)
};
struct CvTap {
  double* minv = nullptr;
  long ld = 0;
  int (*chunk)(void* ctx, const CvBlocks& blocks) = nullptr;
  void* ctx = nullptr;
  double* wblk = nullptr;
  long wld = 0, wsite = 0;
};
int cross_validate_chunk_groups(long N, int B, int ngroups, long max_group);  // folds per chunk of the block route (0: another route)
template <typename T>
int cross_validate(const T* Tm, const T* S, const T* alpha, long N, int n, const int* order, const int* start, int ngroups,
                   long max_group, void* work, double* resid, double* var, double* lpd, int* info, hipStream_t s, Batch bt,
                   const CvTap* tap = nullptr);
#ifdef __HIPCC__
// group g of a site = order[s0 .. s0 + b): bounds clamped to the site and to the route's largest group
__device__ __forceinline__ void cv_bounds(const int* __restrict__ start, int g, int n, int cap, int& s0, int& b) {
  int a = start[g], e = start[g + 1];
  a = min(max(a, 0), n);
  e = min(max(e, a), n);
  s0 = a;
  b = min(e - a, cap);
}
__device__ __forceinline__ int cv_index(const int* __restrict__ order, int p, int n) { return min(max(order[p], 0), n - 1); }
// dgp_lgo.hip reads a fold's weight block against the rows s0 .. of an N-row operand in k-tiles of 16.  A fold whose last tile
// would pass row N is read from `shift` rows earlier instead, and its block is stored `shift` columns to the right (zeros in
// front of it): shift + b <= round_up(b, 16), so the row still fits, and no operand row beyond N - 1 is ever read
__device__ __forceinline__ int cv_wblock_shift(long N, int s0, int b) { return max(0, s0 + ((b + 15) & ~15) - (int)N); }
#endif

// ---- dgp_fisher.hip: the Fisher information's first pass alone (for dgp_sensitivity.hip): D_p = dK/dtheta_p for every p < ntheta,
// slot p (N^2 elements) of G at site stride wbs
template <typename T>
int fisher_dk(int model, int d, const T* Xt, long N, int n, const double* theta, T* G, hipStream_t s, Batch bt, long wbs,
              void* pre_scratch, void* pre_staging, bool upload);

// ---- dgp_sensitivity.hip: its beta = T^T V alone (for dgp_influence.hip; V, beta: N x Mp row-major at site stride wbs)
template <typename T>
int sens_beta(const T* Tm, long N, const T* V, long Mp, T* beta, hipStream_t s, Batch bt, long wbs);

// ---- dgp_censored.hip: censored rows (Tobit likelihood) by the Laplace approximation -- a GP regression on pseudo-data (r~, n~).
// fp64 plans, single-site or batched (blockIdx.z = site, ragged sizes through site_n).  The caller's work area is a
// CensoredLayout; `status` holds one CEN_ST_* block per site, which the host reads in one copy per Newton iteration.
#define CEN_PART 16    // doubles per workgroup of the block partials
#define CEN_NT 8       // step lengths of the line search: 0, 1, 1/2, .. 1/64
#define CEN_CAP 1e-12  // a censored row with W v below this is uninformative: n~ = v / CEN_CAP, d3 = 0
enum {
  CEN_ST_CORR = 0,   // alpha-free part of the NLL correction; then capped rows, bad side values, censored rows (cen_terms)
  CEN_ST_CAPPED,
  CEN_ST_BAD,
  CEN_ST_NCENS,
  CEN_ST_DMAX,       // max |f_new - f| of the proposal (inf when the factorisation failed)
  CEN_ST_T,          // step length taken
  CEN_ST_HALVINGS,
  CEN_ST_INFO,       // DGP_OUT_INFO of the iteration's factorisation
  CEN_ST_PSI0,
  CEN_ST_PSI,
  CEN_ST_NLL_CORR,   // the whole correction NLL_L - NLL_engine
  CEN_ST_DONE,       // 0: the site's mode search is running; -1: it has no censored row (done before the first iteration);
                     // k > 0: it finished in Newton iteration k (converged or not positive definite).  A site that finished in an
                     // EARLIER iteration is frozen: cen_search, cen_update and cen_terms leave everything of it untouched
  CEN_ST_BADBRK,     // rows of side 2 whose `upper` is NaN, infinite or not above y (set by the first pass of a call)
  CEN_ST_LEN = 16
};
// Byte offsets into the work area.  rt (r~), nn (n~) and dnoise are [B][n] at stride n, as fit_step<double> reads its caller
// arrays, and so are the other elementwise vectors; w, u, z (N entries), the partials of the solve and of the sweep and quad form
// one slice per site (`slice` bytes, the first at `slices`): ONE site stride for everything solve_work touches.
struct CensoredLayout {
  size_t rt, nn, dnoise, g, W, d3, corr, logp, delta, acur, part, status, out, slices, total;
  size_t w, u, z, spart, gpart, quad, slice;  // inside a site's slice
  int nblk;  // workgroups per site of the elementwise passes
  int B;
  long n;
};
CensoredLayout censored_layout(long N, long n, int B = 1);
// the terms at f: r~, n~, g, W, d3, per-row correction and log p into the work area, their sums into status[CEN_ST_CORR ..];
// init: the first pass of a call, which also sets every site's CEN_ST_DONE (0 or -1) and clears the search's fields;
// otherwise `it` = the Newton iteration just taken (1-based): sites that finished before it, or failed in it, are skipped.
// upper ([B][n], or null): the upper ends of the rows of side 2 (interval-censored: the truth lies in [y, upper]); with a null
// `upper` 2 is a bad side value and both passes give the bits they gave before brackets existed
int censored_terms(const double* f, const double* y, const int* side, const double* v, const double* m, int n, int init, int it,
                   char* work, const CensoredLayout& L, hipStream_t s, Batch bt = Batch(), const double* upper = nullptr);
// dtheta[p] (+)= sum_ij u_i dK_ij/dtheta_p alpha_j per site (dtheta at site stride dstride); u, alpha and the partials
// (gram_grad_partials(N) elements) at the site strides us / as / ps.  pre_scratch / upload / staging as for gram_grad (a batch of
// more than 8).  Reads Xt, u, alpha only.
template <typename T>
int gram_bilinear(int model, int d, const T* Xt, long N, int n, const double* theta, const T* u, const T* alpha, T* partials,
                  T* dtheta, int accumulate, hipStream_t s, Batch bt = Batch(), long us = 0, long as = 0, long ps = 0, long dstride = 0,
                  void* pre_scratch = nullptr, bool upload = false, void* pre_staging = nullptr);

}  // namespace dgp
