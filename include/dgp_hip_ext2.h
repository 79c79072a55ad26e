/* dgp_hip_ext2.h -- further entry points of libdgp_hip.so declared beside dgp_hip.h, which includes this file inside its
 * extern "C" block: include dgp_hip.h, never this file alone.  Bound through _lib.EXT2_SIGNATURES. */
#ifndef DGP_HIP_EXT2_H
#define DGP_HIP_EXT2_H

/* STREAMED THRESHOLD EXCESS: the moments of dgp_excess_moments (dgp_hip_ext.h: its notation, its decided points, its outputs)
 * of the plan's posterior at Xs, straight from the factorisation the plan holds: the posterior covariance
 * C = K(Xs, Xs) - V^T V is produced panel_rows rows at a time and never stored whole, so a record that the dense pair
 * dgp_posterior_cov + dgp_excess_moments cannot hold (m = 140 000 is 157 GB of covariance) takes one call.
 * p, theta, Xs_dev, m and the padding: as for dgp_posterior_exceedance_moments (batched and ragged plans: one call for all
 *            sites, every array with a leading site dimension);
 * mu_dev     the MAPPED mean s mu + t, sites x m, in the plan's dtype;   scale2_dev: s^2, one double per site;
 * thresh_dev sites x nlevels x m doubles, a = ln tau; -inf (tau = 0) and +inf allowed;
 * w_dev, group_dev, ngroups, extra_var_dev, above: as for dgp_excess_moments; sigma^2 is s^2 (predicted variance + extra_var),
 *            never a panel's diagonal;
 * panel_rows a positive multiple of 128; the pass uses min(panel_rows, M) rows.  Short panels cost time: every group of 8
 *            levels produces all panels again, and a panel launch has only the parallelism of its own rows;
 * mean_dev sites x nlevels x ngroups, cov_dev_out sites x nlevels x ngroups x ngroups, total_dev sites x ngroups doubles.
 * work_dev: dgp_posterior_excess_moments_workspace_bytes(p, m, ngroups, nlevels, panel_rows) bytes, 256-byte aligned -- per
 * site the prediction's layout, one panel of min(panel_rows, M) x M plan-dtype elements and
 * M (3 + 6 L + P min(L, 8)) + P doubles (M = padded m, L = nlevels, P = ngroups); 0 for a null plan or bad sizes.
 * Launches (gridDim.z = sites, one stream), no floating-point atomics: the prediction's front end, dgp_excess_moments' init and
 * prep, then per group of up to 8 levels a zero launch, per panel (ascending) the panel's production ONCE and the pair launches
 * of the group against it (2 levels per launch, one for an odd last level), and one reduce.  Every sum runs in a fixed order:
 * repeated calls are bitwise equal, and a site's numbers do not depend on its batch; another panel_rows regroups the sums over
 * j (agreement to rounding).  The plan's A, T, K^^-1 and alpha stay bitwise intact.
 * DGP_E_ARG: null arguments, bad sizes (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nlevels <= 64), panel_rows not a positive
 * multiple of 128, above not 0 / 1, a misaligned work area; DGP_E_WORKSPACE: work area missing or too small; DGP_E_STATE: no
 * factorisation, or a failed one -- all before any launch. */
size_t dgp_posterior_excess_moments_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups, int nlevels, int panel_rows);
int dgp_posterior_excess_moments(dgp_plan* p, const double* theta, const void* Xs_dev, int64_t m, const void* mu_dev,
                                 const double* scale2_dev, const double* thresh_dev, int nlevels, const double* w_dev,
                                 const int32_t* group_dev, int ngroups, const void* extra_var_dev, int above, int panel_rows,
                                 void* work_dev, size_t work_bytes, double* mean_dev, double* cov_dev_out, double* total_dev,
                                 void* stream);

/* STREAMED VALUE OF ADDITIONAL SAMPLES: dgp_sample_value's gain map and v'_c (dgp_hip.h: its notation -- f ~ N(mu, C), groups,
 * A_i, conditioning rows B with C' = C - B^T B, v'_c, b_ic, the series of nterms terms -- and its outputs) of the plan's
 * posterior at Xs, straight from the factorisation the plan holds: C = K(Xs, Xs) - V^T V is produced panel_rows rows at a time
 * and never stored whole.
 * p, theta, Xs_dev, m and the padding: as for dgp_posterior_exceedance_moments (batched and ragged plans: one call for all
 *            sites, every array with a leading site dimension);
 * a_dev      A_i, sites x m doubles;   scale2_dev: s^2, one double per site;   group_dev, ngroups: as for dgp_sample_value;
 * obs_var_dev null or sites x m in the plan's dtype (tau_c^2);   rows_dev: null or sites x nrows x m doubles, 0 <= nrows <= 64;
 * panel_rows a positive multiple of 128; the pass uses min(panel_rows, M) rows;
 * gain_dev   sites x ngroups x m doubles, var_dev sites x m doubles (v'_c; 0 where it is not > 0: such a candidate has gain 0;
 *            NaN in, NaN out for that candidate alone).
 * C_cc is the PREDICTED variance (dgp_predict's), in v'_c and as the diagonal entry of the sums, never a panel's diagonal.
 * work_dev: dgp_posterior_sample_value_workspace_bytes(p, m, ngroups, nrows, nterms, panel_rows) bytes, 256-byte aligned -- per
 * site the prediction's layout, one panel of min(panel_rows, M) x M plan-dtype elements and M (2 + P K) + P doubles (M = padded
 * m, P = ngroups, K = nterms: the power sums S[p][k][c]); 0 for a null plan or bad sizes.  Its contents before the call do not
 * matter.
 * Launches (gridDim.z = sites, one stream), no floating-point atomics: the prediction's front end, init and prep, per panel
 * (ascending) the panel's production and one sums launch -- every ordered pair (day i, candidate c) lies in exactly one panel:
 * the one that holds row max(i, c) --, one fold.  Every sum runs in a fixed order: repeated calls are bitwise equal, and a
 * site's numbers do not depend on its batch; another panel_rows regroups the sums over the days (agreement to rounding).  The
 * plan's A, T, K^^-1 and alpha stay bitwise intact.
 * DGP_E_ARG: null arguments (rows_dev with nrows > 0), bad sizes (1 <= m <= 2^20, 1 <= ngroups <= 65535, 0 <= nrows <= 64,
 * 1 <= nterms <= 64), panel_rows not a positive multiple of 128, a misaligned work area; DGP_E_WORKSPACE: work area missing or
 * too small; DGP_E_STATE: no factorisation, or a failed one -- all before any launch. */
size_t dgp_posterior_sample_value_workspace_bytes(const dgp_plan* p, int64_t m, int ngroups, int nrows, int nterms, int panel_rows);
int dgp_posterior_sample_value(dgp_plan* p, const double* theta, const void* Xs_dev, int64_t m, const double* a_dev,
                               const double* scale2_dev, const int32_t* group_dev, int ngroups, const void* obs_var_dev,
                               const double* rows_dev, int nrows, int nterms, int panel_rows, void* work_dev, size_t work_bytes,
                               double* gain_dev, double* var_dev, void* stream);

/* COLUMNS OF THE POSTERIOR COVARIANCE: cols_dev[site][t][i] = C[i][idx[t]] = k(x_i, x_c) - sum_n V[n][i] V[n][c], c = idx[t], for
 * 1 <= ncols <= 64 point indices (idx_dev: sites x ncols int32 in 0 .. m-1; an index outside is clamped), as sites x ncols x m
 * doubles, from the same front end -- what the host needs to build conditioning rows without the dense matrix.  The sum runs in
 * double in ascending n.  work_dev: dgp_posterior_cov_columns_workspace_bytes(p, m, ncols) bytes, 256-byte aligned (the
 * prediction's layout plus d x 128 + m plan-dtype elements per site); 0 for a null plan or bad sizes.  Errors as above. */
size_t dgp_posterior_cov_columns_workspace_bytes(const dgp_plan* p, int64_t m, int ncols);
int dgp_posterior_cov_columns(dgp_plan* p, const double* theta, const void* Xs_dev, int64_t m, const int32_t* idx_dev, int ncols,
                              void* work_dev, size_t work_bytes, double* cols_dev, void* stream);

/* PERIOD MOMENTS OF A LOW-RANK COVARIANCE: dgp_period_moments (its modes, mu, scale2, w, group, outputs; no extra_var) on
 * R = B^T B without ever forming R.  rows_dev: B, batch x nrows x m doubles, 1 <= nrows <= 64; mu_dev batch x m DOUBLES.
 *   a_i = w_i exp(mu_i + s^2 R_ii / 2), mean[g] = sum a_i, cov[g][h] = sum a_i a_j expm1(s^2 R_ij)      (mode 1)
 *   mean[g] = sum w_i mu_i, cov[g][h] = s^2 sum w_i w_j R_ij                                            (mode 0)
 * Stateless (no plan).  work_dev: dgp_period_moments_workspace_bytes(m, ngroups, batch) bytes.  Deterministic,
 * batch-independent, exactly symmetric output, no floating-point atomics.  DGP_E_ARG: null arguments, bad mode or sizes;
 * DGP_E_WORKSPACE: work area missing or too small. */
int dgp_lowrank_period_moments(int mode, const double* rows_dev, int nrows, int64_t m, int batch, const double* mu_dev,
                               const double* scale2_dev, const double* w_dev, const int32_t* group_dev, int ngroups, void* work_dev,
                               size_t work_bytes, double* mean_dev, double* cov_dev_out, void* stream);

/* A BLOCK OF THE POSTERIOR COVARIANCE: rows [row0, row1) x columns [col0, row1) of C = K(Xs, Xs) - V^T V of the plan's posterior
 * at Xs, straight from the factorisation the plan holds -- a piece of the covariance of a record too long to hold whole, and the
 * band producer of dgp_posterior_window_variances on its own.
 * p, theta, Xs_dev, m and the padding: as for dgp_posterior_exceedance_moments (batched and ragged plans: one call for all
 *            sites, every array with a leading site dimension);
 * row0, row1, col0  multiples of 128 with 0 <= col0 <= row0 < row1 <= M (M = padded m);
 * out_dev    sites x (row1 - row0) x (row1 - col0) in the plan's dtype: out[site][r][c] = C[row0 + r][col0 + c].  128 x 128 tiles
 *            above the diagonal are not written; inside a diagonal tile the entries on and below the diagonal are valid.
 * The launches are dgp_posterior_cov's restricted to the block's tiles -- the same pair evaluator and pad selects, the same tile
 * core with k ascending over all N rows of V -- so an fp64 entry has the bits it has there.
 * work_dev: dgp_posterior_cov_block_workspace_bytes(p, m, row0, row1, col0) bytes, 256-byte aligned (the prediction's layout
 * plus m plan-dtype elements per site); 0 for a null plan or a bad block.
 * DGP_E_ARG: null arguments, 1 <= m <= 2^20 violated, a bad block, a misaligned work area; DGP_E_WORKSPACE: work area missing or
 * too small; DGP_E_STATE: no factorisation, or a failed one -- all before any launch.  The plan's A, T, K^^-1 and alpha stay
 * bitwise intact. */
size_t dgp_posterior_cov_block_workspace_bytes(const dgp_plan* p, int64_t m, int64_t row0, int64_t row1, int64_t col0);
int dgp_posterior_cov_block(dgp_plan* p, const double* theta, const void* Xs_dev, int64_t m, int64_t row0, int64_t row1, int64_t col0,
                            void* work_dev, size_t work_bytes, void* out_dev, void* stream);

/* VARIANCES OF ROLLING-WINDOW MEANS: mean_i and var_i = (W C W^T)_ii of dgp_window_moments (dgp_hip.h: its notation, modes,
 * weights a, window rules and the meaning of mu / scale2), without the M x Q + Q x Q work area and result: per window
 *     var_i = d_i^-2 sum_{j in win_i} b_j ( b_j phi(C_jj) + 2 sum_{l in [lo_i, j)} b_l phi(C_jl) ),   phi = id / expm1(s^2 .)
 * cov_dev    batch x M x M in dtype (0 f64 / 1 f32), the layout of dgp_posterior_cov: entries on and below the diagonal are read,
 *            the diagonal included;   mu_dev batch x m in dtype;   scale2_dev one double per site (mode 1; may be null in mode 0);
 * a_dev      null (= 1) or batch x m doubles >= 0;   lo_dev, hi_dev batch x q int32, both non-decreasing; clamped to [0, m];
 * mean_dev, var_dev  batch x q doubles; an empty window or a zero weight sum gives 0 and 0.
 * work_dev: dgp_window_variances_workspace_bytes(m, q, batch) bytes, 8-byte aligned: 3 M + 3 Q doubles per site (M, Q the padded
 * sizes) and one int per site; 0 for bad sizes.  Stateless (no plan).  Four launches (points, windows, contraction, finish);
 * every sum runs in one owner in a fixed order in double, no floating-point atomics: repeated calls are bitwise equal and a
 * site's numbers do not depend on its batch.
 * DGP_E_ARG: bad dtype / mode, null arguments, bad sizes (1 <= m, q <= 2^20, 1 <= batch <= 1024), a misaligned work area;
 * DGP_E_WORKSPACE: work area missing or too small. */
size_t dgp_window_variances_workspace_bytes(int64_t m, int64_t q, int batch);
int dgp_window_variances(int dtype, int mode, const void* cov_dev, int64_t m, int batch, const void* mu_dev, const double* scale2_dev,
                         const double* a_dev, const int32_t* lo_dev, const int32_t* hi_dev, int64_t q, void* work_dev,
                         size_t work_bytes, double* mean_dev, double* var_dev, void* stream);

/* STREAMED ROLLING-WINDOW VARIANCES: dgp_window_variances of the plan's posterior at Xs, straight from the factorisation the plan
 * holds.  Only a BAND of C = K(Xs, Xs) - V^T V is ever produced: two points share a window only if |j - l| < reach, so the panel
 * of rows [p0, p1) needs the columns [c0, p1), c0 = 128 floor(max(0, p0 - reach + 1) / 128); every unordered pair (j >= l) lies
 * in exactly one panel, j's, and var_i d_i^2 is accumulated panel by panel in ascending order.
 * p, theta, Xs_dev, m and the padding: as for dgp_posterior_exceedance_moments (batched and ragged plans: one call for all
 *            sites, every array with a leading site dimension);
 * mu_dev     sites x m in the plan's dtype (mode 1: the MAPPED mean);   scale2_dev, a_dev, lo_dev, hi_dev, q, mode, mean_dev,
 *            var_dev: as for dgp_window_variances.  C_jj is the PREDICTED variance (dgp_predict's), in b_j and as the diagonal
 *            term, never a panel's diagonal;
 * reach      >= max_i (hi_i - lo_i) over all sites, 1 .. 2^20.  A window that holds more points is detected on the device:
 *            every column index is clamped into the band, so nothing outside it is read, and the call returns DGP_E_ARG
 *            ("a window holds more than reach points") AFTER the pass; the outputs are then unspecified;
 * panel_rows a positive multiple of 128; the pass uses R = min(panel_rows, M) rows.
 * work_dev: dgp_posterior_window_variances_workspace_bytes(p, m, q, reach, panel_rows) bytes, 256-byte aligned -- per site the
 * prediction's layout, one band of R x (R + round_up(reach, 128)) plan-dtype elements and 3 M + 3 Q doubles, plus one int per
 * site; 0 for a null plan or bad sizes.  Its contents before the call do not matter.
 * Launches (gridDim.z = sites, one stream), no floating-point atomics: the prediction's front end, points, windows, per panel
 * (ascending) the band Gram, the band update (dgp_posterior_cov's evaluator and tile core on the band's tiles) and one
 * contraction, then finish; the call synchronises the stream to read the reach flags.  Every sum runs in one owner in a fixed
 * order: repeated calls are bitwise equal and a site's numbers do not depend on its batch; another panel_rows regroups the
 * sums over j (agreement to rounding).  The plan's A, T, K^^-1 and alpha stay bitwise intact.
 * DGP_E_ARG: null arguments, bad mode, bad sizes (1 <= m, q <= 2^20), reach outside 1 .. 2^20, panel_rows not a positive multiple
 * of 128, a misaligned work area; DGP_E_WORKSPACE: work area missing or too small; DGP_E_STATE: no factorisation, or a failed
 * one -- all before any launch; the reach flag alone is raised after the pass. */
size_t dgp_posterior_window_variances_workspace_bytes(const dgp_plan* p, int64_t m, int64_t q, int64_t reach, int panel_rows);
int dgp_posterior_window_variances(dgp_plan* p, const double* theta, const void* Xs_dev, int64_t m, const void* mu_dev,
                                   const double* scale2_dev, const double* a_dev, const int32_t* lo_dev, const int32_t* hi_dev,
                                   int64_t q, int mode, int64_t reach, int panel_rows, void* work_dev, size_t work_bytes,
                                   double* mean_dev, double* var_dev, void* stream);

/* ---- The exact leave-group-out predictive likelihood as a training objective (csrc/dgp_lgo.hip).
 * With S = (K^)^-1, alpha = S r and disjoint folds B_g (rows in no fold and empty folds are allowed):
 *     G_g = S[B_g, B_g],  C_g = G_g^-1,  e_g = C_g alpha[B_g]                         (as dgp_cross_validate)
 *     L_LGO = sum_g [ 1/2 alpha_g^T e_g - 1/2 log|G_g| + b_g / 2 log 2 pi ]           (minus the sum of dgp_cross_validate's lpd)
 *     c = e_g scattered to the rows' own positions,  b = S c,  W = blockdiag(C_g + e_g e_g^T),  M2 = S W S
 *     dL/dtheta_p = 1/2 tr((M2 - b alpha^T - alpha b^T) dK/dtheta_p),  dL/dr = b,  dL/dnoise_i = 1/2 (M2)_ii - b_i alpha_i
 * Folds of one give dgp_loo_fit_step's objective; one fold of every row gives dgp_fit_step's marginal likelihood.
 * dgp_lgo_fit_step has the arguments, shapes and batching of dgp_fit_step plus the folds and a work area.  order_dev / start_dev
 * ([batch][n] / [batch][ngroups + 1] int32), ngroups and max_group are exactly dgp_cross_validate's; the kernels clamp what they
 * read from them.  It runs dgp_fit_step's launches unchanged into a result row of its own, dgp_cross_validate's fold algebra on
 * the inverse (its three routes by max_group) for e_g, log|G_g| and the pivots, and in addition the full blocks W_g; then
 * G = F W (F = S made full; per fold a product on the MFMA tile cores, 128 x 128 tiles when max_group > 64, 64 x 64 otherwise; for
 * max_group = 1 the column scaling of dgp_loo_fit_step), M2 = F G^T, b = S c and the contraction exactly as dgp_loo_fit_step.
 * out_dev: DGP_OUT_* layout with NLL = L_LGO and DTHETA, SUM_DR, DR_W0.., SUM_DNOISE its gradients; QUAD, LOGDET and INFO are those
 * of the factorisation.  A site one of whose G_g is not positive definite reports 1 + the index of the first such fold in its INFO
 * (when the factorisation's own status is 0) and NaN as its value: the return code stays 0 and the other sites are unaffected.
 * The plan holds afterwards exactly what dgp_fit_step with the same arguments leaves.  No floating-point atomics: bitwise
 * repeatable; a site's result does not depend on its batch (at the same max_group, which picks the route).
 * dgp_lgo_value: out2_dev [batch][2] doubles = (L_LGO, info) from the factorisation the plan holds, when the last step left S in it.
 * Work areas: dgp_lgo_workspace_bytes (three N x N matrices per site, the blocks W_g -- N round_up(max_group, 128) doubles per
 * site and one tile of rows -- and dgp_cross_validate's own area) / dgp_lgo_value_workspace_bytes; 0 for a null or float32 plan
 * or bad sizes.  float64 plans, single-site or batched.  Before any launch: DGP_E_ARG (null plan / argument; a float32 plan -- the
 * text says so; ngroups or max_group outside 1 .. n; misaligned work area), DGP_E_WORKSPACE (work area missing or too small),
 * DGP_E_STATE (no inputs / no inverse). */
size_t dgp_lgo_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group);
size_t dgp_lgo_value_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group);
int dgp_lgo_fit_step(dgp_plan* p, const double* theta_host, const void* r_dev, const void* noise_dev, const int32_t* order_dev,
                     const int32_t* start_dev, int ngroups, int64_t max_group, void* work_dev, size_t work_bytes, void* out_dev,
                     void* dr_dev, void* dnoise_dev, void* stream);
int dgp_lgo_value(dgp_plan* p, const int32_t* order_dev, const int32_t* start_dev, int ngroups, int64_t max_group, void* work_dev,
                  size_t work_bytes, void* out2_dev, void* stream);

/* ORTHANT PROBABILITIES (csrc/dgp_orthant.hip): prob[l] ~ P(lo_l <= f <= hi_l componentwise), f ~ N(0, L L^T) in m dimensions -- the
 * distribution function of a period's maximum (lo = -inf) or the survival function of its minimum (hi = +inf) of a latent
 * posterior whose block of the covariance has the lower factor L and whose mean has been subtracted from the limits.  NOT exact:
 * Genz's separation of variables over nshifts randomly shifted Richtmyer rules of npoints points with the tent transform, unbiased,
 * with its own standard error se[l] (the sample standard deviation of the shifts' estimates / sqrt(nshifts)).  The recurrence,
 * its tail rules and its clamps are stated at the head of csrc/dgp_orthant.hip; a host restatement on the same generators and
 * shifts walks the same points.
 * L_dev      the factor as psd_safe_factor leaves it: row-major, leading dimension ld >= M (M = m rounded up to 128), ld even,
 *            16-byte aligned; read inside the lower triangle of the diagonal 128-blocks and in the blocks below the block
 *            diagonal only, rows < M; the sweep stops at m (the pad is never conditioned on);
 * lo_dev, hi_dev  nlevels x m doubles, the CENTRED limits a - mu and b - mu; -inf / +inf allowed; lo > hi anywhere gives 0;
 * gen_dev    m doubles, the rule's generators (frac sqrt(p_i));   shift_dev  nshifts x m doubles in [0, 1): both come from the host;
 * prob_dev, se_dev  nlevels doubles.  An unconstrained level gives exactly 1 and 0.
 * work_dev: dgp_orthant_probability_workspace_bytes(m, nlevels, nshifts, npoints) bytes, 256-byte aligned: per workgroup -- 128
 * points of one (level, shift) -- its y values, round_up(m, 64) x 128 doubles, and one partial sum; 0 for bad sizes.  Its
 * contents before the call do not matter.
 * Two launches (grid = point chunks x shifts x levels, then one reduce), no floating-point atomics, every sum in a fixed order:
 * repeated calls are bitwise equal, and a level's numbers do not depend on the other levels of the call.
 * DGP_E_ARG: null arguments, bad sizes (1 <= m <= 16384, 1 <= nlevels <= 64, 2 <= nshifts <= 64, 1 <= npoints <= 2^20), ld < M or
 * odd, a misaligned factor or work area; DGP_E_WORKSPACE: work area missing or too small -- all before any launch. */
size_t dgp_orthant_probability_workspace_bytes(int64_t m, int nlevels, int nshifts, int64_t npoints);
int dgp_orthant_probability(const double* L_dev, int64_t m, int64_t ld, const double* lo_dev, const double* hi_dev, int nlevels,
                            const double* gen_dev, const double* shift_dev, int nshifts, int64_t npoints, void* work_dev,
                            size_t work_bytes, double* prob_dev, double* se_dev, void* stream);

/* EXCEEDANCE COUNTS AND SPELLS OF JOINT PATHS (csrc/dgp_counts.hip): for f ~ N(0, L L^T) in m dimensions, drawn over the orthant
 * sweep's nshifts randomly shifted Richtmyer rules of npoints points (f = L y, y_i = clamp(Phi^-1(w_i), -38, 38), nothing
 * truncated), per level l and shift s the histograms over the points of
 *   N = #{i : f_i beyond thr[l][i]}  (above != 0: f_i > thr, else f_i < thr; a NaN threshold never counts)   -> count_hist, and
 *   R = the longest run of consecutive such i, a run being broken at i where link[i] == 0                      -> spell_hist.
 * NOT exact: plain integration of an indicator over the rules, unbiased; the host forms pmf, distribution function, moments and
 * their standard errors over the shifts.  The estimator is stated at the head of csrc/dgp_counts.hip; a host restatement on the
 * same generators and shifts reproduces the integers unless a path lies within rounding of a threshold.
 * L_dev, gen_dev, shift_dev  as for dgp_orthant_probability; the tile core loads rows [m, round_up(m, 128)) of the padded buffer
 *            with the last block and discards their products: no value in a row >= m reaches a result;
 * thr_dev    nlevels x m doubles, the CENTRED thresholds u - mu;
 * link_dev   m int32 (link[0] is ignored), or null: every point continues the run of the point before it;
 * count_hist_dev, spell_hist_dev  nlevels x nshifts x (m + 1) int32 each, zeroed by the call; every [l][s] row sums to npoints.
 * work_dev: dgp_path_counts_workspace_bytes(m, nlevels, nshifts, npoints) bytes, 256-byte aligned: per workgroup -- 128 points of
 * one shift and up to 16 levels -- its draws, round_up(m, 128) x 128 doubles; so 1 .. 16 levels cost the same; 0 for bad sizes.
 * One launch after the two memsets (grid = point chunks x shifts x level chunks); integer atomics only: repeated calls give
 * identical integers, and a level's histograms depend neither on the other levels of the call nor on how they are chunked.
 * Errors: those of dgp_orthant_probability (link_dev may be null), all before any launch. */
size_t dgp_path_counts_workspace_bytes(int64_t m, int nlevels, int nshifts, int64_t npoints);
int dgp_path_counts(const double* L_dev, int64_t m, int64_t ld, const double* thr_dev, int nlevels, int above, const int32_t* link_dev,
                    const double* gen_dev, const double* shift_dev, int nshifts, int64_t npoints, void* work_dev, size_t work_bytes,
                    int32_t* count_hist_dev, int32_t* spell_hist_dev, void* stream);

#endif /* DGP_HIP_EXT2_H */
