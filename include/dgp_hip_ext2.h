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

#endif /* DGP_HIP_EXT2_H */
