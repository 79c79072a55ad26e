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

#endif /* DGP_HIP_EXT2_H */
