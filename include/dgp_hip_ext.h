/* dgp_hip_ext.h -- entry points of libdgp_hip.so declared beside dgp_hip.h, which includes this file inside its extern "C"
 * block: include dgp_hip.h, never this file alone.  Bound through _lib.EXT_SIGNATURES. */
#ifndef DGP_HIP_EXT_H
#define DGP_HIP_EXT_H

/* THRESHOLD EXCESS: exact mean and covariance of the period sums of the excess (or deficit) of a log-transformed latent
 * posterior over per-point thresholds -- the mass above an allowable load, a flood volume above bankfull, a deficit volume
 * below a low-flow threshold.  f ~ N(mu, C) over m points, f' = s f + t, c_i = exp(f'_i); per level l a data-space threshold
 * tau_il = exp(a_il); with m_i the mapped mean, v_i = s^2 (C_ii + extra_var_i), sigma_i = sqrt(v_i), c_ij = s^2 C_ij,
 * rho = c_ij / (sigma_i sigma_j), M_i = m_i + v_i / 2, kappa_i = tau_i exp(-M_i):
 *   above = 1: e_i = max(c_i - tau_i, 0);   above = 0: e_i = max(tau_i - c_i, 0),
 *   E e_i = exp(M_i) (Phi(h1) - kappa Phi(h0)),  h0 = (m_i - a_i) / sigma_i,  h1 = h0 + sigma_i   (above; Phi(-.) and the sign
 *   turned for the deficit),
 *   E e_i e_j = exp(M_i + M_j) (exp(c_ij) P11 - kappa_j P10 - kappa_i P01 + kappa_i kappa_j P00),
 *   P_tu = Phi2((m_i + t v_i + u c_ij - a_i) / sigma_i, (m_j + u v_j + t c_ij - a_j) / sigma_j; rho)   (opposite orthants for
 *   the deficit), each Phi2 taken as (Phi2 - Phi Phi) + Phi Phi with the first part from the exceedance counts' pair function,
 *   mean[l][g] = sum_{i in g} w_i E e_il,   cov[l][g][h] = sum_{i in g} sum_{j in h} w_i w_j Cov(e_il, e_jl),
 *   total[g] = sum_{i in g} w_i exp(M_i)   (the period's expected sum of w_i c_i).
 * The pair value is computed normalised by exp(M_i + M_j) and w_i exp(M_i) applied as a weight, so loads in kg do not overflow.
 * dtype, cov_dev, m, batch, w_dev, group_dev, ngroups, extra_var_dev and the padding: as for dgp_period_moments (extra_var is
 *            in model space and added to the diagonal of C; only the lower triangle of cov_dev is read; everything after the
 *            loads of C and mu is double; a violated group order gives wrong numbers, never an access out of bounds);
 * mu_dev     the MAPPED mean s mu + t, batch x m, in dtype;   scale2_dev: s^2, one double per site;
 * thresh_dev batch x nlevels x m doubles, a = ln tau; -inf (tau = 0) and +inf allowed.
 * A point is DECIDED at a level when v_i <= 0 (e_i = max(+-(exp(m_i) - tau_i), 0), no covariance with any point), when
 * a = -inf (the excess is c_i itself: the lognormal moments of dgp_period_moments; the deficit is 0) or when a = +inf (the
 * excess is 0; the deficit is infinite: mean +inf, covariances NaN).  An excluded point (group -1) contributes nothing; a NaN
 * in a point's inputs reaches every number the point enters.
 * mean_dev batch x nlevels x ngroups, cov_dev_out batch x nlevels x ngroups x ngroups, total_dev batch x ngroups doubles.
 * work_dev: dgp_excess_moments_workspace_bytes(m, ngroups, nlevels, batch) bytes, 256-byte aligned -- per site
 * M (3 + 6 L + P min(L, 2)) + P doubles (M = padded m, L = nlevels, P = ngroups); 0 for bad sizes.
 * Launches (gridDim.z = batch), no floating-point atomics: an init and a prep once, then a pairs and a reduce launch per chunk
 * of two levels (one for a last odd level).  Every sum runs in a fixed order: bitwise repeatable, and a site's numbers do not
 * depend on its batch.  Needs no plan.  DGP_E_ARG: dtype, null arguments, bad sizes (1 <= m <= 2^20, 1 <= ngroups <= 65535,
 * 1 <= nlevels <= 64, 1 <= batch <= 1024), above not 0 / 1, a misaligned work area; DGP_E_WORKSPACE: work area missing or too
 * small -- all before any launch. */
size_t dgp_excess_moments_workspace_bytes(int64_t m, int ngroups, int nlevels, int batch);
int dgp_excess_moments(int dtype, const void* cov_dev, int64_t m, int batch, const void* mu_dev, const double* scale2_dev,
                       const double* thresh_dev, const double* w_dev, const int32_t* group_dev, int ngroups, int nlevels,
                       const void* extra_var_dev, int above, void* work_dev, size_t work_bytes, double* mean_dev,
                       double* cov_dev_out, double* total_dev, void* stream);

#endif /* DGP_HIP_EXT_H */
