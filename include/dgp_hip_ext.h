/* dgp_hip_ext.h -- entry points of libdgp_hip.so added after the host layer's contract (tests/abi_contract.json: every workspace
 * size and every refusal of the entries in dgp_hip.h, exact) was recorded.  They follow every convention of dgp_hip.h -- which
 * includes this file, so that callers see one header -- and are outside the recorded table: their own tests check their sizes and
 * refusals (python: discontinuum_amd/_lib.py::EXT_SIGNATURES).  Do not include this file directly.
 */
#ifndef DGP_HIP_EXT_H
#define DGP_HIP_EXT_H
#ifndef DGP_HIP_H
#error "include dgp_hip.h"
#endif

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

#endif /* DGP_HIP_EXT_H */
