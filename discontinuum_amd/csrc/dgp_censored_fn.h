// dgp_censored_fn.h -- the pointwise functions of the censored likelihoods, shared by the Laplace fit (dgp_censored.hip) and
// the cross-validation of a censored fit (dgp_censored_cv.hip).  Device code only; every function is evaluated exactly as the
// fit evaluates it (the debug-terms entries compare them bitwise).
#pragma once
#include "dgp_common.h"

namespace dgp {

// ---- the four functions of z.  Negative side through erfcx (no underflow, no cancellation in Phi), positive side through
// erfc / log1p.  q = h (z + h) and c3 = h [1 - (z + h)(z + 2 h)] inherit the cancellation of z + h for z << 0 (relative
// error ~ z^2 eps).
struct CenFn {
  double logphi, h, q, c3;
};
__device__ __forceinline__ CenFn cen_fn(double z) {
  CenFn o;
  if (z < 0.0) {
    const double e = erfcx(-z * 0.70710678118654752440);
    o.h = 0.79788456080286535588 / e;
    o.logphi = -0.5 * z * z + log(0.5 * e);
  } else {
    const double tail = 0.5 * erfc(z * 0.70710678118654752440);
    o.h = 0.39894228040143267794 * exp(-0.5 * z * z) / (1.0 - tail);
    o.logphi = log1p(-tail);
  }
  const double zh = z + o.h;
  o.q = o.h * zh;
  o.c3 = o.h * (1.0 - zh * (zh + o.h));
  return o;
}
__device__ __forceinline__ double cen_logphi(double z) {
  if (z < 0.0) return -0.5 * z * z + log(0.5 * erfcx(-z * 0.70710678118654752440));
  return log1p(-0.5 * erfc(z * 0.70710678118654752440));
}

// ---- interval-censored rows (side 2): the truth lies in [y, upper], standardised [za, zb], Delta = zb - za > 0.
//     P = Phi(zb) - Phi(za),  ra = phi(za) / P,  rb = phi(zb) / P
//     log p = log P,   mu = sigma g = ra - rb,   wv = W v = zb rb - za ra + mu^2  in (0, 1],
//     d3 = sigma^3 d^3 log p / d f^3 = ra (za^2 - 1) - rb (zb^2 - 1) - mu (za ra - zb rb) + 2 mu wv
// = mean, 1 - variance and third central moment of a standard normal truncated to [za, zb].  None of this can be evaluated as
// written (P underflows and cancels in a tail; for Delta << 1 wv is a sum of O(1 / Delta^2) terms).  A bracket whose centre c lies
// right of 0 is reflected (mu and d3 change sign); then, with h = Delta / 2,
//   narrow    h <= 1 and |c| h <= 2:  P = h phi(c) I,  I = int_-1^1 exp(-c h t - h^2 t^2 / 2) dt by a fixed 12-point Gauss-Legendre
//             rule (its error for these exponents is below 1e-18); mu = c + h E[t], wv = 1 - h^2 Var[t], d3 = h^3 E[(t - E t)^3]
//             with the central moments taken about the computed mean: nothing cancels as Delta -> 0
//   tail      zb <= 0 (then |c| h > 1):  P = phi(zb) D,  D = M(zb) - rho M(za),  M = Phi / phi = sqrt(pi / 2) erfcx(-z / sqrt 2),
//             rho = phi(za) / phi(zb) = exp(Delta c) <= e^-2: D does not cancel; rb = 1 / D, ra = rho / D, mu = expm1(Delta c) / D
//   straddle  za < 0 < zb (then h > 1):  P = [erf(zb / sqrt 2) + erf(-za / sqrt 2)] / 2, a sum of positive terms
// The tail's wv and d3 keep the cancellation of the one-sided functions above (relative error ~ z^2 eps and z^3 eps).
struct IntFn {
  double logp, mu, wv, d3;
};
constexpr double IV_T[6] = {0.12523340851146891547, 0.36783149899818019375, 0.58731795428661744730,
                            0.76990267419430468704, 0.90411725637047485668, 0.98156063424671925069};
constexpr double IV_W[6] = {0.24914704581340278500, 0.23349253653835480876, 0.20316742672306592175,
                            0.16007832854334622633, 0.10693932599531843096, 0.04717533638651182719};
#define IV_LOGSQRT2PI 0.91893853320467274178
#define IV_NARROW_H 1.0
#define IV_NARROW_A 2.0
// the reflected bracket [a, b] with centre c <= 0; -> true when the caller's bracket was reflected
__device__ __forceinline__ bool iv_reflect(double za, double zb, double delta, double& a, double& b, double& c) {
  const bool flip = za + zb > 0.0;
  a = flip ? -zb : za;
  b = flip ? -za : zb;
  c = flip ? -(za + 0.5 * delta) : za + 0.5 * delta;
  return flip;
}
// the weighted integrand at the twelve nodes (fully unrolled: registers) and its sum
__device__ __forceinline__ double iv_nodes(double c, double h, double (&f)[12]) {
  const double p = -c * h, q = -0.5 * h * h;
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double t = IV_T[k], qt = q * t * t;
    f[2 * k] = IV_W[k] * exp(qt + p * t);
    f[2 * k + 1] = IV_W[k] * exp(qt - p * t);
    tot += f[2 * k] + f[2 * k + 1];
  }
  return tot;
}
__device__ __forceinline__ double iv_logp(double za, double zb, double delta) {
  double a, b, c;
  (void)iv_reflect(za, zb, delta, a, b, c);
  const double h = 0.5 * delta;
  if (h <= IV_NARROW_H && -c * h <= IV_NARROW_A) {
    double f[12];
    return log(h) - 0.5 * c * c - IV_LOGSQRT2PI + log(iv_nodes(c, h, f));
  }
  if (b <= 0.0) {
    const double D = 1.25331413731550025121 * (erfcx(-b * 0.70710678118654752440) - exp(delta * c) * erfcx(-a * 0.70710678118654752440));
    return -0.5 * b * b - IV_LOGSQRT2PI + log(D);
  }
  return log(0.5 * (erf(b * 0.70710678118654752440) + erf(-a * 0.70710678118654752440)));
}
__device__ __forceinline__ IntFn iv_fn(double za, double zb, double delta) {
  IntFn o;
  double a, b, c;
  const bool flip = iv_reflect(za, zb, delta, a, b, c);
  const double h = 0.5 * delta;
  if (h <= IV_NARROW_H && -c * h <= IV_NARROW_A) {
    double f[12];
    const double tot = iv_nodes(c, h, f);
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s1 += IV_T[k] * (f[2 * k] - f[2 * k + 1]);
    const double m1 = s1 / tot;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double dp = IV_T[k] - m1, dm = -IV_T[k] - m1;
      s2 += f[2 * k] * dp * dp + f[2 * k + 1] * dm * dm;
      s3 += f[2 * k] * dp * dp * dp + f[2 * k + 1] * dm * dm * dm;
    }
    o.logp = log(h) - 0.5 * c * c - IV_LOGSQRT2PI + log(tot);
    o.mu = c + h * m1;
    o.wv = 1.0 - h * h * (s2 / tot);
    o.d3 = h * h * h * (s3 / tot);
  } else {
    double ra, rb;
    if (b <= 0.0) {
      const double e1 = expm1(delta * c), rho = 1.0 + e1;
      const double D = 1.25331413731550025121 * (erfcx(-b * 0.70710678118654752440) - rho * erfcx(-a * 0.70710678118654752440));
      ra = rho / D;
      rb = 1.0 / D;
      o.mu = e1 / D;
      o.logp = -0.5 * b * b - IV_LOGSQRT2PI + log(D);
    } else {
      const double P = 0.5 * (erf(b * 0.70710678118654752440) + erf(-a * 0.70710678118654752440));
      ra = exp(-0.5 * a * a - IV_LOGSQRT2PI) / P;
      rb = exp(-0.5 * b * b - IV_LOGSQRT2PI) / P;
      o.mu = ra - rb;
      o.logp = log(P);
    }
    const double A = b * rb - a * ra;
    o.wv = fmin(A + o.mu * o.mu, 1.0);
    o.d3 = ra * (a * a - 1.0) - rb * (b * b - 1.0) + o.mu * A + 2.0 * o.mu * o.wv;
  }
  if (flip) {
    o.mu = -o.mu;
    o.d3 = -o.d3;
  }
  return o;
}

}  // namespace dgp
