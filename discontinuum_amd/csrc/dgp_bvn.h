// dgp_bvn.h -- the pair function of the exceedance counts, D(h, k, rho) = Phi2(h, k; rho) - Phi(h) Phi(k), with its tables, and
// the layout of the work area that the dense pass (dgp_exceed.hip) and the streamed one (dgp_exceed_stream.hip) share.  The
// algorithm and its launches are described at the head of dgp_exceed.hip.
#pragma once
#include <cmath>

#include "dgp_common.h"
#include "dgp_models.h"

namespace dgp {

namespace {

constexpr int EX_ROWS = 64;    // rows of a workgroup of the pairs pass (divides DGP_TILE_HOST, the cov buffer's padding)
constexpr int EX_CHUNK = 8;    // most levels a pairs / reduce pass takes at once
constexpr double EX_ZDET = 38.0;  // |z| beyond which a point is decided: Phi(-38) = 3e-316

// per-site work area, in doubles: w[M], 1 / sigma[M], z[L][M], p[L][M], Y[min(L, EX_CHUNK)][M][P], then 2 P ints
__host__ __device__ inline long ex_site_doubles(long M, int P, int L) {
  return 2 * M + 2 * (long)L * M + (long)(L < EX_CHUNK ? L : EX_CHUNK) * M * P + P;
}

// Gauss-Legendre abscissae |x_n| and weights on [-1, 1], one of each +- pair: 6-, 12- and 20-point rules
__constant__ double ex_gl_c[2][19] = {
    {0.932469514203152, 0.6612093864662645, 0.23861918608319693,
     0.9815606342467192, 0.9041172563704748, 0.7699026741943047, 0.5873179542866175, 0.3678314989981802, 0.1252334085114689,
     0.9931285991850949, 0.9639719272779138, 0.9122344282513258, 0.8391169718222188, 0.7463319064601508, 0.636053680726515,
     0.5108670019508271, 0.37370608871541955, 0.2277858511416451, 0.07652652113349734},
    {0.17132449237916975, 0.36076157304813894, 0.46791393457269137,
     0.04717533638651202, 0.10693932599531888, 0.1600783285433461, 0.20316742672306565, 0.23349253653835464, 0.2491470458134027,
     0.017614007139153273, 0.04060142980038622, 0.06267204833410944, 0.08327674157670467, 0.10193011981724026,
     0.11819453196151825, 0.13168863844917653, 0.14209610931838187, 0.14917298647260366, 0.15275338713072578}};
__shared__ double ex_gl[2][19];

// the tables of the pair function (Gauss-Legendre, exp_nonpos); a barrier must follow before the first bvn_excess
__device__ __forceinline__ void ex_tables_init() {
  exp_table_init<double>();
  if (threadIdx.x >= 64 && threadIdx.x < 64 + 38) (&ex_gl[0][0])[threadIdx.x - 64] = (&ex_gl_c[0][0])[threadIdx.x - 64];
}

__device__ __forceinline__ double ex_phi(double x) { return 0.5 * erfc(-0.70710678118654752440 * x); }

// sin and cos of |t| <= 0.6 by their Taylor series (next terms t^17 / 17! < 5e-19, t^16 / 16! < 2e-17)
__device__ __forceinline__ void ex_sincos_small(double t, double& s, double& c) {
  const double q = t * t;
  double ps = -1.0 / 1307674368000.0;
  ps = __builtin_fma(ps, q, 1.0 / 6227020800.0);
  ps = __builtin_fma(ps, q, -1.0 / 39916800.0);
  ps = __builtin_fma(ps, q, 1.0 / 362880.0);
  ps = __builtin_fma(ps, q, -1.0 / 5040.0);
  ps = __builtin_fma(ps, q, 1.0 / 120.0);
  ps = __builtin_fma(ps, q, -1.0 / 6.0);
  s = __builtin_fma(ps * q, t, t);
  double pc = -1.0 / 87178291200.0;
  pc = __builtin_fma(pc, q, 1.0 / 479001600.0);
  pc = __builtin_fma(pc, q, -1.0 / 3628800.0);
  pc = __builtin_fma(pc, q, 1.0 / 40320.0);
  pc = __builtin_fma(pc, q, -1.0 / 720.0);
  pc = __builtin_fma(pc, q, 1.0 / 24.0);
  pc = __builtin_fma(pc, q, -0.5);
  c = __builtin_fma(pc, q, 1.0);
}

// D(h_l, k_l, rho) for the LC levels of a chunk; ph / pk = Phi(h) / Phi(k) as prep left them (read above |rho| = 0.925 only)
template <int LC>
__device__ __forceinline__ void bvn_excess(const double (&h)[LC], const double (&k)[LC], const double (&ph)[LC],
                                           const double (&pk)[LC], double r, double (&D)[LC]) {
  bool live = false;
#pragma unroll
  for (int l = 0; l < LC; ++l) live |= !(fabs(h[l]) > EX_ZDET || fabs(k[l]) > EX_ZDET);
  if (!live) {  // decided at every level (an excluded point, a zero variance)
#pragma unroll
    for (int l = 0; l < LC; ++l) D[l] = 0.0;
    return;
  }
  r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);  // (comparisons: a NaN stays)
  const double ar = fabs(r);
  if (ar < 0.925) {
    const int n0 = ar < 0.3 ? 0 : (ar < 0.75 ? 3 : 9), n1 = ar < 0.3 ? 3 : (ar < 0.75 ? 9 : 19);
    const double asr = asin(r), half = 0.5 * asr;
    double s0, c0;
    ex_sincos_small(half, s0, c0);
    double hk[LC], hs[LC], acc[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) {
      hk[l] = h[l] * k[l];
      hs[l] = 0.5 * (h[l] * h[l] + k[l] * k[l]);
      acc[l] = 0.0;
    }
    for (int n = n0; n < n1; ++n) {
      double st, ct;
      ex_sincos_small(half * ex_gl[0][n], st, ct);
      const double wn = ex_gl[1][n];
      const double sa = s0 * ct, sb = c0 * st, ca = c0 * ct, cb = s0 * st;
      const double snp = sa + sb, csp = ca - cb, snm = sa - sb, csm = ca + cb;  // the angles half (1 + x), half (1 - x)
      const double ip = 1.0 / (csp * csp), im = 1.0 / (csm * csm);
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        const double e = exp_nonpos(__builtin_fma(snp, hk[l], -hs[l]) * ip) + exp_nonpos(__builtin_fma(snm, hk[l], -hs[l]) * im);
        acc[l] = __builtin_fma(wn, e, acc[l]);
      }
    }
#pragma unroll
    for (int l = 0; l < LC; ++l) D[l] = acc[l] * asr * 0.07957747154594767280;  // 1 / (4 pi)
  } else {
    const bool neg = r < 0.0;
    double kk[LC], hk[LC], bvn[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) {
      kk[l] = neg ? -k[l] : k[l];
      hk[l] = h[l] * kk[l];
      bvn[l] = 0.0;
    }
    if (ar < 1.0) {
      const double as = (1.0 - ar) * (1.0 + ar), a = sqrt(as), ias = 1.0 / as;
      double bs[LC], c[LC], d[LC];
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        const double df = h[l] - kk[l];
        bs[l] = df * df;
        c[l] = (4.0 - hk[l]) * 0.125;
        d[l] = (12.0 - hk[l]) * 0.0625;
        const double asr = -0.5 * (bs[l] * ias + hk[l]);
        if (asr > -100.0)
          bvn[l] = a * exp(asr) * (1.0 - c[l] * (bs[l] - as) * (1.0 - d[l] * bs[l] * 0.2) * (1.0 / 3.0) + c[l] * d[l] * as * as * 0.2);
        if (hk[l] > -100.0) {
          const double b = sqrt(bs[l]);
          bvn[l] -= exp(-0.5 * hk[l]) * 2.50662827463100050242 * ex_phi(-b / a) * b *
                    (1.0 - c[l] * bs[l] * (1.0 - d[l] * bs[l] * 0.2) * (1.0 / 3.0));
        }
      }
      const double a2 = 0.5 * a;
      for (int n = 9; n < 19; ++n) {
        const double xn = ex_gl[0][n], wn = a2 * ex_gl[1][n];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          const double ax = a2 * (sg ? 1.0 + xn : 1.0 - xn);
          const double xs = ax * ax, rs = sqrt(1.0 - xs), ixs = 1.0 / xs, irs = 1.0 / rs;
          const double q = -0.5 * xs / ((1.0 + rs) * (1.0 + rs));
#pragma unroll
          for (int l = 0; l < LC; ++l) {
            const double asr = -0.5 * (bs[l] * ixs + hk[l]);
            if (asr > -100.0) bvn[l] += wn * exp(asr) * (exp(hk[l] * q) * irs - (1.0 + c[l] * xs * (1.0 + d[l] * xs)));
          }
        }
      }
#pragma unroll
      for (int l = 0; l < LC; ++l) bvn[l] *= -0.15915494309189533577;  // -1 / (2 pi)
    }
#pragma unroll
    for (int l = 0; l < LC; ++l) {
      double v;
      if (!neg) {
        v = bvn[l] + (ph[l] < pk[l] ? ph[l] : pk[l]);
      } else {
        v = -bvn[l];
        if (k[l] > -h[l]) v += (ph[l] + pk[l]) - 1.0;
      }
      D[l] = v - ph[l] * pk[l];
    }
  }
#pragma unroll
  for (int l = 0; l < LC; ++l) {
    if (h[l] != h[l] || k[l] != k[l] || r != r) D[l] = __builtin_nan("");
    if (fabs(h[l]) > EX_ZDET || fabs(k[l]) > EX_ZDET) D[l] = 0.0;
  }
}

__device__ __forceinline__ double ex_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ void ex_range(const int* se, int g, int& c0, int& c1) {
  c0 = se[2 * g];
  c1 = se[2 * g + 1];
  if (c1 <= c0) c0 = c1 = 0;  // empty group (start still INT_MAX)
}

struct ExWork {  // the parts of a site's work area
  double *w, *sinv, *z, *p, *Y;
  int* se;
  __device__ ExWork(double* work, long ws, long M, int P, int L) {
    w = work + (long)blockIdx.z * ws;
    sinv = w + M;
    z = sinv + M;
    p = z + (long)L * M;
    Y = p + (long)L * M;
    se = (int*)(Y + (long)(L < EX_CHUNK ? L : EX_CHUNK) * M * P);
  }
};

}  // namespace

}  // namespace dgp
