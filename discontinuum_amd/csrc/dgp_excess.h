// dgp_excess.h -- what the dense excess pass (dgp_excess.hip) and its panel cut (dgp_excess_stream.hip) share: the layout of a
// site's work area, what the pair function reads of a point, and the pair function itself (n_ij of dgp_excess.hip's header).
#pragma once
#include "dgp_bvn.h"

namespace dgp {

constexpr int XS_CHUNK = 2;  // most levels a pairs launch takes at once: 4 tilts each in bvn_excess's 8 slots
constexpr int XS_GROUP = 8;  // levels of Y in the streamed pass: the pairs launches of a group share every panel

// per-site work area, in doubles: W[M], sigma[M], 1 / sigma[M], then h0, kappa, A0, A1, E, V as [L][M] each,
// Y[min(L, YL)][M][P], then 2 P ints.  YL = XS_CHUNK for the dense pass, XS_GROUP for the streamed one
__host__ __device__ inline long xs_site_doubles(long M, int P, int L, int YL) {
  return 3 * M + 6 * (long)L * M + (long)(L < YL ? L : YL) * M * P + P;
}

struct XsWork {  // the parts of a site's work area
  double *W, *sig, *sinv, *h0, *kap, *A0, *A1, *E, *V, *Y;
  int* se;
  __device__ XsWork(double* work, long ws, long M, int P, int L, int YL) {
    W = work + (long)blockIdx.z * ws;
    sig = W + M;
    sinv = sig + M;
    h0 = sinv + M;
    kap = h0 + (long)L * M;
    A0 = kap + (long)L * M;
    A1 = A0 + (long)L * M;
    E = A1 + (long)L * M;
    V = E + (long)L * M;
    Y = V + (long)L * M;
    se = (int*)(Y + (long)(L < YL ? L : YL) * M * P);
  }
};

template <int LV>
struct XsPoint {  // what the pair function reads of a point: sigma, 1 / sigma and, per level of the chunk, h0, kappa, A0, A1
  double s, sinv, h[LV], kap[LV], a0[LV], a1[LV];
  __device__ __forceinline__ void load(const XsWork& wk, long M, int l0, long i) {
    s = wk.sig[i];
    sinv = wk.sinv[i];
#pragma unroll
    for (int l = 0; l < LV; ++l) {
      const long o = (long)(l0 + l) * M + i;
      h[l] = wk.h0[o];
      kap[l] = wk.kap[o];
      a0[l] = wk.A0[o];
      a1[l] = wk.A1[o];
    }
  }
};

// n_ij of dgp_excess.hip's header for the LV levels of a chunk; cij = C_ij s^2 as loaded
template <int LV>
__device__ __forceinline__ void xs_pair(double sg, const XsPoint<LV>& pi, const XsPoint<LV>& pj, double cij, double (&out)[LV]) {
  constexpr int LC = 4 * LV;
  double r = cij * pi.sinv * pj.sinv;
  r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);  // (comparisons: a NaN stays)
  const double ec = exp(r * pi.s * pj.s);
  const double ti = sg * pi.s, tj = sg * pj.s, ui = (sg * r) * pj.s, uj = (sg * r) * pi.s;
  double h[LC], k[LC], ph[LC], pk[LC], D[LC];
#pragma unroll
  for (int l = 0; l < LV; ++l) {  // slots 4 l + (00, 10, 01, 11)
    const double hi = pi.h[l], kj = pj.h[l];
    h[4 * l] = hi;
    k[4 * l] = kj;
    ph[4 * l] = pi.a0[l];
    pk[4 * l] = pj.a0[l];
    h[4 * l + 1] = hi + ti;
    k[4 * l + 1] = kj + uj;
    ph[4 * l + 1] = pi.a1[l];
    pk[4 * l + 1] = ex_phi(k[4 * l + 1]);
    h[4 * l + 2] = hi + ui;
    k[4 * l + 2] = kj + tj;
    ph[4 * l + 2] = ex_phi(h[4 * l + 2]);
    pk[4 * l + 2] = pj.a1[l];
    h[4 * l + 3] = hi + ti + ui;
    k[4 * l + 3] = kj + tj + uj;
    ph[4 * l + 3] = ex_phi(h[4 * l + 3]);
    pk[4 * l + 3] = ex_phi(k[4 * l + 3]);
  }
  bvn_excess<LC>(h, k, ph, pk, r, D);
#pragma unroll
  for (int l = 0; l < LV; ++l) {
    const double ki = pi.kap[l], kj = pj.kap[l];
    const double dpart = (ec * D[4 * l + 3] - kj * D[4 * l + 1]) - ki * D[4 * l + 2] + (ki * kj) * D[4 * l];
    const double bracket = (ec * ph[4 * l + 3] * pk[4 * l + 3] - pi.a1[l] * pj.a1[l]) -
                           kj * pi.a1[l] * (pk[4 * l + 1] - pj.a0[l]) - ki * pj.a1[l] * (ph[4 * l + 2] - pi.a0[l]);
    out[l] = dpart + bracket;
  }
}

}  // namespace dgp
