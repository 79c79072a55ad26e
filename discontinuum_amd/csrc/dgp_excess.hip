// dgp_excess.hip -- exact moments of the excess (or deficit) of a log-transformed Gaussian posterior over a threshold, summed per
// period (dgp_excess_moments): the mass above an allowable load, a flood volume above bankfull, a low-flow deficit volume.
//
// f ~ N(mu, C) over m points, f' = s f + t, c_i = exp(f'_i); per level l a data-space threshold tau_il = exp(a_il), weights w_i
// and group ids g_i (non-decreasing, -1 = excluded).  With m_i the mapped mean, v_i = s^2 (C_ii + extra_var_i),
// sigma_i = sqrt(v_i), c_ij = s^2 C_ij, rho = c_ij / (sigma_i sigma_j), M_i = m_i + v_i / 2, kappa_i = tau_i exp(-M_i) and the
// sign sg = +1 for the excess e_i = (c_i - tau_i)^+, -1 for the deficit e_i = (tau_i - c_i)^+, everything below is NORMALISED by
// exp(M_i) (exp(M_i + M_j) for a pair) and W_i = w_i exp(M_i) is applied as a weight, so loads in kg do not overflow:
//     h0_i = sg (m_i - a_i) / sigma_i,  A0 = Phi(h0),  A1 = Phi(h0 + sg sigma_i),  A2 = Phi(h0 + 2 sg sigma_i),
//     E_i  = E e_i / exp(M_i) = sg (A1 - kappa A0),
//     V_i  = Var e_i / exp(2 M_i) = exp(v_i) A2 - 2 kappa A1 + kappa^2 A0 - E_i^2          (the pair formula at i = j, rho = 1),
//     n_ij = Cov(e_i, e_j) / exp(M_i + M_j) = exp(c_ij) P11 - kappa_j P10 - kappa_i P01 + kappa_i kappa_j P00 - E_i E_j,
//     P_tu = Phi2(h_tu, k_tu; rho),  h_tu = h0_i + sg (t sigma_i + u rho sigma_j),  k_tu = h0_j + sg (u sigma_j + t rho sigma_i)
// (the tilted means of Black-Scholes type; the sign turns both arguments, i.e. takes the opposite orthant, for the deficit).
//     mean_g = sum_{i in g} W_i E_i,   cov_gh = sum_{i in g} sum_{j in h} W_i W_j n_ij  (V_i on the diagonal),   total_g = sum W_i.
//
// The FOUR-TERM form is taken, arranged so that no Phi2 is formed: with D = Phi2 - Phi Phi from bvn_excess (dgp_bvn.h, the pair
// function of the exceedance counts, which subtracts nothing below |rho| = 0.925),
//     n_ij = [exp(c) D11 - kappa_j D10 - kappa_i D01 + kappa_i kappa_j D00]
//          + [exp(c) Phi(h11) Phi(k11) - A1_i A1_j - kappa_j A1_i (Phi(k10) - A0_j) - kappa_i A1_j (Phi(h01) - A0_i)];
// the second bracket is sum coef Phi(h) Phi(k) - E_i E_j after its kappa_i kappa_j terms have cancelled exactly (h10 = h1_i,
// k01 = h1_j, h00 = h0_i, k00 = h0_j); it vanishes at rho = 0 and loses relative, not absolute, accuracy.  The four orthant
// probabilities of a pair share rho, so they go into bvn_excess's slots -- (4 tilts) x (levels of the chunk): LC = 8 is two
// levels, LC = 4 one -- and the rho-dependent node work is done once per pair.
//
// A point is DECIDED at a level when its probability mass cannot reach the threshold's side: v_i <= 0 (h0 = +-inf by the sign
// of m_i - a_i, a tie counts as no excess; sigma = 0, so rho = 0 and c_ij = 0 with every point), a = -+inf, or h0 + 2 sg sigma
// below -EX_ZDET (then h0 = -inf and kappa = 0: the point adds nothing).  a = -inf with sg = +1 is the lognormal itself:
// h0 = +inf, kappa = 0, n_ij = exp(c_ij) Phi(k11) - ... reduces to the covariance of dgp_period_moments.  a = +inf with
// sg = -1 is an infinite deficit: mean +inf, covariances NaN.  An excluded point (group -1) and the padding carry W = 0,
// h0 = -inf, kappa = 0, sigma = 0; a NaN in a point's inputs stays a NaN.
//
// Launches (gridDim.z = sites), no floating-point atomics: a tiny init and a prep once, then per chunk of levels
//   prep    one thread per point: W_i, sigma_i, 1 / sigma_i; h0, kappa, A0, A1, E and V for every level; each group's column range.
//   pairs   one workgroup per (64-row block, group h): Y[l][i][h] = sum_j W_j n_ij over the j of h that the reduce needs -- j < i
//           for g(i) = h, read as C[i][j] (a wave per row, lanes along j); all j of h for g(i) < h, read as C[j][i] (lanes
//           along i, the four waves take every fourth j); nothing for g(i) > h.  Every unordered pair is evaluated once.
//   reduce  one workgroup per (64 columns h, level, group g): cov_gh = sum_{i in g} W_i Y[l][i][h] for h > g, twice that plus
//           sum_i W_i^2 V_i for h = g, written to (g, h) and (h, g) from one value; mean_g and (level 0) total_g beside it.
// Every sum runs in a fixed order: bitwise repeatable, and a site's numbers do not depend on its batch.  All arithmetic after
// the loads of C and mu is double.
//
// The work area's layout, XsPoint and the pair function xs_pair live in dgp_excess.h, shared with the panel cut of the pairs pass
// (dgp_excess_stream.hip), which reaches init + prep and the reduce here through excess_prepare / excess_reduce (dgp_internal.h).
#include <climits>

#include "dgp_excess.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

__global__ __launch_bounds__(256) void xs_init_kernel(double* work, long ws, long M, int P, int L, int YL) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  const XsWork wk(work, ws, M, P, L, YL);
  wk.se[2 * g] = INT_MAX;
  wk.se[2 * g + 1] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void xs_prep_kernel(const T* __restrict__ diag, long dsite, long dstep, long M, int m, int P, int L,
                                                      const T* __restrict__ mu, const double* __restrict__ scale2,
                                                      const double* __restrict__ thresh, const double* __restrict__ w,
                                                      const int* __restrict__ group, const T* __restrict__ ev, double sg, int YL,
                                                      double* work, long ws) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  const XsWork wk(work, ws, M, P, L, YL);
  bool in = false;
  double Wj = 0.0, sj = 0.0, sinv = 0.0, vp = 0.0, muj = 0.0, Mj = 0.0;
  if (j < m) {
    const long k = (long)z * m + j;
    const int g = group[k];
    if (g >= 0 && g < P) {
      in = true;
      muj = (double)mu[k];
      double var = (double)diag[(long)z * dsite + j * dstep];
      if (ev) var += (double)ev[k];
      var *= scale2[z];
      vp = var > 0.0 ? var : (var != var ? var : 0.0);
      sj = sqrt(vp);
      sinv = var > 0.0 ? 1.0 / sj : (var != var ? var : 0.0);
      Mj = muj + 0.5 * vp;
      Wj = w[k] * exp(Mj);
      atomicMin(&wk.se[2 * g], (int)j);
      atomicMax(&wk.se[2 * g + 1], (int)j + 1);
    }
  }
  wk.W[j] = Wj;
  wk.sig[j] = sj;
  wk.sinv[j] = sinv;
  for (int l = 0; l < L; ++l) {
    double h = -INFINITY, kap = 0.0, a0 = 0.0, a1 = 0.0, E = 0.0, V = 0.0;  // excluded / pad: adds nothing
    if (in) {
      const double a = thresh[((long)z * L + l) * m + j];
      if (muj != muj || a != a || vp != vp)
        h = __builtin_nan("");
      else if (vp <= 0.0 || isinf(a))
        h = muj > a ? sg * INFINITY : -sg * INFINITY;
      else
        h = sg * (muj - a) * sinv;
      if (h + 2.0 * sg * sj < -EX_ZDET) {  // no mass on the threshold's side (also a = +inf above, a = -inf below)
        h = -INFINITY;
      } else {
        kap = exp(a - Mj);
        a0 = ex_phi(h);
        a1 = ex_phi(h + sg * sj);
        E = sg * (a1 - kap * a0);
        if (vp > 0.0 || h != h) V = exp(vp) * ex_phi(h + 2.0 * sg * sj) - 2.0 * kap * a1 + kap * kap * a0 - E * E;
      }
    }
    const long o = (long)l * M + j;
    wk.h0[o] = h;
    wk.kap[o] = kap;
    wk.A0[o] = a0;
    wk.A1[o] = a1;
    wk.E[o] = E;
    wk.V[o] = V;
  }
}

// levels l0 .. l0 + LV of Y; see the file header
template <typename T, int LV>
__global__ __launch_bounds__(256) void xs_pairs_kernel(const T* __restrict__ cov, long M, int m, int P, int L, int l0,
                                                       const double* __restrict__ scale2, const int* __restrict__ group, double sg,
                                                       double* __restrict__ work, long ws) {
  const int rb = blockIdx.x, h = blockIdx.y, z = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const XsWork wk(work, ws, M, P, L, XS_CHUNK);
  const int r0 = rb * EX_ROWS;
  int c0, c1;
  ex_range(wk.se, h, c0, c1);
  if (r0 >= c1) {  // every row here lies in a later group (or h is empty): nothing the reduce uses, but it reads numbers
    if (tid < EX_ROWS)
#pragma unroll
      for (int l = 0; l < LV; ++l) wk.Y[((long)l * M + r0 + tid) * P + h] = 0.0;
    return;
  }
  ex_tables_init();
  __shared__ double low[LV][EX_ROWS], up[4][LV][EX_ROWS];
  const T* C = cov + (long)z * M * M;
  const int* gz = group + (long)z * m;
  const double s2 = scale2[z];
  __syncthreads();

  // g(i) = h: the j < i of the group, C[i][j]; a wave per row, lanes along the row
  for (int ii = wave; ii < EX_ROWS; ii += 4) {
    const int i = r0 + ii;
    double acc[LV];
#pragma unroll
    for (int l = 0; l < LV; ++l) acc[l] = 0.0;
    if (i < m && gz[i] == h) {
      const T* row = C + (long)i * M;
      XsPoint<LV> pi;
      pi.load(wk, M, l0, i);
      for (int j = c0 + lane; j < i; j += 64) {
        XsPoint<LV> pj;
        pj.load(wk, M, l0, j);
        double n[LV];
        xs_pair<LV>(sg, pi, pj, (double)row[j] * s2, n);
        const double Wj = wk.W[j];
#pragma unroll
        for (int l = 0; l < LV; ++l) acc[l] = __builtin_fma(Wj, n[l], acc[l]);
      }
    }
#pragma unroll
    for (int l = 0; l < LV; ++l) {
      const double v = ex_wave_sum(acc[l]);
      if (lane == 0) low[l][ii] = v;
    }
  }

  // 0 <= g(i) < h: every j of the group (all beyond i), C[j][i]; lanes along i, wave q takes j = c0 + q, c0 + q + 4, ...
  {
    const int i = r0 + lane;
    double acc[LV];
#pragma unroll
    for (int l = 0; l < LV; ++l) acc[l] = 0.0;
    const int gi = i < m ? gz[i] : -1;
    if (gi >= 0 && gi < h) {
      const T* col = C + i;
      XsPoint<LV> pi;
      pi.load(wk, M, l0, i);
      for (int j = c0 + wave; j < c1; j += 4) {
        XsPoint<LV> pj;
        pj.load(wk, M, l0, j);
        double n[LV];
        xs_pair<LV>(sg, pi, pj, (double)col[(long)j * M] * s2, n);
        const double Wj = wk.W[j];
#pragma unroll
        for (int l = 0; l < LV; ++l) acc[l] = __builtin_fma(Wj, n[l], acc[l]);
      }
    }
#pragma unroll
    for (int l = 0; l < LV; ++l) up[wave][l][lane] = acc[l];
  }
  __syncthreads();
  if (tid < EX_ROWS)
#pragma unroll
    for (int l = 0; l < LV; ++l)
      wk.Y[((long)l * M + r0 + tid) * P + h] = low[l][tid] + ((up[0][l][tid] + up[1][l][tid]) + (up[2][l][tid] + up[3][l][tid]));
}

// blockIdx.x = (64-column chunk of h) * LV + level of the chunk
__global__ __launch_bounds__(256) void xs_reduce_kernel(long M, int P, int L, int l0, int LV, int YL, double* __restrict__ work, long ws,
                                                        double* __restrict__ mean_out, double* __restrict__ cov_out,
                                                        double* __restrict__ total_out) {
  const int hc = blockIdx.x / LV, lc = blockIdx.x % LV, g = blockIdx.y, z = blockIdx.z;
  if (hc > 0 && hc * 64 + 63 < g) return;  // every h of this chunk is < g: the (h, g) workgroup writes those entries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const XsWork wk(work, ws, M, P, L, YL);
  const double* Y = wk.Y + (long)lc * M * P;
  const double* E = wk.E + (long)(l0 + lc) * M;
  const double* V = wk.V + (long)(l0 + lc) * M;
  int c0, c1;
  ex_range(wk.se, g, c0, c1);
  __shared__ double red[4][64];
  __shared__ double mred[256], dred[256], tred[256];
  const int h = hc * 64 + lane;
  double acc = 0.0;
  if (h < P) {
#pragma unroll 4
    for (int i = c0 + wave; i < c1; i += 4) acc += wk.W[i] * Y[(long)i * P + h];
  }
  red[wave][lane] = acc;
  const bool own = g >= hc * 64 && g < hc * 64 + 64;  // this workgroup holds (g, g): it needs the diagonal terms
  if (hc == 0 || own) {
    double s = 0.0, d = 0.0, t = 0.0;
    for (int i = c0 + tid; i < c1; i += 256) {
      const double Wi = wk.W[i];
      s += Wi * E[i];
      d += Wi * Wi * V[i];
      t += Wi;
    }
    mred[tid] = s;
    dred[tid] = d;
    tred[tid] = t;
  }
  __syncthreads();
  if (hc == 0 || own) {
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        mred[tid] += mred[tid + s];
        dred[tid] += dred[tid + s];
        tred[tid] += tred[tid + s];
      }
      __syncthreads();
    }
  }
  if (wave == 0 && h < P && h >= g) {
    double v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    if (h == g) v = 2.0 * v + dred[0];
    double* out = cov_out + ((long)z * L + l0 + lc) * P * P;
    out[(long)g * P + h] = v;
    out[(long)h * P + g] = v;
  }
  if (hc == 0 && tid == 0) {
    mean_out[((long)z * L + l0 + lc) * P + g] = mred[0];
    if (l0 + lc == 0) total_out[(long)z * P + g] = tred[0];
  }
}

template <typename T, int LV>
void xs_chunk(const T* cov, long M, int m, int B, int P, int L, int l0, const double* scale2, const int* group, double sg, double* work,
              long ws, double* mean_out, double* cov_out, double* total_out, hipStream_t s) {
  xs_pairs_kernel<T, LV><<<dim3((unsigned)(M / EX_ROWS), (unsigned)P, (unsigned)B), 256, 0, s>>>(cov, M, m, P, L, l0, scale2, group, sg,
                                                                                                 work, ws);
  excess_reduce(M, B, P, L, l0, LV, XS_CHUNK, work, mean_out, cov_out, total_out, s);
}

}  // namespace

size_t excess_moments_workspace_bytes(long m, int P, int L, int B, int YL) {
  return sizeof(double) * (size_t)B * (size_t)xs_site_doubles(round_up(m, DGP_TILE_HOST), P, L, YL);
}

template <typename T>
void excess_prepare(const T* diag, long dsite, long dstep, long m, int B, const T* mu, const double* scale2, const double* thresh, int L,
                    const double* w, const int* group, int P, const T* ev, double sg, int YL, double* work, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const long ws = xs_site_doubles(M, P, L, YL);
  xs_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(work, ws, M, P, L, YL);
  xs_prep_kernel<T><<<dim3((unsigned)((M + 255) / 256), 1, (unsigned)B), 256, 0, s>>>(diag, dsite, dstep, M, (int)m, P, L, mu, scale2,
                                                                                    thresh, w, group, ev, sg, YL, work, ws);
}

void excess_reduce(long M, int B, int P, int L, int l0, int LV, int YL, double* work, double* mean_out, double* cov_out,
                   double* total_out, hipStream_t s) {
  xs_reduce_kernel<<<dim3((unsigned)(((P + 63) / 64) * LV), (unsigned)P, (unsigned)B), 256, 0, s>>>(
      M, P, L, l0, LV, YL, work, xs_site_doubles(M, P, L, YL), mean_out, cov_out, total_out);
}

template <typename T>
static int excess_moments(const T* cov, long m, int B, const T* mu, const double* scale2, const double* thresh, int L, const double* w,
                          const int* group, int P, const T* ev, int above, double* work, double* mean_out, double* cov_out,
                          double* total_out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const long ws = xs_site_doubles(M, P, L, XS_CHUNK);
  const double sg = above ? 1.0 : -1.0;
  excess_prepare<T>(cov, M * M, M + 1, m, B, mu, scale2, thresh, L, w, group, P, ev, sg, XS_CHUNK, work, s);
  for (int l0 = 0; l0 < L;) {  // chunks of 2 levels, then 1: a function of L alone
    if (L - l0 >= 2) {
      xs_chunk<T, 2>(cov, M, (int)m, B, P, L, l0, scale2, group, sg, work, ws, mean_out, cov_out, total_out, s);
      l0 += 2;
    } else {
      xs_chunk<T, 1>(cov, M, (int)m, B, P, L, l0, scale2, group, sg, work, ws, mean_out, cov_out, total_out, s);
      l0 += 1;
    }
  }
  return (int)hipGetLastError();
}

template void excess_prepare<double>(const double*, long, long, long, int, const double*, const double*, const double*, int,
                                     const double*, const int*, int, const double*, double, int, double*, hipStream_t);
template void excess_prepare<float>(const float*, long, long, long, int, const float*, const double*, const double*, int, const double*,
                                    const int*, int, const float*, double, int, double*, hipStream_t);

}  // namespace dgp

using namespace dgp;

extern "C" {

size_t dgp_excess_moments_workspace_bytes(int64_t m, int ngroups, int nlevels, int batch) {
  if (!ex_sizes_ok(m, ngroups, nlevels, batch)) return 0;
  return excess_moments_workspace_bytes(m, ngroups, nlevels, batch, XS_CHUNK);
}

int dgp_excess_moments(int dtype, const void* cov, int64_t m, int batch, const void* mu, const double* scale2, const double* thresh,
                       const double* w, const int32_t* group, int ngroups, int nlevels, const void* extra_var, int above, void* work,
                       size_t work_bytes, double* mean_out, double* cov_out, double* total_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_excess_moments: dtype must be 0 (f64) or 1 (f32)");
  if (!cov || !mu || !scale2 || !thresh || !w || !group || !mean_out || !cov_out || !total_out)
    return fail(DGP_E_ARG, "dgp_excess_moments: null argument");
  if (!ex_sizes_ok(m, ngroups, nlevels, batch))
    return fail(DGP_E_ARG,
                "dgp_excess_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= nlevels <= 64, 1 <= batch <= 1024)");
  if (above != 0 && above != 1) return fail(DGP_E_ARG, "dgp_excess_moments: above must be 0 (deficit) or 1 (excess)");
  if (int rc = need_work(work, work_bytes, excess_moments_workspace_bytes(m, ngroups, nlevels, batch, XS_CHUNK), "dgp_excess_moments")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64
                     ? excess_moments<double>((const double*)cov, m, batch, (const double*)mu, scale2, thresh, nlevels, w, group, ngroups,
                                              (const double*)extra_var, above, (double*)work, mean_out, cov_out, total_out, s)
                     : excess_moments<float>((const float*)cov, m, batch, (const float*)mu, scale2, thresh, nlevels, w, group, ngroups,
                                             (const float*)extra_var, above, (double*)work, mean_out, cov_out, total_out, s);
  return wrap(rc, "dgp_excess_moments");
}

}  // extern "C"
