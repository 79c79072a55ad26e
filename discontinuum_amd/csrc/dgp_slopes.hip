// dgp_slopes.hip -- the posterior of the fit's INPUT DERIVATIVES from the factorisation a plan holds.
//
// The derivative of a GP is a GP.  With D_0 = id, D_q = d / d x*_{c_q} acting on the test point (c_q the requested raw input
// columns, q = 1 .. ncols, P = 1 + ncols planes), T = L^-1, alpha = K^^-1 r and V_a = T (D_a K)(X, X*):
//     E[D_a f(x*) | y]           = (D_a K)(x*, X) alpha
//     Cov[D_a f, D_b f | y](x*)  = D_a D'_b k(x, x')|_{x = x' = x*} - V_a[:, *]^T V_b[:, *]
//
//   gram_cross_slopes  the P planes side by side in ONE row-major N x (P Mp) matrix (plane a of test point j in column
//                      a Mp + j, Mp = round_up(m, 128)), one Model::slopes call per pair; plane 0 is the value; pad rows and
//                      columns are zero.  gram_cross_terms' tiling.
//   gram_prior_slopes  prior[(a (a + 1) / 2 + b) Mp + j] = D_a D'_b k at test point j, b <= a (Model::prior_slopes).
//   V = T Ks           dgp_chol.hip::predict_v at width P Mp -- the prediction's GEMM, unchanged.
//   slopes_reduce      dgp_terms.hip's two-stage column reduction; the finish pass subtracts from the packed prior block.
// Fixed summation orders, no floating-point atomics: bitwise repeatable.
#include "dgp_internal.h"
#include "dgp_models.h"
#include "dgp_gram_shared.h"

namespace dgp {

// test strip: the features and the slope features (derivatives of the per-point warps at the test point)
template <typename T, typename M>
__device__ __forceinline__ void stage_slope_strip(const T* __restrict__ Xst, long Mp, long base, const typename M::Pre& pre,
                                                  T (*sf)[64], T (*sg)[64], int lane) {
  T x[M::NX], f[M::NF], g[M::NSF];
#pragma unroll
  for (int c = 0; c < M::NX; ++c) x[c] = Xst[(long)c * Mp + base + lane];
  M::features(x, pre, f);
  M::slope_features(x, f, pre, g);
#pragma unroll
  for (int c = 0; c < M::NF; ++c) sf[c][lane] = f[c];
#pragma unroll
  for (int c = 0; c < M::NSF; ++c) sg[c][lane] = g[c];
}

template <typename T, typename M>
__global__ __launch_bounds__(256) void gram_cross_slopes_kernel(const T* __restrict__ Xt, long N, int n,
                                                                const T* __restrict__ Xst, long Mp, int m, const SlopeCols sc,
                                                                const PreBatch<M> pb, T* __restrict__ Ks, long bs, long wbs,
                                                                const int* __restrict__ ns) {
  const typename M::Pre& pre = pb.get();
  Xt = site(Xt, bs);
  Xst = site(Xst, wbs);
  Ks = site(Ks, wbs);
  n = site_n(ns, n);
  __shared__ T sfi[M::NF][64], sfj[M::NF][64], sgj[M::NSF][64];
  const int bi = blockIdx.y, bj = blockIdx.x;
  const int t = threadIdx.x;
  exp_table_init<T>();
  if (t < 64) stage_strip<T, M>(Xt, N, (long)bi * 64, pre, sfi, t);
  else if (t < 128) stage_slope_strip<T, M>(Xst, Mp, (long)bj * 64, pre, sfj, sgj, t - 64);
  __syncthreads();
  const int ty = t >> 4, tx = t & 15;
  const long ld = (long)(1 + sc.ncols) * Mp;
  if constexpr (Interpreted<M>::value) {
    // one entry and one requested column at a time, element stores; every column's call also gives the value
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {  // one flat loop over the thread's 4 x 4 entries: fewer live scalars than two nested ones
      const int ri = ty * 4 + (e >> 2), cj = tx * 4 + (e & 3);
      const long gi = (long)bi * 64 + ri, gj = (long)bj * 64 + cj;
      const auto fi = [&](int q) { return sfi[q][ri]; };
      const auto fj = [&](int q) { return sfj[q][cj]; };
      const bool pad = gi >= n || gj >= m;
      T* dst = Ks + gi * ld + gj;
      T kv = T(0);
#pragma unroll 1
      for (int q = 0; q < sc.ncols; ++q) {
        dst += Mp;
        const T dv = M::slope_col(sc.col[q], fi, fj, pre, &kv);
        *dst = pad ? T(0) : dv;
      }
      dst[-(long)sc.ncols * Mp] = pad ? T(0) : kv;  // every call gives the same value: keep the last
    }
    return;
  } else {
    T fj[4][M::NF], gj[4][M::NSF];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
      for (int c = 0; c < M::NF; ++c) fj[b][c] = sfj[c][tx * 4 + b];
#pragma unroll
      for (int c = 0; c < M::NSF; ++c) gj[b][c] = sgj[c][tx * 4 + b];
    }
#pragma unroll 1
    for (int a = 0; a < 4; ++a) {  // one row at a time: 4 x (1 + NX) results live
      const long gi = (long)bi * 64 + ty * 4 + a;
      T fi[M::NF];
#pragma unroll
      for (int c = 0; c < M::NF; ++c) fi[c] = sfi[c][ty * 4 + a];
      T out[1 + M::NX][4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const long gjx = (long)bj * 64 + tx * 4 + b;
        T k[1 + M::NX];
        M::slopes(fi, fj[b], gj[b], pre, k);
        const bool pad = gi >= n || gjx >= m;
#pragma unroll
        for (int c = 0; c < 1 + M::NX; ++c) out[c][b] = pad ? T(0) : k[c];
      }
      // the evaluator gives every column; plane[c] says where the requested ones go (compile-time c: no indexed registers)
#pragma unroll
      for (int c = 0; c < 1 + M::NX; ++c)
        if (sc.plane[c] >= 0) store4<T>(Ks + gi * ld + (long)sc.plane[c] * Mp + (long)bj * 64 + tx * 4, out[c]);
    }
  }
}

template <typename T, typename M>
__global__ __launch_bounds__(256) void gram_prior_slopes_kernel(const T* __restrict__ Xst, long Mp, int m, const SlopeCols sc,
                                                                const PreBatch<M> pb, T* __restrict__ prior, long wbs) {
  const typename M::Pre& pre = pb.get();
  Xst = site(Xst, wbs);
  prior = site(prior, wbs);
  exp_table_init<T>();
  __syncthreads();
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  const bool live = j < m;
  if constexpr (Interpreted<M>::value) {
#pragma unroll 1
    for (int a = 0; a <= sc.ncols; ++a) {
      const T v = M::prior_col(a == 0 ? -1 : (int)sc.col[a - 1], pre);
#pragma unroll 1
      for (int b = 0; b <= a; ++b) prior[(long)(a * (a + 1) / 2 + b) * Mp + j] = (live && b == a) ? v : T(0);
    }
  } else {
    T x[M::NX], f[M::NF], g[M::NSF], pr[M::NPRIOR];
#pragma unroll
    for (int c = 0; c < M::NX; ++c) x[c] = Xst[(long)c * Mp + j];
    M::features(x, pre, f);
    M::slope_features(x, f, pre, g);
    M::prior_slopes(f, g, pre, pr);
#pragma unroll
    for (int a = 0; a < 1 + M::NX; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        const int pa = sc.plane[a], pb2 = sc.plane[b];
        if (pa < 0 || pb2 < 0) continue;
        const int hi = pa > pb2 ? pa : pb2, lo = pa > pb2 ? pb2 : pa;  // the block is symmetric; columns come in any order
        prior[(long)(hi * (hi + 1) / 2 + lo) * Mp + j] = live ? pr[a * (a + 1) / 2 + b] : T(0);
      }
  }
}

// ------------------------------------------------------------------------------------------
SlopeCols slope_cols(const int* cols, int ncols) {
  SlopeCols sc;
  sc.ncols = ncols;
  for (int c = 0; c < 1 + DGP_C_DMAX; ++c) sc.plane[c] = -1;
  for (int q = 0; q < DGP_C_DMAX; ++q) sc.col[q] = 0;
  sc.plane[0] = 0;
  for (int q = 0; q < ncols; ++q) {
    sc.col[q] = (unsigned char)cols[q];
    sc.plane[1 + cols[q]] = (signed char)(q + 1);
  }
  return sc;
}

template <typename T>
int gram_cross_slopes(int model, int d, const T* Xt, long N, int n, const T* Xst, long Mp, int m, const double* theta,
                      const int* cols, int ncols, T* Ks, hipStream_t s, Batch bt, long wbs, void* pre_scratch, void* pre_staging) {
  const int nt = model_ntheta(model, d);
  if (nt < 0 || ncols < 1 || ncols > d) return -2;
  const SlopeCols sc = slope_cols(cols, ncols);
  dim3 grid((unsigned)(Mp / 64), (unsigned)(N / 64), (unsigned)bt.B);
  DGP_DISPATCH_MODEL(model, d, (gram_cross_slopes_kernel<T, M><<<grid, dim3(256), 0, s>>>(
                                   Xt, N, n, Xst, Mp, m, sc, prepare_batch<M>(theta, nt, bt.B, pre_scratch, true, s, pre_staging), Ks,
                                   bt.ws, wbs, bt.ns)));
  return (int)hipGetLastError();
}

// the hyperparameters of a batch of more than 8 are already in pre_scratch (gram_cross_slopes of the same call)
template <typename T>
int gram_prior_slopes(int model, int d, const T* Xst, long Mp, int m, const double* theta, const int* cols, int ncols, T* prior,
                      hipStream_t s, Batch bt, long wbs, void* pre_scratch) {
  const int nt = model_ntheta(model, d);
  if (nt < 0 || ncols < 1 || ncols > d) return -2;
  const SlopeCols sc = slope_cols(cols, ncols);
  dim3 grid((unsigned)((Mp + 255) / 256), 1, (unsigned)bt.B);
  DGP_DISPATCH_MODEL(model, d, (gram_prior_slopes_kernel<T, M><<<grid, dim3(256), 0, s>>>(
                                   Xst, Mp, m, sc, prepare_batch<M>(theta, nt, bt.B, pre_scratch, false, s), prior, wbs)));
  return (int)hipGetLastError();
}

#define DGP_INST(T)                                                                                                              \
  template int gram_cross_slopes<T>(int, int, const T*, long, int, const T*, long, int, const double*, const int*, int, T*,        \
                                    hipStream_t, Batch, long, void*, void*);                                                       \
  template int gram_prior_slopes<T>(int, int, const T*, long, int, const double*, const int*, int, T*, hipStream_t, Batch, long,   \
                                    void*);
DGP_INST(double)
DGP_INST(float)

}  // namespace dgp
