// dgp_terms.hip -- the posterior of the covariance's ADDITIVE PARTS from the factorisation a plan holds.
//
// K = sum_c K_c (Model::terms, dgp_models.h).  With T = L^-1, alpha = K^^-1 r and V_c = T K_c(X, X*):
//     E[f_c(x*) | y]              = K_c(x*, X) alpha
//     Cov[f_c(x*), f_c'(x*) | y]  = delta_cc' k_c(x*, x*) - V_c[:, *]^T V_c'[:, *]
// The means sum to dgp_predict's latent mean and the C x C covariance at a point to its variance.
//
//   gram_cross_terms   the C cross Grams side by side in ONE row-major N x (C Mp) matrix (term c of test point j in column
//                      c Mp + j, Mp = round_up(m, 128)), one Model::terms call per pair; gram_cross_kernel's tiling.
//   gram_diag_terms    kss[c Mp + j] = k_c(x*_j, x*_j).
//   V = T Ks           dgp_chol.hip::predict_v at width C Mp -- the prediction's GEMM, unchanged.
//   terms_partial /    two-stage column reduction (predict_partial / predict_finish extended): per point and row slab the
//   terms_finish       C sums Ks[i, c Mp + j] alpha_i and the C (C + 1) / 2 sums V[i, c Mp + j] V[i, c' Mp + j], c' <= c; the
//                      finish pass adds the slabs in slab order and subtracts from delta_cc' kss.  V and Ks are read once.
//                      slopes_reduce (dgp_slopes.hip's planes) runs the same two kernels against a packed prior block.
// Fixed summation orders, no floating-point atomics: bitwise repeatable.
#include "dgp_internal.h"
#include "dgp_models.h"
#include "dgp_gram_shared.h"

namespace dgp {

// C planes of the live terms: the fused models write all of M::NTERMS, a composite its descriptor's count (<= DGP_C_TMAX)
template <typename T, typename M>
__global__ __launch_bounds__(256) void gram_cross_terms_kernel(const T* __restrict__ Xt, long N, int n,
                                                               const T* __restrict__ Xst, long Mp, int m, int C,
                                                               const PreBatch<M> pb, T* __restrict__ Ks, long bs, long wbs,
                                                               const int* __restrict__ ns) {
  const typename M::Pre& pre = pb.get();
  Xt = site(Xt, bs);
  Xst = site(Xst, wbs);
  Ks = site(Ks, wbs);
  n = site_n(ns, n);
  __shared__ T sfi[M::NF][64], sfj[M::NF][64];
  const int bi = blockIdx.y, bj = blockIdx.x;
  const int t = threadIdx.x;
  exp_table_init<T>();
  if (t < 64) stage_strip<T, M>(Xt, N, (long)bi * 64, pre, sfi, t);
  else if (t < 128) stage_strip<T, M>(Xst, Mp, (long)bj * 64, pre, sfj, t - 64);
  __syncthreads();
  const int ty = t >> 4, tx = t & 15;
  const long ld = (long)C * Mp;
  if constexpr (Interpreted<M>::value) {
    // one entry and one term at a time, element stores
#pragma unroll 1
    for (int a = 0; a < 4; ++a) {
      const int ri = ty * 4 + a;
      const long gi = (long)bi * 64 + ri;
      const auto fi = [&](int q) { return sfi[q][ri]; };
#pragma unroll 1
      for (int b = 0; b < 4; ++b) {
        const int cj = tx * 4 + b;
        const long gj = (long)bj * 64 + cj;
        const auto fj = [&](int q) { return sfj[q][cj]; };
        const bool pad = gi >= n || gj >= m;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
          const T v = M::term(c, fi, fj, pre);
          Ks[gi * ld + (long)c * Mp + gj] = pad ? T(0) : v;
        }
      }
    }
    return;
  }
  T fj[4][M::NF];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int c = 0; c < M::NF; ++c) fj[b][c] = sfj[c][tx * 4 + b];
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {  // one row at a time: 4 x NTERMS results live, not 16 x NTERMS
    const long gi = (long)bi * 64 + ty * 4 + a;
    T fi[M::NF];
#pragma unroll
    for (int c = 0; c < M::NF; ++c) fi[c] = sfi[c][ty * 4 + a];
    T out[M::NTERMS][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const long gj = (long)bj * 64 + tx * 4 + b;
      T k[M::NTERMS];
      M::terms(fi, fj[b], pre, k);
      const bool pad = gi >= n || gj >= m;
#pragma unroll
      for (int c = 0; c < M::NTERMS; ++c) out[c][b] = pad ? T(0) : k[c];
    }
#pragma unroll
    for (int c = 0; c < M::NTERMS; ++c)
      if (c < C) store4<T>(Ks + gi * ld + (long)c * Mp + (long)bj * 64 + tx * 4, out[c]);
  }
}

template <typename T, typename M>
__global__ __launch_bounds__(256) void gram_diag_terms_kernel(const T* __restrict__ Xst, long Mp, int m, int C,
                                                              const PreBatch<M> pb, T* __restrict__ kss, long wbs) {
  const typename M::Pre& pre = pb.get();
  Xst = site(Xst, wbs);
  kss = site(kss, wbs);
  exp_table_init<T>();
  __syncthreads();
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mp) return;
  T x[M::NX], f[M::NF];
#pragma unroll
  for (int c = 0; c < M::NX; ++c) x[c] = Xst[(long)c * Mp + j];
  M::features(x, pre, f);
  if constexpr (Interpreted<M>::value) {
    const auto fa = [&](int q) { return f[q]; };
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
      const T v = M::term(c, fa, fa, pre);
      kss[(long)c * Mp + j] = j < m ? v : T(0);
    }
  } else {
    T k[M::NTERMS];
    M::terms(f, f, pre, k);
#pragma unroll
    for (int c = 0; c < M::NTERMS; ++c) kss[(long)c * Mp + j] = j < m ? k[c] : T(0);
  }
}

// Column sums over a slab of rows, 64 columns x 4 row lanes per workgroup like predict_partial_kernel.  Quantity q of
// point j and slab z goes to part[(q * PREDICT_SPLIT + z) * Mp + j]: q < C the mean sums, then the packed lower triangle
// (c, c') at C + c (c + 1) / 2 + c'.  C is a compile-time constant (1 .. DGP_C_TMAX): C + C (C + 1) / 2 <= 27 accumulators
// stay in registers.
template <typename T, int C>
__global__ __launch_bounds__(256) void terms_partial_kernel(const T* __restrict__ V, const T* __restrict__ Ks, long N, long Mp,
                                                            const T* __restrict__ alpha, T* __restrict__ part, long bs,
                                                            long wbs) {
  constexpr int P = C + C * (C + 1) / 2;
  V = site(V, wbs);
  Ks = site(Ks, wbs);
  part = site(part, wbs);
  alpha = site(alpha, bs);
  __shared__ T red[3][P][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long j = (long)blockIdx.x * 64 + tx;
  const long ld = (long)C * Mp;
  const long rows = N / PREDICT_SPLIT;  // N % 128 == 0 and PREDICT_SPLIT divides 128
  const long i0 = (long)blockIdx.y * rows, i1 = i0 + rows;
  T acc[P];
#pragma unroll
  for (int q = 0; q < P; ++q) acc[q] = T(0);
  for (long i = i0 + ty; i < i1; i += 4) {
    const T a = alpha[i];
    T v[C], ks[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      v[c] = V[i * ld + (long)c * Mp + j];
      ks[c] = Ks[i * ld + (long)c * Mp + j];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      acc[c] += ks[c] * a;
#pragma unroll
      for (int e = 0; e <= c; ++e) acc[C + c * (c + 1) / 2 + e] += v[c] * v[e];
    }
  }
  if (ty > 0) {
#pragma unroll
    for (int q = 0; q < P; ++q) red[ty - 1][q][tx] = acc[q];
  }
  __syncthreads();
  if (ty == 0) {
#pragma unroll
    for (int q = 0; q < P; ++q)
      part[((long)q * PREDICT_SPLIT + blockIdx.y) * Mp + j] = acc[q] + red[0][q][tx] + red[1][q][tx] + red[2][q][tx];
  }
}

// mean [site][C][m] and cov [site][C (C + 1) / 2][m] (null: not wanted) straight into the caller's arrays.  The prior the sums
// are subtracted from: PACKED = false delta_cc' kss[c Mp + j] (independent parts), PACKED = true a full packed block
// kss[(c (c + 1) / 2 + c') Mp + j] (dgp_slopes.hip: value and input derivatives are correlated a priori).
template <typename T, int C, bool PACKED>
__global__ __launch_bounds__(256) void terms_finish_kernel(const T* __restrict__ part, long Mp, int m, const T* __restrict__ kss,
                                                           T* __restrict__ mean, T* __restrict__ cov, long wbs) {
  constexpr int P = C + C * (C + 1) / 2;
  part = site(part, wbs);
  kss = site(kss, wbs);
  mean = site(mean, (long)C * m);
  if (cov) cov = site(cov, (long)(P - C) * m);
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    T s = T(0);
    for (int z = 0; z < PREDICT_SPLIT; ++z) s += part[((long)c * PREDICT_SPLIT + z) * Mp + j];  // fixed order
    mean[(long)c * m + j] = s;
  }
  if (!cov) return;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int e = 0; e <= c; ++e) {
      const int q = c * (c + 1) / 2 + e;
      T s = T(0);
      for (int z = 0; z < PREDICT_SPLIT; ++z) s += part[((long)(C + q) * PREDICT_SPLIT + z) * Mp + j];
      cov[(long)q * m + j] = (PACKED ? kss[(long)q * Mp + j] : e == c ? kss[(long)c * Mp + j] : T(0)) - s;
    }
}

// ------------------------------------------------------------------------------------------
template <typename T>
int gram_cross_terms(int model, int d, const T* Xt, long N, int n, const T* Xst, long Mp, int m, const double* theta, T* Ks,
                     hipStream_t s, Batch bt, long wbs, void* pre_scratch, void* pre_staging) {
  const int nt = model_ntheta(model, d), C = model_nterms(model, d);
  if (nt < 0 || C < 1) return -2;
  dim3 grid((unsigned)(Mp / 64), (unsigned)(N / 64), (unsigned)bt.B);
  DGP_DISPATCH_MODEL(model, d, (gram_cross_terms_kernel<T, M><<<grid, dim3(256), 0, s>>>(
                                   Xt, N, n, Xst, Mp, m, C, prepare_batch<M>(theta, nt, bt.B, pre_scratch, true, s, pre_staging), Ks,
                                   bt.ws, wbs, bt.ns)));
  return (int)hipGetLastError();
}

// the hyperparameters of a batch of more than 8 are already in pre_scratch (gram_cross_terms of the same call)
template <typename T>
int gram_diag_terms(int model, int d, const T* Xst, long Mp, int m, const double* theta, T* kss, hipStream_t s, Batch bt, long wbs,
                    void* pre_scratch) {
  const int nt = model_ntheta(model, d), C = model_nterms(model, d);
  if (nt < 0 || C < 1) return -2;
  dim3 grid((unsigned)((Mp + 255) / 256), 1, (unsigned)bt.B);
  DGP_DISPATCH_MODEL(model, d, (gram_diag_terms_kernel<T, M><<<grid, dim3(256), 0, s>>>(
                                   Xst, Mp, m, C, prepare_batch<M>(theta, nt, bt.B, pre_scratch, false, s), kss, wbs)));
  return (int)hipGetLastError();
}

long terms_partials(int C, long Mp) { return (long)(C + C * (C + 1) / 2) * PREDICT_SPLIT * Mp; }

template <typename T, int C, bool PACKED = false>
static void terms_reduce_launch(const T* V, const T* Ks, long N, long Mp, int m, const T* alpha, const T* kss, T* part, T* mean,
                                T* cov, hipStream_t s, Batch bt, long wbs) {
  const unsigned Bz = (unsigned)bt.B;
  terms_partial_kernel<T, C><<<dim3((unsigned)(Mp / 64), PREDICT_SPLIT, Bz), 256, 0, s>>>(V, Ks, N, Mp, alpha, part, bt.ws, wbs);
  terms_finish_kernel<T, C, PACKED><<<dim3((unsigned)((m + 255) / 256), 1, Bz), 256, 0, s>>>(part, Mp, m, kss, mean, cov, wbs);
}

template <typename T>
int terms_reduce(int C, const T* V, const T* Ks, long N, long Mp, int m, const T* alpha, const T* kss, T* part, T* mean, T* cov,
                 hipStream_t s, Batch bt, long wbs) {
  switch (C) {
    case 1: terms_reduce_launch<T, 1>(V, Ks, N, Mp, m, alpha, kss, part, mean, cov, s, bt, wbs); break;
    case 2: terms_reduce_launch<T, 2>(V, Ks, N, Mp, m, alpha, kss, part, mean, cov, s, bt, wbs); break;
    case 3: terms_reduce_launch<T, 3>(V, Ks, N, Mp, m, alpha, kss, part, mean, cov, s, bt, wbs); break;
    case 4: terms_reduce_launch<T, 4>(V, Ks, N, Mp, m, alpha, kss, part, mean, cov, s, bt, wbs); break;
    case 5: terms_reduce_launch<T, 5>(V, Ks, N, Mp, m, alpha, kss, part, mean, cov, s, bt, wbs); break;
    case 6: terms_reduce_launch<T, 6>(V, Ks, N, Mp, m, alpha, kss, part, mean, cov, s, bt, wbs); break;
    default: return -2;
  }
  return (int)hipGetLastError();
}

// P planes of dgp_slopes.hip (1 + ncols <= 1 + DGP_C_DMAX) against the packed prior block `prior` (P (P + 1) / 2 x Mp)
template <typename T>
int slopes_reduce(int P, const T* V, const T* Ks, long N, long Mp, int m, const T* alpha, const T* prior, T* part, T* mean, T* cov,
                  hipStream_t s, Batch bt, long wbs) {
  switch (P) {
    case 2: terms_reduce_launch<T, 2, true>(V, Ks, N, Mp, m, alpha, prior, part, mean, cov, s, bt, wbs); break;
    case 3: terms_reduce_launch<T, 3, true>(V, Ks, N, Mp, m, alpha, prior, part, mean, cov, s, bt, wbs); break;
    case 4: terms_reduce_launch<T, 4, true>(V, Ks, N, Mp, m, alpha, prior, part, mean, cov, s, bt, wbs); break;
    case 5: terms_reduce_launch<T, 5, true>(V, Ks, N, Mp, m, alpha, prior, part, mean, cov, s, bt, wbs); break;
    case 6: terms_reduce_launch<T, 6, true>(V, Ks, N, Mp, m, alpha, prior, part, mean, cov, s, bt, wbs); break;
    case 7: terms_reduce_launch<T, 7, true>(V, Ks, N, Mp, m, alpha, prior, part, mean, cov, s, bt, wbs); break;
    default: return -2;
  }
  return (int)hipGetLastError();
}

#define DGP_INST(T)                                                                                                              \
  template int gram_cross_terms<T>(int, int, const T*, long, int, const T*, long, int, const double*, T*, hipStream_t, Batch, long, \
                                   void*, void*);                                                                                 \
  template int gram_diag_terms<T>(int, int, const T*, long, int, const double*, T*, hipStream_t, Batch, long, void*);              \
  template int terms_reduce<T>(int, const T*, const T*, long, long, int, const T*, const T*, T*, T*, T*, hipStream_t, Batch, long); \
  template int slopes_reduce<T>(int, const T*, const T*, long, long, int, const T*, const T*, T*, T*, T*, hipStream_t, Batch, long);
DGP_INST(double)
DGP_INST(float)

}  // namespace dgp
