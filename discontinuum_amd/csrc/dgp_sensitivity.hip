// dgp_sensitivity.hip -- the exact JACOBIANS of the posterior mean and variance with respect to every hyperparameter direction,
// at all m prediction points, from the factorisation a plan holds.
//
// Held: T = L^-1 (K^^-1 = T^T T) and alpha = K^^-1 r.  For test points X*: K* = K(X, X*), V = T K*, beta = T^T V = K^^-1 K*.
// Directions as for dgp_fisher.hip -- the P kernel directions D_p = dK/dtheta_p (with D*_p = dK*/dtheta_p) and E diagonal ones
// diag(d_e) -- plus C right-hand-side columns g_c = dm(X)/draw_c (prior-mean parameters):
//     dmean[p][j]         = sum_i D*_p,ij alpha_i - sum_i beta_ij (D_p alpha)_i
//     dvar [p][j]         = dk(x*_j, x*_j)/dtheta_p - 2 sum_i beta_ij D*_p,ij + beta_j^T D_p beta_j
//     dmean[P + e][j]     = -sum_i beta_ij d_e,i alpha_i          dvar[P + e][j] = sum_i beta_ij^2 d_e,i
//     dmean[P + E + c][j] = -sum_i beta_ij g_c,i                  (the variance does not depend on the prior mean)
// Passes, all with gridDim.z = sites (ragged batches through site_n):
//
//   fisher_dk     dgp_fisher.hip's sweep: all P matrices D_p, each full and symmetric in its own N x N slot (zero in the pad).
//   gram_cross,   K* and V = T K*: the prediction's launches, unchanged (the API layer runs gram_cross).
//   predict_v
//   sens_beta     beta = T^T V on the project's tile cores: T as the k-MAJOR operand (op(i, k) = T[k][i]), the k-range starts at
//                 the tile's block row (T is lower triangular, zeros above the diagonal inside its diagonal blocks) and is visited
//                 from its last k-tile down (REV, as in lauum: the rows of T far below the diagonal hold its smallest entries).
//                 128 x 128 direct-to-LDS tiles, or 64 x 64 register-staged ones while a launch has too few 128-tiles (lauum's
//                 rule and selector); block row 0 -- the longest k-range -- is dispatched first.
//   sens_gcols    G = [D_p alpha | d_e o alpha | g_c], R = P + E + C columns of N doubles: one wave per row and slot reads the
//                 row once (HBM-bound), lanes in a fixed stride, double accumulation, wave shuffle.
//   sens_cross    per pair (i, j) ONE Model::pair<true> evaluation with weight 1 into a zeroed scratch set; its raw derivative
//                 sums are accumulated in DOUBLE against alpha_i and against beta_ij separately (finalize is linear: applied once
//                 per accumulator set, in sens_finish).  A workgroup owns 64 columns and one of SENS_SPLIT row slabs.
//   sens_bg       the same slabs: -beta_ij G[i][.] and beta_ij^2 d_e,i (a second launch: with both accumulator sets of sens_cross
//                 and a pair evaluation live, the R + E sums of this pass would not stay in registers).
//   sens_quad     q_p[j] = beta_j^T D_p beta_j: the product D_p beta (N x N by N x M) on the tile cores -- the dominant cost,
//                 2 P N^2 M flop -- contracted with beta in the tile's EPILOGUE: one FMA per entry in double, per-row-tile column
//                 sums through LDS in a fixed order; the product itself is never stored.
//   sens_finish   adds the slab / row-tile partials in a fixed order, applies finalize, evaluates the prior term from pair<true> on
//                 the point with itself and writes dmean [site][R][m] and dvar [site][P + E][m] in double.
// No floating-point atomics, fixed summation orders: bitwise repeatable, and a site's result does not depend on its batch (the
// tile-size selector does: compare batches against single-site plans under the same selector or within the rounding of the
// plan's dtype).  Reads Xt, T and alpha only.
#include "dgp_gemm.h"
#include "dgp_gemm_dma.h"
#include "dgp_plan.h"
#include "dgp_models.h"
#include "dgp_gram_shared.h"

namespace dgp {

static constexpr int SENS_CHUNK = 8;  // directions per register set of sens_bg

#define SENS_SPLIT 32  // row slabs of its column reductions
struct SensLayout {
  size_t Xst, D, Ks, V, beta, G, pc, pg, pq, total;  // byte offsets into a site's slice
};
static SensLayout sens_layout(long N, long Mp, int d, int nt, int ndiag, int nrhs, size_t elem) {
  SensLayout L;
  const size_t R = (size_t)(nt + ndiag + nrhs), n = (size_t)N, m = (size_t)Mp;
  Carve c;
  L.Xst = c.take(elem * m * (size_t)d);
  L.D = c.o;
  for (int p = 0; p < nt; ++p) c.take(elem * n * n);
  L.Ks = c.take(elem * n * m);
  L.V = c.take(elem * n * m);
  L.beta = c.take(elem * n * m);
  L.G = c.take(sizeof(double) * R * n);
  L.pc = c.take(sizeof(double) * SENS_SPLIT * 2 * (size_t)nt * m);
  L.pg = c.take(sizeof(double) * SENS_SPLIT * (R + (size_t)ndiag) * m);
  L.pq = c.take(sizeof(double) * (size_t)nt * (n / 64) * m);
  L.total = c.o;
  return L;
}
// beta = T^T V in 128 x 128 tiles, 64 x 64 ones while the launch has too few (lauum's rule and selector)
static bool sens_small_tiles(long N, long Mp, const Batch& bt) {
  return (N / DGP_TILE_HOST) * (Mp / DGP_TILE_HOST) * bt.B <= bt.tuning().lauum64_max_tiles;
}

// beta[i][j] = sum_{k >= i} T[k][i] V[k][j].  Operand A = T read k-major from its diagonal block down, operand B = rows of V.
template <typename T>
__global__ __launch_bounds__(256, (TileCore<T, false, false>::OCC)) void sens_beta_kernel(const T* __restrict__ Tm, long N, const T* __restrict__ V,
                                                                                          long M, T* __restrict__ beta, long bs, long wbs) {
  Tm = site(Tm, bs);
  V = site(V, wbs);
  beta = site(beta, wbs);
  using K = TileCore<T, false, false>;
  using G = typename K::G;
  __shared__ T smem[K::SMEM_ELEMS];
  const int nbk = (int)gridDim.y, bi = blockIdx.y, bj = blockIdx.x;  // ascending block row: the long k-ranges first
  typename G::acc_t acc[G::MI][G::NI];
  G::zero(acc);
  K::template run<true>(Tm + (long)bi * DGP_TILE * N + (long)bi * DGP_TILE, N, V + (long)bi * DGP_TILE * M + (long)bj * DGP_TILE, M,
                        (nbk - bi) * (DGP_TILE / 16), smem, acc);
  T* out = beta + (long)bi * DGP_TILE * M + (long)bj * DGP_TILE;
  K::foreach (acc, [&](int r, int c, T& v) { out[(long)r * M + c] = v; });
}

template <typename T>
__global__ __launch_bounds__(256, 2) void sens_beta64_kernel(const T* __restrict__ Tm, long N, const T* __restrict__ V, long M,
                                                             T* __restrict__ beta, long bs, long wbs) {
  Tm = site(Tm, bs);
  V = site(V, wbs);
  beta = site(beta, wbs);
  using G = TileGemm<T, false, false, 64, 64>;
  __shared__ T smem[G::SMEM_ELEMS];
  const int nb64 = (int)gridDim.y, bi = blockIdx.y, bj = blockIdx.x;
  typename G::acc_t acc[G::MI][G::NI];
  G::zero(acc);
  G::template run<1, true>(Tm + (long)bi * 64 * N + (long)bi * 64, N, V + (long)bi * 64 * M + (long)bj * 64, M, (nb64 - bi) * (64 / 16),
                           smem, acc);
  T* out = beta + (long)bi * 64 * M + (long)bj * 64;
  G::foreach (acc, [&](int r, int c, T& v) { out[(long)r * M + c] = v; });
}

// G[k][i], k < R.  blockIdx.y = k; a workgroup's four waves take four consecutive rows i.  k < nt: sum_j D_k[i][j] alpha_j over the
// site's own columns, lane l adds columns l, l + 64, ... in order, then the wave tree; k >= nt: d_e,i alpha_i or g_c,i (0 in the pad).
template <typename T>
__global__ __launch_bounds__(256) void sens_gcols_kernel(const T* __restrict__ D, long N, int n, int nt, int ndiag, const T* __restrict__ alpha,
                                                         const T* __restrict__ diag, const T* __restrict__ rhs, long dstride, long rstride,
                                                         double* __restrict__ G, long bs, long wbs, long ps, const int* __restrict__ ns) {
  const int nrow = n;  // row length of the caller's diag / rhs arrays: the plan's n, whatever the site's own size
  D = site(D, wbs);
  alpha = site(alpha, bs);
  G = site(G, ps);
  n = site_n(ns, n);
  const int k = blockIdx.y, lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  double v = 0.0;
  if (k < nt) {
    if (i < n) {
      const T* row = D + (long)k * N * N + i * N;
      for (long j = lane; j < n; j += 64) v += (double)row[j] * (double)alpha[j];
    }
    v = wave_sum(v);
  } else if (i < n) {
    if (k < nt + ndiag) v = (double)site(diag, dstride)[(long)(k - nt) * nrow + i] * (double)alpha[i];
    else v = (double)site(rhs, rstride)[(long)(k - nt - ndiag) * nrow + i];
  }
  if (lane == 0) G[(long)k * N + i] = v;
}

// pc[slab][0][p][j] = sum_{i in slab} raw_p(x_i, x*_j) alpha_i,  pc[slab][1][p][j] = sum_{i in slab} raw_p(x_i, x*_j) beta_ij, raw_p the
// derivative sums of pair<true> before finalize.  Thread (ty, tx): column tx of the workgroup's 64, rows ty, ty + 4, ... of every
// strip of (at most) 64 rows of the slab; the four row lanes are added in order through LDS.
template <typename T, typename M>
__global__ __launch_bounds__(256) void sens_cross_kernel(const T* __restrict__ Xt, long N, int n, const T* __restrict__ Xst, long Mp, int m,
                                                         int nt, const PreBatch<M> pb, const T* __restrict__ alpha,
                                                         const T* __restrict__ beta, double* __restrict__ pc, long bs, long wbs, long ps,
                                                         const int* __restrict__ ns) {
  const typename M::Pre& pre = pb.get();
  Xt = site(Xt, bs);
  alpha = site(alpha, bs);
  Xst = site(Xst, wbs);
  beta = site(beta, wbs);
  pc = site(pc, ps);
  n = site_n(ns, n);
  __shared__ T sfi[M::NF][64], sfj[M::NF][64], sal[64];
  __shared__ double red[4][64];
  const int t = threadIdx.x, tx = t & 63, ty = t >> 6;
  const long j = (long)blockIdx.x * 64 + tx;
  const long rows = N / SENS_SPLIT, i0 = (long)blockIdx.y * rows, i1 = i0 + rows;
  exp_table_init<T>();
  if (t < 64) stage_strip<T, M>(Xst, Mp, (long)blockIdx.x * 64, pre, sfj, t);
  __syncthreads();
  T fj[M::NF];
#pragma unroll
  for (int c = 0; c < M::NF; ++c) fj[c] = sfj[c][tx];
  double accA[M::NTHETA], accB[M::NTHETA];
#pragma unroll
  for (int p = 0; p < M::NTHETA; ++p) accA[p] = accB[p] = 0.0;
#pragma unroll 1
  for (long s0 = i0; s0 < i1 && s0 < n; s0 += 64) {
    const int cnt = (int)min((long)64, min(i1, (long)n) - s0);
    __syncthreads();  // the previous strip has been read
    if (t < cnt) {
      stage_strip<T, M>(Xt, N, s0, pre, sfi, t);
      sal[t] = alpha[s0 + t];
    }
    __syncthreads();
    if (j < m) {
#pragma unroll 1
      for (int ri = ty; ri < cnt; ri += 4) {
        T fi[M::NF];
#pragma unroll
        for (int c = 0; c < M::NF; ++c) fi[c] = sfi[c][ri];
        const double ai = (double)sal[ri], bij = (double)beta[(s0 + ri) * Mp + j];
        T raw[M::NTHETA];
#pragma unroll
        for (int p = 0; p < M::NTHETA; ++p) raw[p] = T(0);
        (void)M::template pair<true>(fi, fj, pre, T(1), raw);
#pragma unroll
        for (int p = 0; p < M::NTHETA; ++p) {
          accA[p] += (double)raw[p] * ai;
          accB[p] += (double)raw[p] * bij;
        }
      }
    }
  }
  double* out = pc + (long)blockIdx.y * 2 * nt * Mp + j;
#pragma unroll
  for (int q = 0; q < 2 * M::NTHETA; ++q) {
    const int p = q % M::NTHETA;
    if (p < nt) {  // (uniform)
      __syncthreads();
      red[ty][tx] = q < M::NTHETA ? accA[p] : accB[p];
      __syncthreads();
      if (ty == 0) out[(long)((q < M::NTHETA ? 0 : nt) + p) * Mp] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    }
  }
}

// pg[slab][k][j] = sum_{i in slab} beta_ij G[k][i] (k < R) and pg[slab][R + e][j] = sum_{i in slab} beta_ij^2 d_e,i, SENS_CHUNK sums at
// a time.  The slab's column of beta is re-read per chunk (it stays in L2); G and d are read at one address per wave.
template <typename T>
__global__ __launch_bounds__(256) void sens_bg_kernel(const T* __restrict__ beta, long N, int n, long Mp, int R, int nvar,
                                                      const double* __restrict__ G, const T* __restrict__ diag, long dstride,
                                                      double* __restrict__ pg, long wbs, long ps, const int* __restrict__ ns) {
  const int nrow = n;
  beta = site(beta, wbs);
  G = site(G, ps);
  pg = site(pg, ps);
  diag = site(diag, dstride);
  n = site_n(ns, n);
  __shared__ double red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long j = (long)blockIdx.x * 64 + tx;
  const long rows = N / SENS_SPLIT, i0 = (long)blockIdx.y * rows, i1 = min(i0 + rows, (long)n);
  const int total = R + nvar;  // nvar = ndiag, or 0 when the variance is not wanted
  double* out = pg + (long)blockIdx.y * total * Mp + j;
#pragma unroll 1
  for (int k0 = 0; k0 < total; k0 += SENS_CHUNK) {
    double acc[SENS_CHUNK];
#pragma unroll
    for (int q = 0; q < SENS_CHUNK; ++q) acc[q] = 0.0;
    for (long i = i0 + ty; i < i1; i += 4) {
      const double b = (double)beta[i * Mp + j];
#pragma unroll
      for (int q = 0; q < SENS_CHUNK; ++q) {
        const int k = k0 + q;
        if (k < R) acc[q] += b * G[(long)k * N + i];
        else if (k < total) acc[q] += b * b * (double)diag[(long)(k - R) * nrow + i];
      }
    }
#pragma unroll
    for (int q = 0; q < SENS_CHUNK; ++q) {
      if (k0 + q < total) {  // (uniform)
        __syncthreads();
        red[ty][tx] = acc[q];
        __syncthreads();
        if (ty == 0) out[(long)(k0 + q) * Mp] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
      }
    }
  }
}

// The epilogue of a tile of D_p beta: every accumulator entry times the entry of beta it faces, summed over the tile's rows.  A lane
// owns NI column groups; its sums go to LDS by (row group, column) -- 2 wave rows x 4 lane rows -- and one thread per column adds
// the eight in order.  `smem` is the tile core's array, free once the product is complete.
template <typename T, typename G, typename FE, int BT>
__device__ __forceinline__ void sens_contract(typename G::acc_t (&acc)[G::MI][G::NI], const T* __restrict__ btile, long M, T* __restrict__ smem,
                                              double* __restrict__ out) {
  static_assert(sizeof(double) * 8 * BT <= sizeof(T) * (size_t)G::SMEM_ELEMS, "the column sums do not fit the tile core's LDS array");
  double s[G::NI];
#pragma unroll
  for (int ni = 0; ni < G::NI; ++ni) s[ni] = 0.0;
  int cnt = 0;  // (a compile-time constant in every unrolled call: entries come in (mi, ni, r) order)
  FE::foreach (acc, [&](int r, int c, T& v) {
    s[(cnt >> 2) % G::NI] += (double)v * (double)btile[(long)r * M + c];
    ++cnt;
  });
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double* red = reinterpret_cast<double*>(smem);
  __syncthreads();  // every wave is done with the operands' LDS image
#pragma unroll
  for (int ni = 0; ni < G::NI; ++ni) red[((w >> 1) * 4 + (lane >> 4)) * BT + (w & 1) * (BT / 2) + ni * 16 + (lane & 15)] = s[ni];
  __syncthreads();
  if (t < BT) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) v += red[g * BT + t];
    out[t] = v;
  }
}

// pq[p][bi][j] = sum_{i in row tile bi} beta_ij (D_p beta)_ij.  blockIdx.y = p (N / BT) + bi.
template <typename T>
__global__ __launch_bounds__(256, (TileCore<T, true, false>::OCC)) void sens_quad_kernel(const T* __restrict__ D, long N, const T* __restrict__ beta,
                                                                                         long M, double* __restrict__ pq, long wbs, long ps) {
  D = site(D, wbs);
  beta = site(beta, wbs);
  pq = site(pq, ps);
  using K = TileCore<T, true, false>;
  using G = typename K::G;
  __shared__ __attribute__((aligned(16))) T smem[K::SMEM_ELEMS];
  const int nbk = (int)(N / DGP_TILE), p = blockIdx.y / nbk, bi = blockIdx.y % nbk, bj = blockIdx.x;
  typename G::acc_t acc[G::MI][G::NI];
  G::zero(acc);
  K::run(D + (long)p * N * N + (long)bi * DGP_TILE * N, N, beta + (long)bj * DGP_TILE, M, (int)(N / 16), smem, acc);
  sens_contract<T, G, K, DGP_TILE>(acc, beta + (long)bi * DGP_TILE * M + (long)bj * DGP_TILE, M, smem,
                                   pq + ((long)p * nbk + bi) * M + (long)bj * DGP_TILE);
}

template <typename T>
__global__ __launch_bounds__(256, 2) void sens_quad64_kernel(const T* __restrict__ D, long N, const T* __restrict__ beta, long M,
                                                             double* __restrict__ pq, long wbs, long ps) {
  D = site(D, wbs);
  beta = site(beta, wbs);
  pq = site(pq, ps);
  using G = TileGemm<T, true, false, 64, 64>;
  __shared__ __attribute__((aligned(16))) T smem[G::SMEM_ELEMS];
  const int nb64 = (int)(N / 64), p = blockIdx.y / nb64, bi = blockIdx.y % nb64, bj = blockIdx.x;
  typename G::acc_t acc[G::MI][G::NI];
  G::zero(acc);
  G::template run<1, false>(D + (long)p * N * N + (long)bi * 64 * N, N, beta + (long)bj * 64, M, (int)(N / 16), smem, acc);
  sens_contract<T, G, G, 64>(acc, beta + (long)bi * 64 * M + (long)bj * 64, M, smem, pq + ((long)p * nb64 + bi) * M + (long)bj * 64);
}

// One thread per test point: the slab sums in slab order, finalize once per accumulator set, the prior term, the results.
template <typename T, typename M>
__global__ __launch_bounds__(256) void sens_finish_kernel(const T* __restrict__ Xst, long Mp, int m, int nt, int R, int nvar,
                                                          const PreBatch<M> pb, const double* __restrict__ pc, const double* __restrict__ pg,
                                                          const double* __restrict__ pq, int nq, double* __restrict__ dmean,
                                                          double* __restrict__ dvar, long wbs, long ps) {
  const typename M::Pre& pre = pb.get();
  Xst = site(Xst, wbs);
  pc = site(pc, ps);
  pg = site(pg, ps);
  const int total = R + nvar;
  dmean = site(dmean, (long)R * m);
  exp_table_init<T>();
  __syncthreads();
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  T sa[M::NTHETA], sb[M::NTHETA], pr[M::NTHETA];
#pragma unroll
  for (int p = 0; p < M::NTHETA; ++p) {
    double a = 0.0, b = 0.0;
    if (p < nt) {
      for (int z = 0; z < SENS_SPLIT; ++z) {
        a += pc[((long)z * 2 * nt + p) * Mp + j];
        b += pc[((long)z * 2 * nt + nt + p) * Mp + j];
      }
    }
    sa[p] = (T)a;
    sb[p] = (T)b;
    pr[p] = T(0);
  }
  M::finalize(sa, pre);
  M::finalize(sb, pre);
  if (dvar) {
    T x[M::NX], f[M::NF];
#pragma unroll
    for (int c = 0; c < M::NX; ++c) x[c] = Xst[(long)c * Mp + j];
    M::features(x, pre, f);
    (void)M::template pair<true>(f, f, pre, T(1), pr);
    M::finalize(pr, pre);
  }
  auto slabs = [&](int k) {
    double v = 0.0;
    for (int z = 0; z < SENS_SPLIT; ++z) v += pg[((long)z * total + k) * Mp + j];
    return v;
  };
#pragma unroll
  for (int p = 0; p < M::NTHETA; ++p)
    if (p < nt) dmean[(long)p * m + j] = (double)sa[p] - slabs(p);
  for (int k = nt; k < R; ++k) dmean[(long)k * m + j] = -slabs(k);
  if (!dvar) return;
  dvar = site(dvar, (long)(nt + nvar) * m);
  pq = site(pq, ps);
#pragma unroll
  for (int p = 0; p < M::NTHETA; ++p) {
    if (p < nt) {
      double q = 0.0;
      for (int z = 0; z < nq; ++z) q += pq[((long)p * nq + z) * Mp + j];
      dvar[(long)p * m + j] = ((double)pr[p] - 2.0 * (double)sb[p]) + q;
    }
  }
  for (int e = 0; e < nvar; ++e) dvar[(long)(nt + e) * m + j] = slabs(R + e);
}

template <typename T>
int sens_beta(const T* Tm, long N, const T* V, long Mp, T* beta, hipStream_t s, Batch bt, long wbs) {
  const unsigned Bz = (unsigned)bt.B;
  if (sens_small_tiles(N, Mp, bt))  // fewer 128-tiles than CUs: lauum's rule
    sens_beta64_kernel<T><<<dim3((unsigned)(Mp / 64), (unsigned)(N / 64), Bz), 256, 0, s>>>(Tm, N, V, Mp, beta, bt.ws, wbs);
  else
    sens_beta_kernel<T><<<dim3((unsigned)(Mp / DGP_TILE), (unsigned)(N / DGP_TILE), Bz), 256, 0, s>>>(Tm, N, V, Mp, beta, bt.ws, wbs);
  return (int)hipGetLastError();
}
template int sens_beta<double>(const double*, long, const double*, long, double*, hipStream_t, Batch, long);
template int sens_beta<float>(const float*, long, const float*, long, float*, hipStream_t, Batch, long);

// ------------------------------------------------------------------------------------------
// `work`: one site's slice (sens_layout), Xst and Ks already filled by the caller (pack_x + gram_cross: the hyperparameters of a
// batch of more than 8 are in pre_scratch).  wbs / ps: the slices' stride in plan-dtype elements / doubles.
template <typename T>
static int predict_sensitivity(int model, int d, const T* Xt, const T* Tm, const T* alpha, long N, int n, const double* theta, long Mp, int m,
                               const T* diag, int ndiag, const T* rhs, int nrhs, void* work, const SensLayout& L, double* dmean,
                               double* dvar, hipStream_t s, Batch bt, void* pre_scratch) {
  const int nt = model_ntheta(model, d);
  if (nt < 0) return -2;
  const int R = nt + ndiag + nrhs;
  const long nb64 = N / 64, nbk = N / DGP_TILE;
  if ((long)nt * nb64 > 65535 || Mp / 64 > 0x7fffffffL) return -2;  // (grid sizes; such a plan's work area fits no device)
  const long wbs = (long)(L.total / sizeof(T)), ps = (long)(L.total / sizeof(double));
  char* w = (char*)work;
  const T* Xst = (const T*)(w + L.Xst);
  T* D = (T*)(w + L.D);
  const T* Ks = (const T*)(w + L.Ks);
  T* V = (T*)(w + L.V);
  T* beta = (T*)(w + L.beta);
  double* G = (double*)(w + L.G);
  double* pc = (double*)(w + L.pc);
  double* pg = (double*)(w + L.pg);
  double* pq = (double*)(w + L.pq);
  const unsigned Bz = (unsigned)bt.B;
  int rc = fisher_dk<T>(model, d, Xt, N, n, theta, D, s, bt, wbs, pre_scratch, nullptr, false);
  if (rc) return rc;
  if ((rc = predict_v<T>(Tm, N, Ks, Mp, V, s, bt, wbs))) return rc;
  const bool small = sens_small_tiles(N, Mp, bt);
  if ((rc = sens_beta<T>(Tm, N, V, Mp, beta, s, bt, wbs))) return rc;
  sens_gcols_kernel<T><<<dim3((unsigned)(N / 4), (unsigned)R, Bz), 256, 0, s>>>(D, N, n, nt, ndiag, alpha, diag, rhs, (long)ndiag * n,
                                                                              (long)nrhs * n, G, bt.ws, wbs, ps, bt.ns);
  const dim3 slabs((unsigned)(Mp / 64), SENS_SPLIT, Bz);
  DGP_DISPATCH_MODEL(model, d, (sens_cross_kernel<T, M><<<slabs, dim3(256), 0, s>>>(
                                   Xt, N, n, Xst, Mp, m, nt, prepare_batch<M>(theta, nt, bt.B, pre_scratch, false, s), alpha, beta, pc, bt.ws,
                                   wbs, ps, bt.ns)));
  sens_bg_kernel<T><<<slabs, 256, 0, s>>>(beta, N, n, Mp, R, dvar ? ndiag : 0, G, diag, (long)ndiag * n, pg, wbs, ps, bt.ns);
  int nq = 0;
  if (dvar) {
    if (small) {
      nq = (int)nb64;
      sens_quad64_kernel<T><<<dim3((unsigned)(Mp / 64), (unsigned)(nt * nb64), Bz), 256, 0, s>>>(D, N, beta, Mp, pq, wbs, ps);
    } else {
      nq = (int)nbk;
      sens_quad_kernel<T><<<dim3((unsigned)(Mp / DGP_TILE), (unsigned)(nt * nbk), Bz), 256, 0, s>>>(D, N, beta, Mp, pq, wbs, ps);
    }
  }
  if ((rc = (int)hipGetLastError())) return rc;
  DGP_DISPATCH_MODEL(model, d, (sens_finish_kernel<T, M><<<dim3((unsigned)((m + 255) / 256), 1, Bz), dim3(256), 0, s>>>(
                                   Xst, Mp, m, nt, R, dvar ? ndiag : 0, prepare_batch<M>(theta, nt, bt.B, pre_scratch, false, s),
                                   pc, pg, pq, nq, dmean, dvar, wbs, ps)));
  return (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

#define DGP_SENS_MAX_COLS 8
static bool sens_sizes_ok(const dgp_plan* p, int64_t m, int ndiag, int nrhs) {
  return p && m > 0 && m <= 0x7fffffffLL - DGP_TILE_HOST && ndiag >= 0 && ndiag <= DGP_SENS_MAX_COLS && nrhs >= 0 && nrhs <= DGP_SENS_MAX_COLS;
}
template <typename T>
static int sensitivity(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* diag, int ndiag, const void* rhs, int nrhs,
                       void* work, double* dmean, double* dvar, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST);
  const SensLayout L = sens_layout(p->N, M, p->d, p->ntheta, ndiag, nrhs, p->elem);
  char* w = (char*)work;
  const int rc = cross<T>(p, theta, Xs, m, w + L.Xst, w + L.Ks, s, (long)(L.total / sizeof(T)));
  if (rc) return rc;
  return predict_sensitivity<T>(p->model, p->d, (const T*)p->Xt, (const T*)p->Tm, (const T*)p->alpha, p->N, (int)p->n, theta, M, (int)m,
                                (const T*)diag, ndiag, (const T*)rhs, nrhs, work, L, dmean, dvar, s, batch_of<T>(p), p->pre);
}

extern "C" {

size_t dgp_predict_sensitivity_workspace_bytes(const dgp_plan* p, int64_t m, int ndiag, int nrhs) {
  if (!sens_sizes_ok(p, m, ndiag, nrhs)) return 0;
  return sens_layout(p->N, round_up(m, DGP_TILE_HOST), p->d, p->ntheta, ndiag, nrhs, p->elem).total * (size_t)p->B;
}

int dgp_predict_sensitivity(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const void* diag, int ndiag, const void* rhs,
                            int nrhs, void* work, size_t work_bytes, double* dmean, double* dvar, void* stream) {
  const char* where = "dgp_predict_sensitivity";
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !dmean) return fail(DGP_E_ARG, "dgp_predict_sensitivity: null argument");
  if (m <= 0 || m > 0x7fffffffLL - DGP_TILE_HOST) return fail(DGP_E_ARG, "dgp_predict_sensitivity: m must be positive");
  if (ndiag < 0 || ndiag > DGP_SENS_MAX_COLS) return fail(DGP_E_ARG, "dgp_predict_sensitivity: ndiag must be 0..8");
  if (nrhs < 0 || nrhs > DGP_SENS_MAX_COLS) return fail(DGP_E_ARG, "dgp_predict_sensitivity: nrhs must be 0..8");
  if (ndiag > 0 && !diag) return fail(DGP_E_ARG, "dgp_predict_sensitivity: ndiag > 0 needs the diagonal directions");
  if (nrhs > 0 && !rhs) return fail(DGP_E_ARG, "dgp_predict_sensitivity: nrhs > 0 needs the right-hand-side columns");
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  int rc = need_factor(p, where, "call dgp_factorize or dgp_fit_step");
  if (rc || (rc = need_work(work, work_bytes, dgp_predict_sensitivity_workspace_bytes(p, m, ndiag, nrhs), where)) ||
      (rc = factor_ok(p, s, where)))
    return rc;
  rc = DGP_BY_DTYPE(p, sensitivity<double>(p, theta, Xs, m, diag, ndiag, rhs, nrhs, work, dmean, dvar, s),
                    sensitivity<float>(p, theta, Xs, m, diag, ndiag, rhs, nrhs, work, dmean, dvar, s));
  return wrap(rc, where);
}

}  // extern "C"
