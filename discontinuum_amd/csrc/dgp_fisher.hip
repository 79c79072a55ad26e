// dgp_fisher.hip -- the exact FISHER INFORMATION of the hyperparameters from the factorisation a plan holds.
//
// For the Gaussian marginal likelihood the expected information of the covariance parameters is (Mardia & Marshall 1984)
//     F_ab = 1/2 tr(K^^-1 D_a K^^-1 D_b),        D_a = dK^/dtheta_a  (a "direction": a symmetric derivative matrix of K^).
// With T = L^-1 (K^^-1 = T^T T) and the half-sandwich G_a = T D_a T^T (symmetric) this is F_ab = 1/2 <G_a, G_b>_F.
// Directions: the P kernel directions dK/dtheta_p (dense, Model::pair<true> + finalize per entry) and E caller-supplied
// DIAGONAL ones diag(d_e) (learned noise terms).  Only first derivatives of the kernels are needed, and F is positive
// semi-definite by construction.  Passes, all with gridDim.z = sites (ragged batches through site_n):
//
//   fisher_dk       all P matrices D_p at once, each FULL and symmetric in its own N x N slot of the work area: one
//                   pair<true> evaluation with weight 1 into a zeroed accumulator per entry, gram_sym's 64 x 64 tiling over
//                   the whole square.  The identity pad of K^ has derivative 0: rows and columns >= n_b are zero.
//   V_a = T D_a     dgp_chol.hip::predict_v at width N -- the prediction's GEMM, unchanged.  A diagonal direction needs no
//                   GEMM: V_e[i][k] = T[i][k] d_e[k] (fisher_scale).
//   G_a = V_a T^T   fisher_sandwich: lower tiles only, G_a[i][j] = sum_{k <= j} V_a[i][k] T[j][k]; both operands
//                   k-contiguous, the k-range ends with block column j.  The project's tile cores: the direct-to-LDS
//                   128 x 128 one, or 64 x 64 register-staged tiles while a launch has too few 128-tiles (lauum's rule and
//                   selector); k-tiles small-to-large (REV) as in lauum.  G_a overwrites the slot that held D_a.
//   fisher_dot /    1/2 <G_a, G_b> over the full matrices from the lower triangles (off-diagonal entries twice, the diagonal
//   fisher_reduce   once), in DOUBLE whatever the plan's dtype: per 64 x 64 tile and direction a the sums against every
//                   b <= a, then one workgroup per pair adds the tiles in a fixed order and writes F[a][b] and F[b][a].
// No floating-point atomics, fixed summation orders: bitwise repeatable.  Reads T only; A, S, alpha and the result row of the
// fit step are never touched.  Flops: (P + E) (4/3) N^3 on the matrix cores (2/3 N^3 for a diagonal direction).
#include "dgp_gemm.h"
#include "dgp_gemm_dma.h"
#include "dgp_plan.h"
#include "dgp_models.h"
#include "dgp_gram_shared.h"

namespace dgp {

static constexpr int FISHER_MAX_DIR = DGP_MAX_THETA + 8;  // kernel directions + diagonal ones

// D_p[i][j] = dk(x_i, x_j)/dtheta_p for every p < nt, slot p of the work area (slot stride N^2).  One workgroup per
// 64 x 64 tile of the whole square; thread (ty, tx) owns rows ty + 16 a, columns tx + 16 b, so that the 16 lanes of a row
// store one 128-byte line.  One entry at a time like gram_grad_kernel: the derivative expressions are register-hungry.
template <typename T, typename M>
__global__ __launch_bounds__(256) void fisher_dk_kernel(const T* __restrict__ Xt, long N, int n, int nt, const PreBatch<M> pb,
                                                        T* __restrict__ G, long bs, long wbs, const int* __restrict__ ns) {
  const typename M::Pre& pre = pb.get();
  Xt = site(Xt, bs);
  G = site(G, wbs);
  n = site_n(ns, n);
  __shared__ T sfi[M::NF][64], sfj[M::NF][64];
  const int nb = (int)(N / 64);
  const int bi = blockIdx.x / nb, bj = blockIdx.x % nb;
  const int t = threadIdx.x;
  exp_table_init<T>();
  if (t < 64) stage_strip<T, M>(Xt, N, (long)bi * 64, pre, sfi, t);
  else if (t < 128) stage_strip<T, M>(Xt, N, (long)bj * 64, pre, sfj, t - 64);
  __syncthreads();
  const int ty = t >> 4, tx = t & 15;
  const long slot = N * N;
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {
    const int ri = ty + 16 * a;
    const long gi = (long)bi * 64 + ri;
    T fi[M::NF];
#pragma unroll
    for (int c = 0; c < M::NF; ++c) fi[c] = sfi[c][ri];
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
      const int cj = tx + 16 * b;
      const long gj = (long)bj * 64 + cj;
      T fj[M::NF];
#pragma unroll
      for (int c = 0; c < M::NF; ++c) fj[c] = sfj[c][cj];
      T acc[M::NTHETA];
#pragma unroll
      for (int p = 0; p < M::NTHETA; ++p) acc[p] = T(0);
      (void)M::template pair<true>(fi, fj, pre, T(1), acc);
      M::finalize(acc, pre);
      const bool pad = gi >= n || gj >= n;
      T* dst = G + gi * N + gj;
#pragma unroll
      for (int p = 0; p < M::NTHETA; ++p)
        if (p < nt) dst[(long)p * slot] = pad ? T(0) : acc[p];
    }
  }
}

// V[i][k] = T[i][k] d[k] for k <= i, k < n_b; 0 elsewhere (the whole N x N buffer is written).  One workgroup per 128
// consecutive k of one row, rows and row segments folded into blockIdx.x (N / 128 segments a row).
template <typename T>
__global__ __launch_bounds__(128) void fisher_scale_kernel(const T* __restrict__ Tm, long N, int n, const T* __restrict__ dvec,
                                                           long dstride, T* __restrict__ V, long bs, long wbs,
                                                           const int* __restrict__ ns) {
  Tm = site(Tm, bs);
  V = site(V, wbs);
  dvec = site(dvec, dstride);
  n = site_n(ns, n);
  const long seg = N / DGP_TILE;
  const long i = blockIdx.x / seg, k = (blockIdx.x % seg) * DGP_TILE + threadIdx.x;
  V[i * N + k] = (k <= i && k < n) ? Tm[i * N + k] * dvec[k] : T(0);
}

// G[i][j] = sum_{k <= j} V[i][k] T[j][k], lower tiles (bi >= bj).  Operand A = rows of V, operand B = rows of T, both
// k-contiguous; the k-range [0, end of block column bj) is visited from its LAST k-tile down to the first (REV): T's rows
// are largest next to the diagonal, so the small products are summed first, as in lauum.  Above the diagonal inside its
// diagonal blocks T holds zeros (predict_v relies on the same).
template <typename T>
__global__ __launch_bounds__(256, (TileCore<T, true, true>::OCC)) void fisher_sandwich_kernel(const T* __restrict__ V, const T* __restrict__ Tm, long N,
                                                                                              T* __restrict__ G, long bs, long wbs) {
  V = site(V, wbs);
  G = site(G, wbs);
  Tm = site(Tm, bs);
  using K = TileCore<T, true, true>;
  using GT = typename K::G;
  __shared__ T smem[K::SMEM_ELEMS];
  int tr, tc;
  tri_decode(blockIdx.x, tr, tc);
  // the k-range grows with the block COLUMN: the mirrored triangle (still bi >= bj) dispatches the long-K tiles first
  const int nbk = (int)(N / DGP_TILE), bi = nbk - 1 - tc, bj = nbk - 1 - tr;
  typename GT::acc_t acc[GT::MI][GT::NI];
  GT::zero(acc);
  K::template run<true>(V + (long)bi * DGP_TILE * N, N, Tm + (long)bj * DGP_TILE * N, N, (bj + 1) * (DGP_TILE / 16), smem, acc);
  T* out = G + (long)bi * DGP_TILE * N + (long)bj * DGP_TILE;
  K::foreach (acc, [&](int r, int c, T& v) { out[(long)r * N + c] = v; });
}

// the same product in 64 x 64 tiles: four times the workgroups, for matrices whose 128 x 128 tiles do not fill the CUs
template <typename T>
__global__ __launch_bounds__(256, 2) void fisher_sandwich64_kernel(const T* __restrict__ V, const T* __restrict__ Tm, long N,
                                                                   T* __restrict__ G, long bs, long wbs) {
  V = site(V, wbs);
  G = site(G, wbs);
  Tm = site(Tm, bs);
  using GT = TileGemm<T, true, true, 64, 64>;
  __shared__ T smem[GT::SMEM_ELEMS];
  int bi, bj;
  tri_decode(blockIdx.x, bi, bj);
  typename GT::acc_t acc[GT::MI][GT::NI];
  GT::zero(acc);
  GT::template run<1, true>(V + (long)bi * 64 * N, N, Tm + (long)bj * 64 * N, N, (bj + 1) * (64 / 16), smem, acc);
  T* out = G + (long)bi * 64 * N + (long)bj * 64;
  GT::foreach (acc, [&](int r, int c, T& v) { out[(long)r * N + c] = v; });
}

// part[tile][a][b] = sum over the 64 x 64 lower tile of w G_a G_b for every b <= a (a = blockIdx.y), w = 1 below the
// diagonal, 1/2 on it, 0 above: 1/2 <G_a, G_b> over the full symmetric matrices.  Double accumulators, a wave reads one
// 64-element row per instruction; wave shuffle + LDS, fixed order.
template <typename T>
__global__ __launch_bounds__(256) void fisher_dot_kernel(const T* __restrict__ G, long N, int nd, double* __restrict__ part,
                                                         long wbs, long ps) {
  G = site(G, wbs);
  part = site(part, ps);
  __shared__ double red[4][FISHER_MAX_DIR];
  int bi, bj;
  tri_decode(blockIdx.x, bi, bj);
  const int a = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long slot = N * N;
  double acc[FISHER_MAX_DIR];
#pragma unroll
  for (int b = 0; b < FISHER_MAX_DIR; ++b) acc[b] = 0.0;
#pragma unroll 1
  for (int e = 0; e < 16; ++e) {
    const int r = wv + 4 * e;
    const long gi = (long)bi * 64 + r, gj = (long)bj * 64 + lane;
    const T* q = G + gi * N + gj;
    const double w = gj < gi ? 1.0 : (gj == gi ? 0.5 : 0.0);
    const double ga = w == 0.0 ? 0.0 : w * (double)q[(long)a * slot];  // (nothing above the diagonal is read: unspecified there)
#pragma unroll
    for (int b = 0; b < FISHER_MAX_DIR; ++b)
      if (b <= a) acc[b] += w == 0.0 ? 0.0 : ga * (double)q[(long)b * slot];
  }
#pragma unroll
  for (int b = 0; b < FISHER_MAX_DIR; ++b) {
    if (b <= a) {
      const double v = wave_sum(acc[b]);
      if (lane == 0) red[wv][b] = v;
    }
  }
  __syncthreads();
  if (t <= a) part[((long)blockIdx.x * nd + a) * nd + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// F[a][b] = F[b][a] = sum over the tiles, fixed strided order + fixed tree: one workgroup per pair b <= a
__global__ __launch_bounds__(256) void fisher_reduce_kernel(const double* __restrict__ part, long ntile, int nd,
                                                            double* __restrict__ F, long ps) {
  const int a = blockIdx.x, b = blockIdx.y;
  if (b > a) return;
  part = site(part, ps);
  F = site(F, (long)nd * nd);
  __shared__ double red[256];
  double v = 0.0;
  for (long tl = threadIdx.x; tl < ntile; tl += 256) v += part[(tl * nd + a) * nd + b];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    F[(long)a * nd + b] = red[0];
    F[(long)b * nd + a] = red[0];
  }
}

// ------------------------------------------------------------------------------------------
// work area per site: nd + 1 matrices of N x N plan-dtype elements (the nd directions' slots, then V) and
// (N/64)(N/64 + 1)/2 x nd x nd doubles of tile partials.  D_a lives in G_a's slot until its own product overwrites it, so
// no separate buffer for the derivative matrix is needed.
static long fisher_tiles(long N) { return (N / 64) * (N / 64 + 1) / 2; }

struct FisherLayout {
  size_t part, total;  // the matrices come first: slot a at a x Carve::up(elem N^2)
};
static FisherLayout fisher_layout(long N, int nd, size_t elem) {
  FisherLayout L;
  Carve c;
  for (int a = 0; a <= nd; ++a) c.take(elem * (size_t)N * (size_t)N);
  L.part = c.take(sizeof(double) * (size_t)fisher_tiles(N) * (size_t)nd * (size_t)nd);
  L.total = c.o;
  return L;
}
static size_t fisher_site_bytes(long N, int nd, size_t elem) { return fisher_layout(N, nd, elem).total; }

// the sweep's launch, shared with dgp_sensitivity.hip: slot p of G (slot stride N^2, site stride wbs) <- D_p, p < ntheta.
// upload = false: the hyperparameters of a batch of more than 8 are already in pre_scratch (an earlier launcher of the same call).
template <typename T>
int fisher_dk(int model, int d, const T* Xt, long N, int n, const double* theta, T* G, hipStream_t s, Batch bt, long wbs,
              void* pre_scratch, void* pre_staging, bool upload) {
  const int nt = model_ntheta(model, d);
  if (nt < 0) return -2;
  const long nb64 = N / 64;
  DGP_DISPATCH_MODEL(model, d, (fisher_dk_kernel<T, M><<<dim3((unsigned)(nb64 * nb64), 1, (unsigned)bt.B), dim3(256), 0, s>>>(
                                   Xt, N, n, nt, prepare_batch<M>(theta, nt, bt.B, pre_scratch, upload, s, pre_staging), G, bt.ws, wbs,
                                   bt.ns)));
  return (int)hipGetLastError();
}

// F_ab = 1/2 tr(K^^-1 D_a K^^-1 D_b) over the nt kernel directions dK/dtheta_p and `ndiag` diagonal directions diag [B][ndiag][n],
// from T = L^-1.  `work`: fisher_site_bytes per site; F [B][nt + ndiag][nt + ndiag] doubles.  Reads Xt and T only.
template <typename T>
static int fisher(int model, int d, const T* Xt, const T* Tm, long N, int n, const double* theta, const T* diag, int ndiag, void* work,
                  double* F, hipStream_t s, Batch bt, void* pre_scratch, void* pre_staging) {
  const int nt = model_ntheta(model, d);
  if (nt < 0) return -2;
  const int nd = nt + ndiag;
  if (nd > FISHER_MAX_DIR || N * (N / DGP_TILE) > 0x7fffffffL) return -2;  // (grid sizes; such a plan's work area fits no device)
  const size_t site_bytes = fisher_site_bytes(N, nd, sizeof(T));
  const long wbs = (long)(site_bytes / sizeof(T)), ps = (long)(site_bytes / sizeof(double));
  const long slot = N * N;
  T* G = (T*)work;
  T* V = G + (long)nd * slot;
  double* part = (double*)((char*)work + fisher_layout(N, nd, sizeof(T)).part);
  const unsigned Bz = (unsigned)bt.B;
  int rc = fisher_dk<T>(model, d, Xt, N, n, theta, G, s, bt, wbs, pre_scratch, pre_staging, true);
  if (rc) return rc;
  const int nbk = (int)(N / DGP_TILE);
  const int tiles = nbk * (nbk + 1) / 2;
  const bool small = (long)tiles * bt.B <= bt.tuning().lauum64_max_tiles;  // fewer 128-tiles than CUs: lauum's rule
  for (int a = 0; a < nd; ++a) {
    T* Ga = G + (long)a * slot;
    if (a < nt) {
      if ((rc = predict_v<T>(Tm, N, Ga, N, V, s, bt, wbs))) return rc;
    } else {
      fisher_scale_kernel<T><<<dim3((unsigned)(N * (N / DGP_TILE)), 1, Bz), DGP_TILE, 0, s>>>(
          Tm, N, n, diag + (long)(a - nt) * n, (long)ndiag * n, V, bt.ws, wbs, bt.ns);
    }
    if (small) fisher_sandwich64_kernel<T><<<dim3((unsigned)fisher_tiles(N), 1, Bz), 256, 0, s>>>(V, Tm, N, Ga, bt.ws, wbs);
    else fisher_sandwich_kernel<T><<<dim3((unsigned)tiles, 1, Bz), 256, 0, s>>>(V, Tm, N, Ga, bt.ws, wbs);
  }
  fisher_dot_kernel<T><<<dim3((unsigned)fisher_tiles(N), (unsigned)nd, Bz), 256, 0, s>>>(G, N, nd, part, wbs, ps);
  fisher_reduce_kernel<<<dim3((unsigned)nd, (unsigned)nd, Bz), 256, 0, s>>>(part, fisher_tiles(N), nd, F, ps);
  return (int)hipGetLastError();
}

template int fisher_dk<double>(int, int, const double*, long, int, const double*, double*, hipStream_t, Batch, long, void*, void*, bool);
template int fisher_dk<float>(int, int, const float*, long, int, const double*, float*, hipStream_t, Batch, long, void*, void*, bool);

}  // namespace dgp

using namespace dgp;

#define DGP_FISHER_MAX_DIAG 8

extern "C" {

size_t dgp_fisher_workspace_bytes(const dgp_plan* p, int ndiag) {
  if (!p || ndiag < 0 || ndiag > DGP_FISHER_MAX_DIAG) return 0;
  return fisher_site_bytes(p->N, p->ntheta + ndiag, p->elem) * (size_t)p->B;
}

int dgp_fisher(dgp_plan* p, const double* theta, const void* diag, int ndiag, void* work, size_t work_bytes, double* fisher_out,
               void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !fisher_out) return fail(DGP_E_ARG, "dgp_fisher: null argument");
  if (ndiag < 0 || ndiag > DGP_FISHER_MAX_DIAG) return fail(DGP_E_ARG, "dgp_fisher: ndiag must be 0..8");
  if (ndiag > 0 && !diag) return fail(DGP_E_ARG, "dgp_fisher: ndiag > 0 needs the diagonal directions");
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  int rc = need_factor(p, "dgp_fisher", "call dgp_factorize or dgp_fit_step");
  if (rc || (rc = need_work(work, work_bytes, dgp_fisher_workspace_bytes(p, ndiag), "dgp_fisher")) || (rc = factor_ok(p, s, "dgp_fisher")))
    return rc;
  PreSlot slot(p, s);
  rc = DGP_BY_DTYPE(
      p,
      fisher<double>(p->model, p->d, (const double*)p->Xt, (const double*)p->Tm, p->N, (int)p->n, theta, (const double*)diag, ndiag, work,
                     fisher_out, s, batch_of<double>(p), p->pre, slot.staging),
      fisher<float>(p->model, p->d, (const float*)p->Xt, (const float*)p->Tm, p->N, (int)p->n, theta, (const float*)diag, ndiag, work,
                    fisher_out, s, batch_of<float>(p), p->pre, slot.staging));
  return wrap(rc, "dgp_fisher");
}

}  // extern "C"
