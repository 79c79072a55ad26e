// dgp_loo.hip -- the exact LEAVE-ONE-OUT predictive likelihood as a training objective, with its full gradient.  fp64, single-site
// or batched (blockIdx.z = site, ragged sizes through site_n).
//
// With S = K^^-1 and alpha = S r as the fit step leaves them in the plan, k_i = S_ii:
//     L_LOO        = sum_{i < n} [ 1/2 log 2 pi - 1/2 log k_i + alpha_i^2 / (2 k_i) ]      (the negative elpd of cross_validate)
//     w_i          = (1 + alpha_i^2 / k_i) / (2 k_i),   c_i = alpha_i / k_i,   M = S diag(w) S,   b = S c
//     dL/dtheta_p  = 1/2 tr( (2 M - b alpha^T - alpha b^T) dK/dtheta_p ),   dL/dr = b,   dL/dnoise_i = M_ii - b_i alpha_i
// Identity-pad rows (i >= n) have k = 1, alpha = 0: w = 1/2, c = 0; they add nothing to L and reach only M's pad block.
//
//   loo_terms_kernel     one row per thread: k_i from S's diagonal, 2 w_i, c_i and the row's summand; block partials of the sum and
//                        of the first bad row (k_i <= 0 or not finite)
//   loo_mirror_kernel    F = S with its upper triangle filled from the lower (nothing above S's diagonal is read) and
//                        G = F diag(2 w), 64 x 64 tiles through LDS: both written row-major, so that
//   loo_sandwich_kernel  2 M = F G^T is ONE A B^T product of two k-contiguous operands on the tile cores (TileCore: the
//                        direct-to-LDS core for 128 x 128 tiles, the register-staged one for 64 x 64 tiles while a launch has too
//                        few of them -- lauum's rule and selector), lower tiles only, k ascending over the whole range.  The weight
//                        sits on the k index in double (the factor 2 is exact)
//   b = S c              dgp_chol.hip::symv_lower, one read of the lower triangle, fixed-order partials
//   the contraction      gram_grad on 2 M with a zero vector (1/2 tr(2 M dK)), then gram_bilinear(-b, alpha) added in place
//   loo_result_kernel    dr = b, dnoise_i = 1/2 (2 M)_ii - b_i alpha_i and the block partials of the four reduced slots
//   loo_finish_kernel    one workgroup per site: both sets of partials in a fixed order, the result row
// No floating-point atomics, two-stage fixed-order reductions: every result repeats bitwise, and a site's result does not depend on
// the batch it is in.
#include "../../include/dgp_hip.h"
#include "dgp_gemm_dma.h"
#include "dgp_loo.h"
#include "dgp_plan.h"

namespace dgp {

#define LOO_LOG2PI 1.83787706640934548356
LooLayout loo_layout(const dgp_plan* p, bool value_only) {
  const Layout P = layout(p);
  const size_t N = (size_t)p->N, B = (size_t)p->B;
  LooLayout L;
  L.slice = value_only ? 0 : p->site_bytes;
  L.F = P.A;
  L.G = P.Tm;
  L.M = P.S;
  L.zero = P.alpha;
  L.gpart = P.gpart;
  L.nblk = (int)((N + 255) / 256);
  Carve v;  // a site's vectors
  L.w = v.take(sizeof(double) * N);
  L.c = v.take(sizeof(double) * N);
  L.b = v.take(sizeof(double) * N);
  L.negb = v.take(sizeof(double) * N);
  L.spart = v.take(sizeof(double) * (size_t)solve_partials(p->N));
  L.part = v.take(sizeof(double) * (size_t)L.nblk * LOO_PART);
  L.vec = v.o;
  L.vecs = B * L.slice;
  Carve c;
  c.o = L.vecs + B * L.vec;
  L.out0 = c.take(sizeof(double) * B * DGP_OUT_LEN);
  L.total = c.o;
  return L;
}

// fixed order: lanes by the shuffle tree, then the four waves
template <int K>
__device__ __forceinline__ void loo_block_sums(double (&v)[K], double* red /* LDS [4][K] */) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const double x = wave_sum(v[q]);
    if (lane == 0) red[wv * K + q] = x;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void loo_terms_kernel(const double* __restrict__ S, const double* __restrict__ alpha, long N, int n,
                                                        long bs, const int* __restrict__ ns, double* __restrict__ w2,
                                                        double* __restrict__ c, double* __restrict__ part, long vs) {
  n = site_n(ns, n);
  S = site(S, bs);
  alpha = site(alpha, bs);
  w2 = site(w2, vs);
  c = site(c, vs);
  part = site(part, vs);
  __shared__ double red[4 * 2];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double v[2] = {0.0, 0.0};  // the row's summand (the second column is unused)
  double bad = 0.0;
  if (i < N) {
    double wi = 1.0, ci = 0.0;  // the pad: k = 1, alpha = 0
    if (i < n) {
      const double k = S[i * N + i], a = alpha[i];
      const double q = a * a / k;
      wi = (1.0 + q) / k;  // 2 w_i
      ci = a / k;
      v[0] = 0.5 * LOO_LOG2PI - 0.5 * log(k) + 0.5 * q;
      if (!(k > 0.0) || !isfinite(k)) bad = (double)(i + 1);
    }
    w2[i] = wi;
    c[i] = ci;
  }
  // the first bad row of the block: a minimum over the rows that are bad (0 = none), lanes then waves, order-free
  double m = bad > 0.0 ? bad : 1e300;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_down(m, off, 64));
  __shared__ double redm[4];
  if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = m;
  loo_block_sums<2>(v, red);
  if (threadIdx.x == 0) {
    part[(long)blockIdx.x * LOO_PART + 0] = (red[0] + red[2]) + (red[4] + red[6]);
    const double mm = fmin(fmin(redm[0], redm[1]), fmin(redm[2], redm[3]));
    part[(long)blockIdx.x * LOO_PART + 1] = mm < 1e299 ? mm : 0.0;
  }
}

// tile (bi, bj), bi >= bj, of the lower triangle of S -> the tiles (bi, bj) and (bj, bi) of F and G
__global__ __launch_bounds__(256) void loo_mirror_kernel(const double* __restrict__ S, long N, long bs, const double* __restrict__ w2,
                                                         long vs, double* __restrict__ F, double* __restrict__ G) {
  S = site(S, bs);
  w2 = site(w2, vs);
  F = site(F, bs);
  G = site(G, bs);
  __shared__ double tile[64][65];
  int bi, bj;
  tri_decode(blockIdx.x, bi, bj);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)bi * 64, c0 = (long)bj * 64;
  for (int r = ty; r < 64; r += 4) {
    // a diagonal tile is valid on and below its diagonal only
    tile[r][tx] = (bi != bj || tx <= r) ? S[(r0 + r) * N + c0 + tx] : 0.0;
  }
  __syncthreads();
  if (bi != bj) {
    const double wc = w2[c0 + tx], wr = w2[r0 + tx];
    for (int r = ty; r < 64; r += 4) {
      const double v = tile[r][tx];
      F[(r0 + r) * N + c0 + tx] = v;
      G[(r0 + r) * N + c0 + tx] = v * wc;
      const double u = tile[tx][r];  // (row c0 + r, column r0 + tx) of the mirror tile
      F[(c0 + r) * N + r0 + tx] = u;
      G[(c0 + r) * N + r0 + tx] = u * wr;
    }
  } else {
    const double wc = w2[c0 + tx];
    for (int r = ty; r < 64; r += 4) {
      const double v = tx <= r ? tile[r][tx] : tile[tx][r];
      F[(r0 + r) * N + c0 + tx] = v;
      G[(r0 + r) * N + c0 + tx] = v * wc;
    }
  }
}

// (2 M)[I, J] = sum_k F[I, k] G[J, k], I >= J: both operands k-contiguous rows, k ascending over all of 0 .. N - 1
template <int BT>
__global__ __launch_bounds__(256, (TileCore<double, true, true, BT, BT>::OCC)) void loo_sandwich_kernel(const double* __restrict__ F,
                                                                                                         const double* __restrict__ G,
                                                                                                         double* __restrict__ M2, long N,
                                                                                                         long bs) {
  F = site(F, bs);
  G = site(G, bs);
  M2 = site(M2, bs);
  using K = TileCore<double, true, true, BT, BT>;
  using TG = typename K::G;
  __shared__ double smem[K::SMEM_ELEMS];
  int bi, bj;
  tri_decode(blockIdx.x, bi, bj);  // ascending rows; every tile has the same k-range
  typename TG::acc_t acc[TG::MI][TG::NI];
  TG::zero(acc);
  K::run(F + (long)bi * BT * N, N, G + (long)bj * BT * N, N, (int)(N / 16), smem, acc);
  double* out = M2 + (long)bi * BT * N + (long)bj * BT;
  K::foreach (acc, [&](int r, int c, double& v) { out[(long)r * N + c] = v; });
}

__global__ __launch_bounds__(256) void loo_negate_kernel(const double* __restrict__ b, double* __restrict__ negb, long N, long vs) {
  b = site(b, vs);
  negb = site(negb, vs);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < N) negb[i] = -b[i];
}

__global__ __launch_bounds__(256) void loo_result_kernel(const double* __restrict__ M2, const double* __restrict__ alpha, long N, int n,
                                                         long bs, const int* __restrict__ ns, const double* __restrict__ b,
                                                         const double* __restrict__ wts, double* __restrict__ dr,
                                                         double* __restrict__ dnoise, double* __restrict__ part, long vs) {
  const int nfull = n;
  n = site_n(ns, n);
  M2 = site(M2, bs);
  alpha = site(alpha, bs);
  b = site(b, vs);
  part = site(part, vs);
  if (wts) wts = site(wts, 2 * (long)nfull);  // [site][2][n]
  if (dr) dr = site(dr, (long)nfull);
  if (dnoise) dnoise = site(dnoise, (long)nfull);
  __shared__ double red[4 * 4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < nfull) {
    const double bi = i < n ? b[i] : 0.0;
    const double dn = i < n ? 0.5 * M2[i * N + i] - bi * alpha[i] : 0.0;
    if (dr) dr[i] = bi;
    if (dnoise) dnoise[i] = dn;
    v[0] = bi;
    if (wts && i < n) {
      v[1] = bi * wts[i];
      v[2] = bi * wts[nfull + i];
    }
    v[3] = dn;
  }
  loo_block_sums<4>(v, red);
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    part[(long)blockIdx.x * LOO_PART + 2 + q] = (red[q] + red[4 + q]) + (red[8 + q] + red[12 + q]);
  }
}

// one workgroup per site.  full: the result row `out` (DGP_OUT_LEN, dtheta already in place) from the step's own row `out0`;
// else out = [value, info] alone (info0: the plan's factorisation status)
__global__ __launch_bounds__(256) void loo_finish_kernel(const double* __restrict__ part, int nblk, long vs, int ntheta, int full,
                                                         const double* __restrict__ out0, const int* __restrict__ info0, long ibs,
                                                         double* __restrict__ out) {
  part = site(part, vs);
  __shared__ double red[256];
  __shared__ double tot[6];
  const int t = threadIdx.x;
  for (int q = 0; q < (full ? 6 : 2); ++q) {
    double v = q == 1 ? 1e300 : 0.0;
    for (int g = t; g < nblk; g += 256) {
      const double x = part[(long)g * LOO_PART + q];
      v = q == 1 ? (x > 0.0 ? fmin(v, x) : v) : v + x;
    }
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] = q == 1 ? fmin(red[t], red[t + s]) : red[t] + red[t + s];
      __syncthreads();
    }
    if (t == 0) tot[q] = red[0];
    __syncthreads();
  }
  if (t != 0 && !(full && t >= DGP_OUT_DTHETA + ntheta && t < DGP_OUT_LEN)) return;
  double finfo;
  if (full) {
    out0 = site(out0, (long)DGP_OUT_LEN);
    out = site(out, (long)DGP_OUT_LEN);
    finfo = out0[DGP_OUT_INFO];
  } else {
    out = site(out, 2);
    finfo = (double)site(info0, ibs)[0];
  }
  if (t == 0) {
    const double badrow = tot[1] < 1e299 ? tot[1] : 0.0;
    const bool ok = finfo == 0.0 && badrow == 0.0;
    const double value = ok ? tot[0] : __builtin_nan("");
    const double info = finfo != 0.0 ? finfo : badrow;
    if (full) {
      out[DGP_OUT_NLL] = value;
      out[DGP_OUT_QUAD] = out0[DGP_OUT_QUAD];
      out[DGP_OUT_LOGDET] = out0[DGP_OUT_LOGDET];
      out[DGP_OUT_INFO] = info;
    } else {
      out[0] = value;
      out[1] = info;
    }
  } else {
    out[t] = t >= DGP_OUT_SUM_DR ? tot[2 + t - DGP_OUT_SUM_DR] : 0.0;
  }
}

static int loo_terms(const double* S, const double* alpha, long N, int n, char* work, const LooLayout& L, hipStream_t s, const Batch& bt) {
  char* vec = work + L.vecs;
  const long vs = (long)(L.vec / sizeof(double));
  loo_terms_kernel<<<dim3((unsigned)L.nblk, 1, (unsigned)bt.B), 256, 0, s>>>(S, alpha, N, n, bt.ws, bt.ns, (double*)(vec + L.w),
                                                                            (double*)(vec + L.c), (double*)(vec + L.part), vs);
  return (int)hipGetLastError();
}

int loo_finish_value(const int* info, char* work, const LooLayout& L, double* out2, hipStream_t s, const Batch& bt) {
  loo_finish_kernel<<<dim3(1, 1, (unsigned)bt.B), 256, 0, s>>>((const double*)(work + L.vecs + L.part), L.nblk,
                                                              (long)(L.vec / sizeof(double)), 0, 0, nullptr, info,
                                                              bt.ws * (long)sizeof(double) / (long)sizeof(int), out2);
  return (int)hipGetLastError();
}

static int loo_value(const double* S, const double* alpha, const int* info, long N, int n, char* work, const LooLayout& L, double* out2,
              hipStream_t s, Batch bt) {
  int rc;
  if ((rc = loo_terms(S, alpha, N, n, work, L, s, bt))) return rc;
  return loo_finish_value(info, work, L, out2, s, bt);
}

int loo_mirror(const double* S, long N, const double* w2, char* work, const LooLayout& L, hipStream_t s, const Batch& bt) {
  const long nb64 = N / 64;
  loo_mirror_kernel<<<dim3((unsigned)(nb64 * (nb64 + 1) / 2), 1, (unsigned)bt.B), 256, 0, s>>>(
      S, N, bt.ws, w2, (long)(L.vec / sizeof(double)), (double*)(work + L.F), (double*)(work + L.G));
  return (int)hipGetLastError();
}

int loo_tail(int model, int d, const double* Xt, const double* S, const double* alpha, long N, int n, const double* theta,
             const double* wts, char* work, const LooLayout& L, double* out, double* dr, double* dnoise, hipStream_t s, const Batch& bt,
             void* pre_scratch) {
  const int nt = model_ntheta(model, d);
  if (nt < 0) return -2;
  auto W = [&](size_t off) { return (double*)(work + off); };
  auto V = [&](size_t off) { return (double*)(work + L.vecs + off); };
  const long vs = (long)(L.vec / sizeof(double));
  const unsigned Bz = (unsigned)bt.B;
  int rc;
  const long nb64 = N / 64;
  const long nbk = N / DGP_TILE_HOST, tiles = nbk * (nbk + 1) / 2;
  if (tiles * bt.B <= bt.tuning().lauum64_max_tiles)  // fewer 128-tiles than fill the CUs: lauum's rule
    loo_sandwich_kernel<64><<<dim3((unsigned)(nb64 * (nb64 + 1) / 2), 1, Bz), 256, 0, s>>>(W(L.F), W(L.G), W(L.M), N, bt.ws);
  else
    loo_sandwich_kernel<128><<<dim3((unsigned)tiles, 1, Bz), 256, 0, s>>>(W(L.F), W(L.G), W(L.M), N, bt.ws);
  if ((rc = (int)hipGetLastError())) return rc;
  if ((rc = symv_lower<double>(S, N, V(L.c), n, alpha, V(L.b), V(L.spart), nullptr, s, bt, vs))) return rc;
  loo_negate_kernel<<<dim3((unsigned)L.nblk, 1, Bz), 256, 0, s>>>(V(L.b), V(L.negb), N, vs);
  // the zero vector and the partials sit in the work slice where the plan's site has alpha and its gradient partials: gram_grad
  // addresses S, alpha and the partials at ONE site stride.  The step's Gram build left theta in the hyperparameter scratch
  if ((rc = (int)hipMemset2DAsync(work + L.zero, L.slice, 0, sizeof(double) * (size_t)N, (size_t)bt.B, s))) return rc;
  if ((rc = gram_grad<double>(model, d, Xt, N, n, theta, W(L.M), W(L.zero), W(L.gpart), out + DGP_OUT_DTHETA, s, bt, DGP_OUT_LEN,
                              pre_scratch, true, nullptr)))
    return rc;
  if ((rc = gram_bilinear<double>(model, d, Xt, N, n, theta, V(L.negb), alpha, W(L.gpart), out + DGP_OUT_DTHETA, 1, s, bt, vs, bt.ws,
                                  bt.ws, DGP_OUT_LEN, pre_scratch, false, nullptr)))
    return rc;
  loo_result_kernel<<<dim3((unsigned)L.nblk, 1, Bz), 256, 0, s>>>(W(L.M), alpha, N, n, bt.ws, bt.ns, V(L.b), wts, dr, dnoise, V(L.part),
                                                                  vs);
  loo_finish_kernel<<<dim3(1, 1, Bz), 256, 0, s>>>(V(L.part), L.nblk, vs, nt, 1, (const double*)(work + L.out0), nullptr, 0, out);
  return (int)hipGetLastError();
}

static int loo_gradient(int model, int d, const double* Xt, const double* S, const double* alpha, long N, int n, const double* theta,
                 const double* wts, char* work, const LooLayout& L, double* out, double* dr, double* dnoise, hipStream_t s, Batch bt,
                 void* pre_scratch) {
  if (model_ntheta(model, d) < 0) return -2;
  if ((size_t)bt.ws * sizeof(double) != L.slice) return (int)hipErrorInvalidValue;  // the work slices mirror the plan's site stride
  int rc;
  if ((rc = loo_terms(S, alpha, N, n, work, L, s, bt))) return rc;
  if ((rc = loo_mirror(S, N, (const double*)(work + L.vecs + L.w), work, L, s, bt))) return rc;
  return loo_tail(model, d, Xt, S, alpha, N, n, theta, wts, work, L, out, dr, dnoise, s, bt, pre_scratch);
}

}  // namespace dgp

using namespace dgp;

// ---- the entries: dgp_fit_step's launches, untouched, into a scratch result row, then the passes that read the S and alpha it
// left.  The plan's A / T / S / z / alpha stay as the step left them.
static const char* const LOO_F64 =
    "dgp_loo_*: the leave-one-out objective needs a float64 plan (its bilinear gradient pass exists for float64 only: fp32 plans are "
    "not supported)";

extern "C" {

size_t dgp_loo_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64) return 0;
  return loo_layout(p, false).total;
}
size_t dgp_loo_value_workspace_bytes(const dgp_plan* p) {
  if (!p || p->dtype != DGP_F64) return 0;
  return loo_layout(p, true).total;
}

int dgp_loo_fit_step(dgp_plan* p, const double* theta, const void* r, const void* noise, void* work, size_t work_bytes, void* out,
                     void* dr, void* dnoise, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64) return fail(DGP_E_ARG, LOO_F64);
  DGP_CHECK_PLAN(p);
  if (!theta || !r || !noise || !out) return fail(DGP_E_ARG, "dgp_loo_fit_step: null argument");
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_loo_fit_step: call dgp_set_inputs first");
  int rc = need_work(work, work_bytes, dgp_loo_workspace_bytes(p), "dgp_loo_fit_step");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const LooLayout L = loo_layout(p, false);
  rc = fit_step<double>(p, theta, r, noise, (char*)work + L.out0, dr, dnoise, 1, s);
  if (rc) return wrap(rc, "dgp_loo_fit_step");
  rc = loo_gradient(p->model, p->d, (const double*)p->Xt, (const double*)p->S, (const double*)p->alpha, p->N, (int)p->n, theta,
                    (const double*)p->dr_w, (char*)work, L, (double*)out, (double*)dr, (double*)dnoise, s, batch_of<double>(p), p->pre);
  return wrap(rc, "dgp_loo_fit_step");
}

int dgp_loo_value(dgp_plan* p, void* work, size_t work_bytes, void* out2, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64) return fail(DGP_E_ARG, LOO_F64);
  DGP_CHECK_PLAN(p);
  if (!out2) return fail(DGP_E_ARG, "dgp_loo_value: null argument");
  if (!p->have_factor || !p->have_inverse)
    return fail(DGP_E_STATE, "dgp_loo_value: needs the K^^-1 a fit step leaves in the plan (dgp_fit_step or dgp_loo_fit_step; dgp_factorize does not form it)");
  if (int rc = need_work(work, work_bytes, dgp_loo_value_workspace_bytes(p), "dgp_loo_value")) return rc;
  const int rc = loo_value((const double*)p->S, (const double*)p->alpha, p->info, p->N, (int)p->n, (char*)work, loo_layout(p, true),
                           (double*)out2, (hipStream_t)stream, batch_of<double>(p));
  return wrap(rc, "dgp_loo_value");
}

}  // extern "C"
