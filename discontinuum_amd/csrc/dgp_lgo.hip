// dgp_lgo.hip -- the exact LEAVE-GROUP-OUT predictive likelihood as a training objective, with its full gradient.  fp64,
// single-site or batched (ragged sizes through site_n); folds as dgp_cross_validate takes them (order / start, disjoint, rows in
// no fold allowed, empty folds allowed).
//
// With S = K^^-1 and alpha = S r as the fit step leaves them in the plan, and for every fold B_g of b_g rows
//     G_g = S[B_g, B_g],   C_g = G_g^-1,   e_g = C_g alpha[B_g]                       (dgp_crossval.hip)
//     L_LGO        = sum_g [ 1/2 alpha_g^T e_g - 1/2 log|G_g| + b_g / 2 log 2 pi ]    (= - sum_g lpd_g of dgp_cross_validate)
//     c = e_g scattered to the rows' own positions (0 on rows in no fold),   b = S c
//     W = the block-diagonal matrix of W_g = C_g + e_g e_g^T on (B_g, B_g),   M2 = S W S
//     dL/dtheta_p  = 1/2 tr( (M2 - b alpha^T - alpha b^T) dK/dtheta_p ),   dL/dr = b,   dL/dnoise_i = 1/2 (M2)_ii - b_i alpha_i
// Folds of one: W = diag(2 w) of dgp_loo.hip.  One fold of every row: G = S, e = r, L = the marginal likelihood.
//
//   the step             fit_step<double>(with_grad = 1), untouched, into a scratch result row
//   the fold blocks      cross_validate<double> on the valid S (its three routes): e (scattered: that is c), lpd_g and the pivots.
//                        Its tap hands over the rest of a fold: the LDS route writes W_g itself; the block route lends M^-1 of
//                        the fold's factor, of which lauum makes C_g = M^-T M^-1 (lower tiles, tile core) and
//   lgo_wblock_kernel    W_g = C_g + e_g e_g^T made full, to rows start[g] .. of the site's block area (leading dimension
//                        round_up(max_group, 128); the folds are disjoint, so the area has N rows -- and one tile of slack)
//   lgo_terms_kernel     c in the vectors' layout, the weights of folds of one, the block partials of - sum_g lpd_g and of the
//                        first bad fold
//   loo_mirror           F = S made full; G = F diag(w2): final for folds of one, zero otherwise, then
//   lgo_pack_kernel      P = the rows of F in the folds' order (row p of P = row order[p] of F = column order[p] of F), and
//   lgo_fw_kernel        G[:, B_g] = F[:, B_g] W_g for every fold: one tile-core product per (row tile, fold, column tile of the
//                        fold), A = P read transposed from row start[g] on, B = the rows of W_g, k over the fold's own b_g rounded
//                        up to 16 (the rest of a row of W_g is zero; a fold whose last k-tile would pass row N of P is read from
//                        cv_wblock_shift rows earlier against a block stored as many columns in); the columns scatter through
//                        `order`.  128 x 128 tiles on the direct-to-LDS core when max_group > 64, 64 x 64 tiles on the
//                        register-staged one otherwise
//   loo_tail             M2 = F G^T, b = S c, the contraction, dr / dnoise, the result row: dgp_loo.hip's own passes
// No floating-point atomics, fixed summation orders: every result repeats bitwise, and a site's result does not depend on the
// batch it is in (at the same max_group, which picks cross_validate's route).
#include "../../include/dgp_hip.h"
#include "dgp_gemm_dma.h"
#include "dgp_loo.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

struct LgoLayout {
  LooLayout L;
  size_t resid, var, lpd, info, wblk, cv, total;  // byte offsets behind the leave-one-out layout
  long ld;                                        // leading dimension of the weight blocks
  size_t wsite;                                   // doubles of a site's block area
};
LgoLayout lgo_layout(const dgp_plan* p, int ngroups, long max_group, bool value_only) {
  LgoLayout G;
  G.L = loo_layout(p, value_only);
  const size_t N = (size_t)p->N, B = (size_t)p->B, n = (size_t)p->n;
  G.ld = round_up(max_group, DGP_TILE_HOST);
  G.wsite = N * (size_t)G.ld;
  Carve c;
  c.o = G.L.total;
  G.resid = c.take(sizeof(double) * B * n);
  G.var = c.take(sizeof(double) * B * n);
  G.lpd = c.take(sizeof(double) * B * (size_t)ngroups);
  G.info = c.take(sizeof(int) * B * (size_t)ngroups);
  // (one tile of rows behind the last site: a product's last column tile reads whole rows of the area past its fold)
  G.wblk = c.take(value_only || max_group <= 1 ? 0 : sizeof(double) * (B * G.wsite + (size_t)DGP_TILE_HOST * (size_t)G.ld));
  G.cv = c.take(cross_validate_workspace_bytes(p->N, p->B, ngroups, max_group));
  G.total = c.o;
  return G;
}

// row i: c_i and, for folds of one, 2 w_i = C_i + e_i^2; fold g = i: - lpd_g and the first bad fold
__global__ __launch_bounds__(256) void lgo_terms_kernel(const double* __restrict__ resid, const double* __restrict__ var,
                                                        const double* __restrict__ lpd, const int* __restrict__ info, long N, int n,
                                                        const int* __restrict__ ns, int ngroups, int ones, double* __restrict__ w2,
                                                        double* __restrict__ c, double* __restrict__ part, long vs) {
  const int nb = site_n(ns, n);
  resid = site(resid, (long)n);
  var = site(var, (long)n);
  lpd = site(lpd, (long)ngroups);
  info = site(info, (long)ngroups);
  part = site(part, vs);
  __shared__ double red[4];
  __shared__ double redm[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (c && i < N) {
    const double e = i < nb ? resid[i] : 0.0;
    site(c, vs)[i] = e;
    site(w2, vs)[i] = (ones && i < nb) ? var[i] + e * e : 0.0;
  }
  double v = 0.0, bad = 0.0;
  if (i < ngroups) {
    v = -lpd[i];
    if (info[i] != 0) bad = (double)(i + 1);
  }
  double m = bad > 0.0 ? bad : 1e300;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_down(m, off, 64));
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) {
    redm[threadIdx.x >> 6] = m;
    red[threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[(long)blockIdx.x * LOO_PART + 0] = (red[0] + red[1]) + (red[2] + red[3]);
    const double mm = fmin(fmin(redm[0], redm[1]), fmin(redm[2], redm[3]));
    part[(long)blockIdx.x * LOO_PART + 1] = mm < 1e299 ? mm : 0.0;
  }
}

struct LgoFolds {
  const int* ns;
  const int* order;
  const int* start;
  int n, ngroups;
  long ld;  // leading dimension of the weight blocks
  int cap;  // the largest fold of cross_validate's route: the same clamp in both passes
};
__device__ __forceinline__ void lgo_fold(const LgoFolds& f, int sid, int g, int& nb, const int*& ord, int& s0, int& b) {
  nb = f.ns ? f.ns[sid] : f.n;
  ord = f.order + (long)sid * f.n;
  cv_bounds(f.start + (long)sid * (f.ngroups + 1), g, nb, f.cap, s0, b);
}

// block route, slot z = site C + c of a chunk: row i of W_g = C_g (lower stored) + e_g e_g^T, full
__global__ __launch_bounds__(256) void lgo_wblock_kernel(LgoFolds f, const double* __restrict__ Cm, const double* __restrict__ e,
                                                         long stride, long M, long N, int g0, int C, double* __restrict__ wblk, long wsite) {
  const int sid = (int)blockIdx.z / C, g = g0 + (int)blockIdx.z % C;
  if (g >= f.ngroups) return;
  int nb, s0, b;
  const int* ord;
  lgo_fold(f, sid, g, nb, ord, s0, b);
  const int i = (int)blockIdx.x;
  if (i >= b) return;
  Cm += (long)blockIdx.z * stride;
  e += (long)blockIdx.z * stride;
  double* out = wblk + (long)sid * wsite + (long)(s0 + i) * f.ld + cv_wblock_shift(N, s0, b);
  const double ei = e[i];
  for (int j = (int)threadIdx.x; j < b; j += 256) out[j] = (j <= i ? Cm[(long)i * M + j] : Cm[(long)j * M + i]) + ei * e[j];
}

// P[p][:] = F[order[p]][:] for the site's own rows, zero below them
__global__ __launch_bounds__(256) void lgo_pack_kernel(LgoFolds f, const double* __restrict__ F, double* __restrict__ P, long N, long bs) {
  const int sid = (int)blockIdx.z;
  const int nb = f.ns ? f.ns[sid] : f.n;
  const long p = (long)blockIdx.x;
  const double2* src = p < nb ? (const double2*)(F + (long)sid * bs + (long)cv_index(f.order + (long)sid * f.n, (int)p, nb) * N) : nullptr;
  double2* dst = (double2*)(P + (long)sid * bs + p * N);
  for (long c = threadIdx.x; c < N / 2; c += 256) dst[c] = src ? src[c] : make_double2(0.0, 0.0);
}

__device__ __forceinline__ const double* lgo_uniform(const double* p) {  // a workgroup-uniform address, into scalar registers
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const double*)(((unsigned long long)hi << 32) | lo);
}

// G[I, B_g[J]] = sum_k P[start_g + k][I] W_g[J][k]: blockIdx.x = (fold, row tile, column tile of the fold)
template <int BT>
__global__ __launch_bounds__(256, (TileCore<double, false, true, BT, BT>::OCC)) void lgo_fw_kernel(LgoFolds f, const double* __restrict__ P,
                                                                                                    const double* __restrict__ wblk,
                                                                                                    long wsite, double* __restrict__ G,
                                                                                                    long N, long bs, int nrt, int nct) {
  using K = TileCore<double, false, true, BT, BT>;
  using TG = typename K::G;
  __shared__ double smem[K::SMEM_ELEMS];
  const int sid = (int)blockIdx.z;
  // workgroup-uniform values that the vector pipe computes (the divisions) or loads: the direct-to-LDS core takes its operand
  // bases in scalar registers
  const int ct = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % (unsigned)nct));
  const int rt = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)nct % (unsigned)nrt));
  const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / ((unsigned)nct * (unsigned)nrt)));
  int nb, s0, b;
  const int* ord;
  lgo_fold(f, sid, g, nb, ord, s0, b);
  s0 = __builtin_amdgcn_readfirstlane(s0);
  b = __builtin_amdgcn_readfirstlane(b);
  if (ct * BT >= b) return;  // (the whole workgroup)
  P += (long)sid * bs;
  G += (long)sid * bs;
  wblk += (long)sid * wsite;
  typename TG::acc_t acc[TG::MI][TG::NI];
  TG::zero(acc);
  // k-tiles of 16 from row s0; a fold that ends within 15 rows of row N starts earlier, against a block stored that much to the
  // right: rows s0 - shift .. N - 1, never a row beyond the operand
  const int shift = cv_wblock_shift(N, s0, b);
  K::run(lgo_uniform(P + (long)(s0 - shift) * N + (long)rt * BT), N, lgo_uniform(wblk + (long)(s0 + ct * BT) * f.ld), f.ld, (b + 15) / 16, smem,
         acc);
  double* out = G + (long)rt * BT * N;
  K::foreach (acc, [&](int r, int c, double& v) {
    const int j = ct * BT + c;
    if (j < b) out[(long)r * N + cv_index(ord, s0 + j, nb)] = v;
  });
}

struct LgoChunkCtx {
  LgoFolds f;
  double* wblk;
  long wsite, N;
  int B;
  const Tuning* tune;
  hipStream_t s;
};
int lgo_chunk(void* ctx_, const CvBlocks& cb) {
  const LgoChunkCtx& k = *(const LgoChunkCtx*)ctx_;
  Batch bb;  // the chunk's slots as one batch, as cross_validate factors them
  bb.B = cb.C * k.B;
  bb.ws = cb.stride;
  bb.tune = k.tune;
  if (int rc = lauum<double>(cb.minv, cb.M, cb.scratch, k.s, bb)) return rc;
  lgo_wblock_kernel<<<dim3((unsigned)cb.M, 1, (unsigned)bb.B), 256, 0, k.s>>>(k.f, cb.scratch, cb.e, cb.stride, cb.M, k.N, cb.g0, cb.C, k.wblk,
                                                                             k.wsite);
  return (int)hipGetLastError();
}

// the fold blocks and the terms pass; full: also the weight blocks, c and w2
int lgo_folds(const dgp_plan* p, const int* order, const int* start, int ngroups, long max_group, char* work, const LgoLayout& G, bool full,
              hipStream_t s, const Batch& bt) {
  const LgoFolds f{bt.ns, order, start, (int)p->n, ngroups, G.ld, max_group <= CV_SMALL_GROUP ? CV_SMALL_GROUP : (int)G.ld};
  const bool blocks = full && max_group > 1;
  double* wblk = (double*)(work + G.wblk);
  int rc;
  if (blocks && (rc = (int)hipMemsetAsync(wblk, 0, sizeof(double) * (size_t)bt.B * G.wsite, s))) return rc;
  Tuning tune = bt.tuning();
  tune.chain_yield = 0;
  LgoChunkCtx ctx{f, wblk, (long)G.wsite, p->N, bt.B, &tune, s};
  CvTap tap;
  if (blocks) {
    tap.wblk = wblk;
    tap.wld = G.ld;
    tap.wsite = (long)G.wsite;
    tap.chunk = lgo_chunk;
    tap.ctx = &ctx;
  }
  double* resid = (double*)(work + G.resid);
  double* var = (double*)(work + G.var);
  double* lpd = (double*)(work + G.lpd);
  int* info = (int*)(work + G.info);
  if ((rc = cross_validate<double>((const double*)p->Tm, (const double*)p->S, (const double*)p->alpha, p->N, (int)p->n, order, start,
                                   ngroups, max_group, work + G.cv, resid, var, lpd, info, s, bt, blocks ? &tap : nullptr)))
    return rc;
  char* vec = work + G.L.vecs;
  lgo_terms_kernel<<<dim3((unsigned)G.L.nblk, 1, (unsigned)bt.B), 256, 0, s>>>(
      resid, var, lpd, info, p->N, (int)p->n, bt.ns, ngroups, max_group <= 1 ? 1 : 0, full ? (double*)(vec + G.L.w) : nullptr,
      full ? (double*)(vec + G.L.c) : nullptr, (double*)(vec + G.L.part), (long)(G.L.vec / sizeof(double)));
  return (int)hipGetLastError();
}

int lgo_gradient(dgp_plan* p, const double* theta, const int* order, const int* start, int ngroups, long max_group, char* work,
                 const LgoLayout& G, double* out, double* dr, double* dnoise, hipStream_t s, const Batch& bt) {
  const LooLayout& L = G.L;
  if ((size_t)bt.ws * sizeof(double) != L.slice) return (int)hipErrorInvalidValue;  // the work slices mirror the plan's site stride
  const long N = p->N;
  const double* S = (const double*)p->S;
  int rc;
  if ((rc = lgo_folds(p, order, start, ngroups, max_group, work, G, true, s, bt))) return rc;
  if ((rc = loo_mirror(S, N, (const double*)(work + L.vecs + L.w), work, L, s, bt))) return rc;
  if (max_group > 1) {
    const LgoFolds f{bt.ns, order, start, (int)p->n, ngroups, G.ld, max_group <= CV_SMALL_GROUP ? CV_SMALL_GROUP : (int)G.ld};
    const double* F = (const double*)(work + L.F);
    double* P = (double*)(work + L.M);  // 2 M's place is free until the sandwich writes it
    double* Gm = (double*)(work + L.G);
    const double* wblk = (const double*)(work + G.wblk);
    lgo_pack_kernel<<<dim3((unsigned)N, 1, (unsigned)bt.B), 256, 0, s>>>(f, F, P, N, bt.ws);
    if (max_group <= CV_SMALL_GROUP) {
      const int nrt = (int)(N / 64);
      lgo_fw_kernel<64><<<dim3((unsigned)ngroups * (unsigned)nrt, 1, (unsigned)bt.B), 256, 0, s>>>(f, P, wblk, (long)G.wsite, Gm, N, bt.ws,
                                                                                                 nrt, 1);
    } else {
      const int nrt = (int)(N / 128), nct = (int)(G.ld / 128);
      lgo_fw_kernel<128><<<dim3((unsigned)ngroups * (unsigned)nrt * (unsigned)nct, 1, (unsigned)bt.B), 256, 0, s>>>(
          f, P, wblk, (long)G.wsite, Gm, N, bt.ws, nrt, nct);
    }
    if ((rc = (int)hipGetLastError())) return rc;
  }
  return loo_tail(p->model, p->d, (const double*)p->Xt, S, (const double*)p->alpha, N, (int)p->n, theta, (const double*)p->dr_w, work, L,
                  out, dr, dnoise, s, bt, p->pre);
}

}  // namespace

}  // namespace dgp

using namespace dgp;

static const char* const LGO_F64 =
    "dgp_lgo_*: the leave-group-out objective needs a float64 plan (its bilinear gradient pass exists for float64 only: fp32 plans "
    "are not supported)";
static const char* const LGO_SIZE = "dgp_lgo_*: bad size (1 <= ngroups <= n, 1 <= max_group <= n)";

static bool lgo_sizes_ok(const dgp_plan* p, int ngroups, int64_t max_group) {
  // (the products' grids carry fold x row tile x column tile in one dimension)
  return cv_sizes_ok(p, ngroups, max_group) && (double)ngroups * (double)(p->N / 64) * (double)(round_up(max_group, 128) / 128) < 2.0e9;
}

extern "C" {

size_t dgp_lgo_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group) {
  if (!p || p->dtype != DGP_F64 || !lgo_sizes_ok(p, ngroups, max_group)) return 0;
  return lgo_layout(p, ngroups, max_group, false).total;
}
size_t dgp_lgo_value_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group) {
  if (!p || p->dtype != DGP_F64 || !lgo_sizes_ok(p, ngroups, max_group)) return 0;
  return lgo_layout(p, ngroups, max_group, true).total;
}

int dgp_lgo_fit_step(dgp_plan* p, const double* theta, const void* r, const void* noise, const int32_t* order, const int32_t* start,
                     int ngroups, int64_t max_group, void* work, size_t work_bytes, void* out, void* dr, void* dnoise, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64) return fail(DGP_E_ARG, LGO_F64);
  DGP_CHECK_PLAN(p);
  if (!theta || !r || !noise || !order || !start || !out) return fail(DGP_E_ARG, "dgp_lgo_fit_step: null argument");
  if (!lgo_sizes_ok(p, ngroups, max_group)) return fail(DGP_E_ARG, LGO_SIZE);
  int rc = need_work(work, work_bytes, dgp_lgo_workspace_bytes(p, ngroups, max_group), "dgp_lgo_fit_step");
  if (rc) return rc;
  if (!p->have_inputs) return fail(DGP_E_STATE, "dgp_lgo_fit_step: call dgp_set_inputs first");
  hipStream_t s = (hipStream_t)stream;
  const LgoLayout G = lgo_layout(p, ngroups, max_group, false);
  rc = fit_step<double>(p, theta, r, noise, (char*)work + G.L.out0, dr, dnoise, 1, s);
  if (rc) return wrap(rc, "dgp_lgo_fit_step");
  rc = lgo_gradient(p, theta, order, start, ngroups, max_group, (char*)work, G, (double*)out, (double*)dr, (double*)dnoise, s,
                    batch_of<double>(p));
  return wrap(rc, "dgp_lgo_fit_step");
}

int dgp_lgo_value(dgp_plan* p, const int32_t* order, const int32_t* start, int ngroups, int64_t max_group, void* work, size_t work_bytes,
                  void* out2, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (p->dtype != DGP_F64) return fail(DGP_E_ARG, LGO_F64);
  DGP_CHECK_PLAN(p);
  if (!order || !start || !out2) return fail(DGP_E_ARG, "dgp_lgo_value: null argument");
  if (!lgo_sizes_ok(p, ngroups, max_group)) return fail(DGP_E_ARG, LGO_SIZE);
  if (int rc = need_work(work, work_bytes, dgp_lgo_value_workspace_bytes(p, ngroups, max_group), "dgp_lgo_value")) return rc;
  if (!p->have_factor || !p->have_inverse)
    return fail(DGP_E_STATE, "dgp_lgo_value: needs the K^^-1 a fit step leaves in the plan (dgp_fit_step, dgp_loo_fit_step or dgp_lgo_fit_step; dgp_factorize does not form it)");
  hipStream_t s = (hipStream_t)stream;
  const LgoLayout G = lgo_layout(p, ngroups, max_group, true);
  const Batch bt = batch_of<double>(p);
  int rc = lgo_folds(p, order, start, ngroups, max_group, (char*)work, G, false, s, bt);
  if (!rc) rc = loo_finish_value(p->info, (char*)work, G.L, (double*)out2, s, bt);
  return wrap(rc, "dgp_lgo_value");
}

}  // extern "C"
