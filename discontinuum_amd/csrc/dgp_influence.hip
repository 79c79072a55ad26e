// dgp_influence.hip -- the exact INFLUENCE of every fold of observations on every period sum, from the factorisation a plan holds.
//
// Case deletion at fixed hyperparameters is closed-form (the partitioned inverse; Cook & Weisberg's case-deletion diagnostics, the
// delete-a-group jackknife of WRTDS practice).  The reference can only refit once per deletion.  With S = K^^-1 = T^T T,
// alpha = S r, beta = S K* (N x m), a fold F of f training rows, G_F = S_FF = M M^T, u = M^-1 alpha_F, e_F = M^-T u = G_F^-1 alpha_F
// (cross-validation's held-out residual) and z_j = M^-1 beta_{F,j}:
//     mu'_j = mu_j - z_j^T u = mu_j - e_F^T beta_{F,j}            sigma'^2_j = sigma^2_j + |z_j|^2            C'_jl = C_jl + z_j^T z_l
// and for the period sums of dgp_period_moments / dgp_sample_value (a_j as there, s the target's scale):
//     mode 1 (log):     dL[F][g] = sum_{j in g} a_j expm1(s dmu_Fj + s^2 dsigma^2_Fj / 2)              the change of the expected load
//     mode 0 (linear):  dL[F][g] = sum_{j in g} a_j dmu_Fj,   dVar[F][g] = |sum_{j in g} a_j z_j|^2 = |M^-1 (sum_{j in g} a_j beta_{F,j})|^2
// "without the fold minus with it".  Passes, all with gridDim.z = sites (ragged batches through site_n):
//
//   gram_cross, predict_v, sens_beta     K*, V = T K*, beta = T^T V: the launchers of the prediction and of dgp_predict_sensitivity
//   cross_validate (dgp_crossval.hip)    e_F and info for every fold by its three routes; leave-one-out also 1 / S_ii; through its TAP
//                                        the LDS route leaves M^-1 of every fold in the work area and the block route hands over
//                                        every chunk of inverted blocks
//   inf_pack, predict_v<double>          block route only, per chunk: the fold's rows of beta as a zero-padded double panel and
//                                        Z = M^-1 panel on the double tile core (mode 1: |z_j|^2 is needed per test point)
//   inf_sweep                            the N x m sweep.  One WAVE per (fold, slab of test points), lanes along j (beta is read
//                                        coalesced): dmu from e_F, dsigma^2 from a triangular matvec with M^-1 in LDS (folds of up to
//                                        64), from 1 / S_ii (leave-one-out) or from Z (block route); expm1; the SEGMENTED sum into the
//                                        period of j by shuffles in a fixed order (a max-scan makes the ids non-decreasing, so that
//                                        every (wave, period) is written exactly once); the running maximum for the shift
//   inf_sweep<rows>, inf_foldvar         mode 0 with dvar: B[i][g] = sum_{j in g} a_j beta_ij by the same sweep over single rows, then
//                                        per (fold, period) the triangular product M^-1 B[F, g] and its squared norm
//   inf_finish                           adds the slab partials in slab order, NaN for a fold whose block failed
// Everything is double whatever the plan's dtype.  No floating-point atomics, fixed summation orders: bitwise repeatable, and no
// result depends on what the work area held before (pre-filled with NaN it gives the same bits).  One slot IS read unwritten:
// on the LDS route the tap leaves M^-1 of a FAILED fold alone, and the sweep and inf_foldvar still read it; inf_finish and
// inf_foldvar's own info check then overwrite everything that fold produced with NaN.  The slab cut of a fold's test points
// depends on nfolds (in a batch: 1 + the largest fold id of any site) and the route on max_fold, so a site in a batch equals
// its single-site plan bitwise under the same nfolds, max_fold and tile selector of beta, and to rounding otherwise.  order / start / group are clamped wherever
// they index: bad content gives wrong numbers, never an access out of bounds.  Reads T, S, alpha only.
#include "dgp_common.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

constexpr int INF_SMALL = 64;      // largest fold of the LDS route (== cross_validate's)
constexpr int INF_UNITS = 4096;    // (fold, slab) waves a sweep aims at: 16 per compute unit
__device__ __forceinline__ double inf_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

enum { ROUTE_LOO = 0, ROUTE_LDS = 1, ROUTE_BLOCK = 2, ROUTE_ROWS = 3 };

struct InfSweep {  // kernel argument
  long N, Mp, wbs;  // beta: N x Mp row-major, site stride wbs elements
  int n, m, nfolds, ngroups, mode, nslab, slab_len;
  const int *ns, *order, *start, *group;
  const double *resid, *var, *minv;  // e_F per observation, 1 / S_ii (leave-one-out), M^-1 per fold (LDS route, leading dimension ld)
  long ld;
  const double *a, *scale, *inv_sd;
  double *part, *pmax;  // [site][fold][slab][group], [site][fold][slab] (null: no shift)
  const double *panel, *z, *e;  // block route: slot (site C + c): panel / Z at pstride, e_F at estride
  long pstride, estride;
  int g0, C, cap;
};

// one (wave, period) result: zeros for the periods skipped since the last one written, then the sum
__device__ __forceinline__ void inf_flush(double* __restrict__ prow, int g, double v, int& last, int lane) {
  for (int k = last + 1 + lane; k < g; k += 64) prow[k] = 0.0;
  if (lane == 0) prow[g] = v;
  last = g;
}

// 64 consecutive test points: lane `lane` brings the term v of period g (-1: none, v == 0).  The running (carry_g, carry_v) is
// the period still open at the end of the previous 64; every period that ends here is written through inf_flush.
__device__ __forceinline__ void inf_segment(double v, int g, int lane, int& carry_g, double& carry_v, int& last, double* __restrict__ prow) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {  // inclusive max-scan: excluded points join the period before them, ids become non-decreasing
    const int t = __shfl_up(g, d, 64);
    if (lane >= d) g = max(g, t);
  }
  g = max(g, carry_g);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {  // segmented inclusive sum-scan: equal ids at distance d mean one period in between
    const double tv = __shfl_up(v, d, 64);
    const int tg = __shfl_up(g, d, 64);
    if (lane >= d && tg == g) v += tv;
  }
  const int gn = __shfl_down(g, 1, 64);
  unsigned long long tails = __ballot(lane == 63 || gn != g);
  while (tails) {  // (uniform) the runs of this 64 in order: usually one
    const int l = __ffsll((long long)tails) - 1;
    tails &= tails - 1;
    const int rg = __shfl(g, l, 64);
    const double rv = __shfl(v, l, 64);
    if (rg == carry_g) {
      carry_v += rv;
    } else {
      if (carry_g >= 0) inf_flush(prow, carry_g, carry_v, last, lane);
      carry_g = rg;
      carry_v = rv;
    }
  }
}

template <typename T, int ROUTE>
__global__ __launch_bounds__(256) void inf_sweep_kernel(const T* __restrict__ beta, const InfSweep q) {
  constexpr bool LDS = ROUTE == ROUTE_LDS;
  __shared__ double sM[LDS ? INF_SMALL * INF_SMALL : 1];
  __shared__ double sE[LDS ? INF_SMALL : 1];
  __shared__ int sIdx[LDS ? INF_SMALL : 1];
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6, sid = (int)blockIdx.z;
  const int nb = q.ns ? q.ns[sid] : q.n;
  const int* order = q.order + (long)sid * q.n;
  const int* start = q.start + (long)sid * (q.nfolds + 1);
  beta += (long)sid * q.wbs;
  int fold, slab, s0 = 0, b = 0, idx = 0;
  long slot = 0;
  if (ROUTE == ROUTE_LOO || ROUTE == ROUTE_ROWS) {  // no workgroup state: any four (fold, slab) units per workgroup
    const long u = (long)blockIdx.x * 4 + w;
    fold = (int)(u / q.nslab);
    slab = (int)(u % q.nslab);
    if (fold >= q.nfolds) return;
    if (ROUTE == ROUTE_ROWS) {
      b = fold < nb ? 1 : 0;
      idx = fold;
    } else {
      cv_bounds(start, fold, nb, 1, s0, b);
      if (b) idx = cv_index(order, s0, nb);
    }
  } else if (LDS) {  // the four waves share the fold: M^-1, e_F and the fold's rows in LDS
    const int per = q.nslab / 4;
    fold = (int)blockIdx.x / per;
    slab = ((int)blockIdx.x % per) * 4 + w;
    cv_bounds(start, fold, nb, q.cap, s0, b);
    if (t < INF_SMALL) {
      const int i = t < b ? cv_index(order, s0 + t, nb) : 0;
      sIdx[t] = i;
      sE[t] = t < b ? q.resid[(long)sid * q.n + i] : 0.0;
    }
    const double* mi = q.minv + ((long)sid * q.nfolds + fold) * q.ld * q.ld;
    for (int e = t; e < b * b; e += 256) {
      const int i = e / b, j = e % b;
      sM[i * INF_SMALL + j] = mi[(long)i * q.ld + j];
    }
    __syncthreads();
  } else {
    fold = q.g0 + (int)blockIdx.y;
    slab = (int)blockIdx.x * 4 + w;
    if (fold >= q.nfolds) return;
    cv_bounds(start, fold, nb, q.cap, s0, b);
    slot = (long)sid * q.C + (int)blockIdx.y;
  }
  if (slab >= q.nslab) return;
  const int jbeg = min(slab * q.slab_len, q.m), jend = min(q.m, jbeg + q.slab_len);
  double* prow = q.part + (((long)sid * q.nfolds + fold) * q.nslab + slab) * q.ngroups;
  const double* a = q.a + (long)sid * q.m;
  const int* group = q.group + (long)sid * q.m;
  const double* inv_sd = q.inv_sd ? q.inv_sd + (long)sid * q.m : nullptr;
  const double s = q.mode == 1 ? q.scale[sid] : 0.0;
  const double rs = ROUTE == ROUTE_LOO && b ? q.resid[(long)sid * q.n + idx] : 0.0;
  const double iv = ROUTE == ROUTE_LOO && b ? q.var[(long)sid * q.n + idx] : 0.0;
  int carry_g = -1, last = -1;
  double carry_v = 0.0, smax = 0.0;
#pragma unroll 1
  for (int j0 = jbeg; j0 < jend; j0 += 64) {
    const int j = j0 + lane;
    const bool valid = j < jend;
    double v = 0.0;
    int g = -1;
    if (valid) {
      double dmu = 0.0, ds2 = 0.0;
      if (ROUTE == ROUTE_LOO) {
        const double bij = b ? (double)beta[(long)idx * q.Mp + j] : 0.0;
        dmu = -bij * rs;
        ds2 = bij * bij * iv;
      } else if (ROUTE == ROUTE_ROWS) {
        dmu = b ? (double)beta[(long)idx * q.Mp + j] : 0.0;  // the row itself: B[i][g] = sum a_j beta_ij
      } else if (LDS) {
        const T* col = beta + j;
        for (int c = 0; c < b; ++c) dmu -= sE[c] * (double)col[(long)sIdx[c] * q.Mp];
        if (q.mode == 1) {  // z = M^-1 beta_F,j row by row; the fold's rows of beta stay in the vector cache
          for (int r = 0; r < b; ++r) {
            double z = 0.0;
            for (int c = 0; c <= r; ++c) z += sM[r * INF_SMALL + c] * (double)col[(long)sIdx[c] * q.Mp];
            ds2 += z * z;
          }
        }
      } else {
        const double* P = q.panel + slot * q.pstride + j;
        const double* e = q.e + slot * q.estride;
        for (int c = 0; c < b; ++c) dmu -= e[c] * P[(long)c * q.Mp];
        if (q.mode == 1) {
          const double* Z = q.z + slot * q.pstride + j;
          for (int r = 0; r < b; ++r) {
            const double z = Z[(long)r * q.Mp];
            ds2 += z * z;
          }
        }
      }
      g = group[j];
      if (g < 0 || g >= q.ngroups) g = -1;
      if (inv_sd) smax = fmax(smax, fabs(dmu) * inv_sd[j]);
      if (g >= 0) v = (ROUTE != ROUTE_ROWS && q.mode == 1) ? a[j] * expm1(s * dmu + 0.5 * s * s * ds2) : a[j] * dmu;
    }
    inf_segment(v, g, lane, carry_g, carry_v, last, prow);
  }
  if (carry_g >= 0) inf_flush(prow, carry_g, carry_v, last, lane);
  for (int k = last + 1 + lane; k < q.ngroups; k += 64) prow[k] = 0.0;
  if (q.pmax) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) smax = fmax(smax, __shfl_xor(smax, off, 64));
    if (lane == 0) q.pmax[((long)sid * q.nfolds + fold) * q.nslab + slab] = smax;
  }
}

// block route: panel[slot][r][j] = beta[F_r][j] as doubles, zero in the pad rows r >= f and the pad columns j >= m
template <typename T>
__global__ __launch_bounds__(256) void inf_pack_kernel(const T* __restrict__ beta, const InfSweep q, double* __restrict__ panel) {
  const int sid = (int)blockIdx.z / q.C, c = (int)blockIdx.z % q.C, fold = q.g0 + c, r = (int)blockIdx.y;
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= q.Mp) return;
  const int nb = q.ns ? q.ns[sid] : q.n;
  int s0 = 0, b = 0;
  if (fold < q.nfolds) cv_bounds(q.start + (long)sid * (q.nfolds + 1), fold, nb, q.cap, s0, b);
  double v = 0.0;
  if (r < b && j < q.m) v = (double)beta[(long)sid * q.wbs + (long)cv_index(q.order + (long)sid * q.n, s0 + r, nb) * q.Mp + j];
  panel[(long)blockIdx.z * q.pstride + (long)r * q.Mp + j] = v;
}

struct InfVar {  // kernel argument
  const double *bg, *var, *minv;  // B [site][n][group]; 1 / S_ii (leave-one-out: minv == null); M^-1 of fold c of a site at
  long site_stride, fold_stride, ld;  // minv + site site_stride + c fold_stride, leading dimension ld
  const int *ns, *order, *start, *info;
  int n, nfolds, ngroups, cap, g0;
  double* dvar;
};

// dVar[fold][g] = |M^-1 B[F, g]|^2: a wave per row of M^-1 (lanes along the row, wave tree), rows w, w + 4, ... in order per wave
__global__ __launch_bounds__(256) void inf_foldvar_kernel(const InfVar q) {
  __shared__ double sred[4];
  const int g = (int)blockIdx.x, c = (int)blockIdx.y, fold = q.g0 + c, sid = (int)blockIdx.z;
  if (fold >= q.nfolds) return;
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const int nb = q.ns ? q.ns[sid] : q.n;
  const int* order = q.order + (long)sid * q.n;
  int s0, b;
  cv_bounds(q.start + (long)sid * (q.nfolds + 1), fold, nb, q.cap, s0, b);
  const double* bg = q.bg + (long)sid * q.n * q.ngroups + g;
  double acc = 0.0;
  if (!q.minv) {
    if (t == 0 && b) {
      const int i = cv_index(order, s0, nb);
      const double x = bg[(long)i * q.ngroups];
      acc = x * x * q.var[(long)sid * q.n + i];
    }
  } else {
    const double* mi = q.minv + (long)sid * q.site_stride + (long)c * q.fold_stride;
    for (int r = w; r < b; r += 4) {
      double z = 0.0;
      for (int k = lane; k <= r; k += 64) z += mi[(long)r * q.ld + k] * bg[(long)cv_index(order, s0 + k, nb) * q.ngroups];
      z = wave_sum(z);
      acc += z * z;
    }
  }
  if (lane == 0) sred[w] = acc;
  __syncthreads();
  if (t == 0) {
    double v = (sred[0] + sred[1]) + (sred[2] + sred[3]);
    if (q.info[(long)sid * q.nfolds + fold] != 0) v = inf_nan();
    q.dvar[((long)sid * q.nfolds + fold) * q.ngroups + g] = v;
  }
}

// dload[fold][g] = the slab partials in slab order; shift[fold] = their maximum; NaN for a fold whose block failed
__global__ __launch_bounds__(256) void inf_finish_kernel(const double* __restrict__ part, const double* __restrict__ pmax,
                                                         const int* __restrict__ info, int nfolds, int nslab, int ngroups,
                                                         double* __restrict__ dload, double* __restrict__ shift) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, sid = blockIdx.z;
  if (e >= (long)nfolds * ngroups) return;
  const long fold = e / ngroups, g = e % ngroups, f = sid * nfolds + fold;
  const bool bad = info[f] != 0;
  double v = 0.0;
  for (int z = 0; z < nslab; ++z) v += part[(f * nslab + z) * ngroups + g];
  dload[f * ngroups + g] = bad ? inf_nan() : v;
  if (shift && g == 0) {
    double mx = 0.0;
    for (int z = 0; z < nslab; ++z) mx = fmax(mx, pmax[f * nslab + z]);
    shift[f] = bad ? inf_nan() : mx;
  }
}

int inf_route(long max_fold) { return max_fold <= 1 ? ROUTE_LOO : (max_fold <= INF_SMALL ? ROUTE_LDS : ROUTE_BLOCK); }

template <typename T>
struct InfChunkCtx {
  const T* beta;
  InfSweep q;
  InfVar v;
  double *panel, *z;
  bool want_var;
  int B;
  hipStream_t s;
};

template <typename T>
int inf_chunk(void* ctx, const CvBlocks& cb) {
  InfChunkCtx<T>& k = *(InfChunkCtx<T>*)ctx;
  InfSweep q = k.q;
  q.g0 = cb.g0;
  q.C = cb.C;
  q.e = cb.e;
  q.estride = cb.stride;
  const unsigned Z = (unsigned)(cb.C * k.B);
  inf_pack_kernel<T><<<dim3((unsigned)((q.Mp + 255) / 256), (unsigned)cb.M, Z), 256, 0, k.s>>>(k.beta, q, k.panel);
  if (q.mode == 1) {  // Z = M^-1 panel: the prediction's V = T K* on blocks of doubles
    Batch bb;
    bb.B = (int)Z;
    bb.ws = cb.stride;
    const int rc = predict_v<double>(cb.minv, cb.M, k.panel, q.Mp, k.z, k.s, bb, q.pstride);
    if (rc) return rc;
  }
  inf_sweep_kernel<T, ROUTE_BLOCK><<<dim3((unsigned)(q.nslab / 4), (unsigned)cb.C, (unsigned)k.B), 256, 0, k.s>>>(k.beta, q);
  if (k.want_var) {
    InfVar v = k.v;
    v.minv = cb.minv;
    v.site_stride = (long)cb.C * cb.stride;
    v.fold_stride = cb.stride;
    v.ld = cb.M;
    v.g0 = cb.g0;
    inf_foldvar_kernel<<<dim3((unsigned)v.ngroups, (unsigned)cb.C, (unsigned)k.B), 256, 0, k.s>>>(v);
  }
  return (int)hipGetLastError();
}

}  // namespace

// `work`: the B per-site slices (Xst and Ks filled by pack_x + gram_cross), then the shared areas
struct InfluenceLayout {
  size_t Xst, Ks, V, beta, slice;                                   // byte offsets inside a site's slice, and its size
  size_t resid, var, lpd, part, pmax, bg, cv, minv, panel, z, total;  // byte offsets of the shared areas behind the B slices
  int nslab, slab_len, chunk;                                       // slabs of test points per fold; folds per chunk (block route)
  long order;                                                       // block order of the block route
};
static InfluenceLayout influence_layout(long N, int B, int n, int d, long Mp, int m, int nfolds, long max_fold, int ngroups, size_t elem) {
  InfluenceLayout L;
  const size_t nm = elem * (size_t)N * (size_t)Mp, Bz = (size_t)B, P = (size_t)ngroups, F = (size_t)nfolds;
  Carve c;
  L.Xst = c.take(elem * (size_t)Mp * (size_t)d);
  L.Ks = c.take(nm);
  L.V = c.take(nm);
  L.beta = c.take(nm);
  L.slice = c.o;
  const int route = inf_route(max_fold);
  // slabs of test points per fold: enough (fold, slab) waves to fill the device; a function of (m, nfolds) alone, not of the batch size
  const int chunks = (m + 63) / 64;
  int nslab = (INF_UNITS + nfolds - 1) / nfolds;
  nslab = nslab < 1 ? 1 : (nslab > chunks ? chunks : nslab);
  L.slab_len = (int)round_up((m + nslab - 1) / nslab, 64);
  nslab = (m + L.slab_len - 1) / L.slab_len;
  L.nslab = route == ROUTE_LOO ? nslab : (int)round_up(nslab, 4);  // a workgroup of the other routes takes four slabs of one fold
  c.o = Bz * L.slice;
  L.resid = c.take(sizeof(double) * Bz * (size_t)n);
  L.var = c.take(sizeof(double) * Bz * (size_t)n);
  L.lpd = c.take(sizeof(double) * Bz * F);
  L.part = c.take(sizeof(double) * Bz * F * (size_t)L.nslab * P);
  L.pmax = c.take(sizeof(double) * Bz * F * (size_t)L.nslab);
  L.bg = c.take(sizeof(double) * Bz * (size_t)n * P);
  L.cv = c.take(cross_validate_workspace_bytes(N, B, nfolds, max_fold));
  L.minv = c.take(route == ROUTE_LDS ? sizeof(double) * Bz * F * (size_t)(max_fold * max_fold) : 0);
  L.chunk = route == ROUTE_BLOCK ? cross_validate_chunk_groups(N, B, nfolds, max_fold) : 0;
  L.order = route == ROUTE_BLOCK ? round_up(max_fold, DGP_TILE_HOST) : 0;
  const size_t pz = sizeof(double) * (size_t)L.chunk * Bz * (size_t)L.order * (size_t)Mp;
  L.panel = c.take(pz);
  L.z = c.take(pz);
  L.total = c.o;
  return L;
}

// The exact change of every period sum (and, for a linear target, of its variance) when a fold of observations is deleted at fixed
// hyperparameters.  Reads Tm, S (when valid, else null) and alpha only; every result is double.
template <typename T>
static int deletion_influence(const T* Tm, const T* S, const T* alpha, long N, int n, long Mp, int m, const int* order, const int* start,
                              int nfolds, long max_fold, int mode, const double* a, const double* scale, const int* group, int ngroups,
                              const double* inv_sd, void* work, const InfluenceLayout& L, double* dload, double* dvar, double* shift,
                              int* info, hipStream_t s, Batch bt) {
  const int route = inf_route(max_fold);
  const unsigned Bz = (unsigned)bt.B;
  if ((long)L.nslab / 4 * nfolds > 0x7fffffffL || ngroups > 65535) return -2;  // (grid sizes)
  char* w = (char*)work;
  const long wbs = (long)(L.slice / sizeof(T));
  const T* Ks = (const T*)(w + L.Ks);
  T* V = (T*)(w + L.V);
  T* beta = (T*)(w + L.beta);
  double* resid = (double*)(w + L.resid);
  double* var = (double*)(w + L.var);
  double* lpd = (double*)(w + L.lpd);
  double* part = (double*)(w + L.part);
  double* pmax = shift ? (double*)(w + L.pmax) : nullptr;
  double* bg = (double*)(w + L.bg);
  int rc = predict_v<T>(Tm, N, Ks, Mp, V, s, bt, wbs);
  if (rc) return rc;
  if ((rc = sens_beta<T>(Tm, N, V, Mp, beta, s, bt, wbs))) return rc;

  InfSweep q{};
  q.N = N; q.Mp = Mp; q.wbs = wbs;
  q.n = n; q.m = m; q.nfolds = nfolds; q.ngroups = ngroups; q.mode = mode; q.nslab = L.nslab; q.slab_len = L.slab_len;
  q.ns = bt.ns; q.order = order; q.start = start; q.group = group;
  q.resid = resid; q.var = var; q.minv = (const double*)(w + L.minv); q.ld = max_fold;
  q.a = a; q.scale = scale; q.inv_sd = inv_sd;
  q.part = part; q.pmax = pmax;
  q.panel = (const double*)(w + L.panel); q.z = (const double*)(w + L.z);
  q.pstride = L.order * Mp;
  q.cap = route == ROUTE_BLOCK ? (int)L.order : (int)max_fold;  // what the fold's slot in the work area holds
  const bool want_var = mode == 0 && dvar != nullptr;
  if (want_var) {  // B[i][g] = sum_{j in g} a_j beta_ij: the sweep over single rows, one slab, straight into its place
    InfSweep qr = q;
    qr.nfolds = n; qr.nslab = 1; qr.slab_len = (int)round_up(m, 64); qr.mode = 0;
    qr.part = bg; qr.pmax = nullptr; qr.inv_sd = nullptr;
    inf_sweep_kernel<T, ROUTE_ROWS><<<dim3((unsigned)((n + 3) / 4), 1, Bz), 256, 0, s>>>(beta, qr);
    if ((rc = (int)hipGetLastError())) return rc;
  }
  InfVar v{};
  v.bg = bg; v.var = var; v.ns = bt.ns; v.order = order; v.start = start; v.info = info;
  v.n = n; v.nfolds = nfolds; v.ngroups = ngroups; v.cap = q.cap; v.dvar = dvar;
  InfChunkCtx<T> ctx{beta, q, v, (double*)(w + L.panel), (double*)(w + L.z), want_var, bt.B, s};
  CvTap tap;
  if (route == ROUTE_LDS) {
    tap.minv = (double*)(w + L.minv);
    tap.ld = max_fold;
  } else if (route == ROUTE_BLOCK) {
    tap.chunk = inf_chunk<T>;
    tap.ctx = &ctx;
  }
  if ((rc = cross_validate<T>(Tm, S, alpha, N, n, order, start, nfolds, max_fold, w + L.cv, resid, var, lpd, info, s, bt, &tap))) return rc;
  if (route == ROUTE_LOO) {
    const long units = (long)nfolds * L.nslab;
    inf_sweep_kernel<T, ROUTE_LOO><<<dim3((unsigned)((units + 3) / 4), 1, Bz), 256, 0, s>>>(beta, q);
  } else if (route == ROUTE_LDS) {
    inf_sweep_kernel<T, ROUTE_LDS><<<dim3((unsigned)((long)L.nslab / 4 * nfolds), 1, Bz), 256, 0, s>>>(beta, q);
  }
  if (want_var && route != ROUTE_BLOCK) {
    if (route == ROUTE_LDS) {
      v.minv = (const double*)(w + L.minv);
      v.site_stride = (long)nfolds * max_fold * max_fold;
      v.fold_stride = max_fold * max_fold;
      v.ld = max_fold;
    }
    for (int g0 = 0; g0 < nfolds; g0 += 32768) {  // (grid.y)
      InfVar vc = v;
      vc.g0 = g0;
      if (vc.minv) vc.minv += (long)g0 * vc.fold_stride;
      const int cnt = nfolds - g0 < 32768 ? nfolds - g0 : 32768;
      inf_foldvar_kernel<<<dim3((unsigned)ngroups, (unsigned)cnt, Bz), 256, 0, s>>>(vc);
    }
  }
  if ((rc = (int)hipGetLastError())) return rc;
  inf_finish_kernel<<<dim3((unsigned)(((long)nfolds * ngroups + 255) / 256), 1, Bz), 256, 0, s>>>(part, pmax, info, nfolds, L.nslab, ngroups,
                                                                                                  dload, shift);
  return (int)hipGetLastError();
}

}  // namespace dgp

using namespace dgp;

static bool influence_sizes_ok(const dgp_plan* p, int64_t m, int nfolds, int64_t max_fold, int ngroups) {
  return p && m >= 1 && m <= (1 << 20) && nfolds >= 1 && nfolds <= p->n && max_fold >= 1 && max_fold <= p->n && ngroups >= 1 &&
         ngroups <= 65535;
}
static InfluenceLayout influence_layout_of(const dgp_plan* p, int64_t m, int nfolds, int64_t max_fold, int ngroups) {
  return influence_layout(p->N, p->B, (int)p->n, p->d, round_up(m, DGP_TILE_HOST), (int)m, nfolds, max_fold, ngroups, p->elem);
}
template <typename T>
static int influence(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int32_t* order, const int32_t* start, int nfolds,
                     int64_t max_fold, int mode, const double* a, const double* scale, const int32_t* group, int ngroups,
                     const double* inv_sd, void* work, double* dload, double* dvar, double* shift, int32_t* info, hipStream_t s) {
  const InfluenceLayout L = influence_layout_of(p, m, nfolds, max_fold, ngroups);
  char* w = (char*)work;
  const int rc = cross<T>(p, theta, Xs, m, w + L.Xst, w + L.Ks, s, (long)(L.slice / sizeof(T)));
  if (rc) return rc;
  const void* S = p->have_inverse ? p->S : nullptr;  // as dgp_cross_validate: read when the last step left it valid
  return deletion_influence<T>((const T*)p->Tm, (const T*)S, (const T*)p->alpha, p->N, (int)p->n, round_up(m, DGP_TILE_HOST), (int)m, order,
                               start, nfolds, max_fold, mode, a, scale, group, ngroups, inv_sd, work, L, dload, dvar, shift, info, s,
                               batch_of<T>(p));
}

extern "C" {

size_t dgp_deletion_influence_workspace_bytes(const dgp_plan* p, int64_t m, int nfolds, int64_t max_fold, int ngroups) {
  if (!influence_sizes_ok(p, m, nfolds, max_fold, ngroups)) return 0;
  return influence_layout_of(p, m, nfolds, max_fold, ngroups).total;
}

int dgp_deletion_influence(dgp_plan* p, const double* theta, const void* Xs, int64_t m, const int32_t* order, const int32_t* start,
                           int nfolds, int64_t max_fold, int mode, const double* a, const double* scale, const int32_t* group, int ngroups,
                           const double* inv_sd, void* work, size_t work_bytes, double* dload, double* dvar, double* shift,
                           int32_t* info, void* stream) {
  const char* where = "dgp_deletion_influence";
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!theta || !Xs || !order || !start || !a || !scale || !group || !dload || !info)
    return fail(DGP_E_ARG, "dgp_deletion_influence: null argument");
  if (!influence_sizes_ok(p, m, nfolds, max_fold, ngroups))
    return fail(DGP_E_ARG, "dgp_deletion_influence: bad size (1 <= m <= 2^20, 1 <= nfolds <= n, 1 <= max_fold <= n, 1 <= ngroups <= 65535)");
  if (mode != 0 && mode != 1) return fail(DGP_E_ARG, "dgp_deletion_influence: mode must be 0 (linear) or 1 (log)");
  if (mode == 1 && dvar) return fail(DGP_E_ARG, "dgp_deletion_influence: the variance change is exact for mode 0 only (dvar_dev must be NULL)");
  if (shift && !inv_sd) return fail(DGP_E_ARG, "dgp_deletion_influence: shift_dev needs inv_sd_dev");
  DGP_CHECK_PLAN(p);
  hipStream_t s = (hipStream_t)stream;
  int rc = need_factor(p, where, "call dgp_factorize or dgp_fit_step");
  if (rc || (rc = need_work(work, work_bytes, dgp_deletion_influence_workspace_bytes(p, m, nfolds, max_fold, ngroups), where)) ||
      (rc = factor_ok(p, s, where)))
    return rc;
  rc = DGP_BY_DTYPE(p,
                    influence<double>(p, theta, Xs, m, order, start, nfolds, max_fold, mode, a, scale, group, ngroups, inv_sd, work, dload,
                                      dvar, shift, info, s),
                    influence<float>(p, theta, Xs, m, order, start, nfolds, max_fold, mode, a, scale, group, ngroups, inv_sd, work, dload,
                                     dvar, shift, info, s));
  return wrap(rc, where);
}

}  // extern "C"
