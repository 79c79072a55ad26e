// dgp_crossval.hip -- exact leave-one-out / leave-group-out cross-validation from the factorisation a plan holds.
//
// At fixed hyperparameters no fold needs a refit (Rasmussen & Williams section 5.4.2; the block form is the partitioned inverse):
// with T = L^-1, alpha = K^^-1 r and a held-out index set B of b observations
//     G_B   = (K^^-1)_BB = T[:, B]^T T[:, B]                       (b x b, SPD)
//     e_B   = y_B - E[y_B | y_-B] = G_B^-1 alpha_B                  held-out residual
//     C_B   = Cov[y_B | y_-B]     = G_B^-1                          (the held-out observations' own noise included: it is in K^)
//     lpd_B = log p(y_B | y_-B)   = -1/2 alpha_B^T e_B + 1/2 log|G_B| - b/2 log 2 pi
// The reference has no counterpart: gpytorch would refactor per fold behind `self.likelihood(self.model(x))`
// (src/discontinuum/engines/gpytorch.py:599-626).  Three routes, chosen on the host from (max_group, S valid):
//   b == 1 everywhere   one bandwidth-bound pass over the lower triangle of T (column sums of squares in row slabs, summed in a
//                       fixed order by the finish kernel): K^^-1 is never formed
//   b <= 64             one workgroup per (group, site): G_B (from T, k-chunks from the last to the first like lauum, or gathered
//                       from a valid S), its Cholesky factor M, M^-1 and the solves all in LDS
//   larger groups       per chunk of groups: pack T[k0:, B] as a double panel, G_B = P^T P on the MFMA tile core (k-tiles from the
//                       last to the first), the library's own batched potrf / trtri on identity-padded blocks of order
//                       round_up(max_group, 128), then e_B = M^-T M^-1 alpha_B, var = column norms of M^-1, lpd from log|G_B|
// Everything from G_B on is double whatever the plan's dtype.  No floating-point atomics: bitwise repeatable, and a site's
// result does not depend on the batch it is in.  `order` / `start` are validated by the host wrapper; the kernels clamp every
// index and bound they read from them, so bad content gives wrong numbers or a set info, never an access out of bounds.
#include "dgp_common.h"
#include "dgp_gemm.h"
#include "dgp_gemm_dma.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

constexpr double CV_HALF_LOG_2PI = 0.91893853320467274178;
constexpr int CV_SLAB = 128;   // rows per slab of the leave-one-out pass
constexpr int CV_SMALL = CV_SMALL_GROUP;  // largest group of the fused LDS kernel
constexpr int CV_MAX_CHUNK = 1024;

// ---- leave-one-out: part[slab][j] = sum over the slab's rows k >= j of T[k][j]^2 ------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cv_colss_kernel(const T* __restrict__ Tm, long N, long bs, double* __restrict__ part, long ps) {
  Tm = site(Tm, bs);
  part = site(part, ps);
  const int r0 = (int)blockIdx.y * CV_SLAB;
  if (r0 + CV_SLAB <= (int)blockIdx.x * 256) return;  // the slab lies wholly above this column chunk's diagonal
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= N) return;
  const int kbeg = max(r0, j);
  double acc = 0.0;
#pragma unroll 8
  for (int k = r0 + CV_SLAB - 1; k >= kbeg; --k) {
    const double v = (double)Tm[(long)k * N + j];
    acc += v * v;
  }
  part[(long)blockIdx.y * N + j] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void cv_loo_finish_kernel(const double* __restrict__ part, long ps, long N, const T* __restrict__ alpha,
                                                            long bs, const int* __restrict__ ns, int n, const int* __restrict__ order,
                                                            const int* __restrict__ start, int ngroups, double* __restrict__ resid,
                                                            double* __restrict__ var, double* __restrict__ lpd, int* __restrict__ info) {
  const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= ngroups) return;
  part = site(part, ps);
  alpha = site(alpha, bs);
  const int nb = site_n(ns, n);
  order = site(order, (long)n);
  start = site(start, (long)ngroups + 1);
  resid = site(resid, (long)n);
  var = site(var, (long)n);
  lpd = site(lpd, (long)ngroups);
  info = site(info, (long)ngroups);
  int s0, b;
  cv_bounds(start, g, nb, 1, s0, b);
  if (b == 0) {
    lpd[g] = 0.0;
    info[g] = 0;
    return;
  }
  const int i = cv_index(order, s0, nb);
  double ss = 0.0;
  for (int r = (int)(N / CV_SLAB) - 1; r >= 2 * (i / 256); --r) ss += part[(long)r * N + i];  // far rows (small terms) first
  const double a = (double)alpha[i], v = 1.0 / ss, e = a * v;
  const bool ok = ss > 0.0 && ss < 1.0e300;
  resid[i] = e;
  var[i] = v;
  lpd[g] = -0.5 * a * e + 0.5 * log(ss) - CV_HALF_LOG_2PI;
  info[g] = ok ? 0 : 1;
}

// ---- groups of up to 64: everything in LDS ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cv_small_kernel(const T* __restrict__ Tm, const T* __restrict__ S, long N, long bs,
                                                       const T* __restrict__ alpha, const int* __restrict__ ns, int n,
                                                       const int* __restrict__ order, const int* __restrict__ start, int ngroups,
                                                       double* __restrict__ resid, double* __restrict__ var, double* __restrict__ lpd,
                                                       int* __restrict__ info, double* __restrict__ minv, long ld,
                                                       double* __restrict__ wblk, long wld, long wsite) {
  constexpr int LD = CV_SMALL + 1;
  __shared__ double sG[CV_SMALL * LD];  // G_B, then M (lower) with M^-1 transposed above the diagonal
  __shared__ double sP[16 * CV_SMALL];  // 16 rows of the group's columns of T
  __shared__ double sD[CV_SMALL], sA[CV_SMALL], sU[CV_SMALL], sE[CV_SMALL];
  __shared__ int sIdx[CV_SMALL];
  const int g = (int)blockIdx.x, t = (int)threadIdx.x;
  Tm = site(Tm, bs);
  if (S) S = site(S, bs);
  alpha = site(alpha, bs);
  const int nb = site_n(ns, n);
  order = site(order, (long)n);
  start = site(start, (long)ngroups + 1);
  resid = site(resid, (long)n);
  var = site(var, (long)n);
  lpd = site(lpd, (long)ngroups);
  info = site(info, (long)ngroups);
  int s0, b;
  cv_bounds(start, g, nb, CV_SMALL, s0, b);
  if (b == 0) {
    if (t == 0) {
      lpd[g] = 0.0;
      info[g] = 0;
    }
    return;
  }
  if (t < CV_SMALL) {
    const int i = t < b ? cv_index(order, s0 + t, nb) : 0;
    sIdx[t] = i;
    sA[t] = t < b ? (double)alpha[i] : 0.0;
  }
  __syncthreads();
  if (S) {  // K^^-1 is there: gather its block (only the lower triangle of S is stored)
    for (int e = t; e < CV_SMALL * CV_SMALL; e += 256) {
      const int i = e >> 6, j = e & 63;
      double v = i == j ? 1.0 : 0.0;
      if (i < b && j < b) {
        const int oi = sIdx[i], oj = sIdx[j];
        v = (double)S[(long)max(oi, oj) * N + min(oi, oj)];
      }
      sG[i * LD + j] = v;
    }
  } else {  // G_B = T[:, B]^T T[:, B]: chunks of 16 rows from the last to the first; each thread owns a 4 x 4 block of G_B
    int kmin = (int)N;
    for (int c = 0; c < b; ++c) kmin = min(kmin, sIdx[c]);
    const int k0 = kmin & ~15;
    const int ti = t >> 4, tj = t & 15;
    double acc[4][4] = {};
    for (int kc = (int)N - 16; kc >= k0; kc -= 16) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = t + 256 * q, kk = e >> 6, c = e & 63, k = kc + kk;
        double v = 0.0;
        if (c < b && k >= sIdx[c]) v = (double)Tm[(long)k * N + sIdx[c]];  // T is lower: nothing above the diagonal is read
        sP[kk * CV_SMALL + c] = v;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 15; kk >= 0; --kk) {
        double av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          av[q] = sP[kk * CV_SMALL + 4 * ti + q];
          bv[q] = sP[kk * CV_SMALL + 4 * tj + q];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[p][q] += av[p] * bv[q];
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * ti + p, j = 4 * tj + q;
        sG[i * LD + j] = (i < b && j < b) ? acc[p][q] : (i == j ? 1.0 : 0.0);
      }
  }
  // ---- Cholesky of G_B in place (lower), right-looking; every thread sees the same pivots
  double logdet = 0.0;
  int bad = 0;
  for (int j = 0; j < b; ++j) {
    __syncthreads();
    const double d = sG[j * LD + j];
    if (!(d > 0.0) || !(d < 1.0e300)) {
      bad = j + 1;
      break;
    }
    logdet += log(d);
    const double rinv = 1.0 / sqrt(d);
    __syncthreads();
    if (t == j) sG[j * LD + j] = sqrt(d);
    else if (t > j && t < b) sG[t * LD + j] *= rinv;
    __syncthreads();
    for (int e = t; e < CV_SMALL * CV_SMALL; e += 256) {
      const int i = e >> 6, k = e & 63;
      if (k > j && k <= i && i < b) sG[i * LD + k] -= sG[i * LD + j] * sG[k * LD + j];
    }
  }
  __syncthreads();
  if (bad) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if (t < b) {
      resid[sIdx[t]] = qnan;
      var[sIdx[t]] = qnan;
    }
    if (t == 0) {
      lpd[g] = qnan;
      info[g] = bad;
    }
    return;
  }
  // ---- M^-1 column by column (thread j owns column j, kept transposed in row j above the diagonal) and its column norms
  if (t < b) {
    const int j = t;
    const double xj = 1.0 / sG[j * LD + j];
    sD[j] = xj;
    double ss = xj * xj;
    for (int i = j + 1; i < b; ++i) {
      double s = sG[i * LD + j] * xj;
      for (int k = j + 1; k < i; ++k) s += sG[i * LD + k] * sG[j * LD + k];
      const double x = -s / sG[i * LD + i];
      sG[j * LD + i] = x;
      ss += x * x;
    }
    var[sIdx[j]] = ss;
  }
  __syncthreads();
  if (minv && b <= ld) {  // the tap: M^-1 (lower, row-major, leading dimension ld) of this fold for the caller's own passes
    double* out = minv + ((long)blockIdx.z * ngroups + g) * ld * ld;
    for (int e = t; e < b * b; e += 256) {
      const int i = e / b, j = e % b;
      out[(long)i * ld + j] = i == j ? sD[i] : (i > j ? sG[j * LD + i] : 0.0);
    }
  }
  if (t < b) {  // u = M^-1 alpha_B
    double u = sD[t] * sA[t];
    for (int j = 0; j < t; ++j) u += sG[j * LD + t] * sA[j];
    sU[t] = u;
  }
  __syncthreads();
  if (t < b) {  // e_B = M^-T u
    double e = sD[t] * sU[t];
    for (int i = t + 1; i < b; ++i) e += sG[t * LD + i] * sU[i];
    sE[t] = e;
    resid[sIdx[t]] = e;
  }
  __syncthreads();
  if (wblk && b <= wld) {  // the tap: W_g = M^-T M^-1 + e e^T, full, k from the last row to the first that reaches (i, j)
    double* out = wblk + (long)blockIdx.z * wsite + (long)s0 * wld + cv_wblock_shift(N, s0, b);
    for (int e = t; e < b * b; e += 256) {
      const int i = e / b, j = e % b, lo = min(i, j), hi = max(i, j);
      double c = 0.0;
      for (int k = b - 1; k > hi; --k) c += sG[lo * LD + k] * sG[hi * LD + k];
      c += (lo == hi ? sD[hi] : sG[lo * LD + hi]) * sD[hi];
      out[(long)i * wld + j] = c + sE[i] * sE[j];
    }
  }
  if (t == 0) {
    double q = 0.0;
    for (int j = 0; j < b; ++j) q += sA[j] * sE[j];
    lpd[g] = -0.5 * q + 0.5 * logdet - (double)b * CV_HALF_LOG_2PI;
    info[g] = 0;
  }
}

// ---- larger groups: blocks of order M = round_up(max_group, 128) in the work area, `C` groups per chunk -------------------------
// slot z = site * C + c (doubles): A (M x M: G_B, then its factor) | Tm (M^-1) | W (trtri scratch) | scal (16) | a (M) | u (M) |
// e (M) | info (POTRF_INFO_INTS ints)
struct CvSlots {
  long M, A, Tm, W, scal, a, u, e, info, elems;  // offsets in doubles; elems = the slot stride
  explicit CvSlots(long M_) : M(M_) {
    long o = 0;
    A = o; o += M * M;
    Tm = o; o += M * M;
    W = o; o += M * M;
    scal = o; o += 32;
    a = o; o += M;
    u = o; o += M;
    e = o; o += M;
    info = o; o += round_up((long)POTRF_INFO_INTS, 64) / 2;
    elems = round_up(o, 32);
  }
};
struct CvChunk {
  int g0, C, ngroups, n;  // groups g0 .. of this chunk (C slots per site), of ngroups; n = the plan's size
  long N, M;
};

__device__ __forceinline__ bool cv_chunk_group(const CvChunk& ck, const int* __restrict__ ns, const int* __restrict__ order,
                                               const int* __restrict__ start, int& site_id, int& g, int& nb, const int*& ord,
                                               int& s0, int& b) {
  site_id = (int)blockIdx.z / ck.C;
  g = ck.g0 + (int)blockIdx.z % ck.C;
  nb = ns ? ns[site_id] : ck.n;
  ord = order + (long)site_id * ck.n;
  s0 = 0;
  b = 0;
  if (g >= ck.ngroups) return false;
  cv_bounds(start + (long)site_id * (ck.ngroups + 1), g, nb, (int)ck.M, s0, b);
  return true;
}

// per slot: alpha_B (zero pad) and the first panel row k0 = min(B) rounded down to the k-tile
template <typename T>
__global__ __launch_bounds__(256) void cv_prep_kernel(CvChunk ck, CvSlots sl, double* __restrict__ slots, int* __restrict__ meta,
                                                      const T* __restrict__ alpha, long bs, const int* __restrict__ ns,
                                                      const int* __restrict__ order, const int* __restrict__ start) {
  __shared__ int smin[256];
  int sid, g, nb, s0, b;
  const int* ord;
  cv_chunk_group(ck, ns, order, start, sid, g, nb, ord, s0, b);
  double* slot = slots + (long)blockIdx.z * sl.elems;
  const T* al = alpha + (long)sid * bs;
  const int t = (int)threadIdx.x;
  int kmin = nb - 1;
  for (int c = t; c < (int)ck.M; c += 256) {
    double a = 0.0;
    if (c < b) {
      const int i = cv_index(ord, s0 + c, nb);
      kmin = min(kmin, i);
      a = (double)al[i];
    }
    slot[sl.a + c] = a;
  }
  smin[t] = kmin;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) smin[t] = min(smin[t], smin[t + w]);
    __syncthreads();
  }
  if (t == 0) meta[blockIdx.z] = max(smin[0], 0) & ~15;
}

// panel P[(k - k0)][c] = T[k][B_c] (k >= B_c; zero above the diagonal of T and in the pad columns), k0 <= k < N, as doubles
template <typename T>
__global__ __launch_bounds__(256) void cv_pack_kernel(CvChunk ck, const T* __restrict__ Tm, long bs, const int* __restrict__ ns,
                                                      const int* __restrict__ order, const int* __restrict__ start,
                                                      const int* __restrict__ meta, double* __restrict__ panels) {
  int sid, g, nb, s0, b;
  const int* ord;
  cv_chunk_group(ck, ns, order, start, sid, g, nb, ord, s0, b);
  const int k0 = meta[blockIdx.z];
  const int kbase = k0 + (int)blockIdx.y * 64;
  if (kbase >= ck.N) return;
  const int c = (int)blockIdx.x * 128 + ((int)threadIdx.x & 127);
  const T* Ts = Tm + (long)sid * bs;
  double* P = panels + (long)blockIdx.z * ck.N * ck.M;
  const int idx = c < b ? cv_index(ord, s0 + c, nb) : 0;
  for (int r = (int)threadIdx.x >> 7; r < 64; r += 2) {
    const int k = kbase + r;
    if (k >= ck.N) break;
    double v = 0.0;
    if (c < b && k >= idx) v = (double)Ts[(long)k * ck.N + idx];
    P[(long)(k - k0) * ck.M + c] = v;
  }
}

// G_B = P^T P, lower 128-tiles (diagonal tiles complete), k-tiles from the last to the first (the order of lauum)
__global__ __launch_bounds__(256, (TileCore<double, false, false, 128, 128, 1, true>::OCC)) void cv_gram_kernel(
    CvChunk ck, CvSlots sl, const double* __restrict__ panels, const int* __restrict__ meta, double* __restrict__ slots) {
  using K = TileCore<double, false, false, 128, 128, 1, true>;
  using G = typename K::G;
  __shared__ double smem[K::SMEM_ELEMS];
  int bm, bn;
  tri_decode((int)blockIdx.x, bm, bn);
  const double* P = panels + (long)blockIdx.z * ck.N * ck.M;
  const int ktiles = (int)((ck.N - meta[blockIdx.z]) / 16);
  typename G::acc_t acc[G::MI][G::NI];
  G::zero(acc);
  double* out = slots + (long)blockIdx.z * sl.elems + sl.A + (long)bm * 128 * ck.M + (long)bn * 128;
  const long ldc = ck.M;
  auto store = [&]() { K::foreach (acc, [&](int r, int c, double& v) { out[(long)r * ldc + c] = v; }); };
  K::template run_tri<true, TRI_NONE>(P + (long)bm * 128, ck.M, P + (long)bn * 128, ck.M, ktiles, smem, acc, store);
}

// identity pad of a block built by cv_gram_kernel (its pad rows / columns are exact zeros: the panel's pad columns are)
__global__ __launch_bounds__(256) void cv_pad_kernel(CvChunk ck, CvSlots sl, const int* __restrict__ ns, const int* __restrict__ order,
                                                     const int* __restrict__ start, double* __restrict__ slots) {
  int sid, g, nb, s0, b;
  const int* ord;
  cv_chunk_group(ck, ns, order, start, sid, g, nb, ord, s0, b);
  double* A = slots + (long)blockIdx.z * sl.elems + sl.A;
  for (int i = b + (int)threadIdx.x; i < (int)ck.M; i += 256) A[(long)i * ck.M + i] = 1.0;
}

// a valid K^^-1: the block is a gather of S (lower triangle stored), identity pad; lower 128-tiles, diagonal tiles complete
template <typename T>
__global__ __launch_bounds__(256) void cv_gather_kernel(CvChunk ck, CvSlots sl, const T* __restrict__ S, long bs,
                                                        const int* __restrict__ ns, const int* __restrict__ order,
                                                        const int* __restrict__ start, double* __restrict__ slots) {
  __shared__ int sri[128], sci[128];
  int sid, g, nb, s0, b;
  const int* ord;
  cv_chunk_group(ck, ns, order, start, sid, g, nb, ord, s0, b);
  int bm, bn;
  tri_decode((int)blockIdx.x, bm, bn);
  const int t = (int)threadIdx.x;
  if (t < 128) {
    const int i = bm * 128 + t;
    sri[t] = i < b ? cv_index(ord, s0 + i, nb) : -1;
  } else {
    const int j = bn * 128 + t - 128;
    sci[t - 128] = j < b ? cv_index(ord, s0 + j, nb) : -1;
  }
  __syncthreads();
  const T* Ss = S + (long)sid * bs;
  double* A = slots + (long)blockIdx.z * sl.elems + sl.A;
  const int c = t & 127, oj = sci[c], j = bn * 128 + c;
  for (int r = t >> 7; r < 128; r += 2) {
    const int oi = sri[r], i = bm * 128 + r;
    double v = i == j ? 1.0 : 0.0;
    if (oi >= 0 && oj >= 0) v = (double)Ss[(long)max(oi, oj) * ck.N + min(oi, oj)];
    A[(long)i * ck.M + j] = v;
  }
}

// u = M^-1 alpha_B: one wave per row
__global__ __launch_bounds__(256) void cv_trmv_kernel(CvSlots sl, double* __restrict__ slots) {
  double* slot = slots + (long)blockIdx.z * sl.elems;
  const double* Tm = slot + sl.Tm;
  const double* a = slot + sl.a;
  const int lane = (int)threadIdx.x & 63, i = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (i >= sl.M) return;
  double acc = 0.0;
  for (int j = lane; j <= i; j += 64) acc += Tm[(long)i * sl.M + j] * a[j];
  acc = wave_sum(acc);
  if (lane == 0) slot[sl.u + i] = acc;
}

// e_B = M^-T u and var = the column norms of M^-1: one thread per column, rows from the last to the diagonal
__global__ __launch_bounds__(256) void cv_cols_kernel(CvChunk ck, CvSlots sl, const int* __restrict__ ns, const int* __restrict__ order,
                                                      const int* __restrict__ start, double* __restrict__ slots,
                                                      double* __restrict__ resid, double* __restrict__ var) {
  int sid, g, nb, s0, b;
  const int* ord;
  cv_chunk_group(ck, ns, order, start, sid, g, nb, ord, s0, b);
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= b) return;
  double* slot = slots + (long)blockIdx.z * sl.elems;
  const double* Tm = slot + sl.Tm;
  const double* u = slot + sl.u;
  const int bad = ((const int*)(slot + sl.info))[0];
  double e = 0.0, ss = 0.0;
#pragma unroll 4
  for (int i = b - 1; i >= j; --i) {
    const double x = Tm[(long)i * sl.M + j];
    e += x * u[i];
    ss += x * x;
  }
  if (bad) e = ss = __longlong_as_double(0x7ff8000000000000LL);
  slot[sl.e + j] = e;
  const int i = cv_index(ord, s0 + j, nb);
  resid[(long)sid * ck.n + i] = e;
  var[(long)sid * ck.n + i] = ss;
}

// lpd_B = -1/2 alpha_B^T e_B + 1/2 log|G_B| - b/2 log 2 pi; info
__global__ __launch_bounds__(256) void cv_lpd_kernel(CvChunk ck, CvSlots sl, const int* __restrict__ ns, const int* __restrict__ order,
                                                     const int* __restrict__ start, const double* __restrict__ slots,
                                                     double* __restrict__ lpd, int* __restrict__ info) {
  __shared__ double sq[256];
  int sid, g, nb, s0, b;
  const int* ord;
  if (!cv_chunk_group(ck, ns, order, start, sid, g, nb, ord, s0, b)) return;
  const double* slot = slots + (long)blockIdx.z * sl.elems;
  const int t = (int)threadIdx.x;
  double q = 0.0;
  for (int j = t; j < b; j += 256) q += slot[sl.a + j] * slot[sl.e + j];
  sq[t] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) sq[t] += sq[t + w];
    __syncthreads();
  }
  if (t == 0) {
    const int bad = ((const int*)(slot + sl.info))[0];
    lpd[(long)sid * ck.ngroups + g] = b == 0 ? 0.0 : -0.5 * sq[0] + 0.5 * slot[sl.scal] - (double)b * CV_HALF_LOG_2PI;
    info[(long)sid * ck.ngroups + g] = b == 0 ? 0 : bad;
  }
}

long cv_block_order(long max_group) { return round_up(max_group, DGP_TILE_HOST); }
int cv_chunk_groups(long N, int B, int ngroups, long M) {
  long C = N / M;  // the chunk's panels together hold no more than one N x N matrix per site
  if (C > ngroups) C = ngroups;
  if (C > CV_MAX_CHUNK) C = CV_MAX_CHUNK;
  if (C * B > 65535) C = 65535 / B;
  return C < 1 ? 1 : (int)C;
}

}  // namespace

int cross_validate_chunk_groups(long N, int B, int ngroups, long max_group) {
  return max_group <= CV_SMALL ? 0 : cv_chunk_groups(N, B, ngroups, cv_block_order(max_group));
}

size_t cross_validate_workspace_bytes(long N, int B, int ngroups, long max_group) {
  if (max_group <= 1) return Carve::up(sizeof(double) * (size_t)(N / CV_SLAB) * (size_t)N * (size_t)B);
  if (max_group <= CV_SMALL) return 256;
  const long M = cv_block_order(max_group);
  const size_t nz = (size_t)cv_chunk_groups(N, B, ngroups, M) * (size_t)B;
  const CvSlots sl(M);
  return Carve::up(sizeof(double) * nz * (size_t)sl.elems) + Carve::up(sizeof(double) * (nz * (size_t)N + 64) * (size_t)M) + Carve::up(sizeof(int) * nz);
}

template <typename T>
int cross_validate(const T* Tm, const T* S, const T* alpha, long N, int n, const int* order, const int* start, int ngroups,
                   long max_group, void* work, double* resid, double* var, double* lpd, int* info, hipStream_t s, Batch bt, const CvTap* tap) {
  const unsigned Bz = (unsigned)bt.B;
  hipError_t e;
  // observations that no group holds out keep zeros
  if ((e = hipMemsetAsync(resid, 0, sizeof(double) * (size_t)n * Bz, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(var, 0, sizeof(double) * (size_t)n * Bz, s)) != hipSuccess) return (int)e;
  if (max_group <= 1) {
    double* part = (double*)work;
    const long ps = (N / CV_SLAB) * N;
    cv_colss_kernel<T><<<dim3((unsigned)((N + 255) / 256), (unsigned)(N / CV_SLAB), Bz), 256, 0, s>>>(Tm, N, bt.ws, part, ps);
    cv_loo_finish_kernel<T><<<dim3((unsigned)((ngroups + 255) / 256), 1, Bz), 256, 0, s>>>(part, ps, N, alpha, bt.ws, bt.ns, n, order, start,
                                                                                            ngroups, resid, var, lpd, info);
    return (int)hipGetLastError();
  }
  if (max_group <= CV_SMALL) {
    cv_small_kernel<T><<<dim3((unsigned)ngroups, 1, Bz), 256, 0, s>>>(Tm, S, N, bt.ws, alpha, bt.ns, n, order, start, ngroups, resid, var,
                                                                      lpd, info, tap ? tap->minv : nullptr, tap ? tap->ld : 0,
                                                                      tap ? tap->wblk : nullptr, tap ? tap->wld : 0,
                                                                      tap ? tap->wsite : 0);
    return (int)hipGetLastError();
  }
  const long M = cv_block_order(max_group);
  const int C = cv_chunk_groups(N, bt.B, ngroups, M);
  const size_t nz = (size_t)C * Bz;
  const CvSlots sl(M);
  double* slots = (double*)work;
  double* panels = (double*)((char*)work + Carve::up(sizeof(double) * nz * (size_t)sl.elems));
  int* meta = (int*)((char*)panels + Carve::up(sizeof(double) * (nz * (size_t)N + 64) * (size_t)M));  // (64 rows of slack)
  Tuning tune = bt.tuning();
  tune.chain_yield = 0;
  Batch bb;  // the chunk's blocks as one ragged-free batch of the library's own factor-and-invert
  bb.B = (int)nz;
  bb.ws = sl.elems;
  bb.tune = &tune;
  const int nt = (int)(M / DGP_TILE_HOST);
  const unsigned tiles = (unsigned)(nt * (nt + 1) / 2), Z = (unsigned)nz;
  for (int g0 = 0; g0 < ngroups; g0 += C) {
    const CvChunk ck{g0, C, ngroups, n, N, M};
    cv_prep_kernel<T><<<dim3(1, 1, Z), 256, 0, s>>>(ck, sl, slots, meta, alpha, bt.ws, bt.ns, order, start);
    if (S) {
      cv_gather_kernel<T><<<dim3(tiles, 1, Z), 256, 0, s>>>(ck, sl, S, bt.ws, bt.ns, order, start, slots);
    } else {
      cv_pack_kernel<T><<<dim3((unsigned)nt, (unsigned)(N / 64), Z), 256, 0, s>>>(ck, Tm, bt.ws, bt.ns, order, start, meta, panels);
      cv_gram_kernel<<<dim3(tiles, 1, Z), 256, 0, s>>>(ck, sl, panels, meta, slots);
      cv_pad_kernel<<<dim3(1, 1, Z), 256, 0, s>>>(ck, sl, bt.ns, order, start, slots);
    }
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    int rc = potrf<double>(slots + sl.A, M, slots + sl.Tm, slots + sl.scal, (int*)(slots + sl.info), 0, s, nullptr, nullptr, nullptr, bb);
    if (rc) return rc;
    if ((rc = trtri<double>(slots + sl.A, nullptr, M, slots + sl.Tm, slots + sl.W, s, bb))) return rc;
    cv_trmv_kernel<<<dim3((unsigned)(M / 4), 1, Z), 256, 0, s>>>(sl, slots);
    cv_cols_kernel<<<dim3((unsigned)((M + 255) / 256), 1, Z), 256, 0, s>>>(ck, sl, bt.ns, order, start, slots, resid, var);
    cv_lpd_kernel<<<dim3(1, 1, Z), 256, 0, s>>>(ck, sl, bt.ns, order, start, slots, lpd, info);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (tap && tap->chunk) {  // the chunk's blocks are complete on the stream: the caller's passes on them, before the next chunk
      const CvBlocks cb{slots + sl.Tm, slots + sl.e, sl.elems, M, g0, C, slots + sl.W};
      if ((rc = tap->chunk(tap->ctx, cb))) return rc;
    }
  }
  return 0;
}

template int cross_validate<double>(const double*, const double*, const double*, long, int, const int*, const int*, int, long, void*,
                                    double*, double*, double*, int*, hipStream_t, Batch, const CvTap*);
template int cross_validate<float>(const float*, const float*, const float*, long, int, const int*, const int*, int, long, void*, double*,
                                   double*, double*, int*, hipStream_t, Batch, const CvTap*);

}  // namespace dgp

using namespace dgp;

extern "C" {

size_t dgp_cross_validate_workspace_bytes(const dgp_plan* p, int ngroups, int64_t max_group) {
  if (!cv_sizes_ok(p, ngroups, max_group)) return 0;
  return cross_validate_workspace_bytes(p->N, p->B, ngroups, max_group);
}

int dgp_cross_validate(dgp_plan* p, const int32_t* order, const int32_t* start, int ngroups, int64_t max_group, void* work,
                       size_t work_bytes, double* resid, double* var, double* lpd, int32_t* info, void* stream) {
  if (!p) return fail(DGP_E_ARG, "null plan");
  if (!order || !start || !resid || !var || !lpd || !info) return fail(DGP_E_ARG, "dgp_cross_validate: null argument");
  if (!cv_sizes_ok(p, ngroups, max_group))
    return fail(DGP_E_ARG, "dgp_cross_validate: bad size (1 <= ngroups <= n, 1 <= max_group <= n)");
  DGP_CHECK_PLAN(p);
  int rc = need_factor(p, "dgp_cross_validate", "call dgp_factorize or dgp_fit_step");
  if (rc || (rc = need_work(work, work_bytes, dgp_cross_validate_workspace_bytes(p, ngroups, max_group), "dgp_cross_validate"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  // K^^-1 (S) is read when the last step left it valid and never written; after a bare dgp_factorize it is dead and ignored
  const void* S = p->have_inverse ? p->S : nullptr;
  rc = DGP_BY_DTYPE(
      p,
      cross_validate<double>((const double*)p->Tm, (const double*)S, (const double*)p->alpha, p->N, (int)p->n, order, start, ngroups,
                             max_group, work, resid, var, lpd, info, s, batch_of<double>(p)),
      cross_validate<float>((const float*)p->Tm, (const float*)S, (const float*)p->alpha, p->N, (int)p->n, order, start, ngroups, max_group,
                            work, resid, var, lpd, info, s, batch_of<float>(p)));
  return wrap(rc, "dgp_cross_validate");
}

}  // extern "C"
