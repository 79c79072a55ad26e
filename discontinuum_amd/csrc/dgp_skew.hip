// dgp_skew.hip -- the exact THIRD central moment of period sums of a log-transformed Gaussian posterior
// (dgp_period_third_moments): the skewness of annual / monthly loads, beside the mean and covariance of dgp_period_moments.
//
// Setting and notation of dgp_aggregate.hip, mode 1: f ~ N(mu, C) over m points (C: the matrix dgp_posterior_cov leaves, lower
// triangle read, extra_var added on the diagonal), mu already mapped, s2 = s^2, a_i = w_i exp(mu_i + s2 C_ii / 2),
// e_ij = expm1(s2 C_ij), group ids g_i non-decreasing except for -1 (excluded).  For the period sum S_g = sum_{i in g} w_i exp(s f_i + t):
//     k3_g = E[(S_g - E S_g)^3] = sum_{i,j,k in g} a_i a_j a_k (e_ij e_ik e_jk + e_ij e_ik + e_ij e_jk + e_ik e_jk)
//          = sum_{i,j in g} a_i a_j e_ij G_ij  +  3 sum_{i in g} a_i y_i^2,     G = e_gg diag(a_g) e_gg^T,   y_i = sum_{j in g} a_j e_ij
// -- no moment is ever subtracted from another.  Launches (gridDim.z = sites), everything after the loads of C and mu in double:
//   sk_init / sk_prep   one thread per point: a_i, its period (or -1: excluded, pad), each period's column range (integer atomics)
//   sk_blocks           one thread per 64-row block: the union [lo, hi) of the column ranges of the periods its rows lie in
//   sk_mirror           loo_mirror_kernel's pattern: F = e MASKED to the block diagonal of the periods (entries of two different
//                       periods, of excluded points and of the pad are exact zeros), upper triangle filled from the lower, and
//                       Gm = F diag(a); both row-major, so that
//   sk_sandwich         G = F Gm^T is ONE A B^T product of two k-contiguous operands on the tile cores (TileCore<double, true, true>:
//                       the direct-to-LDS core on 128 x 128 tiles, the register-staged one on 64 x 64 tiles while a launch has too
//                       few of them -- lauum's rule), lower tiles only, k clipped to the column ranges both tile rows share (a
//                       pair that shares none is skipped).  G is NOT stored: the epilogue multiplies every accumulator entry by
//                       the Gm_ij = e_ij a_j it faces, sums along the tile's rows (a fixed butterfly, then the two wave columns),
//                       times a_i, twice for a tile below the diagonal: one partial per (tile, row)
//   sk_rows             one wave per row i: the row's partials over its tiles in order, y_i as the row sum of Gm, 3 a_i y_i^2
//   sk_finish           one workgroup per period: its rows' totals in a fixed order
// No floating-point atomics, every sum in a fixed order: results repeat bitwise and a site's numbers do not depend on its batch.
// A violated group order gives wrong numbers only: every column range lies in [0, m] whatever the ids are.
#include <climits>

#include "../../include/dgp_hip.h"
#include "dgp_gemm_dma.h"
#include "dgp_plan.h"

namespace dgp {

namespace {

// byte offsets inside a site's slice of the work area
struct SkLayout {
  size_t a, rowk, gp, se, blk, part, F, Gm, slice;
};
SkLayout sk_layout(long M, int P) {
  const size_t m = (size_t)M, nb64 = m / 64;
  Carve c;
  SkLayout L;
  L.a = c.take(sizeof(double) * m);
  L.rowk = c.take(sizeof(double) * m);
  L.gp = c.take(sizeof(int) * m);
  L.se = c.take(sizeof(int) * 2 * (size_t)P);
  L.blk = c.take(sizeof(int) * 2 * nb64);
  L.part = c.take(sizeof(double) * (nb64 * (nb64 + 1) / 2) * 64);  // (tile, row) partials: the 64-tile count covers the 128-tile one
  L.F = c.take(sizeof(double) * m * m);
  L.Gm = c.take(sizeof(double) * m * m);
  L.slice = c.o;
  return L;
}

template <typename U>
__device__ __forceinline__ U* sk_at(char* work, size_t slice, size_t off) {
  return reinterpret_cast<U*>(work + (size_t)blockIdx.z * slice + off);
}

__global__ __launch_bounds__(256) void sk_init_kernel(char* work, SkLayout L, int P) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  int* se = sk_at<int>(work, L.slice, L.se);
  se[2 * g] = INT_MAX;
  se[2 * g + 1] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void sk_prep_kernel(const T* __restrict__ cov, long M, int m, int P, const T* __restrict__ mu,
                                                      const double* __restrict__ scale2, const double* __restrict__ w,
                                                      const int* __restrict__ group, const T* __restrict__ ev, char* work, SkLayout L) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = blockIdx.z;
  if (j >= M) return;
  double* a = sk_at<double>(work, L.slice, L.a);
  int* gp = sk_at<int>(work, L.slice, L.gp);
  int* se = sk_at<int>(work, L.slice, L.se);
  double av = 0.0;
  int gv = -1;
  if (j < m) {
    const long k = (long)z * m + j;
    const int g = group[k];
    if (g >= 0 && g < P) {
      double cjj = (double)cov[(long)z * M * M + j * (M + 1)];
      if (ev) cjj += (double)ev[k];
      av = w[k] * exp((double)mu[k] + 0.5 * scale2[z] * cjj);
      gv = g;
      // only the ends of a run of equal ids can hold a period's first or last point (whatever the order of the ids): two
      // atomics per run instead of two per point, which all hit one address when the record is one period
      if (j == 0 || group[k - 1] != g) atomicMin(&se[2 * g], (int)j);
      if (j + 1 == m || group[k + 1] != g) atomicMax(&se[2 * g + 1], (int)j + 1);
    }
  }
  a[j] = av;
  gp[j] = gv;
}

__global__ __launch_bounds__(256) void sk_blocks_kernel(long M, char* work, SkLayout L) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= M / 64) return;
  const int* gp = sk_at<int>(work, L.slice, L.gp);
  const int* se = sk_at<int>(work, L.slice, L.se);
  int* blk = sk_at<int>(work, L.slice, L.blk);
  int lo = INT_MAX, hi = 0;
  for (int q = 0; q < 64; ++q) {
    const int g = gp[b * 64 + q];
    if (g >= 0) {
      lo = min(lo, se[2 * g]);
      hi = max(hi, se[2 * g + 1]);
    }
  }
  blk[2 * b] = lo;
  blk[2 * b + 1] = hi;
}

// tile (bi, bj), bi >= bj, of the lower triangle of C -> the tiles (bi, bj) and (bj, bi) of F and Gm
template <typename T>
__global__ __launch_bounds__(256) void sk_mirror_kernel(const T* __restrict__ cov, long M, int m, const double* __restrict__ scale2,
                                                        const T* __restrict__ ev, char* work, SkLayout L) {
  const T* C = cov + (long)blockIdx.z * M * M;
  const double* a = sk_at<double>(work, L.slice, L.a);
  const int* gp = sk_at<int>(work, L.slice, L.gp);
  double* F = sk_at<double>(work, L.slice, L.F);
  double* Gm = sk_at<double>(work, L.slice, L.Gm);
  const double s2 = scale2[blockIdx.z];
  __shared__ double tile[64][65];
  int bi, bj;
  tri_decode(blockIdx.x, bi, bj);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)bi * 64, c0 = (long)bj * 64;
  const int gc = gp[c0 + tx];
  for (int r = ty; r < 64; r += 4) {
    const long i = r0 + r, j = c0 + tx;
    double e = 0.0;
    // same period only (a select: anything else -- pad, excluded, other periods -- is an exact zero); a diagonal tile is valid on
    // and below its diagonal
    if (gc >= 0 && gp[i] == gc && (bi != bj || tx <= r)) {
      double x = (double)C[i * M + j];
      if (i == j && ev) x += (double)ev[(long)blockIdx.z * m + i];
      e = expm1(s2 * x);
    }
    tile[r][tx] = e;
  }
  __syncthreads();
  if (bi != bj) {
    const double ac = a[c0 + tx], ar = a[r0 + tx];
    for (int r = ty; r < 64; r += 4) {
      const double v = tile[r][tx];
      F[(r0 + r) * M + c0 + tx] = v;
      Gm[(r0 + r) * M + c0 + tx] = v * ac;
      const double u = tile[tx][r];  // (row c0 + r, column r0 + tx) of the mirror tile
      F[(c0 + r) * M + r0 + tx] = u;
      Gm[(c0 + r) * M + r0 + tx] = u * ar;
    }
  } else {
    const double ac = a[c0 + tx];
    for (int r = ty; r < 64; r += 4) {
      const double v = tx <= r ? tile[r][tx] : tile[tx][r];
      F[(r0 + r) * M + c0 + tx] = v;
      Gm[(r0 + r) * M + c0 + tx] = v * ac;
    }
  }
}

// G[I, J] = sum_k F[I, k] Gm[J, k], I >= J, contracted in the epilogue: part[tile][r] = f a_i sum_j Gm_ij G_ij over the tile's
// columns j (f = 2 below the diagonal: the mirror tile's share, which belongs to the same periods)
template <int BT>
__global__ __launch_bounds__(256, (TileCore<double, true, true, BT, BT>::OCC)) void sk_sandwich_kernel(long M, char* work, SkLayout L) {
  using K = TileCore<double, true, true, BT, BT>;
  using TG = typename K::G;
  static_assert(2 * BT <= K::SMEM_ELEMS, "the row sums do not fit the tile core's LDS array");
  const double* a = sk_at<double>(work, L.slice, L.a);
  const int* blk = sk_at<int>(work, L.slice, L.blk);
  const double* F = sk_at<double>(work, L.slice, L.F);
  const double* Gm = sk_at<double>(work, L.slice, L.Gm);
  double* part = sk_at<double>(work, L.slice, L.part) + (long)blockIdx.x * BT;
  __shared__ __attribute__((aligned(16))) double smem[K::SMEM_ELEMS];
  int bi, bj;
  tri_decode(blockIdx.x, bi, bj);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // the k-range: the columns of the periods both tile rows touch, widened to the cores' k-tiles of 16 (F is zero outside)
  int k0 = 0, k1 = INT_MAX;
  {
    int loi = INT_MAX, hii = 0, loj = INT_MAX, hij = 0;
#pragma unroll
    for (int q = 0; q < BT / 64; ++q) {
      loi = min(loi, blk[2 * (bi * (BT / 64) + q)]);
      hii = max(hii, blk[2 * (bi * (BT / 64) + q) + 1]);
      loj = min(loj, blk[2 * (bj * (BT / 64) + q)]);
      hij = max(hij, blk[2 * (bj * (BT / 64) + q) + 1]);
    }
    k0 = max(loi, loj);
    k1 = min(hii, hij);
  }
  if (k1 <= k0) {  // (uniform) no common period: the rows pass still reads this tile's partials
    if (t < BT) part[t] = 0.0;
    return;
  }
  k0 &= ~15;
  k1 = min((k1 + 15) & ~15, (int)M);
  typename TG::acc_t acc[TG::MI][TG::NI];
  TG::zero(acc);
  K::run(F + (long)bi * BT * M + k0, M, Gm + (long)bj * BT * M + k0, M, (k1 - k0) / 16, smem, acc);
  const int wm = (w >> 1) * (BT / 2), wn = (w & 1) * (BT / 2);
  const double* Wt = Gm + (long)bi * BT * M + (long)bj * BT;
  __syncthreads();  // every wave is done with the operands' LDS image
#pragma unroll
  for (int mi = 0; mi < TG::MI; ++mi) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ni = 0; ni < TG::NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        s[r] += acc[mi][ni][r] * Wt[(long)(wm + mi * 16 + Mfma<double>::crow(lane, r)) * M + wn + ni * 16 + (lane & 15)];
    // the 16 columns of a sub-tile row (the lanes of one lane >> 4 group), a fixed butterfly
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = s[r];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
      if ((lane & 15) == 0) smem[(w & 1) * BT + wm + mi * 16 + Mfma<double>::crow(lane, r)] = v;
    }
  }
  __syncthreads();
  if (t < BT) part[t] = (bi != bj ? 2.0 : 1.0) * a[(long)bi * BT + t] * (smem[t] + smem[BT + t]);
}

// one wave per row: rowk_i = sum over the row's tiles of its partial + 3 a_i y_i^2
__global__ __launch_bounds__(256) void sk_rows_kernel(long M, int BT, char* work, SkLayout L) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;
  const double* a = sk_at<double>(work, L.slice, L.a);
  const int* gp = sk_at<int>(work, L.slice, L.gp);
  const int* se = sk_at<int>(work, L.slice, L.se);
  const double* part = sk_at<double>(work, L.slice, L.part);
  const double* Gm = sk_at<double>(work, L.slice, L.Gm);
  double* rowk = sk_at<double>(work, L.slice, L.rowk);
  const int g = gp[i];
  double y = 0.0, p = 0.0;
  if (g >= 0) {  // (uniform over the wave)
    const int c0 = se[2 * g], c1 = se[2 * g + 1];
    const double* row = Gm + i * M;
    for (int k = c0 + lane; k < c1; k += 64) y += row[k];
    const long bi = i / BT, r = i % BT, base = bi * (bi + 1) / 2;
    for (long bj = lane; bj <= bi; bj += 64) p += part[(base + bj) * BT + r];
  }
  y = wave_sum(y);
  p = wave_sum(p);
  if (lane == 0) rowk[i] = g >= 0 ? p + 3.0 * a[i] * y * y : 0.0;
}

__global__ __launch_bounds__(256) void sk_finish_kernel(int P, char* work, SkLayout L, double* __restrict__ out) {
  const int g = blockIdx.x, t = threadIdx.x;
  const int* gp = sk_at<int>(work, L.slice, L.gp);
  const int* se = sk_at<int>(work, L.slice, L.se);
  const double* rowk = sk_at<double>(work, L.slice, L.rowk);
  const int c0 = se[2 * g], c1 = se[2 * g + 1];  // an empty period: INT_MAX, 0
  __shared__ double red[256];
  double v = 0.0;
  for (long i = (long)c0 + t; i < c1; i += 256)
    if (gp[i] == g) v += rowk[i];
  red[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) out[(long)blockIdx.z * P + g] = red[0];
}

template <typename T>
int period_third_moments(const T* cov, long m, int B, const T* mu, const double* scale2, const double* w, const int* group, int P,
                         const T* ev, int tile, char* work, double* out, hipStream_t s) {
  const long M = round_up(m, DGP_TILE_HOST), nb64 = M / 64, nbk = M / DGP_TILE_HOST;
  const SkLayout L = sk_layout(M, P);
  const unsigned Bz = (unsigned)B;
  sk_init_kernel<<<dim3((unsigned)((P + 255) / 256), 1, Bz), 256, 0, s>>>(work, L, P);
  sk_prep_kernel<T><<<dim3((unsigned)((M + 255) / 256), 1, Bz), 256, 0, s>>>(cov, M, (int)m, P, mu, scale2, w, group, ev, work, L);
  sk_blocks_kernel<<<dim3((unsigned)((nb64 + 255) / 256), 1, Bz), 256, 0, s>>>(M, work, L);
  sk_mirror_kernel<T><<<dim3((unsigned)(nb64 * (nb64 + 1) / 2), 1, Bz), 256, 0, s>>>(cov, M, (int)m, scale2, ev, work, L);
  const long tiles = nbk * (nbk + 1) / 2;
  if (tile == 0) tile = tiles * B <= default_tuning().lauum64_max_tiles ? 64 : 128;  // fewer 128-tiles than fill the CUs: lauum's rule
  if (tile == 64)
    sk_sandwich_kernel<64><<<dim3((unsigned)(nb64 * (nb64 + 1) / 2), 1, Bz), 256, 0, s>>>(M, work, L);
  else
    sk_sandwich_kernel<128><<<dim3((unsigned)tiles, 1, Bz), 256, 0, s>>>(M, work, L);
  sk_rows_kernel<<<dim3((unsigned)(M / 4), 1, Bz), 256, 0, s>>>(M, tile, work, L);
  sk_finish_kernel<<<dim3((unsigned)P, 1, Bz), 256, 0, s>>>(P, work, L, out);
  return (int)hipGetLastError();
}

bool sk_sizes_ok(int64_t m, int ngroups, int batch) {
  return m > 0 && m <= (1 << 20) && ngroups > 0 && ngroups <= 65535 && batch > 0 && batch <= DGP_MAX_BATCH_SITES;
}

}  // namespace

}  // namespace dgp

using namespace dgp;

extern "C" {

size_t dgp_period_third_moments_workspace_bytes(int64_t m, int ngroups, int batch) {
  if (!sk_sizes_ok(m, ngroups, batch)) return 0;
  return (size_t)batch * sk_layout(round_up(m, DGP_TILE_HOST), ngroups).slice;
}

int dgp_period_third_moments(int dtype, const void* cov, int64_t m, int batch, const void* mu, const double* scale2, const double* w,
                             const int32_t* group, int ngroups, const void* extra_var, int tile, void* work, size_t work_bytes,
                             double* k3_out, void* stream) {
  if (dtype != DGP_F64 && dtype != DGP_F32) return fail(DGP_E_ARG, "dgp_period_third_moments: dtype must be 0 (f64) or 1 (f32)");
  if (!cov || !mu || !scale2 || !w || !group || !k3_out) return fail(DGP_E_ARG, "dgp_period_third_moments: null argument");
  if (!sk_sizes_ok(m, ngroups, batch))
    return fail(DGP_E_ARG, "dgp_period_third_moments: bad size (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= batch <= 1024)");
  if (tile != 0 && tile != 64 && tile != 128) return fail(DGP_E_ARG, "dgp_period_third_moments: tile must be 0 (by size), 64 or 128");
  if (int rc = need_work(work, work_bytes, dgp_period_third_moments_workspace_bytes(m, ngroups, batch), "dgp_period_third_moments"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == DGP_F64 ? period_third_moments<double>((const double*)cov, m, batch, (const double*)mu, scale2, w, group, ngroups,
                                                                 (const double*)extra_var, tile, (char*)work, k3_out, s)
                                  : period_third_moments<float>((const float*)cov, m, batch, (const float*)mu, scale2, w, group, ngroups,
                                                                (const float*)extra_var, tile, (char*)work, k3_out, s);
  return wrap(rc, "dgp_period_third_moments");
}

}  // extern "C"
