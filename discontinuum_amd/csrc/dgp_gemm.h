// dgp_gemm.h -- LDS-tiled MFMA tile-GEMM core shared by the Cholesky / inverse / predict kernels.
//
// One workgroup (256 threads = 4 waves, arranged 2 x 2) accumulates a BM x BN output tile
//     acc[i][j] += sum_k  opA(i, k) * opB(j, k)
// over `ktiles` k-tiles of depth 16.  Each operand is addressed through a base pointer to the
// tile's (row 0, k 0) element and is either
//     KC  ("k-contiguous"):  op(i, k) = p[i * ld + k]     (a row-major panel, rows = i)
//     IC  ("i-contiguous"):  op(i, k) = p[k * ld + i]     (a row-major matrix read transposed)
// so NT / NN / TN products are the same routine.  Roofline: MFMA (fp64 16x16x4 is 64 cycles per
// 2048 flop per SIMD); the LDS image is laid out so every ds_read_b64 fragment read is
// bank-conflict free:  KC -> [row][17] (odd stride), IC -> [k][rows+16] (stride = 128 B mod 256 B).
#pragma once
#include <type_traits>
#include "dgp_common.h"

namespace dgp {

template <typename T, bool KC, int ROWS, int BK_ = 16>
struct OperandTile {
  // depth of a k-tile.  16 everywhere in the product: 32 (half as many barrier episodes per flop) measured +3 % stand-alone
  // on row-contiguous fp64 operands and on fp32 (scripts/gemm_occ.hip: 68.9 -> 70.9, 133.7 -> 137.6 TFLOP/s), -8 % on
  // k-contiguous fp64 ones, and nothing in situ (lauum 89.4 -> 90.1 ms per 32 sites)
  static constexpr int BK = BK_;
  static constexpr int EPT = ROWS * BK / 256;  // elements staged per thread per k-tile (8 or 4)
  static constexpr int STRIDE = KC ? (BK + 1) : (ROWS + 16);
  static constexpr int ELEMS = KC ? ROWS * (BK + 1) : BK * (ROWS + 16);
  static constexpr int VN = Vec16<T>::N;
  static constexpr int NV = EPT / VN;
  using vec_t = typename Vec16<T>::type;
  static_assert(EPT % VN == 0, "staging vector width");

  // Staging map: vector v (VN consecutive elements = 16 bytes) of thread t starts at (r, c) = coords(t, v).
  //   IC: lane l of a load instruction reads bytes [16 l, 16 l + 16) of one k-row, i.e. a wave covers
  //       whole contiguous lines (measured 60.7 -> 68.5 TFLOP/s fp64 against a strided map);
  //   KC: a tile row is only 16 k's (128 B fp64): each thread reads EPT consecutive k's of one row
  //       (measured 68.8 vs 65.8 TFLOP/s for the line-interleaved alternative).
  static __device__ __forceinline__ void coords(int t, int v, int& r, int& c) {
    if (KC) {
      r = t / (BK / EPT);                      // tile row
      c = (t % (BK / EPT)) * EPT + v * VN;     // k offset
    } else {
      const int idx = v * 256 + t;             // linear vector index, k-row major
      r = idx / (ROWS / VN);                   // k
      c = (idx % (ROWS / VN)) * VN;            // tile-row offset
    }
  }
  static __device__ __forceinline__ void load(const T* __restrict__ p, long ld, T (&reg)[EPT], int t) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int r, c;
      coords(t, v, r, c);
      const vec_t x = *reinterpret_cast<const vec_t*>(p + (long)r * ld + c);
#pragma unroll
      for (int e = 0; e < VN; ++e) reg[v * VN + e] = x[e];
    }
  }
  static __device__ __forceinline__ void store(T* __restrict__ s, const T (&reg)[EPT], int t) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int r, c;
      coords(t, v, r, c);
      T* dst = s + r * STRIDE + c;
#pragma unroll
      for (int e = 0; e < VN; ++e) dst[e] = reg[v * VN + e];
    }
  }
  // fragment element for the 16-row group starting at tile row `row0`, k-step ks (4 k's each)
  static __device__ __forceinline__ T frag(const T* __restrict__ s, int row0, int ks, int lane) {
    if (KC) return s[(row0 + (lane & 15)) * STRIDE + ks * 4 + (lane >> 4)];
    return s[(ks * 4 + (lane >> 4)) * STRIDE + row0 + (lane & 15)];
  }
};

template <typename T, bool A_KC, bool B_KC, int BM = 128, int BN = 128, int BK = 16>
struct TileGemm {
  using OA = OperandTile<T, A_KC, BM, BK>;
  using OB = OperandTile<T, B_KC, BN, BK>;
  using acc_t = typename Mfma<T>::acc_t;
  static constexpr int MI = BM / 32;  // 16-row MFMA tiles per wave in M
  static constexpr int NI = BN / 32;
  static constexpr int SMEM_ELEMS = OA::ELEMS + OB::ELEMS;

  static __device__ __forceinline__ void zero(acc_t (&acc)[MI][NI]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = T(0);
  }

  // one k-tile: LDS image from the staged registers, refill them with k-tile `kt + PF`, then the MFMAs
  template <int PF>
  static __device__ __forceinline__ void ktile(const T* __restrict__& A, long lda, const T* __restrict__& B, long ldb,
                                               long stepA, long stepB, int kt, int ktiles, T* __restrict__ sA,
                                               T* __restrict__ sB, T (&ra)[OA::EPT], T (&rb)[OB::EPT],
                                               acc_t (&acc)[MI][NI], int t, int lane, int wm, int wn) {
    __syncthreads();  // everyone is done reading the previous k-tile's LDS image
    OA::store(sA, ra, t);
    OB::store(sB, rb, t);
    __syncthreads();
    if (kt + PF < ktiles) {  // the global loads of a later k-tile fly under this tile's MFMAs
      OA::load(A + PF * stepA, lda, ra, t);
      OB::load(B + PF * stepB, ldb, rb, t);
    }
    A += stepA;
    B += stepB;
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      T fa[MI], fb[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) fa[mi] = OA::frag(sA, wm + mi * 16, ks, lane);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) fb[ni] = OB::frag(sB, wn + ni * 16, ks, lane);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = Mfma<T>::mma(fa[mi], fb[ni], acc[mi][ni]);
    }
  }

  // PF = number of k-tiles the global loads run ahead of the MFMAs (register-staged).  PF = 2 costs one more
  // set of staging registers and pays where the operands miss L2 (long, unsynchronised k-ranges: lauum / trtri).
  // REV: the k-tiles are visited from the LAST to the first (inside a k-tile of 16 the order stays ascending) -- for
  // products whose terms DECAY along k (K^^-1 = L^-T L^-1: k starts at the diagonal block, where L^-1 is largest): summed
  // large-to-small in fp32, every late product below half an ulp of the running sum is dropped, a systematic loss
  // (measured: tr(S K^) - n = -109 at n = 16384, all of the fp32 plans' gradient error); small-to-large keeps them.
  template <int PF = 1, bool REV = false>
  static __device__ __forceinline__ void run(const T* __restrict__ A, long lda, const T* __restrict__ B, long ldb,
                                             int ktiles, T* __restrict__ smem, acc_t (&acc)[MI][NI]) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * (BM / 2), wn = (w & 1) * (BN / 2);
    T* sA = smem;
    T* sB = smem + OA::ELEMS;
    ktiles = ktiles * 16 / BK;  // callers count k in tiles of 16; every k-range is a multiple of 128
    long stepA = A_KC ? BK : BK * lda;
    long stepB = B_KC ? BK : BK * ldb;
    if (REV) {
      A += (long)(ktiles - 1) * stepA;
      B += (long)(ktiles - 1) * stepB;
      stepA = -stepA;
      stepB = -stepB;
    }
    T ra[PF][OA::EPT], rb[PF][OB::EPT];
#pragma unroll
    for (int p = 0; p < PF; ++p)
      if (p < ktiles) {
        OA::load(A + p * stepA, lda, ra[p], t);
        OB::load(B + p * stepB, ldb, rb[p], t);
      }
    for (int kt = 0; kt < ktiles; kt += PF) {
#pragma unroll
      for (int p = 0; p < PF; ++p)
        if (kt + p < ktiles)
          ktile<PF>(A, lda, B, ldb, stepA, stepB, kt + p, ktiles, sA, sB, ra[p], rb[p], acc, t, lane, wm, wn);
    }
  }

  // visit every accumulator element this lane owns: f(tile_row, tile_col, value&)
  template <typename F>
  static __device__ __forceinline__ void foreach (acc_t (&acc)[MI][NI], F f) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * (BM / 2), wn = (w & 1) * (BN / 2);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          T v = acc[mi][ni][r];
          f(wm + mi * 16 + Mfma<T>::crow(lane, r), wn + ni * 16 + (lane & 15), v);
          acc[mi][ni][r] = v;
        }
  }
};

// How a trailing-update tile C -= P_i P_j^T meets its accumulators.
//   fp64: the accumulators START at -C, so the read of C overlaps the first operand loads and the epilogue is
//         store-only:  C_new = -( -C + P_i P_j^T ).
//   fp32: the products are summed FROM ZERO and C joins once at the end.  Started at -C, every one of the pass's K
//         fmaf steps rounds at the magnitude of C while the terms it adds are far smaller: products below half an ulp
//         of C are dropped outright (a Schur-complement diagonal only ever adds squares, so its pivots come out too
//         LARGE -- measured: log-determinant +0.30 at rating n = 16384, growing linearly along the matrix, and the same
//         sign on every matrix tried), and the rest contributes K roundings at |C| per pass instead of one.
// fp32 keeps C in registers from the start of the tile (the loads fly under the first operand loads, as they do in
// the fp64 form) and subtracts the finished sum from it in the epilogue: `keep` has the accumulators' shape.
// G = the tile map the accumulators follow: a TileGemm, or a TileCore (whose map may be the interleaved one, dgp_gemm_dma.h).
// LATE (fp32 only): C is read in the epilogue instead -- the direct-to-LDS core runs at 168 registers per lane, where a
// second accumulator-sized array only survives the k-loop in scratch memory (measured: bulk update 109 -> 101 TFLOP/s).
// The tile of C moves in plain 8-byte (fp32: 4-byte) accesses.  Two other forms were built for the bulk update and measured: loads and
// stores with the non-temporal hint, and 16-byte accesses with a lane-pair swap (fp64).  On the tile alone both gain (scripts/
// syrk_persist.hip, which keeps its own copy of the wide form: K = 512 64.0 -> 68.6 / 69.7 TFLOP/s, both 70.6); in situ every one
// ties or loses -- the hint moves the bulk launches' sum 79.2 -> 75.7 ms and the step not at all; the swap on 128 live accumulator
// registers spills 400 bytes of scratch per lane around every tile: step 275.4 -> 280.2 ms at 32 x n = 8192, 11.90 -> 12.55 for one
// site (EXPERIMENTS.md round 5).  Removed.
// The tile of C on the plain accumulator map through SCALAR row bases + one 32-bit lane offset (round 5).  `G::foreach` hands out
// (row, column) pairs and the obvious `C[row * ld + col]` makes the compiler keep a 64-bit address per access: with the 128
// accumulators of an fp64 128 x 128 tile live at the same time that cost the bulk update 20 spilled registers around every tile.
// Here the part of the address that depends on the lane -- (crow(lane, 0) * ld + (lane & 15)) elements -- is ONE register, the
// rest (wave tile, 16-row group, register index) is wave-uniform and lives in scalar registers, so every access is the saddr
// form of global_load / global_store with an immediate for the 16-column group.  Same elements, same values; measured on the
// bulk tile alone (scripts/syrk_persist.hip, fp64): K = 512 64.3 -> 68.2 TFLOP/s, K = 256 53.2 -> 58.1, no spill, 166 registers.
// f(ptr, mi, ni, r): ptr = the address of the element that accumulator [mi][ni][r] of this lane stands for.
template <typename T, typename G, typename P, typename F>
__device__ __forceinline__ void tile_rows_foreach(P* __restrict__ C, long ld, F f) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const unsigned loff = (unsigned)(((long)Mfma<T>::crow(lane, 0) * ld + (lane & 15)) * (long)sizeof(T));
  char* Cw = (char*)(const_cast<typename std::remove_const<P>::type*>(C) + (long)((w >> 1) * (16 * G::MI)) * ld + (w & 1) * (16 * G::NI));
  const int rstep = Mfma<T>::crow(0, 1);  // rows between consecutive accumulator registers (fp64: 4, fp32: 1)
#pragma unroll
  for (int mi = 0; mi < G::MI; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      char* rp = Cw + (long)(mi * 16 + rstep * r) * ld * (long)sizeof(T);
#pragma unroll
      for (int ni = 0; ni < G::NI; ++ni) f(reinterpret_cast<P*>(rp + ni * 16 * (int)sizeof(T) + loff), mi, ni, r);
    }
}
template <typename T, typename G, bool LATE = false>
__device__ __forceinline__ void trailing_begin(typename G::acc_t (&acc)[G::MI][G::NI], typename G::acc_t (&keep)[G::MI][G::NI],
                                               const T* __restrict__ C, long ld) {
  if (sizeof(T) == 4) {
    if (!LATE) tile_rows_foreach<T, G>(C, ld, [&](const T* q, int mi, int ni, int r) { keep[mi][ni][r] = *q; });
    G::zero(acc);
  } else {
    tile_rows_foreach<T, G>(C, ld, [&](const T* q, int mi, int ni, int r) { acc[mi][ni][r] = -*q; });
  }
}
template <typename T, typename G, bool LATE = false>
__device__ __forceinline__ void trailing_end(typename G::acc_t (&acc)[G::MI][G::NI], typename G::acc_t (&keep)[G::MI][G::NI],
                                             T* __restrict__ C, long ld) {
  if (sizeof(T) == 4 && LATE) {
    tile_rows_foreach<T, G>(C, ld, [&](T* q, int mi, int ni, int r) { acc[mi][ni][r] = *q - acc[mi][ni][r]; });
    tile_rows_foreach<T, G>(C, ld, [&](T* q, int mi, int ni, int r) { *q = (T)acc[mi][ni][r]; });
  } else if (sizeof(T) == 4) {
#pragma unroll
    for (int mi = 0; mi < G::MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < G::NI; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = keep[mi][ni][r] - acc[mi][ni][r];
    tile_rows_foreach<T, G>(C, ld, [&](T* q, int mi, int ni, int r) { *q = (T)acc[mi][ni][r]; });
  } else {
    tile_rows_foreach<T, G>(C, ld, [&](T* q, int mi, int ni, int r) { *q = T(-acc[mi][ni][r]); });
  }
}

}  // namespace dgp
