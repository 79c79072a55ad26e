// dgp_schedule.h -- the batched factorisation's schedule as DATA, and its checker.  Plain C++: no HIP in this file (a host
// program compiles against it alone: tests/test_potrf_schedule_cpu.py).
//
// The matrix is a grid of nbk x nbk 128-blocks, lower triangle.  In fp64 a trailing tile starts its accumulators at -C, adds
// its products in ascending k and stores -acc (dgp_gemm.h::trailing_begin / trailing_end); a store and a reload of a double is
// exact, so one pass over the k-blocks [a, c) leaves the bits of a pass over [a, b) followed by one over [b, c).  Hence
//     every schedule in which each tile receives its k-blocks in ascending, gap-free order gives bitwise the same factor
// and a schedule is free to choose how long its passes are.  An Op is one launch (or one short chain of launches):
//   UPDATE  tiles (i, j), j in [c0, c1), i in [max(r0, j), r1):  -= L[i, ka:kb] L[j, ka:kb]^T              (one launch)
//   PANELS  block columns [c0, c1) factored panel by panel over the block rows < r1: column j receives the k-blocks [c0, j),
//           then its diagonal block is factored and inverted and the rows (j, r1) are solved (r1 = nbk: the chain of
//           dgp_chol.hip::potrf; r1 = c1: only the group's diagonal block D)
//   SOLVE   block rows [c1, nbk) of the columns [c0, c1):  L[i, group] = A[i, group] T_D^T  (trsm_group_kernel, behind PANELS
//           with r1 = c1; not bitwise the panel chain: another association of the same sums)
//   SYNC    stream `stream` records an event, stream c0 waits for it
// on one of two streams (0 = the caller's, 1 = the plan's bulk stream), listed in issue order.
#pragma once
#include <string>
#include <vector>

namespace dgp {
namespace sched {

enum Kind { UPDATE = 0, PANELS = 1, SOLVE = 2, SYNC = 3 };
struct Op {
  int kind, stream;
  int c0, c1;  // block columns [c0, c1)   (SYNC: c0 = the waiting stream)
  int r0, r1;  // block rows [max(r0, column), r1)
  int ka, kb;  // k-blocks [ka, kb)   (UPDATE)
};
// the cut points of the left-looking family (Tuning: potrf_sweep, potrf_tail, potrf_tail_sweep, potrf_solve, potrf_overlap)
struct Cut {
  int sweep = 0;       // panels per SUPER-GROUP (a multiple of G; 0 = the whole matrix): a right-looking UPDATE of the whole trailing
                       // triangle between super-groups, left-looking inside one.  sweep = G is today's flow of data on one stream
  int tail = 0;        // the last `tail` block columns (rounded to whole groups; 0 = none) are a super-group of their own: their
                       // strips are the launches with fewer tiles than the GPU has slots and the longest K
  int tail_sweep = 0;  // panels per super-group inside the tail (0 = the whole tail)
  int solve = 0;       // full groups with rows below them: PANELS on the diagonal block + SOLVE instead of PANELS over the full height
  int overlap = 0;     // with solve: the group's UPDATE below its diagonal block runs on stream 1 beside PANELS
};
// is a right-looking sweep of the trailing triangle issued once the columns < c (a group boundary) are final?
inline bool sweep_point(int nbk, int G, int c, const Cut& cut) {
  if (c <= 0 || c >= nbk) return false;
  const int S = cut.sweep > 0 ? (cut.sweep + G - 1) / G * G : 0, St = cut.tail_sweep > 0 ? (cut.tail_sweep + G - 1) / G * G : 0;
  const int t0 = cut.tail > 0 ? (nbk - cut.tail) / G * G : 0;  // first block column of the tail
  if (t0 > 0 && c >= t0) return c == t0 || (St > 0 && (c - t0) % St == 0);
  return S > 0 && c % S == 0;
}

inline bool solves(int nbk, int G, int k0, const Cut& cut) {
  const int c1 = k0 + G < nbk ? k0 + G : nbk;
  return cut.solve && c1 - k0 == G && c1 < nbk && G >= 4 && (G & (G - 1)) == 0;
}

// today's group-ahead schedule (dgp_chol.hip::potrf): chain on stream 0, bulk launches of K = 128 G on stream 1
inline std::vector<Op> today(int nbk, int G) {
  std::vector<Op> ops;
  const int Q = (nbk + G - 1) / G;
  for (int q = 0; q < Q; ++q) {
    const int k0 = G * q, c1 = k0 + G < nbk ? k0 + G : nbk;
    if (q >= 2) ops.push_back({SYNC, 1, 0, 0, 0, 0, 0, 0});
    if (q >= 1) ops.push_back({UPDATE, 0, k0, c1, k0, nbk, k0 - G, k0});
    if (q >= 1 && k0 + G < nbk) {
      ops.push_back({SYNC, 0, 1, 0, 0, 0, 0, 0});
      ops.push_back({UPDATE, 1, k0 + G, nbk, k0 + G, nbk, k0 - G, k0});
    }
    ops.push_back({PANELS, 0, k0, c1, k0, nbk, 0, 0});
  }
  return ops;
}

// the left-looking family: each group is updated ONCE, just before it is factored, with everything to its left inside its
// super-group (K = 128 (k0 - base)); between super-groups one right-looking sweep of the trailing triangle with the whole
// super-group (K = 128 sweep)
inline std::vector<Op> left_looking(int nbk, int G, const Cut& cut) {
  std::vector<Op> ops;
  bool forked = false;
  int base = 0;  // k-blocks that every column right of the factored ones has received from the sweeps
  for (int k0 = 0; k0 < nbk; k0 += G) {
    const int c1 = k0 + G < nbk ? k0 + G : nbk;
    const bool solve = solves(nbk, G, k0, cut);
    bool split = false;
    if (k0 > base) {
      if (solve && cut.overlap) {
        split = true;
        ops.push_back({UPDATE, 0, k0, c1, k0, c1, base, k0});  // the diagonal block's tiles first
        ops.push_back({SYNC, 0, 1, 0, 0, 0, 0, 0});
        ops.push_back({UPDATE, 1, k0, c1, c1, nbk, base, k0});
        forked = true;
      } else {
        ops.push_back({UPDATE, 0, k0, c1, k0, nbk, base, k0});
      }
    }
    ops.push_back({PANELS, 0, k0, c1, k0, solve ? c1 : nbk, 0, 0});
    if (solve) {
      if (split) {
        ops.push_back({SYNC, 1, 0, 0, 0, 0, 0, 0});
        forked = false;
      }
      ops.push_back({SOLVE, 0, k0, c1, c1, nbk, 0, 0});
    }
    if (sweep_point(nbk, G, c1, cut)) {
      ops.push_back({UPDATE, 0, c1, nbk, c1, nbk, base, c1});
      base = c1;
    }
  }
  if (forked) ops.push_back({SYNC, 1, 0, 0, 0, 0, 0, 0});
  return ops;
}

// tiles of an UPDATE (per site) and its executed work in 128^3 tile products
inline long update_tiles(const Op& o) {
  long t = 0;
  for (int j = o.c0; j < o.c1; ++j) {
    const int lo = o.r0 > j ? o.r0 : j;
    if (o.r1 > lo) t += o.r1 - lo;
  }
  return t;
}

// -> "" if every tile (i, j) receives the k-blocks 0 .. j - 1 in ascending gap-free order exactly once before its column is
// factored, nothing reads a block that is not final, nothing writes a final block, every access across the two streams is
// ordered by a SYNC, and the caller's stream has joined the other at the end; else the first violation
inline std::string check(const std::vector<Op>& ops, int nbk) {
  auto at = [nbk](int i, int j) { return (size_t)i * nbk + j; };
  std::vector<int> applied((size_t)nbk * nbk, 0), wstream((size_t)nbk * nbk, -1), wclock((size_t)nbk * nbk, 0);
  std::vector<char> fin((size_t)nbk * nbk, 0);
  int clock[2] = {0, 0}, seen[2][2] = {{0, 0}, {0, 0}};
  auto where = [](size_t n, const Op& o) {
    return "op " + std::to_string(n) + " (kind " + std::to_string(o.kind) + ", columns " + std::to_string(o.c0) + ".." + std::to_string(o.c1) +
           ", rows " + std::to_string(o.r0) + ".." + std::to_string(o.r1) + ", k " + std::to_string(o.ka) + ".." + std::to_string(o.kb) + "): ";
  };
  for (size_t n = 0; n < ops.size(); ++n) {
    const Op& o = ops[n];
    if (o.stream < 0 || o.stream > 1) return where(n, o) + "bad stream";
    const int X = o.stream;
    auto visible = [&](int i, int j) { return wstream[at(i, j)] < 0 || wstream[at(i, j)] == X || seen[X][wstream[at(i, j)]] >= wclock[at(i, j)]; };
    // block (i, k) of L is read: final, and its writer ordered before this op
    auto readable = [&](int i, int k) { return fin[at(i, k)] && visible(i, k); };
    if (o.kind == SYNC) {
      if (o.c0 < 0 || o.c0 > 1 || o.c0 == X) return where(n, o) + "bad SYNC";
      seen[o.c0][X] = clock[X];
      continue;
    }
    if (o.c0 < 0 || o.c1 > nbk || o.c0 >= o.c1 || o.r0 < o.c0 || o.r1 > nbk) return where(n, o) + "out of range";
    const int now = ++clock[X];
    auto write = [&](int i, int j) {
      wstream[at(i, j)] = X;
      wclock[at(i, j)] = now;
    };
    if (o.kind == UPDATE) {
      if (o.ka < 0 || o.ka >= o.kb || o.kb > o.c0) return where(n, o) + "k-range must lie left of the columns";
      if (update_tiles(o) == 0) return where(n, o) + "empty";
      for (int j = o.c0; j < o.c1; ++j)
        for (int i = (o.r0 > j ? o.r0 : j); i < o.r1; ++i) {
          if (fin[at(i, j)]) return where(n, o) + "writes a final block";
          if (applied[at(i, j)] != o.ka)
            return where(n, o) + "tile (" + std::to_string(i) + ", " + std::to_string(j) + ") has received " + std::to_string(applied[at(i, j)]) + " k-blocks";
          if (!visible(i, j)) return where(n, o) + "tile written on the other stream without a SYNC";
          for (int k = o.ka; k < o.kb; ++k)
            if (!readable(i, k) || !readable(j, k)) return where(n, o) + "reads block column " + std::to_string(k) + " before it is final";
          applied[at(i, j)] = o.kb;
        }
      for (int j = o.c0; j < o.c1; ++j)
        for (int i = (o.r0 > j ? o.r0 : j); i < o.r1; ++i) write(i, j);
    } else if (o.kind == PANELS) {
      if (o.r0 != o.c0 || o.r1 < o.c1) return where(n, o) + "PANELS covers its diagonal block";
      for (int j = o.c0; j < o.c1; ++j)
        for (int i = j; i < o.r1; ++i) {
          if (fin[at(i, j)]) return where(n, o) + "factored twice";
          if (applied[at(i, j)] != o.c0)
            return where(n, o) + "tile (" + std::to_string(i) + ", " + std::to_string(j) + ") has received " + std::to_string(applied[at(i, j)]) + " of " + std::to_string(o.c0) + " k-blocks";
          if (!visible(i, j)) return where(n, o) + "tile written on the other stream without a SYNC";
        }
      for (int j = o.c0; j < o.c1; ++j)
        for (int i = j; i < o.r1; ++i) {
          applied[at(i, j)] = j;
          fin[at(i, j)] = 1;
          write(i, j);
        }
    } else if (o.kind == SOLVE) {
      if (o.r0 != o.c1 || o.r1 != nbk || o.r0 >= o.r1) return where(n, o) + "SOLVE covers the rows below the group's diagonal block";
      for (int j = o.c0; j < o.c1; ++j)
        for (int i = j; i < o.c1; ++i)
          if (!readable(i, j)) return where(n, o) + "the diagonal block is not final";
      for (int j = o.c0; j < o.c1; ++j)
        for (int i = o.r0; i < o.r1; ++i) {
          if (fin[at(i, j)]) return where(n, o) + "solved twice";
          if (applied[at(i, j)] != o.c0)
            return where(n, o) + "tile (" + std::to_string(i) + ", " + std::to_string(j) + ") has received " + std::to_string(applied[at(i, j)]) + " of " + std::to_string(o.c0) + " k-blocks";
          if (!visible(i, j)) return where(n, o) + "tile written on the other stream without a SYNC";
        }
      for (int j = o.c0; j < o.c1; ++j)
        for (int i = o.r0; i < o.r1; ++i) {
          applied[at(i, j)] = j;
          fin[at(i, j)] = 1;
          write(i, j);
        }
    } else {
      return where(n, o) + "unknown kind";
    }
  }
  for (int j = 0; j < nbk; ++j)
    for (int i = j; i < nbk; ++i)
      if (!fin[at(i, j)]) return "block (" + std::to_string(i) + ", " + std::to_string(j) + ") is never factored";
  if (seen[0][1] < clock[1]) return "stream 0 has not joined stream 1 at the end";
  return "";
}

}  // namespace sched
}  // namespace dgp
