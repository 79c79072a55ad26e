// potrf_schedule_check.cpp -- host-only check of the batched factorisation's schedules (csrc/dgp_schedule.h): every
// generated schedule must pass the checker, hand-made violations must not.  No GPU, no HIP.
//   g++ -std=c++17 -I discontinuum_amd/csrc examples/potrf_schedule_check.cpp -o potrf_schedule_check && ./potrf_schedule_check
// prints one line per failure and "ok <schedules checked> <violations rejected>"; exit status 0 only if everything held.
#include <cstdio>
#include <cstdlib>
#include "dgp_schedule.h"

using namespace dgp::sched;

static int failures = 0;
static long accepted = 0, rejected = 0;

static void expect_ok(const char* what, const std::vector<Op>& ops, int nbk, int G) {
  const std::string why = check(ops, nbk);
  if (!why.empty()) {
    std::printf("FAIL %s nbk=%d G=%d: %s\n", what, nbk, G, why.c_str());
    ++failures;
  } else {
    ++accepted;
  }
}
static void expect_bad(const char* what, const std::vector<Op>& ops, int nbk, int G) {
  if (check(ops, nbk).empty()) {
    std::printf("FAIL %s nbk=%d G=%d: a violation was accepted\n", what, nbk, G);
    ++failures;
  } else {
    ++rejected;
  }
}
// executed work in 128^3 tile products: the same for every valid schedule of one (nbk, G) with the panel chain
static long work(const std::vector<Op>& ops) {
  long w = 0;
  for (const Op& o : ops)
    if (o.kind == UPDATE) w += update_tiles(o) * (o.kb - o.ka);
  return w;
}

int main(int argc, char** argv) {
  const int lo = argc > 1 ? std::atoi(argv[1]) : 4, hi = argc > 2 ? std::atoi(argv[2]) : 80;
  const int Gs[3] = {2, 4, 8};
  for (int nbk = lo; nbk <= hi; ++nbk)
    for (int G : Gs) {
      const std::vector<Op> t = today(nbk, G);
      expect_ok("today", t, nbk, G);
      Cut pure;  // pure left-looking, the panel chain over the full height: bitwise today's factor
      const std::vector<Op> ll = left_looking(nbk, G, pure);
      expect_ok("left-looking", ll, nbk, G);
      if (work(ll) != work(t)) {
        std::printf("FAIL nbk=%d G=%d: left-looking executes %ld tile products, today's %ld\n", nbk, G, work(ll), work(t));
        ++failures;
      }
      expect_ok("shipped default", left_looking(nbk, G, Cut()), nbk, G);
      for (int sweep : {0, G, 2 * G, 16})
        for (int tail : {0, 8, 16})
          for (int tail_sweep : {0, 8})
            for (int solve = 0; solve <= 1; ++solve)
              for (int overlap = 0; overlap <= solve; ++overlap) {
                Cut c;
                c.sweep = sweep, c.tail = tail, c.tail_sweep = tail_sweep, c.solve = solve, c.overlap = overlap;
                expect_ok("hybrid", left_looking(nbk, G, c), nbk, G);
              }
      // ---- hand-made violations of the pure left-looking schedule
      if (nbk <= 2 * G) continue;  // (needs at least two UPDATEs)
      int u2 = -1, nupd = 0;       // the second UPDATE: k-range [0, 2 G)
      for (size_t i = 0; i < ll.size(); ++i)
        if (ll[i].kind == UPDATE && ++nupd == 2) u2 = (int)i;
      {
        std::vector<Op> v = ll;  // a skipped k-block
        v[u2].ka = 1;
        expect_bad("skipped k-block", v, nbk, G);
      }
      {
        std::vector<Op> v = ll;  // descending order: the k-blocks [G, 2 G) first, then [0, G)
        Op first = v[u2], second = v[u2];
        first.ka = G, second.kb = G;
        v[u2] = first;
        v.insert(v.begin() + u2 + 1, second);
        expect_bad("descending order", v, nbk, G);
      }
      {
        std::vector<Op> v = ll;  // a column factored early: the group's PANELS before its UPDATE
        std::swap(v[u2], v[u2 + 1]);
        expect_bad("column factored early", v, nbk, G);
      }
      {
        std::vector<Op> v = ll;  // a k-block applied twice
        v.insert(v.begin() + u2, v[u2]);
        expect_bad("k-block applied twice", v, nbk, G);
      }
      {
        std::vector<Op> v = ll;  // a column read before it is final: the UPDATE reaches into its own group
        v[u2].kb += 1;
        expect_bad("reads a column that is not final", v, nbk, G);
      }
      {
        std::vector<Op> v = ll;  // a group never factored
        v.pop_back();
        expect_bad("last group missing", v, nbk, G);
      }
      {
        std::vector<Op> v = t;  // today's schedule without its cross-stream waits
        std::vector<Op> w;
        for (const Op& o : v)
          if (o.kind != SYNC) w.push_back(o);
        if (w.size() != v.size()) expect_bad("missing SYNC", w, nbk, G);
      }
      if (G >= 4 && nbk > 3 * G) {
        Cut c;
        c.solve = 1, c.overlap = 1;
        std::vector<Op> v = left_looking(nbk, G, c), w;  // the overlapped form without the join before SOLVE
        for (const Op& o : v)
          if (!(o.kind == SYNC && o.stream == 1)) w.push_back(o);
        expect_bad("SOLVE without its join", w, nbk, G);
      }
    }
  std::printf("ok %ld %ld\n", accepted, rejected);
  return failures ? 1 : 0;
}
