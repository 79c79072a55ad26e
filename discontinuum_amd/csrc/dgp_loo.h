// dgp_loo.h -- what dgp_loo.hip shares with dgp_lgo.hip: the work area's layout and the launchers of the passes that both
// objectives run (the mirror pass, and everything from the symmetric sandwich to the result row).
#pragma once
#include "dgp_plan.h"

namespace dgp {

#define LOO_PART 8  // doubles per workgroup of the block partials: [0] sum of the summands, [1] first bad row + 1 (0: none);
                    // [2..5] sum b, sum b w0, sum b w1, sum dnoise

// The work area holds one SLICE per site that mirrors the plan's site (same size, same offsets: F where the plan has A, G where it
// has T, 2 M where it has S, a zero vector where it has alpha, the contraction's partials where it has its own -- gram_grad
// addresses all of them at ONE site stride), then the sites' vectors, then the step's own result rows.  value_only: no slices.
struct LooLayout {
  size_t slice, F, G, M, zero, gpart;          // a site's slice and the byte offsets inside it
  size_t w, c, b, negb, spart, part, vec;      // byte offsets inside a site's vectors, and their size
  size_t vecs, out0, total;                    // byte offsets of the vectors and of the scratch result rows [B][DGP_OUT_LEN]
  int nblk;                                    // workgroups per site of the row passes
};
LooLayout loo_layout(const dgp_plan* p, bool value_only);

// F = S made full and G = F diag(w2) into the slices (w2 at the vectors' site stride)
int loo_mirror(const double* S, long N, const double* w2, char* work, const LooLayout& L, hipStream_t s, const Batch& bt);
// 2 M = F G^T, b = S c (c in the vectors), the contraction, dr / dnoise and the result row `out` from the block partials
// [0] / [1] that the caller's terms pass left in the vectors' `part`
int loo_tail(int model, int d, const double* Xt, const double* S, const double* alpha, long N, int n, const double* theta,
             const double* wts, char* work, const LooLayout& L, double* out, double* dr, double* dnoise, hipStream_t s, const Batch& bt,
             void* pre_scratch);
// the value-only finish: out2 = [value, info] per site from the block partials [0] / [1]
int loo_finish_value(const int* info, char* work, const LooLayout& L, double* out2, hipStream_t s, const Batch& bt);

}  // namespace dgp
