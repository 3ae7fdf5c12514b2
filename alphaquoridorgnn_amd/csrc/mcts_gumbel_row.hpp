// mcts_gumbel_row.hpp -- the arithmetic of the Gumbel root search (include/aqgnn.h, "Gumbel root search") that more than one unit
// evaluates, written once: the root score of rule 3 (mcts_step.hip's GUMBEL level 0; mcts_gumbel.hip's finish launch and read-out)
// and the winner of rule 4.  Float32, left to right, no contraction -- gumbel.root_score_reference is the same in numpy.
// __forceinline__ device code only.
#pragma once
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include <cmath>

#ifdef __FAST_MATH__
#error "mcts_gumbel_row.hpp: the root score is float32 as written (no fast-math)"
#endif
// (holds for the rest of the including unit, too)
#pragma clang fp contract(off)
#include "mcts_tree.hpp"

namespace aqg {

// S_i of rule 3: gl + sigma(q) for a visited child, gl for an unvisited one; -inf where the child's visit count is not the
// considered one or the child is not among the sampled (gl = -inf)
__device__ __forceinline__ float gumbel_root_score(float gl, int n, float q, float nmaxf, float c_visit, float c_scale, int v) {
    const float sigma = n > 0 ? ((c_visit + nmaxf) * c_scale) * ((q + 1.0f) * 0.5f) : 0.0f;
    const float s = gl + sigma;
    return (n == v && gl > -INFINITY) ? s : -INFINITY;
}

// Rule 4 over the child block [first, first + cnt) of one root, by one lane: v* = max n over the children with gl > -inf, then the
// first arg-max of S with v = v*; child 0 if nothing exceeds -inf (cnt >= 1; the caller has held the range against the pool)
__device__ __forceinline__ int gumbel_winner(const NodeRec* __restrict__ nodes, int first, int cnt, float c_visit, float c_scale) {
    int nmax = 0, vstar = -1;
    for (int i = 0; i < cnt; ++i) {
        const int n = nodes[first + i].n;
        nmax = max(nmax, n);
        if (nodes[first + i].cp > -INFINITY) vstar = max(vstar, n);
    }
    const float nmaxf = (float)nmax;
    float best = -INFINITY;
    int idx = 0;
    for (int i = 0; i < cnt; ++i) {
        const NodeRec& c = nodes[first + i];
        const float s = gumbel_root_score(c.cp, c.n, c.q, nmaxf, c_visit, c_scale, vstar);
        if (s > best) { best = s; idx = i; }
    }
    return idx;
}

}  // namespace aqg
