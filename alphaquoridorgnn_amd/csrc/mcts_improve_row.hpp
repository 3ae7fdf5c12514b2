// mcts_improve_row.hpp -- the completed-Q improved policy of ONE root in the lanes of its wavefront (include/aqgnn.h, "completed-Q
// policy targets"): everything from the loads of the root's child block to e_i / sum e, written once.  Two units call it:
// mcts_improve.hip (the read-out, rows in legal order) and mcts_record.hip (self-play's record launch, rows dense by action id), so a
// recorded row is the read-out's row bit for bit.  Float64 without contraction, in the order aqgnn.h writes it; the sums and maxima
// are wave reductions by xor-shuffles (every lane ends with the same bits).  No LDS, no atomics; every loop is bounded by MAX_LEGAL.
// The child range is compared with node_cap before it is used as an address.
#pragma once
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include <cmath>

#ifdef __FAST_MATH__
#error "mcts_improve_row.hpp: the completed-Q arithmetic is float64 as written (no fast-math)"
#endif
// every expression is evaluated as aqgnn.h states it (engine.improved_policy_reference is the same in numpy): this holds for the
// rest of the including unit, too
#pragma clang fp contract(off)
#include "mcts_tree.hpp"

namespace aqg {

constexpr int IMP_ROUNDS = (MAX_LEGAL + WAVE - 1) / WAVE;      // 3 lane rounds cover a legal list

// one root's improved policy in the lanes of its wavefront: entry r of a lane is child r * 64 + lane of the root's block
struct ImprovedRow {
    float pi[IMP_ROUNDS];           // pi' of the child, 0 past the count
    uint32_t act[IMP_ROUNDS];       // its action byte, 0xFF past the count
    int cnt;                        // the guarded count (wave-uniform)
    double vmix;                    // the mixed value (wave-uniform; 0 behind a failed guard)
};

// Everything from the loads of slot g's root block to ex / s, once, for the read-out and the record launch.  Called by whole
// wavefronts (the reductions are xor-shuffles over all 64 lanes).
__device__ __forceinline__ ImprovedRow improved_policy_row(const aqg_engine& e, int g, int lane, double c_visit, double c_scale) {
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint4* __restrict__ halves = reinterpret_cast<const uint4*>(nodes);      // record k = halves[2 k] (cold), halves[2 k + 1] (hot)
    const uint4 root_cold = halves[0], root_hot = halves[1];
    const uint32_t kids = root_hot.y;
    const int stored = (int)(kids >> 24), first = (int)(kids & 0xFFFFFF);
    // the guard: a count above MAX_LEGAL or a range that leaves the pool is never used as an address
    const bool inside = stored <= MAX_LEGAL && (long long)first + stored <= (long long)e.node_cap;
    const int cnt = inside ? stored : 0;
    // ---- both halves of the lane's three records, none waiting for another
    uint4 cold[IMP_ROUNDS], hot[IMP_ROUNDS];
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        const int i = r * WAVE + lane;
        const bool in = i < cnt;
        const size_t k = (size_t)(in ? first + i : 0);
        cold[r] = halves[2 * k];
        hot[r] = halves[2 * k + 1];
    }
    double w[IMP_ROUNDS];
    float p[IMP_ROUNDS], q[IMP_ROUNDS];
    int n[IMP_ROUNDS];
    uint32_t act[IMP_ROUNDS];
    long long nsum_part = 0;
    int nmax_part = 0;
    double wsum_part = 0.0, pv_part = 0.0, qv_part = 0.0;
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        const bool in = r * WAVE + lane < cnt;
        w[r] = in ? __hiloint2double((int)cold[r].y, (int)cold[r].x) : 0.0;
        p[r] = in ? __uint_as_float(cold[r].z) : 0.f;
        act[r] = in ? (cold[r].w & 0xFFu) : 0xFFu;
        n[r] = in ? (int)hot[r].x : 0;
        q[r] = in ? __uint_as_float(hot[r].z) : 0.f;
        nsum_part += n[r];
        nmax_part = max(nmax_part, n[r]);
        wsum_part += w[r];
        if (n[r] > 0) {
            pv_part += (double)p[r];
            qv_part += (double)p[r] * (double)q[r];
        }
    }
    // ---- 1 .. 3: the visit totals, the root's network value, the mixed value (wave-uniform)
    const long long nsum = wave_xor_sum(nsum_part);
    const int nmax = wave_xor_max(nmax_part);
    const double vhat = __hiloint2double((int)root_cold.y, (int)root_cold.x) + wave_xor_sum(wsum_part);
    const double pv = wave_xor_sum(pv_part), qv = wave_xor_sum(qv_part);
    const double vmix = inside ? (pv > 0.0 ? (vhat + (double)nsum * (qv / pv)) / (1.0 + (double)nsum) : vhat) : 0.0;
    // ---- 4 .. 6: completed value, transform, softmax
    const double scale = (c_visit + (double)nmax) * c_scale;
    double x[IMP_ROUNDS];
    double m_part = -INFINITY;
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        const bool in = r * WAVE + lane < cnt && p[r] > 0.f;    // p <= 0 or NaN: excluded
        const double c = n[r] > 0 ? (double)q[r] : vmix;
        const double sigma = scale * ((c + 1.0) / 2.0);
        x[r] = in ? log((double)p[r]) + sigma : -INFINITY;
        m_part = fmax(m_part, x[r]);
    }
    const double m = wave_xor_max(m_part);
    const bool any = m > -INFINITY;                             // a prior above 0 exists (wave-uniform)
    double ex[IMP_ROUNDS];
    double s_part = 0.0;
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        ex[r] = (any && x[r] > -INFINITY) ? exp(x[r] - m) : 0.0;
        s_part += ex[r];
    }
    const double s = wave_xor_sum(s_part);
    ImprovedRow row;
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        row.pi[r] = (any && x[r] > -INFINITY) ? (float)(ex[r] / s) : 0.f;
        row.act[r] = act[r];
    }
    row.cnt = cnt;
    row.vmix = vmix;
    return row;
}

}  // namespace aqg
