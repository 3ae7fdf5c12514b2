// mcts_improve.hip -- the completed-Q improved policy of every slot's root, read out of the tree pool in ONE launch (include/aqgnn.h,
// "completed-Q policy targets"; Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022, section 4 and appendix D):
//     pi' = softmax(log p + sigma(completedQ)),   sigma(c) = (c_visit + max n) * c_scale * ((c + 1) / 2)
// over the root's children, where an unvisited child's value is completed by vmix, the prior-weighted mix of the root's own network
// value vhat = root.w + sum w_i and the visited children's q.  Nothing of the search is touched: the step kernels, the captured
// per-move graph and the engine struct are what they were.
//
// The geometry is engine_root_visits_kernel's: one wavefront per slot, four per workgroup; a lane owns children lane, lane + 64 and
// lane + 128, and both 16-byte halves of all three records are in flight before the first reduction.  Everything between the loads
// and the stores is float64 without contraction, in the order aqgnn.h writes it; the sums, the maxima and sum e are wave reductions by
// xor-shuffles (every lane ends with the same bits).  No LDS, no atomics, no workgroup barrier; every loop is bounded by MAX_LEGAL.
// The child range is compared with node_cap before it is used as an address; a range that fails, like a count above MAX_LEGAL, gives
// the zero row (count 0, actions 0xFF, vmix 0).
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include <cmath>

#ifdef __FAST_MATH__
#error "mcts_improve.hip: the completed-Q arithmetic is float64 as written (no fast-math)"
#endif
// every expression is evaluated as aqgnn.h states it (engine.improved_policy_reference is the same in numpy)
#pragma clang fp contract(off)
#include "mcts_tree.hpp"

namespace aqg {

constexpr int IMP_ROUNDS = (MAX_LEGAL + WAVE - 1) / WAVE;      // 3 lane rounds cover a legal list

__device__ __forceinline__ long long improve_wave_sum_ll(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int improve_wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double improve_wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double improve_wave_max_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(256) void engine_root_improved_policy_kernel(aqg_engine e, double c_visit, double c_scale,
                                                                          float* __restrict__ policy, uint8_t* __restrict__ actions,
                                                                          int32_t* __restrict__ count, float* __restrict__ vmix_out) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games) return;                               // wave-uniform
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
    const long long nsum = improve_wave_sum_ll(nsum_part);
    const int nmax = improve_wave_max_i(nmax_part);
    const double vhat = __hiloint2double((int)root_cold.y, (int)root_cold.x) + improve_wave_sum_d(wsum_part);
    const double pv = improve_wave_sum_d(pv_part), qv = improve_wave_sum_d(qv_part);
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
    const double m = improve_wave_max_d(m_part);
    const bool any = m > -INFINITY;                             // a prior above 0 exists (wave-uniform)
    double ex[IMP_ROUNDS];
    double s_part = 0.0;
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        ex[r] = (any && x[r] > -INFINITY) ? exp(x[r] - m) : 0.0;
        s_part += ex[r];
    }
    const double s = improve_wave_sum_d(s_part);
    // ---- the row in the layout of engine_root_visits_kernel: 0 and 0xFF past the count
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        const int i = r * WAVE + lane;
        if (i < MAX_LEGAL) {
            policy[(size_t)g * MAX_LEGAL + i] = (any && x[r] > -INFINITY) ? (float)(ex[r] / s) : 0.f;
            actions[(size_t)g * MAX_LEGAL + i] = (uint8_t)act[r];
        }
    }
    if (lane == 0) {
        count[g] = cnt;
        vmix_out[g] = (float)vmix;
    }
}

void launch_engine_root_improved_policy(const aqg_engine& e, double c_visit, double c_scale, float* policy, uint8_t* actions,
                                        int32_t* count, float* vmix, hipStream_t st) {
    hipLaunchKernelGGL(engine_root_improved_policy_kernel, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, c_visit, c_scale, policy,
                       actions, count, vmix);
}

}  // namespace aqg
