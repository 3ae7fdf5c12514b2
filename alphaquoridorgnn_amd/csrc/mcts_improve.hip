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
//
// The arithmetic is written once, in mcts_improve_row.hpp (improved_policy_row): this unit's read-out returns the rows in legal order,
// and the record launch of self-play (mcts_record.hip) writes the same rows dense by action id into the engine's f32 history.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include <cmath>

#ifdef __FAST_MATH__
#error "mcts_improve.hip: the completed-Q arithmetic is float64 as written (no fast-math)"
#endif
// every expression is evaluated as aqgnn.h states it (engine.improved_policy_reference is the same in numpy)
#pragma clang fp contract(off)
#include "mcts_improve_row.hpp"

namespace aqg {

__global__ __launch_bounds__(256) void engine_root_improved_policy_kernel(aqg_engine e, double c_visit, double c_scale,
                                                                          float* __restrict__ policy, uint8_t* __restrict__ actions,
                                                                          int32_t* __restrict__ count, float* __restrict__ vmix_out) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games) return;                               // wave-uniform
    const ImprovedRow row = improved_policy_row(e, g, lane, c_visit, c_scale);
    // ---- the row in the layout of engine_root_visits_kernel: 0 and 0xFF past the count
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r) {
        const int i = r * WAVE + lane;
        if (i < MAX_LEGAL) {
            policy[(size_t)g * MAX_LEGAL + i] = row.pi[r];
            actions[(size_t)g * MAX_LEGAL + i] = (uint8_t)row.act[r];
        }
    }
    if (lane == 0) {
        count[g] = row.cnt;
        vmix_out[g] = (float)row.vmix;
    }
}

void launch_engine_root_improved_policy(const aqg_engine& e, double c_visit, double c_scale, float* policy, uint8_t* actions,
                                        int32_t* count, float* vmix, hipStream_t st) {
    hipLaunchKernelGGL(engine_root_improved_policy_kernel, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, c_visit, c_scale, policy,
                       actions, count, vmix);
}

}  // namespace aqg
