// mcts_eval.hip -- the evaluation launch of the default self-play chain (map: mcts.hip): engine_eval_kernel, one launch with two kinds of
// workgroup -- in front the legal-move searches of the leaves the step in front has just selected (leaf_legal_role), behind them the
// network trunk's board workgroups over the same leaves (trunk_boards_body, gcn_trunk_body.hpp) -- and launch_engine_eval.
// The step kernel's last phase used to be that search, and nothing in the step launch read its result: the NEXT step's round 1 does,
// and the trunk launch in between needs the leaf's state and flag only.  Here it runs beside the trunk instead of in front of it: the
// step launch ends on the leaf (game_step_fast<.., DEFER>, mcts_step.hip), the graph stays one chain of two launches per simulation.
#define AQG_TRACE_TU eval
#include "aqg_common.hpp"
#include "legal_wave.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "gcn_trunk_body.hpp"
#include "mcts_tree.hpp"

namespace aqg {

int g_legal_beside_trunk = 1;     // option "legal_beside_trunk": 1 = the cache-less step launches with the heads inside leave their leaves' legal-move
                                  // searches to the evaluation launch behind them (engine_eval_kernel), 0 = the step searches, the plain trunk follows

// what the legal-move workgroups read and write of the engine (the trunk's arguments travel beside it)
struct LeafLegalArgs {
    const uint8_t* leaf_flag; const uint8_t* leaf_state;
    uint8_t* legal_order; int32_t* legal_count;
    int32_t* searched;            // counters[6]: leaves searched here
    const int32_t* node_count; PolicyJob* jobs;      // option "policy_beside_step" (jobs == nullptr: off): see leaf_legal_role
    int32_t num_games, prio;
};

// The legal-move search of one deferred leaf, one wave per game, eight games per workgroup (workgroup `blk` of the launch's legal range):
// game g with leaf_flag[g] == 1 and the step's marker legal_count[g] == -1 gets legal_order[g][..] and legal_count[g] exactly as the
// step would have written them -- the same wave_legal_prepare + wave_legal_finish on the same state.  A game whose step searched itself
// (no marker), an idle game and a wave beyond num_games do nothing.
// Option "policy_beside_step": the step launch behind this one expands a marked leaf in a workgroup of its own, beside the game's step
// workgroup -- which overwrites leaf_flag, legal_count and node_count while that workgroup may still be starting.  So the search leaves
// what the expansion needs of the three in the game's job record: {node_count[g], total} for a marked leaf -- node_count does not change
// during an evaluation launch -- and {0, 0} for every other game of the set, whatever an earlier launch left there.
// One workgroup barrier, at the start and for the counter only: wave 0 counts the workgroup's marked games for counters[6] (one atomic
// per workgroup instead of one per game on one address), and behind the barrier no wave has overwritten a marker yet.
template <int N>
__device__ __forceinline__ void leaf_legal_role(const LeafLegalArgs& a, int blk, int wave, int lane) {
    if (a.prio == 1) __builtin_amdgcn_s_setprio(1); else if (a.prio == 2) __builtin_amdgcn_s_setprio(2); else if (a.prio == 3) __builtin_amdgcn_s_setprio(3);
    const int g = blk * NWV + wave, gc = min(g, a.num_games - 1);              // (a wave without a game loads the last game's: no branch)
    const int flag = a.leaf_flag[gc], cnt = a.legal_count[gc];
    const int first_new = a.jobs ? a.node_count[gc] : 0;
    const uint64_t* lq = reinterpret_cast<const uint64_t*>(a.leaf_state) + (size_t)gc * 3;
    const uint64_t q0 = lq[0], q1 = lq[1], q2 = lq[2];
    int marked = 0;
    if (wave == 0) {
        const int gi = min(blk * NWV + (lane & (NWV - 1)), a.num_games - 1);
        const bool m = lane < NWV && blk * NWV + lane < a.num_games && a.leaf_flag[gi] == 1 && a.legal_count[gi] == -1;
        marked = __popcll(__ballot(m));
    }
    const bool mine = g < a.num_games && __builtin_amdgcn_readfirstlane(flag) == 1 && __builtin_amdgcn_readfirstlane(cnt) == -1;
    __syncthreads();
    if (wave == 0 && lane == 0 && marked) atomicAdd(a.searched, marked);
    if (!mine) {
        if (a.jobs && g < a.num_games && lane == 0) a.jobs[g] = PolicyJob{0, 0};
        return;
    }
    QState v;
    v.hw = q0; v.vw = q1;
    v.ppos = (uint8_t)(q2 & 0xff); v.pwl = (uint8_t)((q2 >> 8) & 0xff); v.epos = (uint8_t)((q2 >> 16) & 0xff); v.ewl = (uint8_t)((q2 >> 24) & 0xff);
    v.plies = (uint16_t)((q2 >> 32) & 0xffff); v.pad = 0;
    const QState s = uniform_state(v);
    const LegalPrep prep = wave_legal_prepare<N>(s, lane);
    const int total = wave_legal_finish<N>(s, prep, lane, nullptr, a.legal_order + (size_t)g * MAX_LEGAL);
    if (lane == 0) {
        a.legal_count[g] = total;
        if (a.jobs) a.jobs[g] = PolicyJob{first_new, total};
    }
}

// Workgroups [0, legal_blocks) search, workgroups [legal_blocks, gridDim.x) are the trunk's: the searches come first so that they
// start at once -- the longest of them lasts about as long as the whole trunk launch while walls are in hand.  Trunk-sized
// workgroups and the trunk's launch bound: the register budget is the trunk's (build.sh polices it), and a search workgroup takes one
// trunk slot of its CU for as long as its slowest game, the slot-time the step workgroup spent on it before.
template <int TRACK>
__global__ __launch_bounds__(64 * NWV, 4) void engine_eval_kernel(LeafLegalArgs la, unsigned int legal_blocks, const void* __restrict__ states, int fmt,
                                                                  int B, const float* __restrict__ pk, float* __restrict__ pooled,
                                                                  const uint8_t* __restrict__ active, int phase_delay, int32_t* __restrict__ saturated) {
    AQG_TRACE_BEGIN
    __shared__ TrunkSmemM sm;
    if (blockIdx.x < legal_blocks)
        leaf_legal_role<9>(la, (int)blockIdx.x, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), threadIdx.x & 63);
    else
        trunk_boards_body<TRACK, false, true>(sm, blockIdx.x - legal_blocks, gridDim.x - legal_blocks, states, fmt, B, pk, pooled, active, phase_delay,
                                        saturated, nullptr, nullptr);
    AQG_TRACE_END(2, (unsigned long long)(uintptr_t)pooled)
}
AQG_TRACE_SETTER(set_trace_eval)

// Sets of fewer than this many games defer.  A set of up to 512 games is a latency chain -- every board has a trunk workgroup of its own,
// and what the loop feels is the length of step -> trunk -- and gains 4.7 % games/s (4 x 512 games).  From 1,024 games per set on the
// trunk launch is a persistent walk bound by slot-time, where a search workgroup in a trunk-sized slot costs more than the same search
// inside the leaner step workgroup: +3.9 % at 4 x 640 games, +0.7 % at 4 x 768, -1.4 % at 4 x 1,024, -1.7 % at 4 x 2,048, -3.9 % at 4 x 4,096
// (profiles/leaf_legal_beside_trunk.log).  The boundary is the one the trunk's own priority mode uses (launch_gcn_trunk_split).
constexpr int LEGAL_BESIDE_TRUNK_BELOW = 1024;

// `step_heads`: enqueue_sims' own test for the step launches with the heads inside (9x9 split network, eight games per workgroup,
// no exact-f32 fall-back).  With the evaluation cache on nothing is deferred: a hit supplies the legal list from the table.
bool engine_step_defers_legal(const aqg_engine& e, bool step_heads) {
    return g_legal_beside_trunk && step_heads && !e.eval_cache_keys && e.board_size == 9 && e.prior_mode == 0 &&
           e.num_games < LEGAL_BESIDE_TRUNK_BELOW;
}

// Option "policy_beside_step" (mcts_step.hip): the step launches behind an evaluation launch split the expansion off into policy workgroups.
// Wherever the searches are deferred and the engine has a workspace for the jobs (aqgnn.h, gnn_workspace); no set-size gate of its own:
// deferring ends at 1,024 games.
int g_policy_beside_step = 1;
bool engine_policy_beside_step(const aqg_engine& e, bool defer_legal) {
    return g_policy_beside_step && defer_legal && e.gnn_workspace;
}

// The evaluation launch behind a deferring step: what launch_gcn_forward_boards launches for the engine's leaves without heads -- same
// board workgroups, same options, same profiling bracket -- with ceil(num_games / 8) search workgroups in front.
// `policy_jobs`: the step launch behind this one has policy workgroups, the searches leave them their jobs.
int launch_engine_eval(const aqg_engine& e, hipStream_t st, bool policy_jobs) {
    const int B = e.num_games;
    if (!e.pooled) return fail("pooled workspace is required");
    int grid, opts;
    trunk_split_launch_shape(B, false, grid, opts);
    const unsigned int legal_blocks = (unsigned int)((B + NWV - 1) / NWV);
    const LeafLegalArgs la = {e.leaf_flag, e.leaf_state, e.legal_order, e.legal_count, e.counters + 6,
                              e.node_count, policy_jobs ? aqg::policy_jobs(e) : nullptr, B, g_step_prio & 3};
    const dim3 tg(legal_blocks + grid), tb(64 * NWV);
    int32_t* saturated = e.counters + 5;
    if (g_profile_trunk == 1) profile_mark(st, B);
    if (e.gnn_flags & AQG_GNN_RANGE_PROVEN)
        hipLaunchKernelGGL(engine_eval_kernel<0>, tg, tb, 0, st, la, legal_blocks, (const void*)e.leaf_state, 1, B, e.packed_weights, e.pooled,
                           (const uint8_t*)e.leaf_flag, opts, saturated);
    else
        hipLaunchKernelGGL(engine_eval_kernel<2>, tg, tb, 0, st, la, legal_blocks, (const void*)e.leaf_state, 1, B, e.packed_weights, e.pooled,
                           (const uint8_t*)e.leaf_flag, opts, saturated);
    if (g_profile_trunk == 1) profile_mark(st, -1);
    return check_launch("engine_eval_kernel");
}

}  // namespace aqg
