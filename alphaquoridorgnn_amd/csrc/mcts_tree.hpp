// mcts_tree.hpp -- what the engine's units (mcts_step.hip, mcts_eval.hip, mcts_move.hip) share: of a game's tree pool the node record,
// its accessors and the wave sums (wave_ops.hpp); the initial position; a game's state as wave-uniform scalars (uniform_state); the one
// move transition (engine_transition: mcts_move.hip's finish_move / apply_actions and mcts_gumbel.hip's finish launch end in it).  __forceinline__ device code and declarations only.  The including unit
// sets `#pragma clang fp contract(off)` in front of this header: q_of and the backup are PUCT arithmetic.
#pragma once
#include "aqg_common.hpp"
#include "wave_ops.hpp"
#include "../../include/aqgnn.h"

namespace aqg {

// One reference-"Node" (pv_mcts.py:24-31) per 32-byte record: the statistics, the prior, the action that led here and
// the child range sit in one cache sector, so a descent level is ONE dependent load round (the chosen child's
// `kids` and `action` arrive together with its w/n/p) of two aligned 16-byte loads per child.
struct alignas(32) NodeRec {
    // cold half (bytes 0..15): what a descent needs only of the child it CHOSE
    double w;          // cumulative value (python float in the reference)
    float p;           // prior
    uint32_t action;   // action that led to this node (0xFF for the root)
    // hot half (bytes 16..31): what PUCT scores every child with -- one aligned 16-byte load per child
    int32_t n;         // visit count
    uint32_t kids;     // first child (24 bits) | child count << 24 ; 0 = unexpanded
    float q;           // f32(-w / n) as PUCT adds it (pv_mcts.py:74), 0 while n == 0: maintained by every writer of (w, n), so the
                       // descent reads it with the record instead of doing a float64 division per tree level on its critical path
    float cp;          // f32(C_PUCT * p), the first product of PUCT's exploration term (pv_mcts.py:75, evaluated left to right in f32):
                       // written with p, so the descent's per-level chain starts one multiply later
};
static_assert(sizeof(NodeRec) == 32, "NodeRec must be 32 bytes");

// The exploitation term exactly as the reference forms it: python float division of the float64 sums, rounded to float32 where it
// meets the float32 exploration term (pv_mcts.py:74 under NumPy-2 promotion; pinned by the reference traces).
__device__ __forceinline__ float q_of(double w, int n) { return n ? (float)(-w / (double)n) : 0.0f; }

__device__ __forceinline__ NodeRec* game_nodes(const aqg_engine& e, int g) {
    return reinterpret_cast<NodeRec*>(e.node_rec) + (size_t)g * e.node_cap;
}

// The expansion job of a game (option "policy_beside_step"; the jobs live in the engine's gnn_workspace, which the 9x9 forward leaves
// alone: aqgnn.h): written by the evaluation launch's search of a marked leaf, read and cleared by the policy workgroup of the step
// launch behind it.  first_new = the game's node_count at the time of the
// search (>= 1: the root is node 0; 0 = no job), cnt = the leaf's legal actions.  The step workgroup of the same launch reads the same
// two numbers from node_count / legal_count, so both decide `expanded` alike.
struct PolicyJob { int32_t first_new, cnt; };
__host__ __device__ __forceinline__ PolicyJob* policy_jobs(const aqg_engine& e) { return reinterpret_cast<PolicyJob*>(e.gnn_workspace); }
__device__ __forceinline__ unsigned int head_live(const PolicyJob* jobs, int i) { return jobs[i].first_new > 0 ? 1u : 0u; }    // (heads_body's board mask)

// Backup (pv_mcts.py:36-42,:49-50,:62-64): every node on the path gets w += value, n += 1 with the sign flipping
// per ply.  The path nodes are distinct, so lane d updates path[d] independently (one parallel step instead of a
// serial chain of dependent global read-modify-writes); the sums are the same float64 additions.
__device__ __forceinline__ void backup_path(NodeRec* __restrict__ nodes, const int* __restrict__ path, int depth,
                                            double leaf_value, int lane) {
    for (int d = lane; d <= depth; d += 64) {
        NodeRec& r = nodes[path[d]];
        r.w += ((depth - d) & 1) ? -leaf_value : leaf_value;
        r.n += 1;
        r.q = q_of(r.w, r.n);
    }
}

// the initial position (game_logic.py:25-40): both pawns on the middle of their own back row, no wall placed
__device__ __forceinline__ QState initial_state(int N, int num_walls) {
    QState s;
    s.hw = 0; s.vw = 0;
    s.ppos = (uint8_t)(N * (N - 1) + N / 2); s.pwl = (uint8_t)num_walls;
    s.epos = s.ppos; s.ewl = s.pwl;
    s.plies = 0; s.pad = 0;
    return s;
}

__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// a game's state is the same in every lane of its wavefront: as scalars, next() / is_lose() / is_draw() run on the scalar unit
__device__ __forceinline__ QState uniform_state(const QState& v) {
    QState s;
    s.hw = rfl64(v.hw); s.vw = rfl64(v.vw);
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)v.ppos | ((uint32_t)v.pwl << 8) | ((uint32_t)v.epos << 16) | ((uint32_t)v.ewl << 24)));
    s.ppos = (uint8_t)(m & 0xff); s.pwl = (uint8_t)((m >> 8) & 0xff); s.epos = (uint8_t)((m >> 16) & 0xff); s.ewl = (uint8_t)(m >> 24);
    s.plies = (uint16_t)__builtin_amdgcn_readfirstlane((int)v.plies); s.pad = 0;
    return s;
}

// ------------------------------------------------------------------------------------------------
// One move of the game in slot g (game k, at ply `ply`, position s), by lane 0 of the slot's wave: what a searched move
// (engine_finish_move_kernel) and a caller-given one (engine_apply_actions_kernel) have in common, so that matches and
// self-play record games the same way.  hist_action, next(), plies, lose / draw / z, the counters, game_active.
// ------------------------------------------------------------------------------------------------
// `resigned` (aqgnn.h, "resignation"): the mover gives up at s -- the row's action is 0xFF, no move is applied, and s itself is the
// ended position, lost for its mover.
template <int N>
__device__ __forceinline__ void engine_transition(const aqg_engine& e, int g, int k, int ply, const QState& s, int chosen,
                                                  bool resigned = false) {
    if (chosen < 0) {
        // Dead end: legal_actions() is empty.  The reference would re-predict forever-leaf and np.random.choice([])
        // raises; we abort the game as a draw and count it.
        e.game_active[g] = 0; e.game_result[k] = 0; e.game_done[k] = 1;
        atomicAdd(&e.counters[2], 1); atomicAdd(&e.counters[1], 1); atomicSub(&e.counters[0], 1);
        return;
    }
    if (ply < e.max_plies) e.hist_action[(size_t)k * e.max_plies + ply] = resigned ? (uint8_t)0xFF : (uint8_t)chosen;
    QState t = s;
    if (!resigned) {
        t = next_state<N>(s, chosen);
        store_state(e.root_state, g, t);
    }
    e.game_plies[k] = ply + 1;
    const bool lose = resigned || is_lose<N>(t), draw = !resigned && is_draw(t, e.plies_for_draw);
    if (lose || draw) {
        // first_player_value (self_play.py:22-27): ended state's mover lost; z of ply 0, alternating afterwards (:63-66)
        int z = 0;
        if (lose) z = ((t.plies % 2) == 0) ? -1 : 1;
        e.game_result[k] = (int8_t)z;
        e.game_done[k] = 1;
        e.game_active[g] = 0;                  // engine_refill_kernel may hand the slot its next game
        atomicAdd(&e.counters[1], 1); atomicSub(&e.counters[0], 1);
    }
}

}  // namespace aqg
