// mcts_gumbel.hip -- the Gumbel root search outside the step kernel (map: mcts.hip; include/aqgnn.h, "Gumbel root search"): the root
// launch that turns an expanded root's priors into Gumbel logits (engine_gumbel_root_kernel), the finish-move launch that plays the
// survivor (engine_finish_move_gumbel_kernel) and the read-out (engine_root_gumbel_kernel).  None of them is tuned; one plain launcher
// each, which only enqueues (the entry point checks the launch).  No atomics besides engine_transition's counters, no LDS; every
// loop is bounded by MAX_LEGAL, and a child range is compared with node_cap before it is an address.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "counter_rng.hpp"
#include <cfloat>

// the logits are float64 as written, the scores float32 as written (no fma contraction)
#pragma clang fp contract(off)
#include "mcts_tree.hpp"
#include "mcts_gumbel_row.hpp"

namespace aqg {

// a stored child range that may be used as an address: at most MAX_LEGAL children, inside the pool, behind the root
__device__ __forceinline__ bool gumbel_range_ok(const aqg_engine& e, uint32_t kids) {
    const long long stored = (long long)(kids >> 24), first = (long long)(kids & 0xFFFFFF);
    return stored <= MAX_LEGAL && first >= 1 && first + stored <= (long long)e.node_cap;
}

// Gumbel(0, 1) variate i of the root keyed by `key` (aqgnn.h rule 1; gumbel.draw_gumbel is the same in numpy)
__device__ __forceinline__ double gumbel_variate(uint64_t key, int i) {
    const double u = counter_uniform(stream_key(key, (uint64_t)i), 0);
    double ex = -log(1.0 - u);
    if (ex == 0.0) ex = DBL_MIN;
    return -log(ex);
}

// ------------------------------------------------------------------------------------------------
// the root launch: between the root's expansion and simulation 1.  One wavefront per slot, four per workgroup; lane i + 64 r owns
// child i + 64 r of the root.  Writes gl_i into the child's `cp` and m_g into the slot's word, nothing else.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void engine_gumbel_root_kernel(aqg_engine e, aqg_gumbel gb) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games || !e.game_active[g]) return;
    NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint32_t kids = (uint32_t)__builtin_amdgcn_readfirstlane((int)nodes[0].kids);
    if (!gumbel_range_ok(e, kids) || (kids >> 24) == 0) {
        if (lane == 0) gb.m[g] = 0;
        return;
    }
    const int cnt = (int)(kids >> 24), first = (int)(kids & 0xFFFFFF);
    const uint64_t key = stream_key(stream_key(gb.seed, (uint64_t)(uint32_t)e.slot_game[g]), (uint64_t)load_state(e.root_state, 1, g).plies);
    const double* row = gb.table ? gb.table + (size_t)g * MAX_LEGAL : nullptr;
    int sampled = 0;
#pragma unroll
    for (int r = 0; r < (MAX_LEGAL + 63) / 64; ++r) {
        const int i = lane + 64 * r;
        if (i < cnt) {
            NodeRec& c = nodes[first + i];
            const float p = c.p;
            double gv;
            if (row) { const double x = row[i]; gv = (x >= -DBL_MAX && x <= DBL_MAX) ? x : 0.0; }      // not finite (NaN included): 0
            else gv = gumbel_variate(key, i);
            const double sg = gb.scale * gv;
            const float gl = p > 0.f ? (float)(sg + log((double)p)) : -INFINITY;
            c.cp = gl;
            sampled += gl > -INFINITY ? 1 : 0;
        }
    }
    sampled = wave_xor_sum(sampled);
    if (lane == 0) gb.m[g] = min(gb.considered, sampled);
}

// ------------------------------------------------------------------------------------------------
// finish move: engine_finish_move_kernel's history row (state72, the dense visit row, hist_value), the move by rule 4, the same
// engine_transition.  No uniform, no temperature; the options the entry point refuses have no argument here.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void engine_finish_move_gumbel_kernel(aqg_engine e, float* __restrict__ hist_value, float c_visit, float c_scale) {
    constexpr int A = Geo<N>::A;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games || !e.game_active[g]) return;
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint32_t kids = nodes[0].kids;
    const int cnt = gumbel_range_ok(e, kids) ? (int)(kids >> 24) : 0, first = (int)(kids & 0xFFFFFF);
    const int k = e.slot_game[g];
    const int ply = e.game_plies[k];
    const QState s = load_state(e.root_state, 1, g);
    if (ply < e.max_plies) {
        uint8_t* hs = e.hist_state72 + ((size_t)k * e.max_plies + ply) * STATE72;
        if (lane == 0) pack72(s, N, hs);
        uint16_t* hv = e.hist_visits + ((size_t)k * e.max_plies + ply) * A;
        for (int i = lane; i < cnt; i += 64) { const uint32_t a = nodes[first + i].action; if (a < (uint32_t)A) hv[a] = (uint16_t)nodes[first + i].n; }
    }
    if (lane != 0) return;
    if (hist_value && ply < e.max_plies) {                     // f32(w / n): the bits of -nodes[0].q
        const double w = nodes[0].w;
        const int n = nodes[0].n;
        hist_value[(size_t)k * e.max_plies + ply] = n ? (float)(w / (double)n) : 0.0f;
    }
    int chosen = -1;                                           // cnt = 0: the dead end
    if (cnt > 0) chosen = (int)nodes[first + gumbel_winner(nodes, first, cnt, c_visit, c_scale)].action;
    engine_transition<N>(e, g, k, ply, s, chosen);
}

// ------------------------------------------------------------------------------------------------
// the read-out, for tests and users: the logits as the root's children hold them, the slot's word, the winner by rule 4
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void engine_root_gumbel_kernel(aqg_engine e, aqg_gumbel gb, float* __restrict__ gl, int32_t* __restrict__ m,
                                                                 int32_t* __restrict__ winner) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games) return;
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint32_t kids = nodes[0].kids;
    const int cnt = gumbel_range_ok(e, kids) ? (int)(kids >> 24) : 0, first = (int)(kids & 0xFFFFFF);
    for (int i = lane; i < MAX_LEGAL; i += 64) gl[(size_t)g * MAX_LEGAL + i] = i < cnt ? nodes[first + i].cp : -INFINITY;
    if (lane != 0) return;
    m[g] = gb.m[g];
    winner[g] = cnt > 0 ? gumbel_winner(nodes, first, cnt, gb.c_visit, gb.c_scale) : -1;
}

void launch_engine_gumbel_root(const aqg_engine& e, const aqg_gumbel& gb, hipStream_t st) {
    hipLaunchKernelGGL(engine_gumbel_root_kernel, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, gb);
}

int launch_engine_finish_move_gumbel(const aqg_engine& e, const MoveOptions& opts, hipStream_t st) {
    const aqg_gumbel gb = *opts.gumbel;
    return for_board_size(e.board_size, [&](auto n) {
        hipLaunchKernelGGL(engine_finish_move_gumbel_kernel<decltype(n)::value>, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e,
                           opts.hist_value, gb.c_visit, gb.c_scale);
        return 0;
    });
}

void launch_engine_root_gumbel(const aqg_engine& e, const aqg_gumbel& gb, float* gl, int32_t* m, int32_t* winner, hipStream_t st) {
    hipLaunchKernelGGL(engine_root_gumbel_kernel, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, gb, gl, m, winner);
}

}  // namespace aqg
