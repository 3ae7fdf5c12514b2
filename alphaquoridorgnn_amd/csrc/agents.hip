// agents.hip -- the baseline agents of agents.py in batch, for gfx950: uniformly random moves (agents.py:14-18), random playouts
// (:111-121) and the rollout MCTS built on them (:130-214), plus the two engine entry points a "network vs agent" match needs:
// read every slot's position, apply a move the engine did not search.
//
// One 64-lane wavefront per state / game, as in legal_mask.hip: a playout is legal_actions() -> pick -> next() until the game ends,
// and legal_actions() is the one-lane-per-wall-slot wave of legal_wave.hpp.  The state is the same in every lane; the legal list
// goes through 136 bytes of LDS per wave.  Integer work only except UCB1 (float64, one division and one addition per child).
//
// Every loop ends on an integer cap computed from the arguments (plies left to the draw limit, evaluations, AQG_MAX_LEGAL, the node
// cap, the depth cap), never on a game condition alone.  No atomics on results: two runs give identical bytes.
#include "aqg_common.hpp"
#include "legal_wave.hpp"
#include "launchers.hpp"

#pragma clang fp contract(off)

namespace aqg {

// ------------------------------------------------------------------------------------------------
// random draws: a caller-supplied table, or the counter-based generator documented in include/aqgnn.h
// ------------------------------------------------------------------------------------------------
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {       // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Draws {
    const double* row;   // this state's table row, or nullptr = the generator
    int stride;          // entries of the row
    uint64_t key;        // mix64(seed + GOLDEN * (b + 1))
    int used;            // draws consumed so far
};
__device__ __forceinline__ Draws make_draws(const double* uniforms, int stride, uint64_t seed, int b) {
    Draws d;
    d.row = uniforms ? uniforms + (size_t)b * stride : nullptr;
    d.stride = stride;
    d.key = mix64(seed + GOLDEN * (uint64_t)(b + 1));
    d.used = 0;
    return d;
}
// (a table that is too short yields 0.0 past its end -- never a read out of bounds; the caller sees it in the draw count)
__device__ __forceinline__ double next_uniform(Draws& d) {
    const int i = d.used++;
    if (d.row) return i < d.stride ? d.row[i] : 0.0;
    return (double)(mix64(d.key + GOLDEN * (uint64_t)(i + 1)) >> 11) * 0x1.0p-53;
}
// index = min(count - 1, floor(u * count)); whatever u holds, the result lies in [0, count)
__device__ __forceinline__ int draw_index(double u, int count) {
    const double x = u * (double)count;
    return x >= 0.0 ? (x < (double)count ? (int)x : count - 1) : 0;
}

// the wave that wrote memory is the wave that reads it: a fence around a wave barrier is all the ordering needed
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the state is the same in every lane: say so, and the rules run on the scalar unit
__device__ __forceinline__ QState uniform_of(const QState& s) {
    auto u32 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
    QState r;
    r.hw = ((uint64_t)u32((uint32_t)(s.hw >> 32)) << 32) | u32((uint32_t)s.hw);
    r.vw = ((uint64_t)u32((uint32_t)(s.vw >> 32)) << 32) | u32((uint32_t)s.vw);
    const uint32_t m = u32((uint32_t)s.ppos | ((uint32_t)s.pwl << 8) | ((uint32_t)s.epos << 16) | ((uint32_t)s.ewl << 24));
    r.ppos = (uint8_t)m; r.pwl = (uint8_t)(m >> 8); r.epos = (uint8_t)(m >> 16); r.ewl = (uint8_t)(m >> 24);
    r.plies = (uint16_t)u32(s.plies);
    r.pad = 0;
    return r;
}

// random_action (agents.py:14-18): legal_actions()[index] for one draw, or -1 (and no draw) when there is none.
// `order`: this wave's MAX_LEGAL bytes of LDS.
template <int N>
__device__ __forceinline__ int wave_random_action(const QState& s, int lane, uint8_t* order, Draws& d) {
    wave_sync();                                            // the previous list's readers are done
    const int total = wave_legal_actions<N>(s, lane, nullptr, order);
    wave_sync();
    if (total <= 0) return -1;
    const int idx = draw_index(next_uniform(d), total);
    return __builtin_amdgcn_readfirstlane((int)order[idx]);
}

// playout (agents.py:111-121): -1 / 0 / +1 from the point of view of the mover of the state it starts from.  At most
// plies_for_draw - plies_played moves: the draw limit ends every game.  A position without a legal action ends as a draw.
template <int N>
__device__ __forceinline__ int wave_playout(QState s, int plies_for_draw, int lane, uint8_t* order, Draws& d, int& plies_out,
                                            QState& final_out) {
    int sign = 1, value = 0, plies = 0;
    const int cap = max(0, plies_for_draw - (int)s.plies);
    for (int it = 0; it <= cap; ++it) {
        if (is_lose<N>(s)) { value = -sign; break; }
        if (is_draw(s, plies_for_draw)) break;
        const int a = wave_random_action<N>(s, lane, order, d);
        if (a < 0) break;
        s = uniform_of(next_state<N>(s, a));
        sign = -sign;
        ++plies;
    }
    plies_out = plies;
    final_out = s;
    return value;
}

template <int N>
__global__ __launch_bounds__(64) void agent_random_kernel(const uint8_t* __restrict__ states72, int B, const double* __restrict__ uniforms,
                                                          int stride, uint64_t seed, int32_t* __restrict__ actions) {
    __shared__ uint8_t order[MAX_LEGAL];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= B) return;
    const QState s = uniform_of(unpack72(states72 + (size_t)b * STATE72));
    Draws d = make_draws(uniforms, stride, seed, b);
    const int a = wave_random_action<N>(s, lane, order, d);
    if (lane == 0) actions[b] = a;
}

template <int N>
__global__ __launch_bounds__(64) void playouts_kernel(const uint8_t* __restrict__ states72, int B, int plies_for_draw,
                                                      const double* __restrict__ uniforms, int stride, uint64_t seed,
                                                      int32_t* __restrict__ value, int32_t* __restrict__ plies,
                                                      int32_t* __restrict__ draws, uint8_t* __restrict__ final72) {
    __shared__ uint8_t order[MAX_LEGAL];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= B) return;
    const QState s = uniform_of(unpack72(states72 + (size_t)b * STATE72));
    Draws d = make_draws(uniforms, stride, seed, b);
    int np = 0;
    QState fin;
    const int v = wave_playout<N>(s, plies_for_draw, lane, order, d, np, fin);
    if (lane == 0) {
        value[b] = v;
        if (plies) plies[b] = np;
        if (draws) draws[b] = d.used;
        if (final72) pack72(fin, N, final72 + (size_t)b * STATE72);
    }
}

// ------------------------------------------------------------------------------------------------
// rollout MCTS (agents.py:130-214; the pinned statement is agents._Tree): one wavefront per root, its evaluations in order
// ------------------------------------------------------------------------------------------------
struct alignas(8) AgentNode {
    uint64_t hw, vw;
    uint32_t pawns;      // ppos | pwl << 8 | epos << 16 | ewl << 24
    uint16_t plies;
    uint16_t action;     // the action that led here
    int32_t w, n;        // playout values are -1 / 0 / +1: w is an integer
    int32_t first, count;
    int32_t parent;      // -1 = the root
    int32_t pad;
};
static_assert(sizeof(AgentNode) == 48, "AgentNode must be 48 bytes");

__host__ __device__ inline int agent_node_cap(int evaluations) { return 1 + (1 + evaluations / 10) * MAX_LEGAL; }

__device__ __forceinline__ QState node_state(const AgentNode& r) {
    QState s;
    s.hw = r.hw; s.vw = r.vw;
    s.ppos = (uint8_t)r.pawns; s.pwl = (uint8_t)(r.pawns >> 8); s.epos = (uint8_t)(r.pawns >> 16); s.ewl = (uint8_t)(r.pawns >> 24);
    s.plies = r.plies; s.pad = 0;
    return uniform_of(s);
}
__device__ __forceinline__ void node_init(AgentNode& r, const QState& s, int action, int parent) {
    r.hw = s.hw; r.vw = s.vw;
    r.pawns = (uint32_t)s.ppos | ((uint32_t)s.pwl << 8) | ((uint32_t)s.epos << 16) | ((uint32_t)s.ewl << 24);
    r.plies = s.plies; r.action = (uint16_t)action;
    r.w = 0; r.n = 0; r.first = -1; r.count = 0; r.parent = parent; r.pad = 0;
}

// _Tree.expand: the children of node i are the next() of its legal actions, in order, as consecutive rows
template <int N>
__device__ __forceinline__ void tree_expand(AgentNode* __restrict__ nodes, int i, const QState& s, int& node_count, int node_cap,
                                            int lane, uint8_t* order) {
    wave_sync();
    const int total = wave_legal_actions<N>(s, lane, nullptr, order);
    wave_sync();
    if (total < 0 || total > MAX_LEGAL || node_count + total > node_cap) return;      // cannot happen: the node cap bounds every expansion
    for (int k = lane; k < total; k += 64) {
        const int a = order[k];
        node_init(nodes[node_count + k], next_state<N>(s, a), a, i);
    }
    if (lane == 0) { nodes[i].first = node_count; nodes[i].count = total; }
    node_count += total;
    wave_sync();
}

// _Tree.select: the first child with n == 0, else the FIRST maximum of UCB1 = -w / n + explore[t][n] in float64
__device__ __forceinline__ int tree_select(const AgentNode* __restrict__ nodes, int first, int cnt, int lane, const double* __restrict__ explore,
                                           int evaluations) {
    static_assert(MAX_LEGAL <= 3 * 64, "tree_select gives every lane three children");
    int n[3], w[3];
    int t = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int k = lane + 64 * r;
        n[r] = -1; w[r] = 0;
        if (k < cnt) { n[r] = nodes[first + k].n; w[r] = nodes[first + k].w; t += n[r]; }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint64_t zero = __ballot(n[r] == 0);
        if (zero) return first + 64 * r + (int)__builtin_ctzll(zero);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
    t = min(max(t, 1), evaluations);                        // sum of the children's visits <= evaluations: the table's rows
    const double* __restrict__ row = explore + (size_t)t * (evaluations + 1);
    double bu = 0.0;
    int bk = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (n[r] <= 0) continue;
        const double u = (double)(-w[r]) / (double)n[r] + row[min(n[r], evaluations)];
        if (bk == 0x7fffffff || u > bu) { bu = u; bk = lane + 64 * r; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ou = __shfl_xor(bu, off);
        const int ok = __shfl_xor(bk, off);
        if (ok != 0x7fffffff && (bk == 0x7fffffff || ou > bu || (ou == bu && ok < bk))) { bu = ou; bk = ok; }
    }
    return first + min(bk, cnt - 1);
}

template <int N>
__global__ __launch_bounds__(64) void agent_mcts_kernel(const uint8_t* __restrict__ states72, int B, int evaluations, int plies_for_draw,
                                                        const double* __restrict__ explore, const double* __restrict__ uniforms,
                                                        int stride, uint64_t seed, AgentNode* __restrict__ pool, int node_cap,
                                                        int32_t* __restrict__ action_out, int32_t* __restrict__ visits,
                                                        uint8_t* __restrict__ actions, int32_t* __restrict__ count,
                                                        int32_t* __restrict__ draws) {
    __shared__ uint8_t order[MAX_LEGAL];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= B) return;
    AgentNode* __restrict__ nodes = pool + (size_t)b * node_cap;
    Draws d = make_draws(uniforms, stride, seed, b);
    const QState root = uniform_of(unpack72(states72 + (size_t)b * STATE72));
    if (lane == 0) node_init(nodes[0], root, 0xFFFF, -1);
    int node_count = 1;
    tree_expand<N>(nodes, 0, root, node_count, node_cap, lane, order);          // the root is expanded before the first evaluation
    const int depth_cap = 2 + evaluations / 10;                                 // a path is the root + at most one node per expansion
    for (int ev = 0; ev < evaluations; ++ev) {
        int i = 0, value = 0;
        for (int depth = 0; depth <= depth_cap; ++depth) {
            const QState s = node_state(nodes[i]);
            const bool lose = is_lose<N>(s);
            if (lose || is_draw(s, plies_for_draw)) { value = lose ? -1 : 0; break; }
            const int cnt = __builtin_amdgcn_readfirstlane(nodes[i].count);
            if (cnt == 0) {
                const int visited = __builtin_amdgcn_readfirstlane(nodes[i].n);
                int np;
                QState fin;
                value = wave_playout<N>(s, plies_for_draw, lane, order, d, np, fin);
                if (visited + 1 == 10) tree_expand<N>(nodes, i, s, node_count, node_cap, lane, order);
                break;
            }
            i = __builtin_amdgcn_readfirstlane(tree_select(nodes, __builtin_amdgcn_readfirstlane(nodes[i].first), cnt, lane, explore, evaluations));
        }
        // backup: value is the leaf's own view; every step up the path negates it
        if (lane == 0) {
            int k = i, v = value;
            for (int up = 0; up <= depth_cap + 1 && k >= 0; ++up) {
                nodes[k].w += v; nodes[k].n += 1;
                v = -v;
                k = nodes[k].parent;
            }
        }
        wave_sync();
    }
    // the first most-visited root child
    const int first = __builtin_amdgcn_readfirstlane(nodes[0].first), cnt = __builtin_amdgcn_readfirstlane(nodes[0].count);
    int bn = -1, bk = 0x7fffffff;
    for (int k = lane; k < MAX_LEGAL; k += 64) {
        const int nk = k < cnt ? nodes[first + k].n : 0;
        if (visits) visits[(size_t)b * MAX_LEGAL + k] = nk;
        if (actions) actions[(size_t)b * MAX_LEGAL + k] = k < cnt ? (uint8_t)nodes[first + k].action : 0xFF;
        if (k < cnt && nk > bn) { bn = nk; bk = k; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int on = __shfl_xor(bn, off), ok = __shfl_xor(bk, off);
        if (on > bn || (on == bn && ok < bk)) { bn = on; bk = ok; }
    }
    if (lane == 0) {
        action_out[b] = cnt > 0 ? (int)nodes[first + min(bk, cnt - 1)].action : -1;
        if (count) count[b] = cnt;
        if (draws) draws[b] = d.used;
    }
}

// ------------------------------------------------------------------------------------------------
// engine: the position of every slot, and a move the engine did not search
// ------------------------------------------------------------------------------------------------
__global__ void engine_root_states72_kernel(aqg_engine e, uint8_t* __restrict__ out72) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.num_games) return;
    pack72(load_state(e.root_state, 1, g), e.board_size, out72 + (size_t)g * STATE72);
}

// The transition half of engine_finish_move_kernel (csrc/mcts.hip) with a caller-given action: history row (state72, the action, a
// visit row that is zero except 1 at the action), next(), plies, lose / draw / z / counters / game_active.  A negative action on an
// active slot is the dead end: a draw, counted in counters[2].
template <int N>
__global__ __launch_bounds__(256) void engine_apply_actions_kernel(aqg_engine e, const int32_t* __restrict__ actions) {
    constexpr int A = Geo<N>::A;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games || !e.game_active[g]) return;
    const int k = e.slot_game[g];
    const int ply = e.game_plies[k];
    const int chosen = actions[g];
    const QState s = load_state(e.root_state, 1, g);
    if (chosen >= A) return;                                   // not an action of this board: the slot is left as it is
    if (ply < e.max_plies) {
        if (lane == 0) pack72(s, N, e.hist_state72 + ((size_t)k * e.max_plies + ply) * STATE72);
        uint16_t* hv = e.hist_visits + ((size_t)k * e.max_plies + ply) * A;
        for (int a = lane; a < A; a += 64) hv[a] = (a == chosen) ? 1 : 0;
    }
    if (lane != 0) return;
    if (chosen < 0) {
        e.game_active[g] = 0; e.game_result[k] = 0; e.game_done[k] = 1;
        atomicAdd(&e.counters[2], 1); atomicAdd(&e.counters[1], 1); atomicSub(&e.counters[0], 1);
        return;
    }
    if (ply < e.max_plies) e.hist_action[(size_t)k * e.max_plies + ply] = (uint8_t)chosen;
    const QState t = next_state<N>(s, chosen);
    store_state(e.root_state, g, t);
    e.game_plies[k] = ply + 1;
    const bool lose = is_lose<N>(t), draw = is_draw(t, e.plies_for_draw);
    if (lose || draw) {
        int z = 0;
        if (lose) z = ((t.plies % 2) == 0) ? -1 : 1;          // first_player_value (self_play.py:22-27)
        e.game_result[k] = (int8_t)z;
        e.game_done[k] = 1;
        e.game_active[g] = 0;
        atomicAdd(&e.counters[1], 1); atomicSub(&e.counters[0], 1);
    }
}

// ------------------------------------------------------------------------------------------------
// host-side enqueue (no sync, no allocation)
// ------------------------------------------------------------------------------------------------
#define AQG_AGENT_DISPATCH(N, CALL)                                   \
    switch (N) {                                                      \
        case 3: CALL(3); break;                                       \
        case 5: CALL(5); break;                                       \
        case 7: CALL(7); break;                                       \
        case 9: CALL(9); break;                                       \
        default: return fail("unsupported board_size (odd 3..9)");    \
    }

int launch_agent_random(int N, const uint8_t* states72, int B, const double* uniforms, int stride, uint64_t seed, int32_t* actions,
                        hipStream_t st) {
    if (B <= 0) return 0;
#define CALL_AR(n) hipLaunchKernelGGL(agent_random_kernel<n>, dim3(B), dim3(64), 0, st, states72, B, uniforms, stride, seed, actions)
    AQG_AGENT_DISPATCH(N, CALL_AR)
    return check_launch("agent_random_kernel");
}

int launch_playouts(int N, const uint8_t* states72, int B, int plies_for_draw, const double* uniforms, int stride, uint64_t seed,
                    int32_t* value, int32_t* plies, int32_t* draws, uint8_t* final72, hipStream_t st) {
    if (B <= 0) return 0;
#define CALL_PO(n) hipLaunchKernelGGL(playouts_kernel<n>, dim3(B), dim3(64), 0, st, states72, B, plies_for_draw, uniforms, stride, seed, \
                                      value, plies, draws, final72)
    AQG_AGENT_DISPATCH(N, CALL_PO)
    return check_launch("playouts_kernel");
}

size_t agent_mcts_workspace_bytes(int B, int evaluations) {
    if (B <= 0 || evaluations < 0) return 0;
    return (size_t)B * agent_node_cap(evaluations) * sizeof(AgentNode);
}

int launch_agent_mcts(int N, const uint8_t* states72, int B, int evaluations, int plies_for_draw, const double* explore,
                      const double* uniforms, int stride, uint64_t seed, void* workspace, size_t workspace_bytes, int32_t* action,
                      int32_t* visits, uint8_t* actions, int32_t* count, int32_t* draws, hipStream_t st) {
    if (B <= 0) return 0;
    if (workspace_bytes < agent_mcts_workspace_bytes(B, evaluations)) return fail("aqg_agent_mcts: workspace too small");
    const int cap = agent_node_cap(evaluations);
    AgentNode* pool = reinterpret_cast<AgentNode*>(workspace);
#define CALL_AM(n) hipLaunchKernelGGL(agent_mcts_kernel<n>, dim3(B), dim3(64), 0, st, states72, B, evaluations, plies_for_draw, explore, \
                                      uniforms, stride, seed, pool, cap, action, visits, actions, count, draws)
    AQG_AGENT_DISPATCH(N, CALL_AM)
    return check_launch("agent_mcts_kernel");
}

int engine_root_states72(const aqg_engine& e, uint8_t* out72, hipStream_t st) {
    const int N = e.board_size;
    if (!(N == 3 || N == 5 || N == 7 || N == 9)) return fail("unsupported board_size");
    if (e.num_games <= 0 || !e.root_state) return fail("aqg_engine_root_states72: incomplete engine");
    hipLaunchKernelGGL(engine_root_states72_kernel, dim3((e.num_games + 255) / 256), dim3(256), 0, st, e, out72);
    return check_launch("engine_root_states72_kernel");
}

int engine_apply_actions(const aqg_engine& e, const int32_t* actions, hipStream_t st) {
    if (e.num_games <= 0 || !e.root_state || !e.game_active || !e.slot_game || !e.game_plies || !e.game_result || !e.game_done ||
        !e.counters)
        return fail("aqg_engine_apply_actions: incomplete engine");
    if (e.max_plies > 0 && (!e.hist_state72 || !e.hist_visits || !e.hist_action)) return fail("aqg_engine_apply_actions: history buffers missing");
    if (e.quota < e.num_games) return fail("quota must be >= num_games");
    const dim3 grid((e.num_games + 3) / 4), block(256);
#define CALL_AA(n) hipLaunchKernelGGL(engine_apply_actions_kernel<n>, grid, block, 0, st, e, actions)
    AQG_AGENT_DISPATCH(e.board_size, CALL_AA)
    if (int r = check_launch("engine_apply_actions_kernel")) return r;
    return e.quota > e.num_games ? engine_refill(e, st) : 0;
}

}  // namespace aqg
