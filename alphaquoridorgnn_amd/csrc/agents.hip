// agents.hip -- the baseline agents of agents.py in batch, for gfx950: uniformly random moves (agents.py:14-18), random playouts
// (:111-121), the rollout MCTS built on them (:130-214) and depth-limited alpha-beta (:22-107).  (The two engine entry points a "network
// vs agent" match needs -- read every slot's position, apply a move the engine did not search -- are the engine's: mcts_move.hip.)
//
// One 64-lane wavefront per state / game, as in legal_mask.hip: a playout is legal_actions() -> pick -> next() until the game ends,
// and legal_actions() is the one-lane-per-wall-slot wave of legal_wave.hpp.  The state is the same in every lane; the legal list
// goes through 136 bytes of LDS per wave.  Integer work only except UCB1 (float64, one division and one addition per child).
//
// Every loop ends on an integer cap computed from the arguments (plies left to the draw limit, evaluations, AQG_MAX_LEGAL, the node
// cap, the depth cap), never on a game condition alone.  No atomics on results: two runs give identical bytes.
//
// Alpha-beta (agents.py:22-107) is served here too: the jump-aware shortest paths of its leaf evaluator, one lane per position, and
// the search itself, one wavefront per (state, root action) -- see the comment above ab_search's kernels.
#include "aqg_common.hpp"
#include "legal_wave.hpp"
#include "launchers.hpp"
#include "counter_rng.hpp"

#pragma clang fp contract(off)

namespace aqg {

// ------------------------------------------------------------------------------------------------
// random draws: a caller-supplied table, or the counter-based generator documented in include/aqgnn.h (counter_rng.hpp)
// ------------------------------------------------------------------------------------------------
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
    d.key = stream_key(seed, (uint64_t)b);
    d.used = 0;
    return d;
}
// (a table that is too short yields 0.0 past its end -- never a read out of bounds; the caller sees it in the draw count)
__device__ __forceinline__ double next_uniform(Draws& d) {
    const int i = d.used++;
    if (d.row) return i < d.stride ? d.row[i] : 0.0;
    return counter_uniform(d.key, (uint64_t)i);
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
// shortest paths (agents.py:27-54): the leaf evaluator of alpha-beta
// ------------------------------------------------------------------------------------------------
// Plies each side needs to reach its goal row over legal_actions_pos -- jumps allowed, the other pawn frozen -- or -1 when it is
// walled in: `sp` for the mover, `se` for the other side.  A level-synchronous fill over the open-edge boards (the three-word form of
// can_reach2_w3, without a candidate wall): the round in which the fill first touches the goal row is the depth at which the
// reference's first-in-first-out search pops its first goal tile.  The other side's search runs in the mover's frame -- start, goal
// row and obstacle rotated by 180 degrees instead of the walls -- which leaves every distance as it is.  At most V rounds.  The state
// may differ from lane to lane: nothing here is wave-uniform.
template <int N>
__device__ __forceinline__ void shortest_paths2(const QState& s, int& sp, int& se) {
    constexpr int V = Geo<N>::V;
    const Open o = make_open<N>(s.hw, s.vw);
    const W3 oU = w3(o.U), oD = w3(o.D), oL = w3(o.L), oR = w3(o.R);
    const int me = min((int)s.ppos, V - 1), other = V - 1 - min((int)s.epos, V - 1);      // (a malformed record stays on the board)
    const W3 nA = ~w3_bit(other), nB = ~w3_bit(me);
    const W3 gA = w3(mask_row<N>(0)), gB = w3(mask_row<N>(N - 1));
    W3 JA[4], JB[4];
    int qA[4], qB[4];
    jump_landings_w3<N>(oU, oD, oL, oR, other, JA, qA);
    jump_landings_w3<N>(oU, oD, oL, oR, me, JB, qB);
    W3 rA = w3_bit(me), rB = w3_bit(other);
    int dA = -1, dB = -1, done = 0;
    for (int it = 0; it < V; ++it) {
        if (!(done & 1) && w3_any(rA & gA)) { dA = it; done |= 1; }
        if (!(done & 2) && w3_any(rB & gB)) { dB = it; done |= 2; }
        if (done == 3) break;
        W3 a = (rA | w3_shl<N>(rA & oD) | w3_shr<N>(rA & oU) | w3_shl<1>(rA & oR) | w3_shr<1>(rA & oL)) & nA;
        W3 b = (rB | w3_shl<N>(rB & oD) | w3_shr<N>(rB & oU) | w3_shl<1>(rB & oR) | w3_shr<1>(rB & oL)) & nB;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t mA = w3_mask_of(rA, qA[d]), mB = w3_mask_of(rB, qB[d]);
            a.a |= JA[d].a & mA; a.b |= JA[d].b & mA; a.c |= JA[d].c & mA;
            b.a |= JB[d].a & mB; b.b |= JB[d].b & mB; b.c |= JB[d].c & mB;
        }
        if (w3_eq(a, rA)) done |= 1;                       // a fixpoint without the goal: walled in
        if (w3_eq(b, rB)) done |= 2;
        if (done == 3) break;
        rA = a; rB = b;
    }
    sp = dA; se = dB;
}

template <int N>
__global__ __launch_bounds__(256) void agent_shortest_paths_kernel(const uint8_t* __restrict__ states72, int B, int32_t* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int sp, se;
    shortest_paths2<N>(unpack72(states72 + (size_t)b * STATE72), sp, se);
    out[2 * (size_t)b] = sp;
    out[2 * (size_t)b + 1] = se;
}

// ------------------------------------------------------------------------------------------------
// alpha-beta (agents.py:58-107; the pinned statement is host_agents.cpp): one wavefront per (state, root action)
// ------------------------------------------------------------------------------------------------
// What the design rests on:
//  * Only true negamax values decide the action.  The reference searches root child i with the window (-inf, -alpha), alpha the
//    running best: the child's score is exact whenever it exceeds alpha and <= alpha otherwise, so the answer is the FIRST root
//    action with the maximal true depth-limited negamax value -- whatever the order of evaluation, and under any bound that never
//    exceeds the true running best.  Here: pass 0 searches root child 0 of every state with the full window (one wave per state);
//    pass 1 searches children 1..n-1 in parallel (one wave each) under the value of child 0; a third launch takes the first
//    maximum.  Root pruning is weaker than the reference's, parallelism ~130 times larger at 9x9.
//  * All scores compare as integers.  A leaf scores (se - sp) / max_dist, a lost position -1, a drawn one 0: the tree holds the
//    numerators se - sp, -max_dist and 0.  Distinct numerators are distinct doubles and negation is exact, so every comparison falls
//    as the host's float64 one does.  No floating point in the tree.
//  * The sentinel.  A position that is not over but has no legal action returns its incoming alpha; under a root child searched
//    from -inf that is -inf, and the root action scores +inf.  -inf is AB_INF here, an integer beyond every numerator, negated like
//    the others.
//  * The last ply is data-parallel.  At a node whose children are leaves the value is max over children of -h(child): one lane per
//    child does next(), lose / draw and the two fills, 64 children a round, and the cut-off is taken between rounds instead of
//    between children.  A cut-off node returns some value >= beta either way, which its parent discards either way.
// Above the last ply the search walks the tree with an explicit stack of max_depth frames (position, window, legal list, next
// child) in LDS.  Every loop ends on an integer cap: MAX_LEGAL, the V rounds of a fill, the step cap of ab_search.
constexpr int AB_MAX_DEPTH = AQG_AGENT_AB_MAX_DEPTH;
constexpr int AB_INF = 1 << 20;
static_assert(AB_MAX_DEPTH >= 1 && AB_MAX_DEPTH <= 4, "the step cap of ab_search is MAX_LEGAL^(depth - 1) in 64 bits; nodes are counted in 32");

struct AbFrame {
    QState s;
    int32_t alpha, beta, n, idx;
};

// the depth-0 value of a position from its mover's point of view, as a numerator over max_dist (per lane)
template <int N>
__device__ __forceinline__ int ab_leaf(const QState& t, int plies_for_draw, int max_dist) {
    if (is_lose<N>(t)) return -max_dist;
    if (is_draw(t, plies_for_draw)) return 0;
    int sp, se;
    shortest_paths2<N>(t, sp, se);
    return se - sp;
}

// a node whose children are leaves: alpha after the children, 64 per round; returns as soon as a round lifts it to beta
template <int N>
__device__ __forceinline__ int ab_last_ply(const QState& s, const uint8_t* list, int n, int alpha, int beta, int plies_for_draw,
                                           int max_dist, int lane, uint32_t& visited) {
    for (int r = 0; r < MAX_LEGAL; r += 64) {
        if (r >= n) break;
        const int k = r + lane;
        int sc = -AB_INF;
        if (k < n) sc = -ab_leaf<N>(next_state<N>(s, list[k]), plies_for_draw, max_dist);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sc = max(sc, __shfl_xor(sc, off));
        sc = __builtin_amdgcn_readfirstlane(sc);
        visited += (uint32_t)min(64, n - r);
        alpha = max(alpha, sc);
        if (alpha >= beta) break;
    }
    return alpha;
}

// alpha_beta(c, alpha, beta, depth) of agents.py:58-86 for a wave-uniform position c.  lists / fr: `depth` rows of this wave's LDS.
template <int N>
__device__ __forceinline__ int ab_search(const QState& c, int alpha, int beta, int depth, int plies_for_draw, int max_dist, int lane,
                                         uint8_t (*lists)[MAX_LEGAL], AbFrame* fr, uint32_t& visited) {
    visited = 1;
    if (depth <= 0 || is_lose<N>(c) || is_draw(c, plies_for_draw)) return ab_leaf<N>(c, plies_for_draw, max_dist);
    auto push = [&](int L, const QState& s, int a, int b) {
        wave_sync();                                        // the readers of this row's previous list are done
        const int n = wave_legal_actions<N>(s, lane, nullptr, lists[L]);
        if (lane == 0) { fr[L].s = s; fr[L].alpha = a; fr[L].beta = b; fr[L].n = n; fr[L].idx = 0; }
        wave_sync();
    };
    push(0, c, alpha, beta);
    // every step opens a child, closes a node, or takes a returned value: at most three per node above the last ply
    uint64_t inner = 0, level = 1;
    for (int j = 0; j < depth; ++j) { inner += level; level *= MAX_LEGAL; }
    const uint64_t cap = 3 * inner + 3;
    int L = 0, ret = alpha;
    bool returned = false;                                  // `ret` holds the value of a child of frame L
    for (uint64_t step = 0; step < cap; ++step) {
        int a = __builtin_amdgcn_readfirstlane(fr[L].alpha);
        const int b = __builtin_amdgcn_readfirstlane(fr[L].beta);
        bool close = false;
        if (returned) {
            returned = false;
            if (-ret > a) {
                a = -ret;
                wave_sync();
                if (lane == 0) fr[L].alpha = a;
                wave_sync();
            }
            close = a >= b;                                 // beta cut-off
        }
        if (!close) {
            const QState s = uniform_of(fr[L].s);
            const int n = __builtin_amdgcn_readfirstlane(fr[L].n);
            if (depth - L == 1) {
                a = ab_last_ply<N>(s, lists[L], n, a, b, plies_for_draw, max_dist, lane, visited);
                close = true;
            } else {
                const int idx = __builtin_amdgcn_readfirstlane(fr[L].idx);
                if (idx >= n) {
                    close = true;
                } else {
                    const QState t = uniform_of(next_state<N>(s, lists[L][idx]));
                    wave_sync();
                    if (lane == 0) fr[L].idx = idx + 1;
                    wave_sync();
                    ++visited;
                    if (is_lose<N>(t) || is_draw(t, plies_for_draw)) {
                        ret = ab_leaf<N>(t, plies_for_draw, max_dist);
                        returned = true;
                    } else {
                        ++L;
                        push(L, t, -b, -a);
                    }
                    continue;
                }
            }
        }
        ret = a;                                            // frame L is done: its value goes to its parent
        returned = true;
        if (L == 0) break;
        --L;
    }
    return ret;
}

// The workspace of one call: per state MAX_LEGAL scores and MAX_LEGAL node counts (32 bits each), the root's legal list, its length.
struct AbWorkspace {
    int32_t* score;      // [B, MAX_LEGAL] the root child's negamax score (exact, or a bound <= child 0's)
    uint32_t* visited;   // [B, MAX_LEGAL] positions visited under it
    int32_t* count;      // [B]
    uint8_t* action;     // [B, MAX_LEGAL]
};
__host__ __device__ inline size_t ab_workspace_bytes(int B) { return (size_t)B * (MAX_LEGAL * 9 + 4); }
__host__ __device__ inline AbWorkspace ab_workspace(void* p, int B) {
    AbWorkspace w;
    w.score = reinterpret_cast<int32_t*>(p);
    w.visited = reinterpret_cast<uint32_t*>(w.score + (size_t)B * MAX_LEGAL);
    w.count = reinterpret_cast<int32_t*>(w.visited + (size_t)B * MAX_LEGAL);
    w.action = reinterpret_cast<uint8_t*>(w.count + B);
    return w;
}

// pass 0: block = state, root child 0, full window.  pass 1: block = state * (MAX_LEGAL - 1) + (root child - 1), under child 0's score.
template <int N>
__global__ __launch_bounds__(64) void agent_alpha_beta_kernel(const uint8_t* __restrict__ states72, int B, const uint8_t* __restrict__ active,
                                                              int plies_for_draw, int max_dist, int max_depth, int pass, AbWorkspace w) {
    __shared__ uint8_t root_list[MAX_LEGAL];
    __shared__ uint8_t lists[AB_MAX_DEPTH][MAX_LEGAL];
    __shared__ AbFrame frames[AB_MAX_DEPTH];
    const int lane = threadIdx.x;
    const int b = pass == 0 ? (int)blockIdx.x : (int)(blockIdx.x / (MAX_LEGAL - 1));
    const int k = pass == 0 ? 0 : 1 + (int)(blockIdx.x % (MAX_LEGAL - 1));
    if (b >= B || (active && !active[b])) return;
    const QState root = uniform_of(unpack72(states72 + (size_t)b * STATE72));
    const int n = wave_legal_actions<N>(root, lane, nullptr, root_list);
    wave_sync();
    if (pass == 0) {
        if (lane == 0) w.count[b] = n;
        for (int i = lane; i < MAX_LEGAL; i += 64) w.action[(size_t)b * MAX_LEGAL + i] = root_list[i];
    }
    if (k >= n || n > MAX_LEGAL) return;
    const int bound = pass == 0 ? -AB_INF : w.score[(size_t)b * MAX_LEGAL];
    const QState c = uniform_of(next_state<N>(root, root_list[k]));
    uint32_t visited;
    const int v = ab_search<N>(c, -AB_INF, -bound, max_depth, plies_for_draw, max_dist, lane, lists, frames, visited);
    if (lane == 0) {
        w.score[(size_t)b * MAX_LEGAL + k] = -v;
        w.visited[(size_t)b * MAX_LEGAL + k] = visited;
    }
}

// the first maximum (agents.py:98-107: strictly greater than the running best, from -inf); 0 on a masked slot, -1 without an action
__global__ __launch_bounds__(256) void agent_alpha_beta_pick_kernel(int B, const uint8_t* __restrict__ active, AbWorkspace w,
                                                                    int32_t* __restrict__ action, int64_t* __restrict__ nodes) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int best = -1, alpha = -AB_INF;
    int64_t total = 0;
    if (active && !active[b]) {
        best = 0;
    } else {
        const int n = min(w.count[b], MAX_LEGAL);
        for (int k = 0; k < n; ++k) {
            const int sc = w.score[(size_t)b * MAX_LEGAL + k];
            total += w.visited[(size_t)b * MAX_LEGAL + k];
            if (sc > alpha) { alpha = sc; best = w.action[(size_t)b * MAX_LEGAL + k]; }
        }
    }
    action[b] = best;
    if (nodes) nodes[b] = total;
}

// ------------------------------------------------------------------------------------------------
// host-side enqueue (no sync, no allocation)
// ------------------------------------------------------------------------------------------------
int launch_agent_random(int N, const uint8_t* states72, int B, const double* uniforms, int stride, uint64_t seed, int32_t* actions,
                        hipStream_t st) {
    if (B <= 0) return 0;
    return for_board_size(N, [&](auto n) {
        hipLaunchKernelGGL(agent_random_kernel<decltype(n)::value>, dim3(B), dim3(64), 0, st, states72, B, uniforms, stride, seed, actions);
        return check_launch("agent_random_kernel");
    });
}

int launch_playouts(int N, const uint8_t* states72, int B, int plies_for_draw, const double* uniforms, int stride, uint64_t seed,
                    int32_t* value, int32_t* plies, int32_t* draws, uint8_t* final72, hipStream_t st) {
    if (B <= 0) return 0;
    return for_board_size(N, [&](auto n) {
        hipLaunchKernelGGL(playouts_kernel<decltype(n)::value>, dim3(B), dim3(64), 0, st, states72, B, plies_for_draw, uniforms, stride, seed,
                           value, plies, draws, final72);
        return check_launch("playouts_kernel");
    });
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
    return for_board_size(N, [&](auto n) {
        hipLaunchKernelGGL(agent_mcts_kernel<decltype(n)::value>, dim3(B), dim3(64), 0, st, states72, B, evaluations, plies_for_draw, explore,
                           uniforms, stride, seed, pool, cap, action, visits, actions, count, draws);
        return check_launch("agent_mcts_kernel");
    });
}

int launch_agent_shortest_paths(int N, const uint8_t* states72, int B, int32_t* out, hipStream_t st) {
    if (B <= 0) return 0;
    return for_board_size(N, [&](auto n) {
        hipLaunchKernelGGL(agent_shortest_paths_kernel<decltype(n)::value>, dim3((B + 255) / 256), dim3(256), 0, st, states72, B, out);
        return check_launch("agent_shortest_paths_kernel");
    });
}

constexpr int AB_MAX_STATES = 1 << 23;       // B * (MAX_LEGAL - 1) blocks fit a grid

size_t agent_alpha_beta_workspace_bytes(int N, int B, int max_depth) {
    if (!board_size_supported(N) || B <= 0 || B > AB_MAX_STATES || max_depth < 0 || max_depth > AB_MAX_DEPTH) return 0;
    return ab_workspace_bytes(B);
}

int launch_agent_alpha_beta(int N, const uint8_t* states72, int B, const uint8_t* active, int plies_for_draw, int max_dist,
                            int max_depth, void* workspace, size_t workspace_bytes, int32_t* action, int64_t* nodes, hipStream_t st) {
    if (B <= 0) return 0;
    if (B > AB_MAX_STATES) return fail("aqg_agent_alpha_beta: too many states in one call");
    if (workspace_bytes < ab_workspace_bytes(B)) return fail("aqg_agent_alpha_beta: workspace too small");
    const AbWorkspace w = ab_workspace(workspace, B);
    const int launched = for_board_size(N, [&](auto n) {
        constexpr int NN = decltype(n)::value;
        hipLaunchKernelGGL(agent_alpha_beta_kernel<NN>, dim3(B), dim3(64), 0, st, states72, B, active, plies_for_draw, max_dist, max_depth, 0, w);
        if (int r = check_launch("agent_alpha_beta_kernel (root child 0)")) return r;
        hipLaunchKernelGGL(agent_alpha_beta_kernel<NN>, dim3((unsigned)B * (MAX_LEGAL - 1)), dim3(64), 0, st, states72, B, active,
                           plies_for_draw, max_dist, max_depth, 1, w);
        return check_launch("agent_alpha_beta_kernel (root children 1..)");
    });
    if (launched) return launched;
    hipLaunchKernelGGL(agent_alpha_beta_pick_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, active, w, action, nodes);
    return check_launch("agent_alpha_beta_pick_kernel");
}

}  // namespace aqg
