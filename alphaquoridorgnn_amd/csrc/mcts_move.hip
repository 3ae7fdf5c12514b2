// mcts_move.hip -- what the engine does once per move or once per engine (map: mcts.hip): reset, set_roots, begin_move, the `fake`
// evaluator, root noise, finish_move / apply_actions over one transition, refill, and the read-outs of the roots.  None of these
// kernels is tuned; each has one plain launcher that does its own board-size dispatch and only enqueues (the caller checks).
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "counter_rng.hpp"
#include <cfloat>

// the root-noise mix and the np.random.choice cumulative sums must be evaluated exactly as written (no fma contraction)
#pragma clang fp contract(off)
#include "mcts_tree.hpp"

namespace aqg {

// ------------------------------------------------------------------------------------------------
// reset: every slot -> initial position (game_logic.py:25-40), active
// ------------------------------------------------------------------------------------------------
// (aqgnn.h, "start positions") START = the game's first position comes from the caller's table: row index[k], or k % count, of game k;
// a row number outside the table -- the host refuses such an index before any launch -- starts from the opening record.  The plain
// instantiations are the kernels as they were.
__device__ __forceinline__ QState start_state(const aqg_engine& e, const aqg_start_table& t, int k) {
    if (t.count <= 0) return initial_state(e.board_size, e.num_walls);
    const int row = t.index ? t.index[k] : k % t.count;
    if (row < 0 || row >= t.count) return initial_state(e.board_size, e.num_walls);
    return unpack72(t.states72 + (size_t)row * STATE72);
}

template <class... Table>      // <> = the plain kernel, <aqg_start_table> = with the table as a second argument
__global__ void engine_reset_kernel(aqg_engine e, Table... table) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) {
        e.counters[0] = e.num_games;          // active slots
        e.counters[1] = 0;                    // finished games
        e.counters[2] = 0;                    // dead-end aborts
        e.counters[3] = e.num_games;          // next game index to hand out (slot refill)
        for (int i = 4; i < 8; ++i) e.counters[i] = 0;
    }
    if (g < e.quota) {                        // per-game records (quota >= num_games)
        e.game_plies[g] = 0;
        e.game_result[g] = 0;
        e.game_done[g] = 0;
        e.game_slot[g] = g < e.num_games ? g : -1;
        e.game_first_move[g] = 0;
    }
    if (g >= e.num_games) return;
    if constexpr (sizeof...(Table) != 0) store_state(e.root_state, g, start_state(e, table..., g));
    else store_state(e.root_state, g, initial_state(e.board_size, e.num_walls));
    e.game_active[g] = 1;
    e.slot_game[g] = g;
    e.node_count[g] = 0;
    e.leaf_flag[g] = 0;
    e.stat_leaf_evals[g] = 0;
    e.stat_terminal_sims[g] = 0;
    if (e.eval_cache_keys) { e.stat_cache_hits[g] = 0; e.eval_cache_slot[g] = -1; e.eval_mask[g] = 0; }
}

__global__ void engine_set_roots_kernel(aqg_engine e, const uint8_t* __restrict__ roots72) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.num_games) return;
    store_state(e.root_state, g, unpack72(roots72 + (size_t)g * STATE72));
    e.game_active[g] = 1;
    e.slot_game[g] = g;
    e.game_plies[g] = 0;
}

// ------------------------------------------------------------------------------------------------
// begin move: fresh tree per move (pv_mcts.py:81: no tree reuse) -- except in a slot that engine_keep_subtrees_kernel (mcts_reuse.hip)
// has marked in `kept` (nullptr = tree reuse off): its pool holds the chosen child's subtree, re-rooted, and node_count its size
// ------------------------------------------------------------------------------------------------
__global__ void engine_begin_move_kernel(aqg_engine e, const uint8_t* __restrict__ kept) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (e.eval_count) for (int i = g; i <= e.sims; i += gridDim.x * blockDim.x) e.eval_count[i] = 0;      // evaluation cache: entries of each simulation's list
    if (g >= e.num_games || !e.game_active[g]) return;
    if (!(kept && kept[g])) {
        NodeRec root;
        root.w = 0.0; root.p = 0.f; root.n = 0; root.kids = 0; root.action = 0xFF; root.q = 0.f; root.cp = 0.f;
        game_nodes(e, g)[0] = root;
        e.node_count[g] = 1;
    }
    const int k = e.slot_game[g];                  // the game this slot is playing
    const int ply = e.game_plies[k];
    if (e.hist_visits && ply < e.max_plies) {      // clear this ply's dense visit row (filled by finish_move)
        const int A = e.board_size * e.board_size + 2 * (e.board_size - 1) * (e.board_size - 1);
        uint16_t* hv = e.hist_visits + ((size_t)k * e.max_plies + ply) * A;
        for (int a = 0; a < A; ++a) hv[a] = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// `fake` evaluator (tests): oracle/mcts.py FakeModel, exact integer hash -> f32 priors (written over the
// first `count` entries of policy[g]) and value.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fnv1a_state72(const uint8_t* r68, int plies) {
    uint32_t h = 0x811C9DC5u;
    for (int i = 0; i < 68; ++i) { h ^= r68[i]; h *= 0x01000193u; }
    h ^= (uint32_t)(plies & 0xFF); h *= 0x01000193u;
    h ^= (uint32_t)((plies >> 8) & 0xFF); h *= 0x01000193u;
    return h;
}

template <int N>
__global__ __launch_bounds__(256) void engine_fake_eval_kernel(aqg_engine e) {
    constexpr int V = N * N, A = Geo<N>::A;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games || e.leaf_flag[g] != 1) return;
    const QState s = load_state(e.leaf_state, 1, g);
    uint8_t rec[STATE72];
    pack72(s, N, rec);
    const uint32_t h = fnv1a_state72(rec, s.plies);
    const int cnt = e.legal_count[g];
    const uint8_t* ord = e.legal_order + (size_t)g * MAX_LEGAL;
    const int prow = s.ppos / N;
    int rl[3]; int tot = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = lane + 64 * r;
        rl[r] = 0;
        if (i < cnt) {
            const int a = ord[i];
            uint32_t x = ((h ^ ((uint32_t)(a + 1) * 0x9E3779B1u)) * 0x85EBCA6Bu) >> 22;
            int rr = (int)x + 1;
            if (a < V && (a / N) < prow) rr *= 1 + e.fake_bias;
            rl[r] = rr; tot += rr;
        }
    }
    tot = wave_xor_sum(tot);
    float* pol = e.policy + (size_t)g * A;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = lane + 64 * r;
        if (i < cnt) pol[i] = (float)rl[r] / (float)tot;
    }
    if (lane == 0) e.value[g] = (float)((int)((h * 0xC2B2AE35u) >> 16) - 32768) / 32768.0f;
}

// ------------------------------------------------------------------------------------------------
// root exploration noise (aqgnn.h, "root exploration noise"): p' = (1 - eps) p + eps eta, eta ~ Dir(alpha), mixed into the root's
// priors between the evaluation of simulation 0 and the step of simulation 1.  One wavefront per slot; lane i + 64 r owns legal
// action i + 64 r.  The step kernel is not changed: a root whose priors were mixed is handed to it as leaf_flag 2 -- "the row holds
// normalised priors in legal order" -- which it expands from the row as it stands and never writes into the evaluation cache, so
// the table only ever holds the network's own priors.
// ------------------------------------------------------------------------------------------------
constexpr int ROOT_NOISE_ATTEMPTS = 64;      // cap of the Marsaglia-Tsang rejection loop (acceptance is above 95 % per attempt)
// Gamma(alpha, 1) of one component's sub-stream, the recipe of aqgnn.h (engine.draw_root_noise is the same in numpy)
__device__ __forceinline__ double root_noise_gamma(uint64_t key, double alpha) {
    const bool boost = alpha < 1.0;
    const double a = boost ? alpha + 1.0 : alpha;
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double val = d;                          // cap exhausted: the value of v = 1
    for (int t = 0; t < ROOT_NOISE_ATTEMPTS; ++t) {
        const double u1 = counter_uniform(key, 1 + 3 * t), u2 = counter_uniform(key, 2 + 3 * t), u3 = counter_uniform(key, 3 + 3 * t);
        const double x = sqrt(-2.0 * log(1.0 - u1)) * cospi(2.0 * u2);      // Box-Muller
        const double v1 = 1.0 + c * x;
        if (v1 <= 0.0) continue;
        const double v = v1 * v1 * v1;
        if (log(1.0 - u3) < 0.5 * x * x + d - d * v + d * log(v)) { val = d * v; break; }
    }
    if (boost) val = val * pow(1.0 - counter_uniform(key, 0), 1.0 / alpha);
    return fmax(val, DBL_MIN);               // u ^ (1 / alpha) may underflow: a variate is never 0
}

// eta of one root, the recipe of aqgnn.h: lane i + 64 r gets eta[r] = f32(g_i / S) of legal action i + 64 r from the caller's table or
// from the generator's stream of (seed, game, plies).  false = no usable noise (S is 0 or not finite): the root keeps its priors.
__device__ __forceinline__ bool root_noise_eta(const aqg_engine& e, int g, int plies, int cnt, int lane, float (&eta)[3]) {
    double gv[3] = {0.0, 0.0, 0.0};
    if (e.root_noise) {
        const double* row = e.root_noise + (size_t)g * MAX_LEGAL;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = lane + 64 * r;
            if (i < cnt) { const double x = row[i]; gv[r] = (x > 0.0 && x <= DBL_MAX) ? x : 0.0; }      // not > 0 or not finite: 0
        }
    } else {
        const uint64_t key = stream_key(stream_key(e.root_noise_seed, (uint64_t)(uint32_t)e.slot_game[g]), (uint64_t)plies);
        const double alpha = (double)e.root_noise_alpha;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = lane + 64 * r;
            if (i < cnt) gv[r] = root_noise_gamma(stream_key(key, (uint64_t)i), alpha);
        }
    }
    const double S = wave_xor_sum((gv[0] + gv[1]) + gv[2]);
    if (!(S > 0.0 && S <= DBL_MAX)) return false;
#pragma unroll
    for (int r = 0; r < 3; ++r) eta[r] = (float)(gv[r] / S);
    return true;
}

template <int N>
__global__ __launch_bounds__(256) void engine_root_noise_kernel(aqg_engine e) {
    constexpr int A = Geo<N>::A;
    static_assert(A <= 256 && MAX_LEGAL <= 192, "three lane rounds cover the legal list, four the dense row");
    __shared__ float polbuf[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = blockIdx.x * 4 + w;
    if (g >= e.num_games || !e.game_active[g]) return;
    const int flag = __builtin_amdgcn_readfirstlane((int)e.leaf_flag[g]);
    if ((flag != 1 && flag != 2) || e.path_len[g] != 0) return;          // the pending leaf is not the root
    const int cnt = __builtin_amdgcn_readfirstlane(min(e.legal_count[g], (int)MAX_LEGAL));
    if (cnt <= 0) return;
    float* pol = e.policy + (size_t)g * A;
    const bool gather = e.prior_mode == 0 && flag == 1;
    float pl[3] = {0.f, 0.f, 0.f};
    if (gather) {                            // the arithmetic of game_step_fast: gather at the legal actions, divide by the sum unless 0
        const uint8_t* ord = e.legal_order + (size_t)g * MAX_LEGAL;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int a = lane + 64 * r; polbuf[w][a] = (a < A) ? pol[a] : 0.f; }
        wave_lds_sync();
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = lane + 64 * r;
            pl[r] = (i < cnt) ? polbuf[w][ord[i]] : 0.f;
            sum += pl[r];
        }
        sum = wave_xor_sum(sum);
        const float den = (sum != 0.f) ? sum : 1.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) pl[r] = pl[r] / den;
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) { const int i = lane + 64 * r; pl[r] = (i < cnt) ? pol[i] : 0.f; }
    }
    // the gamma variates: the caller's table, or the generator's stream of (seed, game, ply), one sub-stream per component
    float eta[3] = {0.f, 0.f, 0.f};
    if (!root_noise_eta(e, g, e.root_noise ? 0 : (int)load_state(e.leaf_state, 1, g).plies, cnt, lane, eta)) return;      // the root keeps its priors, untouched
    const float eps = e.root_noise_eps, keep = 1.0f - eps;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = lane + 64 * r;
        if (i < cnt) {
            const float x = keep * pl[r], y = eps * eta[r];
            pol[i] = x + y;
        }
    }
    if (lane == 0) {
        if (gather) e.leaf_flag[g] = 2;                                  // the row is now legal-ordered and normalised
        if (e.eval_cache_keys) e.eval_cache_slot[g] = -1;                // ... and must never be stored under the position's key
    }
}

// Root noise of a KEPT root (aqgnn.h, "tree reuse"): the root is expanded already, so the launch above -- which acts on a root that is
// the pending leaf -- skips it.  Same formula, same key, same table; p' goes into the stored p of the root's children and cp =
// f32(c_puct * p') is rewritten with it, in front of simulation 0's step, so every selection at the root sees the mixed priors.  These
// children were an inner node's until the keep launch: no prior is ever mixed twice.  The evaluation cache is not involved.
__global__ __launch_bounds__(256) void engine_kept_root_noise_kernel(aqg_engine e, const uint8_t* __restrict__ kept) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games || !e.game_active[g] || !kept[g]) return;
    NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint32_t kids = nodes[0].kids;
    const int cnt = __builtin_amdgcn_readfirstlane(min((int)(kids >> 24), (int)MAX_LEGAL)), first = (int)(kids & 0xFFFFFF);
    if (cnt <= 0 || first + cnt > e.node_cap) return;
    float eta[3] = {0.f, 0.f, 0.f};
    if (!root_noise_eta(e, g, e.root_noise ? 0 : (int)load_state(e.root_state, 1, g).plies, cnt, lane, eta)) return;
    const float eps = e.root_noise_eps, keep = 1.0f - eps;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = lane + 64 * r;
        if (i < cnt) {
            NodeRec& c = nodes[first + i];
            const float x = keep * c.p, y = eps * eta[r];
            const float p = x + y;
            c.p = p; c.cp = e.c_puct * p;
        }
    }
}

// (engine_transition, the one move transition behind finish_move, apply_actions and the Gumbel finish launch: mcts_tree.hpp)

// ------------------------------------------------------------------------------------------------
// finish move: visits -> policy (pv_mcts.py:88-95), record, np.random.choice, next(), terminal handling
// The two training-target options of aqgnn.h ("self-play targets") are kernel arguments, not engine fields -- this launch is not part
// of the captured graph: temperature_plies K > 0 = a root at ply >= K takes the first maximum, as temperature 0 does; hist_value !=
// nullptr = the root's search value w / n from the mover's side, f32 [quota, max_plies] beside hist_action.  (0, nullptr) = neither.
// Tree reuse (aqgnn.h, "tree reuse"): child_index != nullptr = the slot's marker is cleared -- its root changes -- and the index of the
// chosen child in the root's block is left for engine_keep_subtrees_kernel, -1 where the game does not go on.
// Resignation (aqgnn.h, "resignation"): rs.resign_min != nullptr = on.  The pass over the children that finds the arg-max / the
// sampling total also finds the first maximum of the visit counts; m = max(root value, that child's q) goes into the running
// minimum of (game, side), and an enabled game whose m is below -threshold ends here with the mover as loser.  An all-zero rs =
// off: nothing below reads or writes through it.
// ------------------------------------------------------------------------------------------------
// Start positions (aqgnn.h, "start positions"): GAME_PLY = the two ply tests below -- the temperature schedule's and resign_min_ply's --
// count the plies played in THIS game (game_plies) instead of reading the record's counter; from the opening the two are one number,
// and the plain instantiation is the kernel as it was.
template <int N, bool GAME_PLY = false>
__global__ __launch_bounds__(256) void engine_finish_move_kernel(aqg_engine e, const double* __restrict__ uniforms, int temperature_plies,
                                                                 float* __restrict__ hist_value, int32_t* __restrict__ child_index,
                                                                 uint8_t* __restrict__ kept, aqg_resign rs) {
    constexpr int A = Geo<N>::A;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games || !e.game_active[g]) return;
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint32_t kids = nodes[0].kids;
    const int cnt = (int)(kids >> 24), first = (int)(kids & 0xFFFFFF);
    const int k = e.slot_game[g];                  // history, plies and result are kept per GAME: a slot plays several
    const int ply = e.game_plies[k];
    QState s = load_state(e.root_state, 1, g);

    // history row: state72 + dense visit counts
    if (ply < e.max_plies) {
        uint8_t* hs = e.hist_state72 + ((size_t)k * e.max_plies + ply) * STATE72;
        if (lane == 0) pack72(s, N, hs);
        uint16_t* hv = e.hist_visits + ((size_t)k * e.max_plies + ply) * A;
        for (int i = lane; i < cnt; i += 64) hv[nodes[first + i].action] = (uint16_t)nodes[first + i].n;
    }
    if (lane != 0) return;
    if (hist_value && ply < e.max_plies) {                     // f32(w / n): the bits of -nodes[0].q
        const double w = nodes[0].w;
        const int n = nodes[0].n;
        hist_value[(size_t)k * e.max_plies + ply] = n ? (float)(w / (double)n) : 0.0f;
    }

    int chosen = -1, idx = -1, best = 0;                      // best: the first maximum of the visit counts
    if (cnt > 0) {
        idx = 0;
        const bool late = temperature_plies > 0 && (GAME_PLY ? ply : (int)s.plies) >= temperature_plies;      // the schedule: arg-max from ply K on
        if (e.temperature == 0.f || late) {                    // one-hot at the first maximum, then choice(p=one-hot)
            int bestn = -1;
            for (int i = 0; i < cnt; ++i) { const int n = nodes[first + i].n; if (n > bestn) { bestn = n; idx = i; } }
            best = idx;
        } else {
            // boltzman (pv_mcts.py:106-109): xs = n ** (1/T); p = x / sum(xs).  T == 1 is exact (n ** 1.0 == float(n)).
            const double invT = 1.0 / (double)e.temperature;
            double tot = 0.0;
            int bestn = -1;
            for (int i = 0; i < cnt; ++i) {
                const int n = nodes[first + i].n;
                if (n > bestn) { bestn = n; best = i; }
                const double x = (double)n;
                tot += (e.temperature == 1.f) ? x : pow(x, invT);
            }
            // np.random.choice: cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(cdf, u, side='right')
            double last = 0.0;
            for (int i = 0; i < cnt; ++i) {
                const double x = (double)nodes[first + i].n;
                last += ((e.temperature == 1.f) ? x : pow(x, invT)) / tot;
            }
            const double u = uniforms[g];
            double acc = 0.0;
            idx = 0;
            for (int i = 0; i < cnt; ++i) {
                const double x = (double)nodes[first + i].n;
                acc += ((e.temperature == 1.f) ? x : pow(x, invT)) / tot;
                if (acc / last <= u) idx = i + 1;
            }
            if (idx >= cnt) idx = cnt - 1;
        }
        chosen = (int)nodes[first + idx].action;
    }
    bool resigned = false;
    const int p = (int)s.plies;
    if (rs.resign_min && cnt > 0 && (GAME_PLY ? ply : p) >= rs.min_ply) {
        const double rw = nodes[0].w, cw = nodes[first + best].w;
        const int rn = nodes[0].n, cn = nodes[first + best].n;
        const float v_root = rn ? (float)(rw / (double)rn) : 0.0f;
        const float v_best = cn ? (float)(-cw / (double)cn) : 0.0f;
        const float m = fmaxf(v_root, v_best);
        float* lo = rs.resign_min + (size_t)k * 2 + (p & 1);   // this game's, this side's: only this lane writes it
        if (m < *lo) *lo = m;
        const bool enabled = counter_uniform(stream_key(rs.seed, (uint64_t)(uint32_t)k), 0) >= rs.disable_fraction;
        resigned = enabled && m < -rs.threshold;
        if (resigned) rs.game_resigned[k] = 1;
    }
    engine_transition<N>(e, g, k, ply, s, chosen, resigned);
    if (child_index) { child_index[g] = e.game_active[g] ? idx : -1; kept[g] = 0; }
}

// ------------------------------------------------------------------------------------------------
// slot refill: a rank plays a QUOTA of games on its G slots (the reference's plain loop over games, self_play.py:81-84).
// After every move the idle slots -- in slot order, so that the assignment is deterministic -- take the next game
// indices not yet handed out and start from the initial position; once the quota is exhausted a finished slot stays
// idle.  One workgroup: a block-wide exclusive scan over the slots' "idle" flags.
// ------------------------------------------------------------------------------------------------
template <class... Table>
__global__ __launch_bounds__(1024) void engine_refill_kernel(aqg_engine e, Table... table) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) base = e.counters[3];
    __syncthreads();
    const int move_index = e.counters[4] + 1;               // counters[4] = moves finished before this one; new games join the next
    __syncthreads();
    for (int g0 = 0; g0 < e.num_games; g0 += 1024) {
        const int g = g0 + tid;
        const int idle = (g < e.num_games && !e.game_active[g] && e.slot_game[g] >= 0) ? 1 : 0;
        int x = idle;                                        // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off); if (lane >= off) x += y; }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < 16; ++i) { if (i < w) before += wsum[i]; total += wsum[i]; }
        const int k = base + before + x - idle;              // this slot's next game, if any is left
        if (idle) {
            if (k < e.quota) {
                if constexpr (sizeof...(Table) != 0) store_state(e.root_state, g, start_state(e, table..., k));
                else store_state(e.root_state, g, initial_state(e.board_size, e.num_walls));
                e.slot_game[g] = k;
                e.game_slot[k] = g;
                e.game_first_move[k] = move_index;
                e.game_active[g] = 1;
                e.leaf_flag[g] = 0;
            } else {
                e.slot_game[g] = -1;                         // retired
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int handed = min(total, max(e.quota - base, 0));
            base += total;
            if (handed) atomicAdd(&e.counters[0], handed);
        }
        __syncthreads();
    }
    if (tid == 0) { e.counters[3] = min(base, e.quota); e.counters[4] = move_index; }
}

template <int N>
__global__ __launch_bounds__(256) void engine_root_visits_kernel(aqg_engine e, int32_t* __restrict__ visits,
                                                                 uint8_t* __restrict__ actions, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games) return;
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint32_t kids = nodes[0].kids;
    const int cnt = (int)(kids >> 24), first = (int)(kids & 0xFFFFFF);
    for (int i = lane; i < MAX_LEGAL; i += 64) {
        visits[(size_t)g * MAX_LEGAL + i] = (i < cnt) ? nodes[first + i].n : 0;
        actions[(size_t)g * MAX_LEGAL + i] = (i < cnt) ? (uint8_t)nodes[first + i].action : 0xFF;
    }
    if (lane == 0) count[g] = cnt;
}

__global__ __launch_bounds__(256) void engine_root_priors_kernel(aqg_engine e, float* __restrict__ priors, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games) return;
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const uint32_t kids = nodes[0].kids;
    const int cnt = (int)(kids >> 24), first = (int)(kids & 0xFFFFFF);
    for (int i = lane; i < MAX_LEGAL; i += 64) priors[(size_t)g * MAX_LEGAL + i] = (i < cnt) ? nodes[first + i].p : 0.f;
    if (lane == 0) count[g] = cnt;
}

// the root's search value from the mover's side, one lane per slot: the expression engine_finish_move_kernel stores into hist_value
__global__ __launch_bounds__(256) void engine_root_values_kernel(aqg_engine e, float* __restrict__ value) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.num_games) return;
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const double w = nodes[0].w;
    const int n = nodes[0].n;
    value[g] = n ? (float)(w / (double)n) : 0.0f;
}

// ------------------------------------------------------------------------------------------------
// engine: the position of every slot, and a move the engine did not search
// ------------------------------------------------------------------------------------------------
__global__ void engine_root_states72_kernel(aqg_engine e, uint8_t* __restrict__ out72) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.num_games) return;
    pack72(load_state(e.root_state, 1, g), e.board_size, out72 + (size_t)g * STATE72);
}

// engine_transition with a caller-given action behind its own history row (state72, a visit row that is zero except 1 at the
// action).  A negative action on an active slot is the dead end: a draw, counted in counters[2].
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
    engine_transition<N>(e, g, k, ply, s, chosen);
}

// ------------------------------------------------------------------------------------------------
// host-side enqueue (no sync, no allocation): one launcher per kernel.  The entry points of mcts.hip validate in front of them and
// check the launch behind them; a launcher's own status is the board-size dispatch's.
// ------------------------------------------------------------------------------------------------
void launch_engine_reset(const aqg_engine& e, hipStream_t st, const aqg_start_table* start) {
    const dim3 grid((max(e.num_games, e.quota) + 255) / 256), block(256);
    if (start) hipLaunchKernelGGL(engine_reset_kernel<aqg_start_table>, grid, block, 0, st, e, *start);
    else hipLaunchKernelGGL(engine_reset_kernel<>, grid, block, 0, st, e);
}

void launch_engine_set_roots(const aqg_engine& e, const uint8_t* roots72, hipStream_t st) {
    hipLaunchKernelGGL(engine_set_roots_kernel, dim3((e.num_games + 255) / 256), dim3(256), 0, st, e, roots72);
}

void launch_engine_begin_move(const aqg_engine& e, hipStream_t st, const uint8_t* kept) {
    hipLaunchKernelGGL(engine_begin_move_kernel, dim3((e.num_games + 255) / 256), dim3(256), 0, st, e, kept);
}

void launch_engine_kept_root_noise(const aqg_engine& e, const uint8_t* kept, hipStream_t st) {
    hipLaunchKernelGGL(engine_kept_root_noise_kernel, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, kept);
}

int launch_engine_fake_eval(const aqg_engine& e, hipStream_t st) {
    return for_board_size(e.board_size, [&](auto n) {
        hipLaunchKernelGGL(engine_fake_eval_kernel<decltype(n)::value>, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e);
        return 0;
    });
}

int launch_engine_root_noise(const aqg_engine& e_in, hipStream_t st) {
    aqg_engine e = e_in;                     // modes 3 and 4 leave a dense row like mode 0 (see launch_engine_step)
    if (e.prior_mode == 3 || e.prior_mode == 4) e.prior_mode = 0;
    return for_board_size(e.board_size, [&](auto n) {
        hipLaunchKernelGGL(engine_root_noise_kernel<decltype(n)::value>, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e);
        return 0;
    });
}

int launch_engine_finish_move(const aqg_engine& e, const double* uniforms, const MoveOptions& opts, hipStream_t st) {
    const aqg_resign rs = opts.resign ? *opts.resign : aqg_resign{};     // all zero = off
    int32_t* child_index = opts.reuse ? opts.reuse->child_index : nullptr;
    uint8_t* kept = opts.reuse ? opts.reuse->kept : nullptr;
    return for_board_size(e.board_size, [&](auto n) {
        if (opts.start)
            hipLaunchKernelGGL((engine_finish_move_kernel<decltype(n)::value, true>), dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, uniforms,
                               opts.temperature_plies, opts.hist_value, child_index, kept, rs);
        else
            hipLaunchKernelGGL(engine_finish_move_kernel<decltype(n)::value>, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, uniforms,
                               opts.temperature_plies, opts.hist_value, child_index, kept, rs);
        return 0;
    });
}

void launch_engine_refill(const aqg_engine& e, hipStream_t st, const aqg_start_table* start) {
    if (start) hipLaunchKernelGGL(engine_refill_kernel<aqg_start_table>, dim3(1), dim3(1024), 0, st, e, *start);
    else hipLaunchKernelGGL(engine_refill_kernel<>, dim3(1), dim3(1024), 0, st, e);
}

int launch_engine_root_visits(const aqg_engine& e, int32_t* visits, uint8_t* actions, int32_t* count, hipStream_t st) {
    return for_board_size(e.board_size, [&](auto n) {
        hipLaunchKernelGGL(engine_root_visits_kernel<decltype(n)::value>, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, visits, actions, count);
        return 0;
    });
}

void launch_engine_root_priors(const aqg_engine& e, float* priors, int32_t* count, hipStream_t st) {
    hipLaunchKernelGGL(engine_root_priors_kernel, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, priors, count);
}

void launch_engine_root_values(const aqg_engine& e, float* value, hipStream_t st) {
    hipLaunchKernelGGL(engine_root_values_kernel, dim3((e.num_games + 255) / 256), dim3(256), 0, st, e, value);
}

// the two entry points a "network vs agent" match needs, with their own argument checks: read every slot's position, apply a move
// the engine did not search
int engine_root_states72(const aqg_engine& e, uint8_t* out72, hipStream_t st) {
    const int N = e.board_size;
    if (!board_size_supported(N)) return fail("unsupported board_size");
    if (e.num_games <= 0 || !e.root_state) return fail("aqg_engine_root_states72: incomplete engine");
    hipLaunchKernelGGL(engine_root_states72_kernel, dim3((e.num_games + 255) / 256), dim3(256), 0, st, e, out72);
    return check_launch("engine_root_states72_kernel");
}

int engine_apply_actions(const aqg_engine& e, const int32_t* actions, hipStream_t st, const aqg_start_table* start) {
    if (e.num_games <= 0 || !e.root_state || !e.game_active || !e.slot_game || !e.game_plies || !e.game_result || !e.game_done ||
        !e.counters)
        return fail("aqg_engine_apply_actions: incomplete engine");
    if (e.max_plies > 0 && (!e.hist_state72 || !e.hist_visits || !e.hist_action)) return fail("aqg_engine_apply_actions: history buffers missing");
    if (e.quota < e.num_games) return fail("quota must be >= num_games");
    const dim3 grid((e.num_games + 3) / 4), block(256);
    const int launched = for_board_size(e.board_size, [&](auto n) {
        hipLaunchKernelGGL(engine_apply_actions_kernel<decltype(n)::value>, grid, block, 0, st, e, actions);
        return check_launch("engine_apply_actions_kernel");
    });
    if (launched) return launched;
    return e.quota > e.num_games ? engine_refill(e, st, start) : 0;
}

}  // namespace aqg
