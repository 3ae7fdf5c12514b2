// mcts.hip -- K4: batched lock-step PV-MCTS + self-play move loop for gfx950.
//
// Semantics reproduced per game (exactly, given the same evaluator outputs and uniforms):
//   pv_mcts.py:20-95   Node/evaluate/next_child_node/pv_mcts_policy   (C_PUCT 1.25, first-max argmax,
//                      float32 PUCT arithmetic under NumPy-2 promotion, float64 w accumulators)
//   self_play.py:40-68 play(): record (state, visit distribution), sample like np.random.choice, next(), z.
//
// Layout: one 64-lane wavefront per game.  A game's tree is a flat pool of 32-byte reference-"Node" records
// (w, p, n, first-child|count, action); children of a node are contiguous, in State.legal_actions() order,
// so the PUCT arg-max is a strided wave reduction and "first maximum wins" is (max score, min index).
// Child STATES are never stored: the descent re-applies next() from the root's 24-byte packed state, so
// a node costs 32 bytes instead of the reference's full State copy.
// One simulation = fused step kernel (expand/backup of the previous leaf, select, legal actions of the new leaf)
// -> GNN trunk -> GNN heads on the leaf batch;
// every game has exactly one leaf in flight, so no virtual loss is needed and per-game semantics equal the
// sequential reference.
//
// Map of the engine's files:
//   mcts_tree.hpp   NodeRec (the 32-byte node record), q_of, game_nodes, backup_path, the wave sums, initial_state: what the two
//                   device units share.  Device code and declarations only.
//   mcts_step.hip   the simulation step and nothing else: step_round1, game_step_fast, engine_step_fast_kernel, the options
//                   step_waves / step_prio / step_fast_depth / step_heads, set_trace_mcts, launch_engine_step.  The tuned unit: build.sh
//                   polices its register budget.
//   mcts_eval.hip   the evaluation launch behind a step that defers its leaves' legal-move searches: leaf_legal_role, engine_eval_kernel (search
//                   workgroups in front of the trunk's board workgroups), the option legal_beside_trunk, launch_engine_eval.
//   mcts_move.hip   once per move or once per engine: reset, set_roots, begin_move, the `fake` evaluator, root noise, finish_move and
//                   apply_actions (one engine_transition behind both), refill, root_visits / root_priors / root_states72; one plain
//                   launcher per kernel.
//   mcts_gumbel.hip the Gumbel root search outside the step kernel: engine_gumbel_root_kernel (Gumbel logits into the root's children, m_g),
//                   engine_finish_move_gumbel_kernel (the survivor is played), engine_root_gumbel_kernel (read-out); the shared score is
//                   mcts_gumbel_row.hpp's, which the step kernel's GUMBEL instantiations evaluate at level 0.
//   mcts_reuse.hip  tree reuse: engine_keep_subtrees_kernel, the in-place re-rooting of a pool at the chosen child, and its launcher.
//   mcts_improve.hip  the completed-Q improved policy of the roots: engine_root_improved_policy_kernel, a read-out of the pool in
//                   float64 (aqgnn.h, "completed-Q policy targets"), and its launcher.  It changes nothing the search reads.
//   mcts_record.hip   the same rows recorded during self-play: engine_record_improved_policy_kernel writes them dense by action id
//                   into the f32 history, between a move's search and its finish-move launch; the arithmetic of both units is
//                   mcts_improve_row.hpp's.
//   mcts.hip        this file, host code only: validate and validate_move (every refusal of a move, in one order), the simulation loop
//                   (enqueue_sims), its hipGraph cache (run_sims), the end of a move (finish_and_refill) and the engine_* entry points:
//                   engine_move and engine_finish_move take the move's options as one MoveOptions value (launchers.hpp).  It launches
//                   no kernel itself.
#include "aqg_common.hpp"
#include <vector>
#include <cmath>
#include <cstring>
#include "../../include/aqgnn.h"
#include "launchers.hpp"

namespace aqg {

int g_use_graph = 1;       // aqg_set_option("use_graph", 0) forces plain launches

// ------------------------------------------------------------------------------------------------
// host-side enqueue (no sync, no allocation)
// ------------------------------------------------------------------------------------------------
// The temperature a move can sample at (aqgnn.h, `temperature`): finite and >= 0, and when > 0 small enough an exponent that every
// term n ** (1 / T) of boltzman (pv_mcts.py:106-109), n <= `visits`, is below 2^1016 -- the sum of at most AQG_MAX_LEGAL < 2^8 of them
// is then finite.  The reference raises for a negative one (0 ** negative) and for a too small one (OverflowError); the kernel would
// form inf / inf and play child 0 without a word.
static int validate_temperature(float temperature, long long visits) {
    if (!(temperature >= 0.f) || std::isinf(temperature)) return fail("temperature must be finite and >= 0");      // NaN fails the first
    if (temperature > 0.f && !(std::log2((double)visits) / (double)temperature <= 1016.0))
        return fail("temperature is too small for sims (+ keep_visits): log2(visits) / temperature must be <= 1016");
    return 0;
}

static int validate(const aqg_engine& e) {
    const int N = e.board_size;
    if (!board_size_supported(N)) return fail("unsupported board_size");
    if (e.num_games <= 0 || e.sims <= 0) return fail("num_games and sims must be positive");
    if (int r = validate_temperature(e.temperature, e.sims)) return r;
    if ((long long)e.node_cap >= (1 << 24)) return fail("node_cap must be < 2^24");
    if (e.node_cap < 1 + MAX_LEGAL) return fail("node_cap too small");
    if (e.prior_mode == 0 && N != 9 && !e.gnn_workspace) return fail("boards other than 9x9 need gnn_workspace for the GNN evaluator");
    if (e.prior_mode < 0 || e.prior_mode > 4) return fail("prior_mode must be 0, 1, 2, 3 or 4");
    if (e.prior_mode == 4) {
        const char* why = "";
        if (check_cnn_net(&e.cnn_net, N, &why)) return fail("prior_mode 4 needs a complete cnn_net", why);
        if (e.cnn_net.policy_size != N * N + 2 * (N - 1) * (N - 1)) return fail("prior_mode 4: cnn_net.policy_size must be the board's action count");
        if (!e.gnn_workspace) return fail("prior_mode 4 needs gnn_workspace (aqg_cnn_workspace_floats)");
    }
    if (e.prior_mode == 3) {
        const char* why = "";
        if (check_general_net(&e.general_net, &why)) return fail("prior_mode 3 needs a complete general_net", why);
        if (e.general_net.policy_size != N * N + 2 * (N - 1) * (N - 1)) return fail("prior_mode 3: general_net.policy_size must be the board's action count");
        if (!e.gnn_workspace) return fail("prior_mode 3 needs gnn_workspace (aqg_gcn_boards_general_workspace_floats)");
    }
    if (e.quota < e.num_games) return fail("quota must be >= num_games");
    if (!e.slot_game || !e.game_done || !e.game_slot || !e.game_first_move) return fail("slot_game / game_done / game_slot / game_first_move are required");
    if (e.eval_cache_keys) {
        if (e.prior_mode != 0 && e.prior_mode != 3 && e.prior_mode != 4) return fail("the evaluation cache serves the network evaluators only (prior_mode 0, 3 or 4)");
        if (!e.eval_cache_rows || !e.eval_cache_slot || !e.eval_mask || !e.stat_cache_hits) return fail("eval_cache_rows / eval_cache_slot / eval_mask / stat_cache_hits are required with eval_cache_keys");
        if ((e.eval_list == nullptr) != (e.eval_count == nullptr)) return fail("eval_list and eval_count come together");
        if (e.eval_cache_log2 < 6 || e.eval_cache_log2 > 20) return fail("eval_cache_log2 must be 6..20");
    }
    if (!(e.root_noise_eps >= 0.f && e.root_noise_eps < 1.f)) return fail("root_noise_eps must be in [0, 1)");
    if (e.root_noise_eps > 0.f && !(e.root_noise_alpha > 0.f && e.root_noise_alpha <= 100.f)) return fail("root_noise_alpha must be in (0, 100]");
    return 0;
}

// what the tree-reuse entry points refuse, before anything is launched (aqgnn.h, "tree reuse")
static int validate_reuse(const aqg_engine& e, const aqg_tree_reuse& ru) {
    if (ru.keep_visits < 0) return fail("tree reuse: keep_visits must be >= 0");
    if ((long long)ru.keep_visits + e.sims > 32767) return fail("tree reuse: keep_visits + sims must be <= 32767 (the visit row is read out as int16)");
    if (int r = validate_temperature(e.temperature, (long long)ru.keep_visits + e.sims)) return r;
    if ((long long)e.node_cap < 1 + ((long long)ru.keep_visits + e.sims) * MAX_LEGAL) return fail("tree reuse: node_cap must be >= 1 + (keep_visits + sims) * AQG_MAX_LEGAL");
    if (e.prior_mode == 2) return fail("tree reuse: not with prior_mode 2 (the external evaluator)");
    if (!ru.kept || !ru.child_index || !ru.stat_moves_kept || !ru.stat_visits_kept) return fail("tree reuse: kept / child_index / stat_moves_kept / stat_visits_kept are required");
    return 0;
}

// what the resignation entry points refuse, before anything is launched (aqgnn.h, "resignation")
static int validate_resign(const aqg_engine& e, const aqg_resign& rs) {
    if (!(rs.threshold > 0.f && rs.threshold <= 1.f)) return fail("resignation: threshold must be in (0, 1]");
    if (rs.min_ply < 0) return fail("resignation: min_ply must be >= 0");
    if (!(rs.disable_fraction >= 0.0 && rs.disable_fraction <= 1.0)) return fail("resignation: disable_fraction must be in [0, 1]");
    if (!rs.resign_min || !rs.game_resigned) return fail("resignation: resign_min / game_resigned are required");
    if (e.max_plies <= 0) return fail("resignation needs a history (max_plies > 0)");
    return 0;
}

// what the policy-record entry points refuse, before anything is launched (aqgnn.h, "recording completed-Q targets during self-play")
static int validate_policy_record(const aqg_engine& e, const aqg_policy_record& pr) {
    if (!pr.hist_policy) return fail("policy record: hist_policy is required");
    if (e.max_plies <= 0) return fail("policy record needs a history (max_plies > 0)");
    if (!(pr.c_visit >= 0.0) || std::isinf(pr.c_visit)) return fail("policy record: c_visit must be finite and >= 0");      // NaN fails the first
    if (!(pr.c_scale >= 0.0) || std::isinf(pr.c_scale)) return fail("policy record: c_scale must be finite and >= 0");
    return 0;
}

// what the start-position entry points refuse, before anything is launched (aqgnn.h, "start positions"): the rows and the index are
// device memory and were checked by the caller (aqg_states72_check; index[k] in [0, count)) -- the kernels fall back to the opening record
// on a row number outside the table
int validate_start_table(const aqg_engine& e, const aqg_start_table* start, const char* what) {
    (void)e;
    if (!start) return 0;
    if (!start->states72) return fail(what, "states72 is required");
    if (start->count <= 0) return fail(what, "count must be >= 1");
    return 0;
}

// what the Gumbel entry points refuse, before anything is launched and in this order (aqgnn.h, "Gumbel root search")
static int validate_gumbel(const aqg_engine& e, const MoveOptions& o) {
    const aqg_gumbel& gb = *o.gumbel;
    if (e.sims < 2) return fail("Gumbel root search: sims must be >= 2 (simulation 0 evaluates the root)");
    if (gb.considered < 1 || gb.considered > 64) return fail("Gumbel root search: considered must be in 1..64");
    if (!(gb.scale >= 0.0) || std::isinf(gb.scale)) return fail("Gumbel root search: scale must be finite and >= 0");      // NaN fails the first
    if (e.root_noise_eps > 0.f) return fail("Gumbel root search: not with root noise (the Gumbel variates are the exploration)");
    if (o.reuse) return fail("Gumbel root search: not with tree reuse (a kept root's children hold no Gumbel logits)");
    if (o.resign) return fail("Gumbel root search: not with resignation");
    if (o.temperature_plies > 0) return fail("Gumbel root search: not with temperature_plies (the move is the survivor, no temperature is read)");
    if (e.prior_mode == 2) return fail("Gumbel root search: not with prior_mode 2 (the external evaluator)");
    if (!(gb.c_visit >= 0.f) || std::isinf(gb.c_visit)) return fail("Gumbel root search: c_visit must be finite and >= 0");
    if (!(gb.c_scale >= 0.f) || std::isinf(gb.c_scale)) return fail("Gumbel root search: c_scale must be finite and >= 0");
    if (!gb.schedule || !gb.m) return fail("Gumbel root search: schedule and m are required");
    return 0;
}

// Everything a move refuses, before anything is launched.  The order is part of the interface -- the first failing check names the
// error: the engine, the Gumbel root search if it is on, the two targets, tree reuse if it is on, resignation if it is on, the
// policy record if it is on.
static int validate_move(const aqg_engine& e, const MoveOptions& o) {
    if (int r = validate(e)) return r;
    if (o.gumbel) if (int r = validate_gumbel(e, o)) return r;
    if (o.temperature_plies < 0) return fail("temperature_plies must be >= 0");
    if (o.hist_value && e.max_plies <= 0) return fail("hist_value needs a history (max_plies > 0)");
    if (o.reuse) if (int r = validate_reuse(e, *o.reuse)) return r;
    if (o.resign) if (int r = validate_resign(e, *o.resign)) return r;
    if (o.policy) if (int r = validate_policy_record(e, *o.policy)) return r;
    if (o.start) if (int r = validate_start_table(e, o.start, "start positions")) return r;
    return 0;
}

// `reuse` != nullptr (tree reuse, aqgnn.h): begin_move leaves the marked slots' pools alone, a kept root's noise is mixed into its
// children in front of simulation 0's step, and the step launches get `es`, the struct with sims = keep_visits + sims: the stride of
// e.path and the bound of the path lanes, which is all the step kernel reads `sims` for.  Every other reader of `sims` -- begin_move's
// eval_count, this loop, list_sim -- sees the real count.
// `gumbel` != nullptr (Gumbel root search, aqgnn.h): the three-launch simulation form around the root launch -- step(0, 1), evaluate;
// step(1, 0), the root's expansion and backup in memory; the root launch; then per simulation step<GUMBEL>, evaluate; the last
// expansion.  Two launches more per move than the three-launch PUCT form; no step_heads, no legal_beside_trunk, no policy_beside_step.
static int enqueue_sims(const aqg_engine& e, hipStream_t st, const aqg_tree_reuse* reuse = nullptr, const aqg_gumbel* gumbel = nullptr) {
    if (e.prior_mode == 2) return fail("prior_mode 2 (external evaluator): drive the move with aqg_engine_begin_move / _step / _finish_move");
    const int N = e.board_size;
    aqg_engine es = e;
    if (reuse) es.sims = e.sims + reuse->keep_visits;
    launch_engine_begin_move(e, st, reuse ? reuse->kept : nullptr);
    if (reuse && e.root_noise_eps > 0.f) launch_engine_kept_root_noise(e, reuse->kept, st);
    // evaluation cache on a set larger than the trunk's grid: the leaves that miss the cache go to the trunk as a compact list
    const bool use_list = e.prior_mode == 0 && e.eval_cache_keys && e.eval_list && N == 9 && e.num_games > 512 && g_trunk_variant >= 3 && !(e.gnn_flags & AQG_GNN_EXACT_F32);
    // heads inside the step (option "step_heads"): the 9x9 split network with eight games per step workgroup -- the NEXT step launch
    // computes policy and value of this simulation's leaves from the pooled rows, so the simulation is two launches, step -> trunk.
    // Everything else keeps the heads launch: other boards and evaluators, step_waves != 8, the exact kernels behind a range-guard report.
    const bool step_heads = !gumbel && g_step_heads && e.prior_mode == 0 && N == 9 && g_trunk_variant >= 3 && !(e.gnn_flags & AQG_GNN_EXACT_F32) && g_step_waves == 8;
    // legal moves beside the trunk (option "legal_beside_trunk"; cache off): such a step ends on its leaf, and the evaluation launch behind
    // it carries the leaves' legal-move searches in front of the trunk's board workgroups (mcts_eval.hip) -- still two launches, one chain.
    // Simulation 0's step does not expand, so it is not the form with the heads inside: it searches itself and the plain trunk follows.
    const bool defer_legal = engine_step_defers_legal(e, step_heads);
    // the policy head beside the step (option "policy_beside_step"): every evaluation launch leaves its marked leaves' expansion jobs, and
    // the step launch behind it -- simulations 2 .. sims - 1 and the last expansion -- expands them in policy workgroups beside its step
    // workgroups.  Simulation 1's step follows the plain trunk and searched its leaf (the root) itself: no job, today's form.
    const bool policy_beside = engine_policy_beside_step(e, defer_legal);
    // the evaluation of simulation `sim`'s leaves, behind its step launch
    auto evaluate = [&](int sim, bool defer) -> int {
        if (defer) {
            if (int r = launch_engine_eval(e, st, policy_beside)) return r;
        } else if (e.prior_mode == 0) {
            // (simulation 0 -- the root's evaluation -- keeps its heads launch: root noise reads the root's row and value from e.policy /
            //  e.value, and without noise the launch is there only so that these buffers hold the root's evaluation after a search, as
            //  they always did after a one-simulation search (tests/test_gpu_parity.py::test_engine_masked_trunk_launch reads them).
            //  Simulation 1's step computes the same heads again from the same pooled rows -- equal results; 1 launch in `sims`.)
            const bool heads_launch = !step_heads || sim == 0;
            // 9x9: the fused trunk; smaller boards: plain kernels over e.gnn_workspace
            if (int r = launch_gcn_forward_boards_any(N, e.leaf_state, 1, e.num_games, e.packed_weights, e.gnn_workspace,
                                                      e.gnn_workspace ? boards_any_workspace_floats(N, e.num_games) : 0, e.pooled, nullptr,
                                                      heads_launch ? e.policy : nullptr, nullptr, heads_launch ? e.value : nullptr,
                                                      e.eval_cache_keys ? e.eval_mask : e.leaf_flag, e.gnn_flags, e.counters + 5, st,
                                                      use_list ? e.eval_list : nullptr, use_list ? e.eval_count + sim : nullptr))
                return r;
        } else if (e.prior_mode == 3) {
            // the any-shape network: featuriser, one fused launch per GCN layer, heads -- all over e.gnn_workspace
            if (int r = launch_gcn_forward_boards_general(N, e.leaf_state, 1, e.num_games, &e.general_net,
                                                          e.eval_cache_keys ? e.eval_mask : e.leaf_flag, e.gnn_workspace,
                                                          boards_general_workspace_floats(N, e.general_net.hidden, e.general_net.policy_size,
                                                                                          e.num_games),
                                                          nullptr, nullptr, e.policy, nullptr, e.value, st))
                return r;
        } else if (e.prior_mode == 4) {
            // the residual CNN: featuriser, one implicit-GEMM launch per conv, heads -- all over e.gnn_workspace
            if (int r = launch_cnn_forward_boards(N, e.leaf_state, 1, e.num_games, &e.cnn_net, e.eval_cache_keys ? e.eval_mask : e.leaf_flag,
                                                  e.gnn_workspace,
                                                  cnn_workspace_floats(N, e.cnn_net.num_filters, e.cnn_net.policy_size, e.num_games),
                                                  nullptr, nullptr, e.policy, nullptr, e.value, st))
                return r;
        } else {
            if (int r = launch_engine_fake_eval(e, st)) return r;
        }
        return 0;
    };
    if (gumbel) {
        GumbelStep gs{gumbel->schedule, gumbel->m, gumbel->c_visit, gumbel->c_scale, gumbel->considered, e.sims - 1, 0};
        if (int r = launch_engine_step(es, 0, 1, st, use_list ? 0 : -1, false)) return r;
        if (int r = evaluate(0, false)) return r;
        if (int r = launch_engine_step(es, 1, 0, st, -1, false)) return r;           // the root's expansion and backup, in memory
        launch_engine_gumbel_root(e, *gumbel, st);
        for (int sim = 1; sim < e.sims; ++sim) {
            gs.sim = sim;
            if (int r = launch_engine_step(es, sim > 1 ? 1 : 0, 1, st, use_list ? sim : -1, false, false, false, &gs)) return r;
            if (int r = evaluate(sim, false)) return r;
        }
        if (int r = launch_engine_step(es, 1, 0, st, -1, false)) return r;
        return check_launch("engine simulation kernels");
    }
    for (int sim = 0; sim < e.sims; ++sim) {
        const bool defer = defer_legal && sim > 0;
        if (int r = launch_engine_step(es, sim > 0 ? 1 : 0, 1, st, use_list ? sim : -1, step_heads, defer, policy_beside && sim > 1)) return r;
        if (int r = evaluate(sim, defer)) return r;
        if (sim == 0 && e.root_noise_eps > 0.f)                                    // the root's priors, before simulation 1 expands it
            if (int r = launch_engine_root_noise(e, st)) return r;
    }
    if (int r = launch_engine_step(es, 1, 0, st, -1, step_heads, false, policy_beside && e.sims > 1)) return r;  // expand + backup of the last simulation
    return check_launch("engine simulation kernels");
}

// One move's search is 3 * sims + 2 launches (2 * sims + 3 with the heads inside the step; one more with root noise on, and with tree reuse a second one for the kept roots;
// 3 * sims + 4 with the Gumbel root search: the three-launch form, the root's own step(1, 0) and the root launch) with constant arguments: on a capturable (non-default) stream it is
// captured once into a hipGraph and replayed per move, so the host cost per move is one graph launch instead of ~600
// kernel launches (with several game sets on several streams the host is otherwise the bottleneck).  The cache key is
// the engine struct itself plus the trunk options the launches read.
// (Host entry points are called from one host thread per process, like the reference's single-threaded loop; the cache
// below and the library's other host-side globals are not synchronised.)
struct SimGraph {
    aqg_engine e;
    int opts[7];
    const uint8_t* kept;      // tree reuse: the two arguments its captured launches bake in (nullptr, 0 = a plain move)
    int keep_visits;
    bool has_gumbel;          // Gumbel root search: the struct its captured launches bake in, field by field (padding is not compared)
    aqg_gumbel gumbel;
    hipGraphExec_t exec;
    hipEvent_t last;          // recorded behind every replay: eviction waits for THIS graph's last replay, not for the device
};
static std::vector<SimGraph> g_sim_graphs;
constexpr size_t SIM_GRAPH_CACHE = 64;   // engines x game sets that can alternate without re-capturing (4 sets per engine: 16 engines)

static int replay(SimGraph& g, hipStream_t st) {
    if (hipGraphLaunch(g.exec, st) != hipSuccess) return fail("hipGraphLaunch");
    if (hipEventRecord(g.last, st) != hipSuccess) return fail("hipEventRecord");
    return 0;
}

static bool same_gumbel(const SimGraph& g, const aqg_gumbel* gb) {
    if (g.has_gumbel != (gb != nullptr)) return false;
    if (!gb) return true;
    const aqg_gumbel& a = g.gumbel;
    return a.table == gb->table && a.seed == gb->seed && !memcmp(&a.scale, &gb->scale, sizeof(double)) && a.considered == gb->considered &&
           !memcmp(&a.c_visit, &gb->c_visit, sizeof(float)) && !memcmp(&a.c_scale, &gb->c_scale, sizeof(float)) && a.schedule == gb->schedule && a.m == gb->m;
}

static int run_sims(const aqg_engine& e, hipStream_t st, const aqg_tree_reuse* reuse = nullptr, const aqg_gumbel* gumbel = nullptr) {
    if (!g_use_graph || g_profile_trunk || st == nullptr || e.sims < 4) return enqueue_sims(e, st, reuse, gumbel);
    const uint8_t* kept = reuse ? reuse->kept : nullptr;
    const int keep_visits = reuse ? reuse->keep_visits : 0;
    // every option a captured launch bakes in is part of the key: a changed option must never replay a stale graph
    const int opts[7] = {g_trunk_variant, g_trunk_grid, g_trunk_phase_delay, g_trunk_delay_min_boards, e.board_size, g_step_fast_depth, ((g_trunk_prio & 0xff) << 8) | (g_step_waves << 16) | (g_step_prio << 24) | (g_heads_prio << 28) | (g_step_heads & 1) | ((g_legal_beside_trunk & 1) << 1) | ((g_policy_beside_step & 1) << 2)};
    for (SimGraph& g : g_sim_graphs)
        if (!memcmp(&g.e, &e, sizeof(aqg_engine)) && !memcmp(g.opts, opts, sizeof(opts)) && g.kept == kept && g.keep_visits == keep_visits && same_gumbel(g, gumbel)) return replay(g, st);
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return enqueue_sims(e, st, reuse, gumbel);           // stream not capturable: plain launches
    }
    const int r = enqueue_sims(e, st, reuse, gumbel);
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(st, &graph);
    if (r) { if (graph) (void)hipGraphDestroy(graph); return r; }
    if (ec != hipSuccess || !graph) return fail("hipStreamEndCapture");
    SimGraph g;
    memcpy(&g.e, &e, sizeof(aqg_engine));
    memcpy(g.opts, opts, sizeof(opts));
    g.kept = kept; g.keep_visits = keep_visits;
    g.has_gumbel = gumbel != nullptr;
    g.gumbel = gumbel ? *gumbel : aqg_gumbel{};
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) return fail("hipGraphInstantiate");
    if (hipEventCreateWithFlags(&g.last, hipEventDisableTiming) != hipSuccess) { (void)hipGraphExecDestroy(g.exec); return fail("hipEventCreate"); }
    if (g_sim_graphs.size() >= SIM_GRAPH_CACHE) {            // FIFO: engines come and go
        SimGraph& old = g_sim_graphs.front();
        (void)hipEventSynchronize(old.last);                 // its last replay may still be running on ANOTHER stream: wait for that
        (void)hipGraphExecDestroy(old.exec);                 // replay only -- the other game sets' streams keep running
        (void)hipEventDestroy(old.last);
        g_sim_graphs.erase(g_sim_graphs.begin());
    }
    g_sim_graphs.push_back(g);
    return replay(g_sim_graphs.back(), st);
}

// the end of a move: choose and apply (finish_move), then hand the idle slots their next games (refill) while a quota is left to play
// (outside the captured graph, so the two target options are plain kernel arguments: 0 / nullptr = off)
// (tree reuse: finish_move leaves the chosen child's index, the keep launch re-roots the pools of the games that go on -- in front of the
//  refill, whose new games start in slots that are inactive here and therefore never marked)
// (resignation: the option is the finish-move launch's last argument; a resigned slot is inactive behind it, like any finished one)
// (policy record: one launch in front of the finish-move launch, which still sees the slot active and its ply unchanged)
static int finish_and_refill(const aqg_engine& e, const double* uniforms, const MoveOptions& o, hipStream_t st) {
    if (o.policy) if (int r = launch_engine_record_improved_policy(e, *o.policy, st)) return r;
    if (o.gumbel) { if (int r = launch_engine_finish_move_gumbel(e, o, st)) return r; }      // (rule 4: no uniform is read)
    else if (int r = launch_engine_finish_move(e, uniforms, o, st)) return r;
    if (o.reuse) launch_engine_keep_subtrees(e, *o.reuse, o.reuse->child_index, st);
    if (e.quota > e.num_games) launch_engine_refill(e, st, o.start);
    return check_launch("engine_finish_move_kernel");
}

// External-evaluator mode (prior_mode 2): the caller runs the simulation loop itself -- begin, then per simulation
// step(expand the previous leaf, select the next) -> its OWN evaluator fills policy[g][0 .. legal_count[g]) (a PMF over
// legal_actions() in order, the BaseNetwork.predict contract BaseNetwork.py:36-40) and value[g] for every game with
// leaf_flag[g] == 1 -> ... -> step(expand, no select) -> finish.  Same kernels, same per-game semantics; the library
// merely launches no evaluator between the steps.
int engine_begin_move(const aqg_engine& e, hipStream_t st) {
    if (int r = validate(e)) return r;
    launch_engine_begin_move(e, st);
    return check_launch("engine_begin_move_kernel");
}

int engine_step(const aqg_engine& e, int do_expand, int do_select, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (int r = launch_engine_step(e, do_expand, do_select, st, -1, false)) return r;
    return check_launch("engine_step_fast_kernel");
}

int engine_finish_move(const aqg_engine& e, const double* uniforms, const MoveOptions& o, hipStream_t st) {
    if (int r = validate_move(e, o)) return r;
    return finish_and_refill(e, uniforms, o, st);
}

int engine_clear_eval_cache(const aqg_engine& e, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (!e.eval_cache_keys) return 0;
    if (hipMemsetAsync(e.eval_cache_keys, 0, ((size_t)e.num_games << e.eval_cache_log2) * 32, st) != hipSuccess) return fail("hipMemsetAsync(eval_cache_keys)");
    return 0;
}

int engine_reset(const aqg_engine& e, hipStream_t st, const aqg_start_table* start) {
    if (int r = validate(e)) return r;
    if (int r = validate_start_table(e, start, "aqg_engine_reset_start")) return r;
    if (int r = engine_clear_eval_cache(e, st)) return r;
    launch_engine_reset(e, st, start);
    return check_launch("engine_reset_kernel");
}

int engine_move(const aqg_engine& e, const double* uniforms, const MoveOptions& o, hipStream_t st) {
    if (int r = validate_move(e, o)) return r;
    if (int r = run_sims(e, st, o.reuse, o.gumbel)) return r;
    return finish_and_refill(e, uniforms, o, st);
}

int engine_keep_subtrees(const aqg_engine& e, const aqg_tree_reuse& ru, const int32_t* child_index, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (int r = validate_reuse(e, ru)) return r;
    launch_engine_keep_subtrees(e, ru, child_index, st);
    return check_launch("engine_keep_subtrees_kernel");
}

int engine_reset_reuse(const aqg_engine& e, const aqg_tree_reuse& ru, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (int r = validate_reuse(e, ru)) return r;
    if (hipMemsetAsync(ru.kept, 0, (size_t)e.num_games, st) != hipSuccess) return fail("hipMemsetAsync(kept)");
    return 0;
}

int engine_reset_resign(const aqg_engine& e, const aqg_resign& rs, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (int r = validate_resign(e, rs)) return r;
    if (hipMemsetD32Async((hipDeviceptr_t)rs.resign_min, 0x7F800000, (size_t)e.quota * 2, st) != hipSuccess) return fail("hipMemsetD32Async(resign_min)");      // +inf
    if (hipMemsetAsync(rs.game_resigned, 0, (size_t)e.quota, st) != hipSuccess) return fail("hipMemsetAsync(game_resigned)");
    return 0;
}

int engine_set_roots(const aqg_engine& e, const uint8_t* roots72, hipStream_t st) {
    if (int r = validate(e)) return r;
    launch_engine_set_roots(e, roots72, st);
    return check_launch("engine_set_roots_kernel");
}

int engine_search(const aqg_engine& e, const uint8_t* roots72, hipStream_t st) {
    if (int r = validate(e)) return r;
    launch_engine_set_roots(e, roots72, st);
    return run_sims(e, st);
}

// the Gumbel root search without a move (aqgnn.h, "Gumbel root search"): the search of caller-given roots, the root launch alone and
// the read-out.  Each refuses what a move with the option refuses.
static int validate_gumbel_alone(const aqg_engine& e, const aqg_gumbel& gb) {
    if (int r = validate(e)) return r;
    MoveOptions o{};
    o.gumbel = &gb;
    return validate_gumbel(e, o);
}

int engine_search_gumbel(const aqg_engine& e, const uint8_t* roots72, const aqg_gumbel& gb, hipStream_t st) {
    if (int r = validate_gumbel_alone(e, gb)) return r;
    launch_engine_set_roots(e, roots72, st);
    return run_sims(e, st, nullptr, &gb);
}

int engine_gumbel_root(const aqg_engine& e, const aqg_gumbel& gb, hipStream_t st) {
    if (int r = validate_gumbel_alone(e, gb)) return r;
    launch_engine_gumbel_root(e, gb, st);
    return check_launch("engine_gumbel_root_kernel");
}

int engine_root_gumbel(const aqg_engine& e, const aqg_gumbel& gb, float* gl, int32_t* m, int32_t* winner, hipStream_t st) {
    if (int r = validate_gumbel_alone(e, gb)) return r;
    launch_engine_root_gumbel(e, gb, gl, m, winner, st);
    return check_launch("engine_root_gumbel_kernel");
}

// the noise launch alone: behind the caller's own evaluation of simulation 0 (prior_mode 2), and for tests
int engine_root_noise(const aqg_engine& e, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (!(e.root_noise_eps > 0.f)) return 0;
    if (int r = launch_engine_root_noise(e, st)) return r;
    return check_launch("engine_root_noise_kernel");
}

int engine_root_priors(const aqg_engine& e, float* priors, int32_t* count, hipStream_t st) {
    if (int r = validate(e)) return r;
    launch_engine_root_priors(e, priors, count, st);
    return check_launch("engine_root_priors_kernel");
}

int engine_root_values(const aqg_engine& e, float* value, hipStream_t st) {
    if (int r = validate(e)) return r;
    launch_engine_root_values(e, value, st);
    return check_launch("engine_root_values_kernel");
}

// the completed-Q improved policy of the roots (mcts_improve.hip): the constants are refused here, before the launch
int engine_root_improved_policy(const aqg_engine& e, double c_visit, double c_scale, float* policy, uint8_t* actions, int32_t* count,
                                float* vmix, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (!(c_visit >= 0.0) || std::isinf(c_visit)) return fail("aqg_engine_root_improved_policy: c_visit must be finite and >= 0");      // NaN fails the first
    if (!(c_scale >= 0.0) || std::isinf(c_scale)) return fail("aqg_engine_root_improved_policy: c_scale must be finite and >= 0");
    launch_engine_root_improved_policy(e, c_visit, c_scale, policy, actions, count, vmix, st);
    return check_launch("engine_root_improved_policy_kernel");
}

// the record launch alone (mcts_record.hip), for the tests: what a move with the option refuses, then the one launch
int engine_record_improved_policy(const aqg_engine& e, const aqg_policy_record& pr, hipStream_t st) {
    if (int r = validate(e)) return r;
    if (int r = validate_policy_record(e, pr)) return r;
    if (int r = launch_engine_record_improved_policy(e, pr, st)) return r;
    return check_launch("engine_record_improved_policy_kernel");
}

// the slot refill alone, for a move that was applied rather than searched (engine_apply_actions, mcts_move.hip)
int engine_refill(const aqg_engine& e, hipStream_t st, const aqg_start_table* start) {
    launch_engine_refill(e, st, start);
    return check_launch("engine_refill_kernel");
}

int engine_root_visits(const aqg_engine& e, int32_t* visits, uint8_t* actions, int32_t* count, hipStream_t st) {
    if (int r = launch_engine_root_visits(e, visits, actions, count, st)) return r;
    return check_launch("engine_root_visits_kernel");
}

}  // namespace aqg
