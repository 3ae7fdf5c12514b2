// mcts_step.hip -- the simulation step of the engine (map: mcts.hip): step_round1, game_step_fast, engine_step_fast_kernel, the
// options that shape its launch, and launch_engine_step.  Nothing else lives here: this is the unit whose register budget
// build.sh polices, and whoever edits anything else of the engine does not recompile it.
#define AQG_TRACE_TU mcts
#include "aqg_common.hpp"
#include "legal_wave.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "gcn_heads_split.hpp"
#include <cfloat>

// PUCT scores must be evaluated exactly as written (no fma contraction, IEEE divide/sqrt).
#pragma clang fp contract(off)
#include "mcts_tree.hpp"
#include "mcts_gumbel_row.hpp"
#include <type_traits>

namespace aqg {

// Wave-wide maximum on DPP (row operations inside the SIMD) instead of ds_bpermute shuffles through the LDS crossbar: the
// step kernel is one wavefront's dependent chain, and a six-round bpermute reduction costs it more than the tree level's
// arithmetic.  Result in an SGPR (lane 63 holds the total after the row_bcast steps).
// Six v_max_f32 with DPP operands, written out: as six __builtin_amdgcn_update_dpp + fmaxf steps hipcc made v_mov_dpp + a
// canonicalising v_max + v_max of each -- 24 instructions and their wait states on the step kernel's per-level chain (that form
// is retired).  A DPP operand needs two wait states behind the VALU write of its source: s_nop 1 between the steps (nothing is
// padded inside an asm statement).
__device__ __forceinline__ float wave_max_dpp_asm(float x) {
    asm("s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(x));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
// ------------------------------------------------------------------------------------------------
// The simulation step of one game, run by one wavefront (game_step_fast).  A launch does two things:
//   expand + backup of the PREVIOUS simulation's leaf (pv_mcts.py:45-57, :59-66): the evaluator's policy is gathered at the
//             leaf's legal actions and renormalised (pv_network_cnn.py:129-132; the other evaluators deliver priors in legal
//             order), the children become contiguous NodeRecs, and every node of the old path gets w += +-value, n += 1 with the
//             sign flipping per ply (:62);
//   select    (pv_mcts.py:33-45 via next_child_node :69-78): from the root, the child with the largest PUCT score -- the first
//             one among equals, np.argmax -- until a terminal position (backed up at once, :35-42) or an unexpanded leaf, whose
//             state and legal actions are written out for the evaluator.
// The step is a latency chain of one wave, so its dependent memory rounds are cut to the minimum:
//   round 1   everything whose address follows from (game, lane) alone is requested at once: scalars, root state,
//             legal list, old path, the whole policy row, the root record AND the root's children (node 1 ...: the root
//             is expanded first in every move, so its children always start at node 1);
//   no store -> load dependency inside a launch: the previous simulation's backup and expansion are APPLIED IN
//             REGISTERS to whatever the descent loads (a child on the old path gets w += +-v, n += 1 -- the same
//             float64 addition the store performs; the old leaf's children are the records just built), and written to
//             memory behind the descent.  No value the step uses is loaded from bytes this launch has written (the old
//             leaf's new children are never read back: the descent stops there and takes their first), so every load
//             sees the state the previous launch left, whatever the timing, and the descent's only dependent rounds are
//             the child blocks of levels >= 2;
//   the policy gather at the legal actions goes through 1 KB of LDS instead of a second global round.
// Hand-over past `fast_depth` (option "step_fast_depth", 61 by default: never reached in play).  The register form keeps a
// path in the wave's lanes, so it ends before depth 63: when the old path is deeper than fast_depth, its backup is a plain
// read-modify-write through memory in front of the descent; when the new descent reaches fast_depth, the pending updates are
// flushed.  Either way a workgroup-scope release / acquire fence follows -- the wave that stored is the wave that loads --
// and from there every level reads memory, which is then current; path entries beyond depth 63 live in path[] alone.  Same
// arithmetic, same visit order on both sides of the hand-over: bit-exact with the reference traces (the tests run the
// recordings with fast_depth 0, 1, 2 and 5 to exercise every hand-over point).
// ------------------------------------------------------------------------------------------------
// Diagnostic build only (-DAQG_STAMP, tools/stamp_step.py; never shipped): lane 0 of every game adds the cycles spent in each
// phase of the step to pooled[g][2 i .. 2 i + 1] as u64 (the fake-evaluator runs the tool uses never touch `pooled`).
#ifdef AQG_STAMP
#define STEP_STAMP_DECL unsigned long long sp_prev = __builtin_readcyclecounter(), sp_loc[5] = {0, 0, 0, 0, 0};
#define STEP_STAMP(i) { const unsigned long long sp_now = __builtin_readcyclecounter(); if (lane == 0) reinterpret_cast<unsigned long long*>(e.pooled + (size_t)g * 128)[i] += sp_now - sp_prev; sp_loc[i] = sp_now - sp_prev; sp_prev = sp_now; }
#define LEVEL_STAMP(i) { const unsigned long long lv_now = __builtin_readcyclecounter(); if (lane == 0) reinterpret_cast<unsigned long long*>(e.pooled + (size_t)g * 128)[i] += lv_now - lv_prev; lv_prev = lv_now; }
#else
#define STEP_STAMP_DECL
#define STEP_STAMP(i)
#endif
constexpr int EVAL_CACHE_ROW = 704;          // f32 priors[MAX_LEGAL] + u8 actions[MAX_LEGAL], padded to 64 bytes (aqgnn.h)
static_assert(MAX_LEGAL * 5 <= EVAL_CACHE_ROW && MAX_LEGAL % 4 == 0, "evaluation cache row");
__device__ __forceinline__ uint32_t eval_cache_misc(const QState& s) {
    return (uint32_t)s.ppos | ((uint32_t)s.pwl << 8) | ((uint32_t)s.epos << 16) | ((uint32_t)s.ewl << 24);
}

int g_step_prio = 1;               // wave priority of the fast step kernel (0..3)
int g_step_waves = 8;              // games (wavefronts) per workgroup of the fast step kernel (1, 2, 4 or 8).  Round 4: 8 -- at 96 registers two step
                                   // waves per SIMD fit beside one trunk workgroup, half as many workgroups: +0.5-0.8 % games/s at 2,048 and 16,384 games
int g_step_fast_depth = 61;
int g_step_heads = 1;              // option "step_heads": 1 = the expanding step launches of the 9x9 split network compute the heads of their own leaves
                                   // (engine_step_fast_kernel<N, CACHE, true>; enqueue_sims then launches no gcn_heads_mm_kernel), 0 = three launches per simulation

// a packed 24-byte state from its three words (what load_state(base, 1, g) makes of them)
__device__ __forceinline__ QState state_of_words(uint64_t q0, uint64_t q1, uint64_t m) {
    QState s;
    s.hw = q0; s.vw = q1;
    s.ppos = (uint8_t)(m & 0xff); s.pwl = (uint8_t)((m >> 8) & 0xff);
    s.epos = (uint8_t)((m >> 16) & 0xff); s.ewl = (uint8_t)((m >> 24) & 0xff);
    s.plies = (uint16_t)((m >> 32) & 0xffff); s.pad = 0;
    return s;
}

// Round 1 of a step (see above): everything whose address follows from (game, lane) alone, requested at once.
struct StepRound1 {
    int active, flag, depth_old, cnt_new, first_new, cslot, pnode;
    float value;
    // (plain members, no arrays: the struct must dissolve into registers in every instantiation -- and every member is a loaded value AS
    //  IT ARRIVES, the packed states included: an instruction that reads one inside the loader would wait for the round right there)
    uint64_t root_q0, root_q1, root_q2, leaf_q0, leaf_q1, leaf_q2;
    uint32_t oa0, oa1, oa2;
    float polr0, polr1, polr2, polr3;
    NodeRec rootrec;
    u32x4 hot0, hot1, hot2, cold0, cold1, cold2;
};
// HEADS: the step kernel has computed the leaves' policy rows itself (they are in LDS); what is left to fetch of e.policy is the
// legal-ordered row of a leaf_flag 2 leaf (three lane rounds instead of the dense row's four)
// LEAN (the step workgroups of option "policy_beside_step", whose round 1 is in flight beside the value head's operands): without what only
// a leaf_flag 2 leaf needs -- its value, its legal-ordered row, the legal list beyond the first action; such a leaf is never seen there,
// and game_step_fast<.., PB> fetches them itself if it meets one
template <int N, bool CACHE, bool HEADS, bool LEAN = false>
__device__ __forceinline__ void step_round1(const aqg_engine& e, int g, int lane, int do_expand, StepRound1& r1) {
    constexpr int A = Geo<N>::A;
    const NodeRec* __restrict__ nodes = game_nodes(e, g);
    const int* path = e.path + (size_t)g * (e.sims + 2);
    const uint8_t* ord = e.legal_order + (size_t)g * MAX_LEGAL;
    const float* pol = e.policy + (size_t)g * A;
    r1.active = e.game_active[g];
    const uint64_t* rq = reinterpret_cast<const uint64_t*>(e.root_state) + (size_t)g * 3;
    r1.root_q0 = rq[0]; r1.root_q1 = rq[1]; r1.root_q2 = rq[2];
    int flag = 0, depth_old = 0, cnt_new = 0, first_new = 0, cslot = -1, pnode = 0;
    float value = 0.f;
    uint32_t oa[3] = {0u, 0u, 0u};
    float polr[4] = {0.f, 0.f, 0.f, 0.f};
    r1.leaf_q0 = r1.leaf_q1 = r1.leaf_q2 = 0;       // the previous simulation's leaf (its key, when its evaluation goes into the table)
    if (HEADS) {
        // (always an expanding launch.  No branch around any load -- indices are clamped, and the consumer masks what a clamped index
        //  fetched -- so that the compiler can COUNT the loads in flight: behind a divergent region its waits become s_waitcnt vmcnt(0),
        //  and the heads' policy layer in front of the step would wait for this whole round)
        flag = e.leaf_flag[g]; depth_old = e.path_len[g]; cnt_new = e.legal_count[g]; first_new = e.node_count[g];
        if (!LEAN) value = e.value[g];
        if (CACHE) {
            cslot = e.eval_cache_slot[g];
            const uint64_t* lq = reinterpret_cast<const uint64_t*>(e.leaf_state) + (size_t)g * 3;
            r1.leaf_q0 = lq[0]; r1.leaf_q1 = lq[1]; r1.leaf_q2 = lq[2];
        }
        static_assert(!HEADS || MAX_LEGAL <= A, "the legal-ordered row fits the dense one");
        static_assert(128 < MAX_LEGAL && MAX_LEGAL <= 192, "lane rounds 0 and 1 lie inside the legal list, round 2 is masked by the consumer");
        if (LEAN) oa[0] = (uint32_t)ord[lane];
        else {
#pragma unroll
            for (int r = 0; r < 3; ++r) { const int i = min(lane + 64 * r, MAX_LEGAL - 1); oa[r] = (uint32_t)ord[i]; polr[r] = pol[i]; }
        }
        pnode = path[min(lane, e.sims + 1)];
    } else if (do_expand) {
        flag = e.leaf_flag[g]; depth_old = e.path_len[g]; cnt_new = e.legal_count[g]; first_new = e.node_count[g]; value = e.value[g];
        if (CACHE) {
            cslot = e.eval_cache_slot[g];
            const uint64_t* lq = reinterpret_cast<const uint64_t*>(e.leaf_state) + (size_t)g * 3;
            r1.leaf_q0 = lq[0]; r1.leaf_q1 = lq[1]; r1.leaf_q2 = lq[2];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) { const int i = lane + 64 * r; oa[r] = (i < MAX_LEGAL) ? (uint32_t)ord[i] : 0u; }
        pnode = (lane < e.sims + 2) ? path[lane] : 0;
        if (e.prior_mode == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int a = lane + 64 * r; polr[r] = (a < A) ? pol[a] : 0.f; }
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) { const int i = lane + 64 * r; polr[r] = (i < MAX_LEGAL && i < A) ? pol[i] : 0.f; }
        }
    }
    r1.flag = flag; r1.depth_old = depth_old; r1.cnt_new = cnt_new; r1.first_new = first_new; r1.cslot = cslot; r1.pnode = pnode; r1.value = value;
    r1.oa0 = oa[0]; r1.oa1 = oa[1]; r1.oa2 = oa[2];
    r1.polr0 = polr[0]; r1.polr1 = polr[1]; r1.polr2 = polr[2]; r1.polr3 = polr[3];
    r1.rootrec = nodes[0];
    // (children travel as the record's two aligned 16-byte halves -- [2 i] = {w.lo, w.hi, p, action}, [2 i + 1] = {n, kids, q, cp} -- and
    //  stay vectors: as separate scalars their loop-carried copies were made behind an s_waitcnt at the descent loop's back edge)
    const u32x4* __restrict__ nhalf = reinterpret_cast<const u32x4*>(nodes);
    u32x4 hot[3], cold[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = min(1 + lane + 64 * r, e.node_cap - 1);
        cold[r] = nhalf[2 * i]; hot[r] = nhalf[2 * i + 1];
    }
    r1.hot0 = hot[0]; r1.hot1 = hot[1]; r1.hot2 = hot[2]; r1.cold0 = cold[0]; r1.cold1 = cold[1]; r1.cold2 = cold[2];
}

// CACHE: the evaluation cache's code is compiled in (its own kernel instantiation: the cache-less kernel carries none of it)
// HEADS: the kernel ran heads_body for the workgroup's leaves in front of this: a leaf_flag 1 leaf's softmax row is in `polbuf`
// (dense, by action), its value in `head_value`; nothing of either came through global memory
// DEFER (cache-less HEADS launches in front of engine_eval_kernel, option "legal_beside_trunk"): the new leaf's legal-move search is
// left to the evaluation launch that follows on the stream -- nothing in this launch reads its result -- and the step ends on the
// leaf's state with legal_count = -1, the marker that search looks for (leaf_legal_role, mcts_eval.hip)
// PB (cache-less HEADS launches behind engine_eval_kernel, option "policy_beside_step"): the workgroup computed the value head only, and
// the expansion of the old leaf is split with the game's policy workgroup (policy_beside_role below), which gathers the priors and
// writes the new children.  This wave keeps what the descent and the backup need: the old leaf's `kids`, node_count, and -- of the
// FIRST new child alone -- the fields w, n, kids, q: a descent that reaches the old leaf takes that child, and if its position is
// terminal this launch backs the simulation up into its record.  The policy workgroup writes that record's other fields (p, action,
// cp: disjoint bytes) and the other children's whole records, which nothing in this launch touches.  Whatever the timing of the two
// workgroups, memory ends as the one-workgroup form leaves it.  No value the step uses is loaded from those records: past the
// hand-over to memory, too, the old leaf is recognised by its node index and its first child taken without a look at the records.
// A leaf_flag 2 leaf (never seen behind an evaluation launch) has no job and is expanded here as ever.
// GUMBEL (the plain forms only; aqgnn.h, "Gumbel root search"): level 0 scores the root's children by rule 3 -- gl_i travels in their
// `cp` word, m_g and the lanes' schedule entries came with round 1 (GumbelRound1) -- and every other level is PUCT as ever.  The
// pending backup's patched neff / pqv are used exactly as PUCT uses them; nmax is one more wave maximum over neff.
struct GumbelRound1 {
    int m, vrow;                 // the slot's m_g; T[min(lane + 1, considered)][sim - 1]: row m' >= 1 sits in lane m' - 1
    float c_visit, c_scale;
    int32_t* mword;              // the slot's word (written only by the branch that cannot occur)
};
template <int N, bool CACHE, bool HEADS, bool DEFER = false, bool PB = false, bool GUMBEL = false>
__device__ __forceinline__ void game_step_fast(const aqg_engine& e, int g, int lane, int do_expand, int do_select, int fast_depth,
                                               float* __restrict__ polbuf /* this wave's 256 floats of LDS */, int list_sim,
                                               const StepRound1& r1, float head_value, const GumbelRound1& gz = GumbelRound1{}) {
    static_assert(!GUMBEL || (!HEADS && !DEFER && !PB), "Gumbel root search: the plain forms only");
    constexpr int A = Geo<N>::A;
    NodeRec* __restrict__ nodes = game_nodes(e, g);
    int* path = e.path + (size_t)g * (e.sims + 2);
    STEP_STAMP_DECL
    // ---------------- round 1 (step_round1)
    const int active = r1.active;
    const QState s_loaded = state_of_words(r1.root_q0, r1.root_q1, r1.root_q2);
    int flag = r1.flag, depth_old = r1.depth_old, cnt_new = r1.cnt_new, first_new = r1.first_new;
    float value = r1.value;
    // (HEADS: its loader clamps indices instead of branching around loads)
    uint8_t oa[3] = {(uint8_t)r1.oa0, (uint8_t)r1.oa1, (uint8_t)((HEADS && lane + 128 >= MAX_LEGAL) ? 0u : r1.oa2)};
    const int pnode = (HEADS && lane >= e.sims + 2) ? 0 : r1.pnode;
    float polr[4] = {r1.polr0, r1.polr1, r1.polr2, r1.polr3};
    // evaluation cache (aqgnn.h, ABI 10): a per-slot table of the positions this slot's games have already sent through the network
    constexpr bool cache_on = CACHE;
    int cslot = r1.cslot;
    const QState leaf_prev = (cache_on && do_expand) ? state_of_words(r1.leaf_q0, r1.leaf_q1, r1.leaf_q2) : s_loaded;
    const NodeRec rootrec = r1.rootrec;
    const u32x4* __restrict__ nhalf = reinterpret_cast<const u32x4*>(nodes);
    u32x4 hot[3] = {r1.hot0, r1.hot1, r1.hot2}, cold[3] = {r1.cold0, r1.cold1, r1.cold2};
    if (!do_expand) flag = 0;
    // (wave-uniform values the compiler cannot know to be uniform: as scalars they steer branches and v_readlane)
    flag = __builtin_amdgcn_readfirstlane(flag); depth_old = __builtin_amdgcn_readfirstlane(depth_old);
    cnt_new = __builtin_amdgcn_readfirstlane(cnt_new); first_new = __builtin_amdgcn_readfirstlane(first_new);
    // leaf_flag 2: the leaf was served from the evaluation cache -- policy[g][0 .. cnt) already holds the renormalised priors over its
    // legal actions in order (the layout of the other evaluator modes), legal_order / legal_count / value came with them
    const bool hit_old = flag == 2;
    if (hit_old) flag = 1;
    if (PB && hit_old) {             // (the lean round 1 left these out)
        const uint8_t* ord = e.legal_order + (size_t)g * MAX_LEGAL;
        const float* pol = e.policy + (size_t)g * A;
        value = e.value[g];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = min(lane + 64 * r, MAX_LEGAL - 1);
            oa[r] = (lane + 64 * r < MAX_LEGAL) ? ord[i] : (uint8_t)0;
            polr[r] = pol[i];
        }
    }
    if (HEADS && !hit_old) value = head_value;
    if (flag != 1 && !do_select) return;
#ifdef AQG_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    STEP_STAMP(0)

    // ---------------- previous simulation: priors, new children, backup deltas (registers; stores issued, nothing re-read)
    const bool expanded = flag == 1 && cnt_new > 0 && first_new + cnt_new <= e.node_cap;
    const int leaf_old = flag == 1 ? (depth_old < 64 ? __builtin_amdgcn_readlane(pnode, depth_old & 63) : path[depth_old]) : -1;
    float pl[3] = {0.f, 0.f, 0.f};
    if (flag == 1) {
        if (e.prior_mode == 0 && !hit_old) {     // P0: gather at the legal actions, divide by the sum unless 0 (pv_network_cnn.py:129-132)
            if (!HEADS) {                        // (HEADS: the row is in polbuf already, behind a workgroup barrier)
#pragma unroll
                for (int r = 0; r < 4; ++r) polbuf[lane + 64 * r] = polr[r];
                wave_lds_sync();
            }
            if (!PB) {                           // (PB: the policy workgroup's, policy_beside_role)
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int i = lane + 64 * r;
                    pl[r] = (i < cnt_new) ? polbuf[oa[r]] : 0.f;
                    sum += pl[r];
                }
                sum = wave_xor_sum(sum);
                const float den = (sum != 0.f) ? sum : 1.f;
#pragma unroll
                for (int r = 0; r < 3; ++r) pl[r] = pl[r] / den;
            }
        } else {                     // fake / external evaluator, or a leaf served from the evaluation cache: legal-ordered normalised priors
#pragma unroll
            for (int r = 0; r < 3; ++r) { const int i = lane + 64 * r; pl[r] = (i < cnt_new) ? polr[r] : 0.f; }
        }
        if (cache_on && !hit_old) {
            // this evaluation goes into the entry the select step reserved: the row first (priors + actions, defined over all
            // MAX_LEGAL places), then the key record that makes it findable.  Only this wave ever touches this slot's table.
            cslot = __builtin_amdgcn_readfirstlane(cslot);
            if (cslot >= 0) {
                const size_t ent = ((size_t)g << e.eval_cache_log2) + (size_t)cslot;
                unsigned char* row = reinterpret_cast<unsigned char*>(e.eval_cache_rows) + ent * EVAL_CACHE_ROW;
                float* rp = reinterpret_cast<float*>(row);
                uint8_t* ro = row + MAX_LEGAL * sizeof(float);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int i = lane + 64 * r;
                    if (i < MAX_LEGAL) { rp[i] = pl[r]; ro[i] = (i < cnt_new) ? oa[r] : (uint8_t)0xFF; }
                }
                if (lane == 0) {
                    const QState k = uniform_state(leaf_prev);
                    u32x4* kr = reinterpret_cast<u32x4*>(e.eval_cache_keys) + 2 * ent;
                    kr[0] = (u32x4){(uint32_t)k.hw, (uint32_t)(k.hw >> 32), (uint32_t)k.vw, (uint32_t)(k.vw >> 32)};
                    kr[1] = (u32x4){eval_cache_misc(k), 2u, (uint32_t)cnt_new, __builtin_bit_cast(uint32_t, value)};
                }
            }
        }
        if (expanded) {                  // pv_mcts.py:52-56: one child per legal action, in legal_actions() order, with its prior
            if (!PB || hit_old) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int i = lane + 64 * r;
                    if (i < cnt_new) {
                        NodeRec c;
                        c.w = 0.0; c.p = pl[r]; c.n = 0; c.kids = 0; c.action = oa[r]; c.q = 0.f; c.cp = e.c_puct * pl[r];
                        nodes[first_new + i] = c;
                    }
                }
            } else if (lane == 0) {      // the first child's statistics: this wave's (see PB above)
                NodeRec& c = nodes[first_new];
                c.w = 0.0; c.n = 0; c.kids = 0; c.q = 0.f;
            }
            if (lane == 0) {
                nodes[leaf_old].kids = (uint32_t)first_new | ((uint32_t)cnt_new << 24);
                e.node_count[g] = first_new + cnt_new;
            }
        }
        if (lane == 0) e.stat_leaf_evals[g] += 1;
    }
    const uint32_t kids_new = expanded ? ((uint32_t)first_new | ((uint32_t)cnt_new << 24)) : 0u;
    const double v_old = (double)value;                              // value.item() -> python float
    // lane d <= depth_old holds the old path node at depth d: its record after the backup (pv_mcts.py:49-50 for the leaf, :62-65 above
    // it: `value = -child.evaluate()`, so the sign flips with every ply between the node and the leaf), store pending
    double bw = 0.0; int bn = 0;
    float bq = 0.f;                   // ... and its exploitation term after the backup: ONE float64 division per step, off the
                                      // descent's per-level chain (the levels below the root read it by v_readlane)
    const bool fast_old = flag == 1 && depth_old <= fast_depth && depth_old < 63;
    if (flag == 1 && fast_old) {
        if (lane <= depth_old) {
            const NodeRec& r = nodes[pnode];
            bw = r.w + (((depth_old - lane) & 1) ? -v_old : v_old);
            bn = r.n + 1;
            bq = q_of(bw, bn);
        }
    }
    bool pending = fast_old;          // the old path's updated (w, n) are in registers, not in memory
    auto flush_old = [&]() {
        if (pending && lane <= depth_old) { NodeRec& r = nodes[pnode]; r.w = bw; r.n = bn; r.q = bq; }
        pending = false;
    };
    if (flag == 1 && !fast_old) {     // deep old path: plain read-modify-write through memory, then everything below reads memory
        if (lane <= depth_old && lane < 64) {
            NodeRec& r = nodes[pnode];
            r.w += ((depth_old - lane) & 1) ? -v_old : v_old;
            r.n += 1;
            r.q = q_of(r.w, r.n);
        }
        for (int d = lane + 64; d <= depth_old; d += 64) {
            NodeRec& r = nodes[path[d]];
            r.w += ((depth_old - d) & 1) ? -v_old : v_old;
            r.n += 1;
            r.q = q_of(r.w, r.n);
        }
    }
    if (!do_select) { flush_old(); return; }
    if (!active) { flush_old(); if (lane == 0) { e.leaf_flag[g] = 0; if (cache_on) e.eval_mask[g] = 0; } return; }
    if (lane == 0) { e.leaf_flag[g] = 0; if (cache_on) e.eval_mask[g] = 0; }
    STEP_STAMP(1)

    // ---------------- descent (pv_mcts.py:33-66 via :69-78)
    // A tree level is one dependent chain -- children arrive -> scores -> arg-max -> the chosen child's range -> next fetch -- and the
    // step kernel is one wave per SIMD, so everything that does NOT depend on the children is moved off that chain:
    //   * t = sum of the children's visit counts (pv_mcts.py:71) is the parent's own n minus one -- a node is visited once when it is
    //     expanded and once more for every descent into a child (pv_mcts.py:49-50, :62-64) -- so sqrt(t) is formed from the parent's
    //     record while the children's loads are in flight (no wave reduction, no square root behind the loads);
    //   * C_PUCT * p comes with the record (NodeRec::cp);
    //   * the pending backup patches the one child that lies on the old path with n + 1 and the q its own lane already holds; its w
    //     is never needed here: if the new path stays on the old one, lane d already owns that node's updated (w, n) -- bw, bn;
    //   * the next level's children are requested as soon as the chosen child's range is known; next() of the game state, the path
    //     bookkeeping and the chosen child's statistics follow behind the loads;
    //   * validity is a scalar mask, slots beyond the node's child count are skipped by scalar branches (no exec-mask regions), the
    //     wave maximum is six v_max_f32 with DPP operands.
    QState s = uniform_state(s_loaded);
    bool regs = true;                 // round-1 / register copies are current (false after a fall-back to memory)
    if (flag == 1 && !fast_old) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        regs = false;
    }
    int node = 0, depth = 0;
    int mynode = 0;                   // lane d: new path node at depth d ...
    double nw = 0.0; int nn = 0;      // ... and its current (w, n), pending updates included
    const bool pend0 = flag == 1 && fast_old;                        // (wave-uniform) the old path's backup is pending in registers
    if (lane == 0 && regs) { nw = pend0 ? bw : rootrec.w; nn = pend0 ? bn : rootrec.n; }
    bool onpath = pend0;              // the current node IS the old path's node at this depth
    int terminal = 0;
    double tvalue = 0.0;
    uint32_t kids = regs ? ((onpath && depth_old == 0) ? kids_new : rootrec.kids) : nodes[0].kids;
    kids = (uint32_t)__builtin_amdgcn_readfirstlane((int)kids);
    // n of the current node with the pending backup applied (lane 0 holds the root's)
    int npar = __builtin_amdgcn_readfirstlane(regs ? (pend0 ? bn : rootrec.n) : nodes[0].n);
    // One level's selection (pv_mcts.py:69-78) from the children's records `hot` / `cold`; results in the scalars below.  The records
    // are never modified in registers: the pending backup's patch goes into temporaries.
    uint32_t kids_n = 0u; int action = 0, cn = 0, besti = 0; double cw = 0.0;
    auto select_level = [&](const u32x4 (&hot)[3], const u32x4 (&cold)[3], auto root_level) {
        const int cnt = (int)(kids >> 24), first = (int)(kids & 0xFFFFFF);
        // the old path's child of this node: its index among these children, and its exploitation term after the pending backup --
        // lane depth + 1 computed it from that node's own record (one division per step, started before the descent); at the root
        // it is formed below from the round-1 copy, so that level 0 does not wait for the second load round
        const bool patch = regs && onpath && depth < depth_old;
        const int pidx = patch ? __builtin_amdgcn_readlane(pnode, (depth + 1) & 63) - first : -1;
        const float pq = (patch && depth > 0) ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bq), (depth + 1) & 63)) : 0.f;
        // f32(math.sqrt(t)) of pv_mcts.py:74, t = npar - 1 (:72): t < 2^24 is exact in f32 and the compiler's f32 square root is
        // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt, the default), and rounding sqrt to 53 bits first never changes
        // the 24-bit result (a binary64 square root cannot land within half an ulp of a binary32 midpoint unless it IS one:
        // 53 >= 2*24 + 2) -- so no f64 square root is needed on the level's chain.  The reference traces pin it.
        const float st = sqrtf((float)(npar - 1));
        // At the root the patched child's q cannot come from lane 1 (that lane's record is the second load round): it is formed from
        // the round-1 copy of the child itself -- one float64 division per step, under a scalar branch, in front of the scores
        float q0fix = 0.f;
        if (patch && depth == 0) {
            const int ps = pidx >> 6;
            const u32x4 cc = ps == 0 ? cold[0] : (ps == 1 ? cold[1] : cold[2]);
            const u32x4 hh = ps == 0 ? hot[0] : (ps == 1 ? hot[1] : hot[2]);
            const uint32_t w0 = cc[0], w1 = cc[1], nb = hh[0];
            const double wr = __builtin_bit_cast(double, ((uint64_t)w1 << 32) | w0);
            q0fix = q_of(wr + (((depth_old - 1) & 1) ? -v_old : v_old), (int)nb + 1);   // (only the lane of the patched child uses it)
        }
        const float pqv = depth == 0 ? q0fix : pq;
        const bool leafnext = patch && depth + 1 == depth_old;     // the patched child is the old leaf: it has children now
        float sc[3];
        int neff[3];
        uint32_t keff[3];
        // straight-line scores: the slots' chains (patch by selects, int -> float, multiply, IEEE division, add) are independent, so
        // that the in-order issue of a lone wave interleaves them; nodes with at most 64 children (every node once the walls are
        // placed) take the one-slot copy of the same code
        // PUCT, pv_mcts.py:74: (-w / n if n else 0.0) + C_PUCT * p * sqrt(t) / (1 + n), the exploration term left to right in f32
        auto score = [&](int r) {
            // (elements go through scalars: __builtin_bit_cast of a vector ELEMENT expression reads element 0 with hipcc 7.2)
            const uint32_t nb = hot[r][0], kb = hot[r][1], qb = hot[r][2], cb = hot[r][3];
            const bool me = patch && (lane + 64 * r == pidx);
            neff[r] = (int)nb + (me ? 1 : 0);
            keff[r] = (me && leafnext) ? kids_new : kb;
            const float q = me ? pqv : __builtin_bit_cast(float, qb);          // q = f32(-w / n) travels with the record (NodeRec::q)
            const float u = (__builtin_bit_cast(float, cb) * st) / (float)(1 + neff[r]);
            sc[r] = (lane + 64 * r < cnt) ? q + u : -INFINITY;
        };
        if constexpr (GUMBEL && decltype(root_level)::value) {
            // rule 3 of aqgnn.h: v = T[m_g][sim - 1] by v_readlane from the row the lanes loaded in round 1 (no dependent load);
            // the statistics first, then nmax over the node's children, then the scores
            const int mg = __builtin_amdgcn_readfirstlane(gz.m);
            const int v = __builtin_amdgcn_readlane(gz.vrow, (max(mg, 1) - 1) & 63);
            float gl[3], qe[3];
            auto stat = [&](int r) {
                const uint32_t nb = hot[r][0], kb = hot[r][1], qb = hot[r][2], cb = hot[r][3];
                const bool me = patch && (lane + 64 * r == pidx);
                neff[r] = (int)nb + (me ? 1 : 0);
                keff[r] = (me && leafnext) ? kids_new : kb;
                qe[r] = me ? pqv : __builtin_bit_cast(float, qb);
                gl[r] = __builtin_bit_cast(float, cb);
            };
            const int rounds = cnt <= 64 ? 1 : 3;
            float nm = 0.f;                                     // (n < 2^24: exact in f32, and rule 3 wants float(nmax))
            stat(0);
            if (rounds == 3) { stat(1); stat(2); }
            else { neff[1] = neff[2] = 0; keff[1] = keff[2] = 0u; gl[1] = gl[2] = -INFINITY; qe[1] = qe[2] = 0.f; }
#pragma unroll
            for (int r = 0; r < 3; ++r) if (r < rounds && lane + 64 * r < cnt) nm = fmaxf(nm, (float)neff[r]);
            const float nmaxf = wave_max_dpp_asm(nm);
#pragma unroll
            for (int r = 0; r < 3; ++r)
                sc[r] = (r < rounds && lane + 64 * r < cnt) ? gumbel_root_score(gl[r], neff[r], qe[r], nmaxf, gz.c_visit, gz.c_scale, v) : -INFINITY;
        } else if (cnt <= 64) {
            score(0);
            sc[1] = sc[2] = -INFINITY; neff[1] = neff[2] = 0; keff[1] = keff[2] = 0u;
        } else {
            score(0); score(1); score(2);
        }
        // np.argmax (pv_mcts.py:78): the first index of the maximum.  Wave maximum by DPP, then the lowest child index holding it from up to three
        // ballots (children lane, lane + 64, lane + 128 in that order), masked to the node's children.  NaN scores never equal the
        // maximum; if nothing matches (all NaN) child 0 is taken, as np.argmax does.
        const float best = wave_max_dpp_asm(fmaxf(fmaxf(sc[0], sc[1]), sc[2]));
        const uint64_t v0 = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull);
        const uint64_t m0 = __ballot(sc[0] == best) & v0;
        int bi = 0;
        if (m0) bi = __builtin_ctzll(m0);
        else if (cnt > 64) {
            const uint64_t v1 = cnt >= 128 ? ~0ull : ((1ull << (cnt - 64)) - 1ull);
            const uint64_t m1 = __ballot(sc[1] == best) & v1;
            if (m1) bi = 64 + __builtin_ctzll(m1);
            else if (cnt > 128) {
                const uint64_t m2 = __ballot(sc[2] == best) & ((1ull << (cnt - 128)) - 1ull);
                if (m2) bi = 128 + __builtin_ctzll(m2);
            }
        }
        besti = __builtin_amdgcn_readfirstlane(bi);
        const int slot = besti >> 6, src = besti & 63;          // wave-uniform: the winner's fields come by v_readlane
        uint32_t wlo, whi;
        auto pick = [&](const u32x4 c, uint32_t k, int n) {
            const uint32_t c0 = c[0], c1 = c[1], c3 = c[3];
            kids_n = (uint32_t)__builtin_amdgcn_readlane((int)k, src);
            action = __builtin_amdgcn_readlane((int)c3, src);
            cn = __builtin_amdgcn_readlane(n, src);
            wlo = (uint32_t)__builtin_amdgcn_readlane((int)c0, src);
            whi = (uint32_t)__builtin_amdgcn_readlane((int)c1, src);
        };
        if (slot == 0) pick(cold[0], keff[0], neff[0]); else if (slot == 1) pick(cold[1], keff[1], neff[1]); else pick(cold[2], keff[2], neff[2]);
        cw = __builtin_bit_cast(double, ((uint64_t)whi << 32) | wlo);   // (used only if the path ends on a terminal node off the old path)
        node = first + besti;
        onpath = patch && besti == pidx;                        // the new path follows the old one a level further
        // (every element of the six vectors stays allocated up to here: the record's p is never read, and the allocator handed the
        //  register of that dead element of an IN-FLIGHT load to the next temporary -- a write-after-write hazard it then covered with an
        //  s_waitcnt vmcnt(0) right behind the request)
#pragma unroll
        for (int r = 0; r < 3; ++r) asm volatile("" :: "v"(hot[r]), "v"(cold[r]));
    };
    // what stops the descent at the current node: 1 terminal, 2 unexpanded leaf, 3 the old leaf (expanded a moment ago: its children are
    // the records built above -- handled behind the loop, no record is needed there), 0 go on
    auto stop_here = [&]() -> int {
        const bool lose = is_lose<N>(s), draw = is_draw(s, e.plies_for_draw);
        if (lose || draw) { tvalue = lose ? -1.0 : 0.0; terminal = 1; return 1; }   // pv_mcts.py:35-42
        if ((kids >> 24) == 0) return 2;                                            // pv_mcts.py:45 unexpanded leaf
        if (regs && onpath && depth == depth_old) return 3;
        if (PB && !regs && node == leaf_old) return 3;                              // (PB: the new children are another workgroup's to write)
        return 0;
    };
    // Children travel as the record's two aligned 16-byte halves and are requested for all three slots whatever the child count (lanes /
    // slots beyond it read the last child, or node 0 for an unexpanded child: same cache lines, no divergent region around the loads).
    // They are loaded and consumed inside ONE loop iteration -- a loop-carried record cost a copy of every register behind an
    // s_waitcnt at the back edge -- and what the previous level's choice still owes (next() of the game state, the path, the chosen
    // child's statistics for its lane) is done between the request and the first use: behind the loads, off the level's chain.
    bool at_old_leaf = false;
#ifdef AQG_STAMP_LEVELS
    unsigned long long lv_prev = __builtin_readcyclecounter();
#endif
    int stop = stop_here();
    if (stop == 0) {
        if (!regs) {                      // (deep old path, written through memory above: the round-1 copies are stale)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int i = (int)(kids & 0xFFFFFF) + max(min(lane + 64 * r, (int)(kids >> 24) - 1), 0);
                cold[r] = nhalf[2 * i]; hot[r] = nhalf[2 * i + 1];
            }
        }
        select_level(hot, cold, std::bool_constant<GUMBEL>{});          // level 0: the root's children came with round 1
#ifdef AQG_STAMP_LEVELS
        lv_prev = __builtin_readcyclecounter();
#endif
        for (;;) {
            // next level's children (hand-over to memory first: flush what is pending, fence, go on reading memory)
            if (regs && depth + 1 >= fast_depth) {
                flush_old();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                regs = false;
                onpath = false;
            }
            // (Requesting the old path's next child block speculatively, before the scores are computed, was tried: the level
            //  got 14 % SLOWER -- a wrong guess costs a second round.)
            u32x4 h[3], c[3];
#ifdef AQG_STAMP_LEVELS
            LEVEL_STAMP(11)                                  // child chosen -> next request (hand-over test, addresses)
#endif
            {
                const int cnt = (int)(kids_n >> 24), first = (int)(kids_n & 0xFFFFFF);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int i = first + max(min(lane + 64 * r, cnt - 1), 0);
                    c[r] = nhalf[2 * i]; h[r] = nhalf[2 * i + 1];
                }
            }
            // ... and behind the loads: the chosen child becomes the current node
            ++depth;
            kids = kids_n;
            npar = cn;
            s = next_state<N>(s, action);
            // (the path stays in registers -- lane d owns depth d -- and is written once behind the descent: a store per level sat in
            //  the same in-order counter as the next level's loads.  Depths beyond 63, never seen, go through memory at once.)
            if (depth >= 64 && lane == 0) path[depth] = node;
            if (lane == (depth & 63) && depth < 64) { mynode = node; nw = onpath ? bw : cw; nn = onpath ? bn : cn; }
#ifdef AQG_STAMP
            if (lane == 0) reinterpret_cast<unsigned long long*>(e.pooled + (size_t)g * 128)[6] += 1;     // levels descended
#endif
            stop = stop_here();
            if (stop) break;
#ifdef AQG_STAMP_LEVELS
            LEVEL_STAMP(8)                                   // request -> state advanced, stop test done (work behind the loads)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            LEVEL_STAMP(9)                                   // ... -> children arrived (what is left of the load latency)
#endif
            select_level(h, c, std::false_type{});
#ifdef AQG_STAMP_LEVELS
            LEVEL_STAMP(10)                                  // ... -> child chosen (scores, arg-max, the winner's fields)
#endif
        }
    }
    at_old_leaf = stop == 3;
    if (GUMBEL && at_old_leaf && depth == 0) {
        // The root is the pending leaf: its children were written by this very launch and carry no Gumbel logits yet (their cp is
        // c_puct * p).  enqueue_sims never launches this form in front of the root launch; if somebody does, the simulation is
        // dropped and the slot's word says so (-1, aqg_engine_root_gumbel shows it; it stays -1 for the rest of the search)
        // instead of child 0 being taken without a word.  The early return leaves path[] and path_len unwritten with
        // leaf_flag = 0, and the next expanding step relies on exactly that: it reads leaf_flag first and, finding 0, neither
        // expands nor backs up, so the stale path is never followed.
        flush_old();
        if (lane == 0) gz.mword[g] = -1;
        return;
    }
    if (at_old_leaf) {
        // The descent has followed the old path down to the old leaf, whose children are the records built above (n = 0, q = 0).  Their
        // visit counts sum to t = 0, so every score is 0 + (cp * 0) / 1 = 0 (or NaN for a NaN prior: never the maximum) and np.argmax
        // takes the FIRST child (pv_mcts.py:72-78) -- no record is needed to know that, and the child is a fresh leaf
        // (or a terminal position): the descent ends one level below.
        node = (int)(kids & 0xFFFFFF);
        s = next_state<N>(s, __builtin_amdgcn_readlane((int)oa[0], 0));
        ++depth;
        if (depth >= 64 && lane == 0) path[depth] = node;
        if (lane == (depth & 63) && depth < 64) { mynode = node; nw = 0.0; nn = 0; }
        const bool lose = is_lose<N>(s), draw = is_draw(s, e.plies_for_draw);
        if (lose || draw) { tvalue = lose ? -1.0 : 0.0; terminal = 1; }
#ifdef AQG_STAMP
        if (lane == 0) reinterpret_cast<unsigned long long*>(e.pooled + (size_t)g * 128)[6] += 1;
#endif
    }
    if (lane <= min(depth, 63)) path[lane] = mynode;             // the new path, depths 0..63 (lane 0: the root, node 0)
#ifdef AQG_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    STEP_STAMP(2)
    if (terminal) {
        // backup of THIS simulation (pv_mcts.py:36-42).  Pending old-path stores go first; the new path's stores carry both
        // updates for the nodes the two paths share (same wavefront, same address: stores keep their order).
        if (regs) {
            flush_old();
            if (lane <= depth && lane < 64) {
                NodeRec& r = nodes[mynode];
                r.w = nw + (((depth - lane) & 1) ? -tvalue : tvalue);
                r.n = nn + 1;
                r.q = q_of(r.w, r.n);
            }
        } else {
            if (lane <= depth && lane < 64) {
                NodeRec& r = nodes[mynode];
                r.w += ((depth - lane) & 1) ? -tvalue : tvalue;
                r.n += 1;
                r.q = q_of(r.w, r.n);
            }
        }
        if (lane == 0) {
            e.stat_terminal_sims[g] += 1;
            for (int d = 64; d <= depth; ++d) {
                NodeRec& r = nodes[path[d]];
                r.w += ((depth - d) & 1) ? -tvalue : tvalue;
                r.n += 1;
                r.q = q_of(r.w, r.n);
            }
        }
    } else {
        flush_old();
        // Evaluation cache: has this slot asked the network for this position before?  One probe round -- lane i compares the key
        // record of table entry (home + i) -- decides; a hit copies the entry's priors, actions, count and value to where the
        // evaluator and wave_legal_actions would have put them, and the leaf is sent neither through the legal-move search nor
        // through the network (eval_mask 0).  A miss reserves the first empty entry of the window (or replaces one) for the
        // evaluation that the next step's expansion will see.
        bool hit = false;
        int newslot = -1;
        LegalPrep prep;
        if (!cache_on && !DEFER) prep = wave_legal_prepare<N>(s, lane);
        if (cache_on) {
            const uint32_t misc = eval_cache_misc(s);
            uint64_t h = s.hw * 0x9E3779B97F4A7C15ull ^ s.vw * 0xC2B2AE3D27D4EB4Full ^ (uint64_t)misc * 0x165667B19E3779F9ull;
            h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
            const uint32_t cmask = (1u << e.eval_cache_log2) - 1u, home = (uint32_t)h & cmask;
            const size_t base = (size_t)g << e.eval_cache_log2;
            const u32x4* keys = reinterpret_cast<const u32x4*>(e.eval_cache_keys) + 2 * base;
            const uint32_t idx = (home + (uint32_t)lane) & cmask;
            const u32x4 k0 = keys[2 * idx], k1 = keys[2 * idx + 1];
            // ... and while the probe is in flight: the part of legal_actions() that needs no memory (placement masks, touch-count
            // prefilter: scalar mask algebra) -- a miss has it ready, a hit has lost nothing
            prep = wave_legal_prepare<N>(s, lane);
            // (elements through scalars: __builtin_bit_cast / readlane of a vector ELEMENT expression reads element 0 with hipcc 7.2)
            const uint32_t a0 = k0[0], a1 = k0[1], a2 = k0[2], a3 = k0[3], b0 = k1[0], b1 = k1[1], b2 = k1[2], b3 = k1[3];
            const bool match = a0 == (uint32_t)s.hw && a1 == (uint32_t)(s.hw >> 32) && a2 == (uint32_t)s.vw && a3 == (uint32_t)(s.vw >> 32) &&
                               b0 == misc && b1 == 2u;
            const uint64_t mb = __ballot(match);
            if (mb) {
                hit = true;
                const int src = __builtin_ctzll(mb);
                const uint32_t hs = (home + (uint32_t)src) & cmask;
                const int cnt = __builtin_amdgcn_readlane((int)b2, src);
                const uint32_t vbits = (uint32_t)__builtin_amdgcn_readlane((int)b3, src);
                const unsigned char* row = reinterpret_cast<const unsigned char*>(e.eval_cache_rows) + (base + hs) * EVAL_CACHE_ROW;
                const float* rp = reinterpret_cast<const float*>(row);
                float* pdst = e.policy + (size_t)g * A;
#pragma unroll
                for (int r = 0; r < 3; ++r) { const int i = lane + 64 * r; if (i < cnt) pdst[i] = rp[i]; }
                if (lane < MAX_LEGAL / 4)
                    reinterpret_cast<uint32_t*>(e.legal_order + (size_t)g * MAX_LEGAL)[lane] = reinterpret_cast<const uint32_t*>(row + MAX_LEGAL * sizeof(float))[lane];
                STEP_STAMP(3)
                if (lane == 0) {
                    store_state(e.leaf_state, g, s);
                    e.legal_count[g] = cnt;
                    e.path_len[g] = depth;
                    e.value[g] = __builtin_bit_cast(float, vbits);
                    e.leaf_flag[g] = 2;
                    e.stat_cache_hits[g] += 1;
                }
            } else {
                const uint64_t eb = __ballot(b1 == 0u);
                newslot = (int)((home + (uint32_t)(eb ? __builtin_ctzll(eb) : (int)((h >> 40) & 63u))) & cmask);
            }
        }
        if (DEFER) {
            static_assert(!DEFER || !CACHE, "a cache hit supplies the legal list from the table");
            STEP_STAMP(3)
            if (lane == 0) {
                store_state(e.leaf_state, g, s);
                e.legal_count[g] = -1;
                e.path_len[g] = depth;
                e.leaf_flag[g] = 1;
            }
        } else if (!hit) {
            const int total = wave_legal_finish<N>(s, prep, lane, nullptr, e.legal_order + (size_t)g * MAX_LEGAL);
            STEP_STAMP(3)
            if (lane == 0) {
                store_state(e.leaf_state, g, s);
                e.legal_count[g] = total;
                e.path_len[g] = depth;
                e.leaf_flag[g] = 1;
                if (cache_on) {
                    e.eval_mask[g] = 1; e.eval_cache_slot[g] = newslot;
                    // large sets: the leaves the network must evaluate, as a compact list for the trunk launch of this simulation (the
                    // order of the entries is whatever order the waves arrive in -- every board's evaluation is independent of it)
                    if (list_sim >= 0) e.eval_list[atomicAdd(e.eval_count + list_sim, 1)] = g;
                }
            }
        }
    }
#ifdef AQG_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STEP_STAMP(4)
    if (lane == 0) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(e.pooled + (size_t)g * 128);
        o[7] += 1;                                                                                    // steps
        // the tail: this game's LONGEST step (a launch lasts as long as the slowest game of its set) with its phases and depth, and a
        // histogram of step lengths in 2,048-cycle buckets
        const unsigned long long tot = sp_loc[0] + sp_loc[1] + sp_loc[2] + sp_loc[3] + sp_loc[4];
        if (tot > o[16]) { o[16] = tot; for (int i = 0; i < 5; ++i) o[17 + i] = sp_loc[i]; o[22] = (unsigned long long)depth; o[23] = (unsigned long long)terminal; }
        const unsigned long long bk = tot >> 11;
        o[24 + (bk < 39 ? bk : 39)] += 1;
    }
#endif
}

// The policy workgroup of eight games (engine_step_fast_kernel<.., PB>, option "policy_beside_step"; workgroup `blk` of the launch's policy
// range, same grouping as the step workgroups): the policy half of heads_body for the games' leaves, then -- one wave per game -- the
// expansion the one-workgroup form does in game_step_fast: the gather at the legal actions, wave_xor_sum, the division, the child records,
// in the same order of operations.  Its per-game inputs are the job record the evaluation launch's search left (leaf_legal_role,
// mcts_eval.hip), legal_order[g] and the pooled row: nothing the step workgroups of this launch write.  leaf_flag, legal_count and
// node_count, which they overwrite, are not read here.  Of the first child it writes p, action and cp only (see PB above).
// Nothing waits for another workgroup; the job is cleared behind its use; counters[7] counts the jobs taken.
template <int N>
__device__ __forceinline__ void policy_beside_role(const aqg_engine& e, int blk, int wave, int lane, HeadsSmem& hsm, float (*polbuf)[256]) {
    PolicyJob* jobs = policy_jobs(e);
    const int g = blk * 8 + wave, gc = min(g, e.num_games - 1);                    // (a wave without a game loads the last game's: no branch)
    const int b0 = blk * 8, bend = min(e.num_games, b0 + 8);
    // requested in front of the heads' operands: the job and the legal list
    const PolicyJob job = jobs[gc];
    // counters[7]: the jobs taken here, one atomic per workgroup -- wave 0 counts them from loads of its own, requested with everything
    // else (every job of the workgroup is cleared behind the barriers below, not before)
    int taken = 0;
    if (wave == 0) {
        const int gi = min(b0 + (lane & 7), e.num_games - 1);
        taken = __popcll(__ballot(lane < 8 && b0 + lane < e.num_games && jobs[gi].first_new > 0));
    }
    const uint8_t* ord = e.legal_order + (size_t)gc * MAX_LEGAL;
    uint32_t oa[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) oa[r] = (uint32_t)ord[min(lane + 64 * r, MAX_LEGAL - 1)];
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(e.pooled, 0, e.num_games * (HID * 4), 0x00020000);
    heads_half<HEADS_POLICY>(hsm, prs, b0, bend, Geo<N>::A, packed_rsrc(e.packed_weights), e.packed_weights, nullptr, nullptr, nullptr, nullptr,
                                   (const PolicyJob*)jobs, e.counters + 5, wave, lane, polbuf, nullptr);
    __syncthreads();                             // the rows are complete: each wave reads its own game's
    if (wave == 0 && lane == 0 && taken) atomicAdd(e.counters + 7, taken);
    const int first_new = __builtin_amdgcn_readfirstlane(job.first_new), cnt_new = __builtin_amdgcn_readfirstlane(job.cnt);
    if (g >= e.num_games || first_new <= 0) return;
    NodeRec* __restrict__ nodes = game_nodes(e, g);
    const float* row = polbuf[wave];
    float pl[3];
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {                // P0: gather at the legal actions, divide by the sum unless 0 (pv_network_cnn.py:129-132)
        const int i = lane + 64 * r;
        pl[r] = (i < cnt_new) ? row[oa[r] & 0xFF] : 0.f;
        sum += pl[r];
    }
    sum = wave_xor_sum(sum);
    const float den = (sum != 0.f) ? sum : 1.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) pl[r] = pl[r] / den;
    if (cnt_new > 0 && first_new + cnt_new <= e.node_cap) {      // `expanded`, from the numbers the step workgroup has
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = lane + 64 * r;
            if (i < cnt_new) {
                NodeRec c;
                c.w = 0.0; c.p = pl[r]; c.n = 0; c.kids = 0; c.action = oa[r]; c.q = 0.f; c.cp = e.c_puct * pl[r];
                if (i == 0) { NodeRec& d = nodes[first_new]; d.p = c.p; d.action = c.action; d.cp = c.cp; }
                else nodes[first_new + i] = c;
            }
        }
    }
    if (lane == 0) jobs[g] = PolicyJob{0, 0};
}

// ------------------------------------------------------------------------------------------------
// fused simulation step, one wavefront per game:
//   [expand + backup of the PREVIOUS simulation's leaf]  ->  [select the next leaf + its legal actions]
// Both halves touch only this game's pools, and one wave does both, so no ordering between waves is needed.  Per simulation
// the engine then launches step -> GNN trunk -> GNN heads (3 kernels instead of select / legal / trunk / heads / expand).
// ------------------------------------------------------------------------------------------------
// HEADS (expanding launches of the 9x9 split network, eight games per workgroup; option "step_heads"): the workgroup first runs the
// network's heads (heads_body, gcn_heads_split.hpp) for the leaves of its own eight games -- boards 8 wg .. 8 wg + 7 of the pooled rows
// the trunk launch in front has written, a half-filled 16-board tile, live where leaf_flag is 1 -- and hands each game's softmax row
// and value to its wave through LDS: no heads launch, no dispatch gap in front of it, and neither row nor value travels through
// global memory.  The load rounds are ordered by what 128 registers hold: the heads' fragments and pooled rows go out at kernel entry
// (96 registers of operands), the step's own round 1 (about 50) as soon as the hidden layer's MFMAs are issued and their operands are
// dead -- it is in flight under the hidden layer's epilogue, the policy layer, the softmax and three barriers, not behind them.
// Nothing waits for another workgroup: every input was written by a launch that has finished.
// PB (cache-less HEADS launches behind engine_eval_kernel; option "policy_beside_step"): two kinds of workgroup, selected by block range
// like engine_eval_kernel's.  Workgroups [0, gridDim.x / 2) are the step's: they compute the VALUE half of the heads only -- waves 4..7
// one hidden tile each, a quarter of the operands, so the step's own round 1 is requested beside them at entry -- and leave the policy
// layer, the softmax with its barriers, the gather and the child records to workgroups [gridDim.x / 2, gridDim.x), one per eight games
// in the same grouping (policy_beside_role): nothing of that is on the way to the next leaf.  The step workgroups come first, so that
// they start at once.
// GUMBEL (aqgnn.h, "Gumbel root search"; <N, CACHE, false, false, false, GumbelStep>, the plain forms only): the launch takes the GumbelStep
// as one more argument -- the other instantiations have none, they are the kernels as they were -- and game_step_fast scores level 0 by
// rule 3.  The two words it adds to round 1 (m_g, the lane's schedule entry) have addresses that follow from (game, lane) alone.
template <int N, bool CACHE, bool HEADS, bool DEFER = false, bool PB = false, class... Gumbel>
__global__ __launch_bounds__(512, HEADS ? 4 : 1) void engine_step_fast_kernel(aqg_engine e, int do_expand, int do_select, int fast_depth, int list_sim,
                                                                              Gumbel... gumbel) {
    static_assert(!PB || (HEADS && !CACHE), "policy workgroups: the cache-less form with the heads inside");
    static_assert(sizeof...(Gumbel) == 0 || (sizeof...(Gumbel) == 1 && !HEADS && !DEFER && !PB), "Gumbel root search: the plain forms only");
    __shared__ float polbuf[8][256];
    AQG_TRACE_BEGIN
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // 1, 2, 4 or 8 games per workgroup (option "step_waves")
    // a game's wave is a latency-bound chain that issues little: at priority 1 it wins the arbitration against a co-resident trunk
    // workgroup's vector work, finishes sooner and gives its CU's second trunk slot back sooner (option "step_prio")
    { const int pr = (fast_depth >> 8) & 3; if (pr == 1) __builtin_amdgcn_s_setprio(1); else if (pr == 2) __builtin_amdgcn_s_setprio(2); else if (pr == 3) __builtin_amdgcn_s_setprio(3); }
    fast_depth &= 0xFF;
    StepRound1 r1;
    if constexpr (PB) {                          // (launched with do_expand set, eight waves and twice the step's workgroups)
        __shared__ HeadsSmem hsm;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int nstep = (int)(gridDim.x >> 1);
        if ((int)blockIdx.x >= nstep) {
            policy_beside_role<N>(e, (int)blockIdx.x - nstep, wave, lane, hsm, polbuf);
        } else {
            const int b0 = blockIdx.x * 8, bend = min(e.num_games, b0 + 8);
            const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(e.pooled, 0, e.num_games * (HID * 4), 0x00020000);
            const float hv = heads_half<HEADS_VALUE>(hsm, prs, b0, bend, Geo<N>::A, packed_rsrc(e.packed_weights), e.packed_weights, nullptr, nullptr,
                                                           nullptr, nullptr, (const uint8_t*)e.leaf_flag, nullptr, wave, lane, nullptr, nullptr,
                                                           [&]() { step_round1<N, CACHE, true, true>(e, min(g, e.num_games - 1), lane, 1, r1); });
            if (g < e.num_games) game_step_fast<N, CACHE, true, DEFER, true>(e, g, lane, do_expand, do_select, fast_depth, polbuf[wave], list_sim, r1, hv);
        }
    } else if constexpr (HEADS) {                // (launched with do_expand set and eight waves only)
        __shared__ HeadsSmem hsm;
        __shared__ float hval[16];
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int b0 = blockIdx.x * 8, bend = min(e.num_games, b0 + 8);
        const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(e.pooled, 0, e.num_games * (HID * 4), 0x00020000);
        heads_body<true>(hsm, prs, b0, bend, Geo<N>::A, packed_rsrc(e.packed_weights), e.packed_weights, nullptr, nullptr, nullptr, nullptr,
                         e.leaf_flag, e.counters + 5, wave, lane, polbuf, hval,
                         [&]() { step_round1<N, CACHE, true>(e, min(g, e.num_games - 1), lane, 1, r1); });     // (a wave without a game loads the last game's: no branch)
        __syncthreads();                         // the rows and values are complete: each wave reads its own game's
        if (g < e.num_games) game_step_fast<N, CACHE, true, DEFER>(e, g, lane, do_expand, do_select, fast_depth, polbuf[wave], list_sim, r1, hval[wave]);
    } else if (g < e.num_games) {
        step_round1<N, CACHE, false>(e, g, lane, do_expand, r1);
        if constexpr (sizeof...(Gumbel) != 0) {
            const GumbelStep gs = (gumbel, ...);
            GumbelRound1 gz;
            gz.m = gs.m[g];
            gz.vrow = gs.schedule[(size_t)min(lane + 1, gs.considered) * gs.stride + (gs.sim - 1)];
            gz.c_visit = gs.c_visit; gz.c_scale = gs.c_scale; gz.mword = gs.m;
            game_step_fast<N, CACHE, false, false, false, true>(e, g, lane, do_expand, do_select, fast_depth, polbuf[threadIdx.x >> 6], list_sim, r1, 0.f, gz);
        } else
            game_step_fast<N, CACHE, false>(e, g, lane, do_expand, do_select, fast_depth, polbuf[threadIdx.x >> 6], list_sim, r1, 0.f);
    }
    AQG_TRACE_END(1, (unsigned long long)(uintptr_t)e.pooled)
}
AQG_TRACE_SETTER(set_trace_mcts)

// One step launch; only enqueues (the caller checks the launch).  `heads`: the launch computes the heads of its leaves itself (see the
// kernel; the caller has checked that the form applies).  `list_sim` >= 0: the leaves that miss the evaluation cache are listed for
// the trunk launch of that simulation.  `defer_legal`: the caller launches engine_eval_kernel behind this step, which then leaves its
// leaves' legal-move searches to it (only the cache-less `heads` form of a selecting step does; any other form searches itself).
// `policy_beside`: the launch in front was engine_eval_kernel with the expansion jobs (the caller has checked that the form applies): the
// fused cache-less launch gets its policy workgroups behind the step's.
int launch_engine_step(const aqg_engine& e_in, int do_expand, int do_select, hipStream_t st, int list_sim, bool heads, bool defer_legal,
                       bool policy_beside, const GumbelStep* gumbel) {
    // prior_mode 3 and 4 leave the network's dense [G,A] policy in e.policy exactly like prior_mode 0: the step kernels gather,
    // renormalise and cache it as mode 0 -- they are handed the struct with prior_mode 0, so no step kernel knows mode 3 or 4
    aqg_engine e = e_in;
    if (e.prior_mode == 3 || e.prior_mode == 4) e.prior_mode = 0;
    const int wpb = (g_step_waves == 1 || g_step_waves == 2 || g_step_waves == 8) ? g_step_waves : 4;
    const int fd = g_step_fast_depth | ((g_step_prio & 3) << 8);
    const dim3 sg((e.num_games + wpb - 1) / wpb), sb(64 * wpb);
    const bool cache = e.eval_cache_keys && e.prior_mode == 0;
    if (!cache) list_sim = -1;
    return for_board_size(e.board_size, [&](auto n) {
        constexpr int N = decltype(n)::value;
        if (g_profile_trunk == 2) profile_mark(st, e.num_games);       // measurement mode 2: the event pairs bracket the step launches
        bool fused = false;
        if constexpr (N == 9) fused = heads && do_expand && wpb == 8 && e.prior_mode == 0 && !gumbel;      // (the only board with HEADS instantiations)
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, sg, sb, 0, st, e, do_expand, do_select, fd, list_sim); };
        if constexpr (N == 9) {
            if (fused) {
                if (cache) launch(engine_step_fast_kernel<N, true, true>);
                else if (policy_beside)          // (DEFER shapes the select half only: the last expansion, which selects nothing, runs the same kernel)
                    hipLaunchKernelGGL((engine_step_fast_kernel<N, false, true, true, true>), dim3(2 * sg.x), sb, 0, st, e, do_expand, do_select, fd, list_sim);
                else if (defer_legal && do_select) launch(engine_step_fast_kernel<N, false, true, true>);
                else launch(engine_step_fast_kernel<N, false, true>);
            }
        }
        if (gumbel) {                    // (the caller asks for neither `heads` nor the forms beside it: aqgnn.h, "Gumbel root search")
            if (cache) hipLaunchKernelGGL((engine_step_fast_kernel<N, true, false, false, false, GumbelStep>), sg, sb, 0, st, e, do_expand, do_select, fd, list_sim, *gumbel);
            else hipLaunchKernelGGL((engine_step_fast_kernel<N, false, false, false, false, GumbelStep>), sg, sb, 0, st, e, do_expand, do_select, fd, list_sim, *gumbel);
        } else if (!fused) { if (cache) launch(engine_step_fast_kernel<N, true, false>); else launch(engine_step_fast_kernel<N, false, false>); }
        if (g_profile_trunk == 2) profile_mark(st, -1);
        return 0;
    });
}

}  // namespace aqg
