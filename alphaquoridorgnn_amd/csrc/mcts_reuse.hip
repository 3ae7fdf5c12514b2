// mcts_reuse.hip -- tree reuse (aqgnn.h, "tree reuse"; map: mcts.hip): engine_keep_subtrees_kernel re-roots a slot's pool at the child
// its move chose, in place and in the old index order.  One launch per move behind engine_finish_move_kernel, outside the captured
// graph; not tuned.  One wavefront per slot, four per workgroup, no atomics, no LDS, every loop bounded by node_count[g].
//
// The kernel SWEEPS THE USED POOL; it does not walk the kept subtree.  A record does not name its parent, but a node's child block
// always lies behind the node's own block (it is allocated when the node is expanded, which is after the node exists), so one
// ascending pass from the chosen child's block on can decide every record: a record is kept iff its parent was, and its parent has
// been decided by then.  A walk of the subtree would visit the kept blocks in tree order and would then have to sort up to
// keep_visits blocks by their old position to copy them in that order -- a side table whose size the caller chooses; the sweep reads
// contiguous 2 KB per wave-instruction pair (64 records, two aligned 16-byte halves per lane: the coalesced shape) and needs no
// table at all: the mark of a kept record and, once known, its new index travel in the 24 spare bits of the record's own `action`
// word, which every writer of the pool leaves zero.  So there is one path for every pool size and nothing to fall back from.
//   pass 1, ascending, a window of 256 records per round: a kept expanded record marks its children (a one-byte store per child);
//           marks that land inside the window are picked up by re-reading the window's action words behind a fence, until a round
//           marks nothing there (at most one round per record).  A decided window's kept records get consecutive new indices.
//   pass 2, ascending: every kept record is copied to its new index with its child range renamed to the new index of the range's
//           first record.  New indices never exceed old ones and are monotone, and a window is read completely (the renaming
//           look-ups included) before it is written, so no unread record is ever overwritten.
// The chosen child becomes record 0 with a fresh root's action / p / cp; its own child block is the first one kept and lands at
// index 1, where step_round1 expects the root's children.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "mcts_tree.hpp"

namespace aqg {

typedef uint32_t rec16 __attribute__((ext_vector_type(4)));      // one aligned half of a NodeRec

constexpr int KEEP_ROUNDS = 4;                                   // lane rounds per window: 256 records
constexpr uint32_t KEEP_INDEX_SHIFT = 8;                         // action word: action | (new index + 1) << 8; 0xFF.. = marked, undecided

// the wave that stored is the wave that loads (the hand-over of mcts_step.hip)
__device__ __forceinline__ void wave_memory_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// child_index [G]: index of the chosen child in the root's child block, < 0 = do not keep.  Kept iff the slot is active, the index
// names a child, the child is expanded with its block inside the used pool, and child.n <= keep_visits.
__global__ __launch_bounds__(256) void engine_keep_subtrees_kernel(aqg_engine e, aqg_tree_reuse ru, const int32_t* __restrict__ child_index) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= e.num_games || !e.game_active[g]) return;            // inactive: pool, node_count and marker stay as they are
    NodeRec* nodes = game_nodes(e, g);                             // (the views below alias: no __restrict__)
    rec16* half = reinterpret_cast<rec16*>(nodes);
    uint32_t* words = reinterpret_cast<uint32_t*>(nodes);
    uint8_t* bytes = reinterpret_cast<uint8_t*>(nodes);
    const int count = __builtin_amdgcn_readfirstlane(min(e.node_count[g], e.node_cap));
    const int idx = __builtin_amdgcn_readfirstlane(child_index[g]);
    bool keep = idx >= 0 && count > 1;
    uint32_t ckids = 0;
    NodeRec c;
    c.w = 0.0; c.n = 0; c.q = 0.f;
    if (keep) {
        const uint32_t rkids = nodes[0].kids;
        const int rcnt = (int)(rkids >> 24), rfirst = (int)(rkids & 0xFFFFFF);
        keep = idx < rcnt && rfirst >= 1 && rfirst + rcnt <= count;
        if (keep) {
            c = nodes[rfirst + idx];
            ckids = c.kids;
            const int ccnt = (int)(ckids >> 24), cfirst = (int)(ckids & 0xFFFFFF);
            keep = ccnt > 0 && c.n <= ru.keep_visits && cfirst >= rfirst + rcnt && cfirst + ccnt <= count;
        }
    }
    keep = __builtin_amdgcn_readfirstlane(keep ? 1 : 0) != 0;
    if (!keep) {
        if (lane == 0) ru.kept[g] = 0;
        return;
    }
    ckids = (uint32_t)__builtin_amdgcn_readfirstlane((int)ckids);
    const int F = (int)(ckids & 0xFFFFFF), ccnt = (int)(ckids >> 24);

    // ---------------- pass 1: marks and new indices
    for (int j = lane; j < ccnt; j += 64) bytes[(size_t)(F + j) * 32 + 13] = 0xFF;       // the chosen child's own block
    wave_memory_handover();
    int base = 1;                                                 // next new index (0 is the new root)
    for (int b = F; b < count; b += 64 * KEEP_ROUNDS) {
        uint32_t kids[KEEP_ROUNDS], act[KEEP_ROUNDS];
        bool done[KEEP_ROUNDS];
#pragma unroll
        for (int r = 0; r < KEEP_ROUNDS; ++r) {
            const int i = b + lane + 64 * r;
            kids[r] = 0u; act[r] = 0u; done[r] = false;
            if (i < count) { kids[r] = words[(size_t)i * 8 + 5]; act[r] = words[(size_t)i * 8 + 3]; }
        }
        for (int it = 0; it <= 64 * KEEP_ROUNDS; ++it) {         // every round but the last settles at least one record of the window
            bool inside = false, any = false;
#pragma unroll
            for (int r = 0; r < KEEP_ROUNDS; ++r) {
                const bool go = (act[r] >> KEEP_INDEX_SHIFT) != 0u && !done[r] && (kids[r] >> 24) != 0u;
                uint64_t m = __ballot(go);
                done[r] = done[r] || go;
                while (m) {                                       // one kept expanded record at a time: the wave marks its children
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)kids[r], src);
                    const int first = (int)(k & 0xFFFFFF), cnt = (int)(k >> 24);
                    for (int j = lane; j < cnt; j += 64)
                        if (first + j < count) bytes[(size_t)(first + j) * 32 + 13] = 0xFF;
                    any = true;
                    inside = inside || first < b + 64 * KEEP_ROUNDS;
                }
            }
            if (any) wave_memory_handover();                      // later windows (and this one, below) load what was marked
            if (!inside) break;
#pragma unroll
            for (int r = 0; r < KEEP_ROUNDS; ++r) {
                const int i = b + lane + 64 * r;
                if (i < count) act[r] = words[(size_t)i * 8 + 3];
            }
        }
#pragma unroll
        for (int r = 0; r < KEEP_ROUNDS; ++r) {
            const int i = b + lane + 64 * r;
            const bool marked = (act[r] >> KEEP_INDEX_SHIFT) != 0u;
            const uint64_t m = __ballot(marked);
            const int rank = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (marked && i < count) words[(size_t)i * 8 + 3] = (act[r] & 0xFFu) | ((uint32_t)(rank + 1) << KEEP_INDEX_SHIFT);
            base += __builtin_popcountll(m);
        }
    }
    wave_memory_handover();

    // ---------------- pass 2: copy forward, child ranges renamed
    for (int b = F; b < count; b += 64 * KEEP_ROUNDS) {
        rec16 cold[KEEP_ROUNDS], hot[KEEP_ROUNDS];
        uint32_t nfw[KEEP_ROUNDS];
#pragma unroll
        for (int r = 0; r < KEEP_ROUNDS; ++r) {
            const int i = min(b + lane + 64 * r, count - 1);
            cold[r] = half[2 * (size_t)i]; hot[r] = half[2 * (size_t)i + 1];
        }
#pragma unroll
        for (int r = 0; r < KEEP_ROUNDS; ++r) {                   // the new index of each child range's first record
            const uint32_t k = hot[r][1];
            const int fo = min((int)(k & 0xFFFFFF), count - 1);
            nfw[r] = words[(size_t)fo * 8 + 3];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the window is read, look-ups included, before it is written
#pragma unroll
        for (int r = 0; r < KEEP_ROUNDS; ++r) {
            const int i = b + lane + 64 * r;
            const uint32_t a = cold[r][3], k = hot[r][1];
            if (i < count && (a >> KEEP_INDEX_SHIFT) != 0u) {
                const int ni = (int)(a >> KEEP_INDEX_SHIFT) - 1;
                if (ni > i) continue;                             // (never in a pool the engine built: a new index does not exceed the old one)
                rec16 co = cold[r], ho = hot[r];
                co[3] = a & 0xFFu;
                ho[1] = (k >> 24) ? (((nfw[r] >> KEEP_INDEX_SHIFT) - 1u) & 0xFFFFFFu) | (k & 0xFF000000u) : 0u;
                half[2 * (size_t)ni] = co; half[2 * (size_t)ni + 1] = ho;
            }
        }
    }
    if (lane == 0) {
        NodeRec root;
        root.w = c.w; root.p = 0.f; root.action = 0xFF; root.n = c.n; root.kids = 1u | ((uint32_t)ccnt << 24); root.q = c.q; root.cp = 0.f;
        nodes[0] = root;
        e.node_count[g] = base;
        ru.kept[g] = 1;
        ru.stat_moves_kept[g] += 1;
        ru.stat_visits_kept[g] += c.n;
    }
}

void launch_engine_keep_subtrees(const aqg_engine& e, const aqg_tree_reuse& ru, const int32_t* child_index, hipStream_t st) {
    hipLaunchKernelGGL(engine_keep_subtrees_kernel, dim3((e.num_games + 3) / 4), dim3(256), 0, st, e, ru, child_index);
}

}  // namespace aqg
