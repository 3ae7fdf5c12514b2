// tests/hostcheck/witnesscheck.cpp -- TEST INFRASTRUCTURE ONLY (like hostcheck.cpp: the rule header compiled for the host).
//
// 1. What the wavefront's step 1 leaves to search for one position: placeable candidates that the touch-count prefilter keeps.
//    The layout tests need that count (one fill per lane at <= 32, interleaved above).
// 2. The host statement of the WITNESS-PATH FILTER, a documented experiment that does NOT ship: in front of the fills on the GPU it
//    cost every leaf more than the rounds it removed (profiles/leaf_wall_search_filter_and_lane_split_ab.log), so no
//    kernel contains it.  It is kept here, host-only, with the property that made it admissible -- it never clears a candidate
//    that the two searches reject -- checked on random play and hand-built positions (tests/test_witness_filter_cpu.py).
#include "../../alphaquoridorgnn_amd/csrc/quoridor_core.hpp"
using namespace aqg;

namespace aqg {
// ---------------------------------------------------------------------------------------------
// Witness paths: which wall candidates can NOT block a pawn, decided once per position.
// A plain path -- steps over open edges that never enter the other pawn's tile, no jumps -- is also a path of the reference's
// jump-aware search (game_logic.py:309-324 expands with legal_actions_pos: a step onto a free tile is always among them).  A
// candidate wall closes two edges; if neither lies on the path, the path survives the wall and the pawn still reaches its goal
// row, so the candidate's flood fill for this pawn would succeed.  witness_path() finds one such path by a breadth-first fill
// from `start`, walks it back from the goal row through the fill's frontiers and ORs the slots that cut one of its edges into
// cutH / cutV: edge (a, a+N) is cut by the H slots whose top-left tile is a or a-1, edge (a, a+1) by the V slots with top-left
// tile a or a-N (the geometry of add_wall).  Returns false -- masks untouched -- when no plain path exists (the other pawn plugs
// a corridor) or the path is longer than the frontiers kept: the caller then searches every candidate.
// ---------------------------------------------------------------------------------------------
constexpr int WITNESS_LAYERS = 64;
struct WitnessLayers {
    BB l[WITNESS_LAYERS];
    void put(int k, BB f) { l[k] = f; }
    BB get(int k) const { return l[k]; }
};
static inline int bb_lowest(BB x) { return x.lo ? __builtin_ctzll(x.lo) : 64 + __builtin_ctzll(x.hi); }   // x must not be empty

// tile grid (row stride N) -> slot mask (row stride S): the inverse of spread_slots, tiles outside the S x S corner dropped
template <int N> static inline uint64_t compress_slots(BB t) {
    constexpr int S = N - 1;
    uint64_t m = 0;
#pragma unroll
    for (int sx = 0; sx < S; ++sx) {
        const int off = N * sx;
        uint64_t row;
        if (off >= 64) row = t.hi >> (off - 64);
        else if (off + S > 64) row = (t.lo >> off) | (t.hi << (64 - off));
        else row = t.lo >> off;
        m |= (row & ((1ull << S) - 1)) << (S * sx);
    }
    return m;
}

template <int N> static inline bool witness_path(const Open& o, int start, int obst, int goal_row, uint64_t& cutH, uint64_t& cutV) {
    const BB goal = mask_row<N>(goal_row), notobst = ~bb_bit(obst);
    WitnessLayers L;
    BB reach = bb_bit(start), front = reach;
    int D = -1;
    for (int k = 0; k < WITNESS_LAYERS; ++k) {
        L.put(k, front);
        if (bb_any(front & goal)) { D = k; break; }
        const BB nr = (bb_shl<N>(front & o.D) | bb_shr<N>(front & o.U) | bb_shl<1>(front & o.R) | bb_shr<1>(front & o.L)) & notobst & ~reach;
        if (!bb_any(nr)) return false;
        reach = reach | nr;
        front = nr;
    }
    if (D < 0) return false;
    // walk back: a tile of frontier k has a neighbour over an open edge in frontier k-1 (open edges are symmetric)
    int t = bb_lowest(front & goal);
    BB ev = bb(0, 0), eh = bb(0, 0);                   // bit a: edge (a, a+N) / edge (a, a+1) is on the path
    for (int k = D; k > 0; --k) {
        const BB b = bb_bit(t);
        const BB nb = (bb_shl<N>(b & o.D) | bb_shr<N>(b & o.U) | bb_shl<1>(b & o.R) | bb_shr<1>(b & o.L)) & L.get(k - 1);
        const int u = bb_lowest(nb);
        const int a = u < t ? u : t, d = u < t ? t - u : u - t;
        if (d == N) ev = ev | bb_bit(a); else eh = eh | bb_bit(a);
        t = u;
    }
    // (a slot position outside the S x S corner -- column or row N-1, or a shift across a row end -- is dropped by compress_slots)
    cutH |= compress_slots<N>(ev | bb_shr<1>(ev));
    cutV |= compress_slots<N>(eh | bb_shr<N>(eh));
    return true;
}

// The filter of one position: the slots whose H / V candidate must still be searched.  Mover towards row 0 with the other pawn
// as obstacle, enemy (mover's frame) towards row N-1 with the mover as obstacle; all ones when either has no plain path.
template <int N> static inline void witness_masks(const Open& o, int me, int other, uint64_t& cutH, uint64_t& cutV) {
    uint64_t h = 0, v = 0;
    const bool ok = witness_path<N>(o, me, other, 0, h, v) && witness_path<N>(o, other, me, N - 1, h, v);
    cutH = ok ? h : ~0ull;
    cutV = ok ? v : ~0ull;
}

}  // namespace aqg

template <int N>
static int survivors(const uint8_t* rec, uint64_t* out) {
    constexpr int V = N * N;
    const QState s = unpack72(rec);
    const Open base = make_open<N>(s.hw, s.vw);
    uint64_t hp, vp, hb, vb, ch = 0, cv = 0, th = 0, tv = 0;
    placeable_masks<N>(s.hw, s.vw, hp, vp);
    possibly_blocking_masks<N>(s.hw, s.vw, hb, vb);
    const int me = s.ppos, other = V - 1 - s.epos;
    const bool pm = witness_path<N>(base, me, other, 0, th, tv);
    const bool pe = witness_path<N>(base, other, me, N - 1, th, tv);
    witness_masks<N>(base, me, other, ch, cv);
    out[0] = hp & hb; out[1] = vp & vb;           // after the prefilter: what the kernels search
    out[2] = hp & hb & ch; out[3] = vp & vb & cv; // what the witness filter would leave
    // candidates the filter clears although a search rejects them: must be none
    uint64_t bad = 0;
    for (int orient = 1; orient <= 2; ++orient) {
        const uint64_t cleared = orient == 1 ? (hp & hb & ~ch) : (vp & vb & ~cv);
        for (int pos = 0; pos < Geo<N>::NW; ++pos) {
            if (!((cleared >> pos) & 1)) continue;
            const Open o = add_wall<N>(base, orient, pos);
            if (!(can_reach<N>(o, me, other, mask_row<N>(0)) && can_reach<N>(o, other, me, mask_row<N>(N - 1)))) ++bad;
        }
    }
    out[4] = bad;
    return (pm ? 1 : 0) | (pe ? 2 : 0);           // which pawns have a plain path
}

extern "C" int wc_survivors(int N, const uint8_t* rec, uint64_t* out) {
    return with_board_size(N, -1, [&](auto n) { return survivors<decltype(n)::value>(rec, out); });
}
