// state_check.hip -- may a state72 record start a game?  (aqgnn.h, "start positions")
//
// The one predicate, check_record<N>, is written on the QHD functions of quoridor_core.hpp, so the kernel and aqg_host_check_state run
// the same code (as aqg_host_next runs next_state).  This is the unit that sees garbage by design: it reads bytes 0..3, the board's
// (N-1)^2 wall bytes, and bytes 68..70 of its own record and nothing else, never indexes by a record byte it has not bounded, loops
// over constants of N only and uses no atomics.  One thread per record; not on a hot path (a table is checked once, when an engine or
// a book is built).
#include "aqg_common.hpp"
#include "launchers.hpp"

namespace aqg {

template <int N> QHD uint8_t check_record(const uint8_t* r, int num_walls, int plies_for_draw) {
    constexpr int V = N * N, S = N - 1, NW = S * S;
    int flags = 0;
    const int ppos = r[0], pwl = r[1], epos = r[2], ewl = r[3];
    const int plies = (int)r[68] | ((int)r[69] << 8);
    if (r[70] != N || ppos >= V || epos >= V) flags |= AQG_CHECK_BOARD;
    // the wall bytes: a byte above 2 is no wall (and is not counted as placed); the masks hold the valid ones only
    uint64_t hw = 0, vw = 0;
    int placed = 0;
    bool bad_wall = false;
    for (int i = 0; i < NW; ++i) {
        const int b = r[4 + i];
        if (b > 2) bad_wall = true;
        else if (b == 1) { hw |= 1ull << i; ++placed; }
        else if (b == 2) { vw |= 1ull << i; ++placed; }
    }
    uint64_t col0 = 0;
    for (int sx = 0; sx < S; ++sx) col0 |= 1ull << (sx * S);
    // what can_place_wall refuses (game_logic.py:199-223): H beside H in one row of slots, V above V in one column of slots
    if (bad_wall || (hw & (hw << 1) & ~col0) != 0 || (vw & (vw << S)) != 0) flags |= AQG_CHECK_WALLS;
    if (pwl > num_walls || ewl > num_walls || pwl + ewl + placed != 2 * num_walls) flags |= AQG_CHECK_WALL_COUNT;
    if (ppos == V - 1 - epos) flags |= AQG_CHECK_SAME_SQUARE;                  // the frame change of legal_wave.hpp
    if (epos / N == 0 || ppos / N == 0 || plies >= plies_for_draw) flags |= AQG_CHECK_OVER;
    if (plies & 1) flags |= AQG_CHECK_ODD_PLY;
    if (!(flags & (AQG_CHECK_BOARD | AQG_CHECK_WALLS | AQG_CHECK_SAME_SQUARE))) {
        // both pawns are tiles of the board, on different squares, and the masks are a legal wall set: the fill's indices are in range.
        // The fill of the wall-legality search with no candidate wall and the OTHER PAWN TAKEN OFF the board (obstacle = the start tile
        // itself, which no path needs twice): a wall is legal while both jump-aware paths exist, but a pawn may later step into the
        // other's only corridor -- positions of real games (3x3: pawns on 8 and 6, walls 0 2 1 0, ply 8) have no jump-aware path for the
        // mover and must not be refused.  What the rules keep invariant is the path through the walls alone.
        const Open base = make_open<N>(hw, vw);
        const int other = V - 1 - epos;
        const bool mine = can_reach1_w3<N>(base, 0, 0, ppos, ppos, mask_row<N>(0));
        const bool theirs = can_reach1_w3<N>(base, 0, 0, other, other, mask_row<N>(N - 1));
        if (!(mine && theirs)) flags |= AQG_CHECK_NO_PATH;
    }
    return (uint8_t)flags;
}

template <int N>
__global__ __launch_bounds__(256) void states72_check_kernel(const uint8_t* __restrict__ in, int B, int num_walls, int draw,
                                                             uint8_t* __restrict__ flags) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    flags[b] = check_record<N>(in + (size_t)b * STATE72, num_walls, draw);
}

int launch_states72_check(int N, const uint8_t* in, int B, int num_walls, int draw, uint8_t* flags, hipStream_t st) {
    if (B <= 0) return 0;
    dim3 grid((B + 255) / 256), block(256);
    return for_board_size(N, [&](auto n) {
        hipLaunchKernelGGL(states72_check_kernel<decltype(n)::value>, grid, block, 0, st, in, B, num_walls, draw, flags);
        return check_launch("states72_check_kernel");
    });
}

int host_check_state(int N, const uint8_t* rec72, int num_walls, int draw) {
    return with_board_size(N, -1, [&](auto n) { return (int)check_record<decltype(n)::value>(rec72, num_walls, draw); });
}

}  // namespace aqg
