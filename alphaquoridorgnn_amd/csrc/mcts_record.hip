// mcts_record.hip -- self-play's record launch: the completed-Q improved policy of every ACTIVE slot's root, written dense by action
// id into the engine's f32 history beside hist_visits (include/aqgnn.h, "recording completed-Q targets during self-play").  The
// arithmetic is mcts_improve_row.hpp's -- the read-out's (mcts_improve.hip), in the same device function -- and the geometry the
// read-out's: one wavefront per slot, four per workgroup.  This unit alone stages a row through LDS.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "mcts_improve_row.hpp"

namespace aqg {

// The record launch (aqgnn.h, "recording completed-Q targets during self-play"): the same row, written dense by action id into the
// history row engine_finish_move_kernel is about to fill -- slot g's game k = slot_game[g] at ply = game_plies[k] -- for every ACTIVE
// slot whose ply is inside the history.  Behind the last step of the move's search and in front of the finish-move launch, on its
// stream.  The row goes through LDS, one [PASSES * 64] f32 row per wavefront (4 KB per workgroup at 9x9): zeros, the entries at their
// action ids (an id >= A is dropped; the ids of one root are distinct), then read back lane-contiguous, so every address of the row
// is stored exactly once, 64 consecutive floats per store.  The row belongs to one wavefront: wave-scope fences order the phases,
// there is no workgroup barrier and nothing is atomic.  A root without children or behind a failed guard gives the zero row.  The
// game and the ply are compared with quota and max_plies before they are used as an address; no other byte of hist_policy is touched.
template <int N>
__global__ __launch_bounds__(256) void engine_record_improved_policy_kernel(aqg_engine e, double c_visit, double c_scale,
                                                                            float* __restrict__ hist_policy) {
    constexpr int A = Geo<N>::A;
    constexpr int PASSES = (A + WAVE - 1) / WAVE;               // 1, 1, 2, 4 at 3x3 .. 9x9
    static_assert(A <= 256, "an action id is a byte");
    __shared__ float stage[4][PASSES * WAVE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * 4 + wave;
    if (g >= e.num_games || !e.game_active[g]) return;          // wave-uniform, like every return below
    const int k = e.slot_game[g];
    if (k < 0 || k >= e.quota) return;
    const int ply = e.game_plies[k];
    if (ply < 0 || ply >= e.max_plies) return;
    const ImprovedRow row = improved_policy_row(e, g, lane, c_visit, c_scale);
    float* __restrict__ mine = stage[wave];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) mine[p * WAVE + lane] = 0.0f;
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < IMP_ROUNDS; ++r)
        if (r * WAVE + lane < row.cnt && row.act[r] < (uint32_t)A) mine[row.act[r]] = row.pi[r];
    wave_lds_sync();
    float* __restrict__ out = hist_policy + ((size_t)k * e.max_plies + ply) * A;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int j = p * WAVE + lane;
        if (j < A) out[j] = mine[j];
    }
}

int launch_engine_record_improved_policy(const aqg_engine& e, const aqg_policy_record& pr, hipStream_t st) {
    return for_board_size(e.board_size, [&](auto nn) {
        hipLaunchKernelGGL((engine_record_improved_policy_kernel<decltype(nn)::value>), dim3((e.num_games + 3) / 4), dim3(256), 0, st, e,
                           pr.c_visit, pr.c_scale, pr.hist_policy);
        return 0;
    });
}

}  // namespace aqg
