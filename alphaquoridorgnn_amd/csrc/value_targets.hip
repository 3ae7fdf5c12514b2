// value_targets.hip -- self-play's value targets: the lambda-return of every finished game's recorded search values (include/aqgnn.h,
// "lambda-return value targets").  Independent of the board: the launch reads the engine's per-game words and its [quota, hp] f32
// search values through plain pointers and fills a [quota, hp] f32 tensor of the same layout.  engine.lambda_values_reference is the
// same function in numpy, bit for bit: three f32 operations per ply, each rounded, which is why the arithmetic is uncontracted.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"

#include <cstdint>

namespace aqg {

#pragma clang fp contract(off)

// Rounds of 64 plies a wavefront holds in registers at once: 256 plies, above every board's draw rule (116 at 9x9), so a row of the
// engine's is loaded whole, every round requested before the first use.  A longer row goes in chunks of this many rounds, from the
// last ply down, the chain's value carried from chunk to chunk.
constexpr int LV_ROUNDS = 4;

// One wavefront per game, four per workgroup (the read-out kernels' geometry); no LDS, no atomics, no workgroup barrier.  Game k is
// processed iff k < quota, game_done[k] != 0 and 1 <= game_plies[k] <= hp -- all wave-uniform, checked before anything forms an
// address -- and then out[k, t] is written for t < game_plies[k] and no other float.  Lane l owns the plies t with t % 64 == l: its
// loads and stores are 64 consecutive floats per round.  The recurrence G_t = a q_t + lambda (-G_{t+1}) is one wave-uniform chain
// from ply T - 1 down: q_t comes out of its owner's register by v_readlane, every lane computes the same G_t, and the owner keeps it.
// The top of the chain is the same expression with -G_T := z_{T-1}, the outcome from the last mover's side (-(float)r at an odd
// ply: a draw's -0.0f included, as the numpy statement has it).
__global__ __launch_bounds__(256) void lambda_values_kernel(int quota, int hp, const int32_t* __restrict__ game_plies,
                                                            const int8_t* __restrict__ game_result,
                                                            const uint8_t* __restrict__ game_done,
                                                            const float* __restrict__ hist_value, float lambda,
                                                            float* __restrict__ out) {
    const unsigned lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= quota || !game_done[k]) return;                    // wave-uniform, like the return below
    const int plies = game_plies[k];
    if (plies < 1 || plies > hp) return;
    const unsigned T = (unsigned)plies;
    const float a = 1.0f - lambda;
    const float r = (float)game_result[k];
    float G = ((T - 1) & 1) ? r : -r;                           // -z_{T-1}: negated once more below, which is exact
    const float* __restrict__ row = hist_value + (size_t)k * (size_t)hp;
    float* __restrict__ dst = out + (size_t)k * (size_t)hp;
    for (unsigned hi = (T + 63) >> 6; hi > 0; hi = hi > LV_ROUNDS ? hi - LV_ROUNDS : 0) {       // rounds [lo, hi) of the row
        const unsigned lo = hi > LV_ROUNDS ? hi - LV_ROUNDS : 0;
        float q[LV_ROUNDS], g[LV_ROUNDS];
#pragma unroll
        for (int c = 0; c < LV_ROUNDS; ++c) {
            const unsigned t = (lo + c) * 64 + lane;
            q[c] = (lo + c < hi && t < T) ? row[t] : 0.0f;
            g[c] = 0.0f;
        }
#pragma unroll
        for (int c = LV_ROUNDS - 1; c >= 0; --c) {
            if (lo + c >= hi) continue;
            const unsigned first = (lo + c) * 64;
            const int top = (int)(T - first < 64 ? T - first : 64);      // the round's plies: first .. first + top - 1, all < T
            for (int j = top - 1; j >= 0; --j) {
                const float qt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q[c]), j));
                const float x = a * qt;
                const float y = lambda * (-G);
                G = x + y;
                g[c] = lane == (unsigned)j ? G : g[c];
            }
        }
#pragma unroll
        for (int c = 0; c < LV_ROUNDS; ++c) {
            const unsigned t = (lo + c) * 64 + lane;
            if (lo + c < hi && t < T) dst[t] = g[c];
        }
    }
}

int launch_lambda_values(int quota, int hp, const int32_t* game_plies, const int8_t* game_result, const uint8_t* game_done,
                         const float* hist_value, float lambda, float* out, hipStream_t st) {
    if (quota < 0) return fail("aqg_lambda_values: negative quota");
    if (hp < 1) return fail("aqg_lambda_values: hp must be >= 1");
    if (!(lambda >= 0.f && lambda <= 1.f)) return fail("aqg_lambda_values: lambda must be in [0, 1]");      // NaN fails both
    if (quota == 0) return 0;               // nothing to write: the pointers are not looked at (an empty array's may be NULL)
    if (!game_plies || !game_result || !game_done || !hist_value || !out)
        return fail("aqg_lambda_values: game_plies, game_result, game_done, hist_value and out must be given");
    if (overlap(out, (size_t)quota * hp * sizeof(float), hist_value, (size_t)quota * hp * sizeof(float)))
        return fail("aqg_lambda_values: out overlaps hist_value");
    hipLaunchKernelGGL(lambda_values_kernel, dim3(((unsigned)quota + 3) / 4), dim3(256), 0, st, quota, hp, game_plies, game_result,
                       game_done, hist_value, lambda, out);
    return check_launch("lambda_values_kernel");
}

}  // namespace aqg
