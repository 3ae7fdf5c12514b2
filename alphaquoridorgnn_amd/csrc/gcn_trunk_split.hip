// gcn_trunk_split.hip -- the default trunk and heads of GraphPolicyValueNetwork.forward (pv_network_gnn.py:53-64) on 9x9 boards
// (trunk_variant 3): linear maps and neighbourhood aggregation on the 16-bit matrix pipe with every f32 operand split into two fp16
// numbers (split_mfma.hpp), fp32-equivalent, behind an fp16 range guard whose reports the host serves with the exact kernels
// (gcn_trunk_exact.hip).
//
//   trunk   gcn_trunk_boards_mm_kernel<TRACK, LIST>: one 8-wave workgroup walks boards, two workgroups per CU
//           (its body, trunk_boards_body, lives in gcn_trunk_body.hpp: the engine's evaluation launch of mcts_eval.hip runs it too)
//   heads   gcn_heads_mm_kernel: policy MLP 128->64->A (+Softmax) and value MLP 128->64->1 (+Tanh), 16 boards per workgroup
//           (its body, heads_body, lives in gcn_heads_split.hpp: the MCTS step kernel of mcts_step.hip runs it too)
//
// Both kernels log into this file's trace buffer in the -DAQG_TRACE build (kernel ids 2 and 3; aqg_common.hpp), which is why they
// share a translation unit.
#define AQG_TRACE_TU gcn
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "gcn_trunk_body.hpp"

namespace aqg {

__global__ __launch_bounds__(64 * HEADS_WAVES, 4) void gcn_heads_mm_kernel(float* __restrict__ pooled, int B, int A,
                                                                           const float* __restrict__ pk, float* __restrict__ logits,
                                                                           float* __restrict__ policy, float* __restrict__ value_pre,
                                                                           float* __restrict__ value, const uint8_t* __restrict__ active, int prio,
                                                                           int32_t* __restrict__ saturated) {
    __shared__ HeadsSmem sm;
    AQG_TRACE_BEGIN
    // a short latency chain that shares its CUs with other game sets' trunk workgroups: at a higher wave priority it is out of their
    // way sooner (option "heads_prio", 0..3)
    if (prio == 1) __builtin_amdgcn_s_setprio(1); else if (prio == 2) __builtin_amdgcn_s_setprio(2); else if (prio == 3) __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pooled, 0, B * (HID * 4), 0x00020000);
    heads_body(sm, prs, blockIdx.x * 16, B, A, packed_rsrc(pk), pk, logits, policy, value_pre, value, active, saturated, wave, lane);
    AQG_TRACE_END(3, (unsigned long long)(uintptr_t)pooled)
}

// The plain trunk launch: every workgroup walks boards (trunk_boards_body, gcn_trunk_body.hpp).
template <int TRACK, bool LIST>
__global__ __launch_bounds__(64 * NWV, 4) void gcn_trunk_boards_mm_kernel(const void* __restrict__ states, int fmt, int B, const float* __restrict__ pk,
                                                                          float* __restrict__ pooled, const uint8_t* __restrict__ active,
                                                                          int phase_delay, int32_t* __restrict__ saturated,
                                                                          const int32_t* __restrict__ list_arg, const int32_t* __restrict__ list_count) {
    AQG_TRACE_BEGIN
    __shared__ TrunkSmemM sm;
    trunk_boards_body<TRACK, LIST>(sm, blockIdx.x, gridDim.x, states, fmt, B, pk, pooled, active, phase_delay, saturated, list_arg, list_count);
    AQG_TRACE_END(2, (unsigned long long)(uintptr_t)pooled)
}


AQG_TRACE_SETTER(set_trace_gcn)

int g_heads_prio = 3;             // wave priority of the heads kernel (option "heads_prio", 0..3): round 3, same-box runs: 0 -> 1,626 / 1,641 games/s,
                                  // 1 -> 1,644 / 1,648, 2 -> 1,646, 3 -> 1,657 (profiles/r03_trunk_ab_runs.log)
int g_trunk_prio = -1;            // wave priorities (bit 0: waves 4-7, bit 1: second-resident workgroups, bit 2: first, bit 3: the two workgroups
                                  // of a CU alternate at priority 1 phase by phase); -1 = by launch size: alternation at >= 1024 boards
                                  // (+2-3 %: 45.3 M boards/s at 4,096, 47.9 M at 65,536; tools/prio_scan.py), none below (no gain at 480 and
                                  // it would outrank the other sets' step kernels: -2 % games/s)
int g_trunk_phase_delay = 100;   // x 64 cycles: start offset of the second-resident workgroups, applied to launches of
                                 // >= 8192 boards (+4-11 % there; a wash at the ~2,000-board launches of the MCTS; tools/phase_scan.py)
int g_trunk_delay_min_boards = 2048;   // launches below this many boards start all workgroups together (tools/phase_scan.py:
                                       // +4 % at 2,048 boards, +8 % at 4,096, +15-19 % from 8,192 on the three-per-CU form)
int g_trunk_grid = 0;      // 0 = default persistent grid; otherwise override (diagnostics)

// The board workgroups of a trunk launch over B boards and the kernel's option word (start offset | priorities << 16): shared with the
// engine's evaluation launch (mcts_eval.hip), whose board workgroups are launched exactly like these.
void trunk_split_launch_shape(int B, bool list, int& grid, int& opts) {
    // two 8-wave workgroups per CU (a wave owns 16 feature columns): shortest latency per board AND, with four waves per
    // SIMD to hide each other's vector work, the highest throughput at every launch size (tools/trunk_scan.py)
    grid = B < 512 ? B : 512;
    if (g_trunk_grid > 0 && g_trunk_grid < grid) grid = g_trunk_grid;
    opts = ((B >= g_trunk_delay_min_boards && !list) ? g_trunk_phase_delay : 0) |     // (a list is a fraction of B: no start offset)
           ((g_trunk_prio >= 0 ? g_trunk_prio : (B >= 1024 ? 8 : 0)) << 16);
}

// TRACK: the range guard's mode (see the kernel); a `list` selects the LIST instantiation.  Enqueue only: the caller checks the launch.
void launch_gcn_trunk_split(int track, const void* states, int fmt, int B, const float* packed, float* pooled, const uint8_t* active,
                            int32_t* saturated, const int32_t* list, const int32_t* list_count, hipStream_t st) {
    int grid, opts;
    trunk_split_launch_shape(B, list != nullptr, grid, opts);
    const dim3 tg(grid), tb(64 * NWV);
    if (track == 0) {
        if (list) hipLaunchKernelGGL((gcn_trunk_boards_mm_kernel<0, true>), tg, tb, 0, st, states, fmt, B, packed, pooled, active, opts, saturated, list, list_count);
        else hipLaunchKernelGGL((gcn_trunk_boards_mm_kernel<0, false>), tg, tb, 0, st, states, fmt, B, packed, pooled, active, opts, saturated, list, list_count);
    } else {
        if (list) hipLaunchKernelGGL((gcn_trunk_boards_mm_kernel<2, true>), tg, tb, 0, st, states, fmt, B, packed, pooled, active, opts, saturated, list, list_count);
        else hipLaunchKernelGGL((gcn_trunk_boards_mm_kernel<2, false>), tg, tb, 0, st, states, fmt, B, packed, pooled, active, opts, saturated, list, list_count);
    }
}

int launch_gcn_heads_split(float* pooled, int B, int A, const float* packed, float* logits, float* policy, float* value_pre,
                           float* value, const uint8_t* active, int32_t* saturated, hipStream_t st) {
    hipLaunchKernelGGL(gcn_heads_mm_kernel, dim3((B + 15) / 16), dim3(64 * HEADS_WAVES), 0, st, pooled, B, A, packed,
                       logits, policy, value_pre, value, active, g_heads_prio, saturated);
    return check_launch("gcn_heads_mm_kernel");
}

}  // namespace aqg
