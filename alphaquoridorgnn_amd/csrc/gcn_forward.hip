// gcn_forward.hip -- the front door of GraphPolicyValueNetwork.forward (hidden width 128) on 9x9 board records
// (include/aqgnn.h, aqg_gcn_forward_boards*): picks the trunk variant and its instantiation, enqueues trunk and heads through the
// launchers of the kernel files, and brackets the trunk launch with the optional profiling events.
//
//   packed weights   gcn_packed.hpp (layout), gcn_pack.hip (host packing)
//   trunk + heads    gcn_trunk_split.hip (default: fp16-split matrix pipe), gcn_trunk_exact.hip (exact f32; the range guard's fallback)
//   other sizes      gcn_boards_plain.hip (3x3 / 5x5 / 7x7) on board_featuriser.hip; any (x, edge_index, batch) graph: gcn_general.hip
//
// Also here: the LDS poisoning kernel of the parity tests.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include <vector>

namespace aqg {

// Trunk variants (aqg_set_option("trunk_variant", v)):
//   0 exact f32-input MFMA + VALU gather, weights resident, 1 workgroup/CU      1 the same, 2 workgroups/CU
//   3 all-MFMA fp16 split trunk [default] (6 = the same): 8 waves per board x 2 workgroups/CU
// (Retired: a split kernel with the VALU gather on 16-bit planes -- it read plane bytes no wave had written, see DESIGN.md section 3 --,
//  the 4-wave x 2 form, the pair form and the per-board VALU heads inside the trunk: all measured slower, all in the history.)
int g_trunk_variant = 3;

// Diagnostic: fill every CU's LDS with NaN bit patterns so that any read-before-write in a later kernel shows up
// deterministically (used by the parity tests; LDS contents are otherwise whatever the previous kernel left).
__global__ __launch_bounds__(256, 2) void poison_lds_kernel(unsigned int* sink) {
    __shared__ unsigned int buf[20000];     // 80,000 B: two workgroups per CU cover 160 KB
    for (int i = threadIdx.x; i < 20000; i += 256) buf[i] = 0xFFFFFFFFu;
    __syncthreads();
    if (sink && buf[(threadIdx.x * 77) % 20000] == 0x12345678u) sink[0] = 1;   // keep the stores alive
}
int launch_poison_lds(hipStream_t st) {
    hipLaunchKernelGGL(poison_lds_kernel, dim3(2048), dim3(256), 0, st, (unsigned int*)nullptr);
    return check_launch("poison_lds_kernel");
}

// Optional launch profiling of the dominant kernel (aqg_set_option("profile_trunk", 1)): a HIP event pair is
// recorded around every trunk launch on the launch stream; aqg_profile_collect() reads them back.
int g_profile_trunk = 0;
static std::vector<hipEvent_t> g_prof_events;
static size_t g_prof_used = 0;
static double g_prof_ms = 0.0;
static long long g_prof_launches = 0;
static long long g_prof_boards = 0;

static hipEvent_t prof_event() {
    if (g_prof_used == g_prof_events.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        g_prof_events.push_back(e);
    }
    return g_prof_events[g_prof_used++];
}

// one event on `st`; units >= 0 marks the BEGIN of a bracket and adds to the unit counter (boards / games), < 0 marks its end
void profile_mark(hipStream_t st, long long units) {
    (void)hipEventRecord(prof_event(), st);
    if (units > 0) g_prof_boards += units;
}

int profile_collect(double* total_ms, long long* launches, long long* boards, int reset) {
    if (g_prof_used) {
        for (size_t i = 0; i + 1 < g_prof_used; i += 2) {
            float ms = 0.f;
            // launches may sit on several streams (engine.MultiSetSelfPlay): wait for every pair, not just the last one
            if (hipEventSynchronize(g_prof_events[i + 1]) != hipSuccess) return fail("hipEventSynchronize");
            if (hipEventElapsedTime(&ms, g_prof_events[i], g_prof_events[i + 1]) != hipSuccess) return fail("hipEventElapsedTime");
            g_prof_ms += ms;
            ++g_prof_launches;
        }
        g_prof_used = 0;
    }
    if (total_ms) *total_ms = g_prof_ms;
    if (launches) *launches = g_prof_launches;
    if (boards) *boards = g_prof_boards;
    if (reset) { g_prof_ms = 0.0; g_prof_launches = 0; g_prof_boards = 0; }
    return 0;
}

int launch_gcn_forward_boards(int N, const void* states, int fmt, int B, const float* packed, float* pooled,
                              float* logits, float* policy, float* value_pre, float* value, const uint8_t* active,
                              int flags, int32_t* saturated, hipStream_t st, const int32_t* list, const int32_t* list_count) {
    if (N != 9) return fail("fused board trunk is built for 9x9; use aqg_gcn_forward_boards_any for other sizes");
    if (B <= 0) return 0;
    if (!pooled) return fail("pooled workspace is required");
    if (N * N + 2 * (N - 1) * (N - 1) > 248) return fail("policy size exceeds 248");
    const int A = N * N + 2 * (N - 1) * (N - 1);
    const int variant = (flags & 1) ? (g_trunk_variant == 0 ? 0 : 1) : g_trunk_variant;   // AQG_GNN_EXACT_F32
    if (g_profile_trunk == 1) { (void)hipEventRecord(prof_event(), st); g_prof_boards += B; }
    if (variant == 0 || variant == 1) {
        launch_gcn_trunk_exact(variant, states, fmt, B, packed, pooled, active, st);
    } else {
        const int track = ((flags & AQG_GNN_RANGE_PROVEN) && saturated) ? 0 : 2;
        launch_gcn_trunk_split(track, states, fmt, B, packed, pooled, active, saturated, list, list_count, st);
    }
    if (g_profile_trunk == 1) (void)hipEventRecord(prof_event(), st);
    if (int r = check_launch("gcn_trunk_boards_kernel")) return r;
    if (!logits && !policy && !value_pre && !value) return 0;   // trunk only (bench: time the dominant kernel alone)
    if (variant >= 3 && A <= 14 * 16) {
        return launch_gcn_heads_split(pooled, B, A, packed, logits, policy, value_pre, value, active, saturated, st);
    }
    return launch_gcn_heads_exact(pooled, B, A, packed, logits, policy, value_pre, value, active, st);
}

}  // namespace aqg
