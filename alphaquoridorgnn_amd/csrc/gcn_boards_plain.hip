// gcn_boards_plain.hip -- GraphPolicyValueNetwork.forward (hidden width 128) on boards of 3x3 / 5x5 / 7x7 from the packed weight
// buffer (include/aqgnn.h, aqg_gcn_forward_boards_any); 9x9 goes to the fused trunks through launch_gcn_forward_boards.
//
//   featuriser   boards_prep_kernel (board_featuriser.hip): x0 [B*V, 6] + the normalised wall-cut grid as ELL rows of 5
//   3 layers     graph_linear_kernel, then ell_gather_kernel (+ bias + ReLU); board_pool_kernel after the third
//   heads        gcn_heads_kernel (gcn_trunk_exact.hip)
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "gcn_packed.hpp"

namespace aqg {

// ---------------------------------------------------------------------------------------------
// the VALU linear map of the any-size board path below
// ---------------------------------------------------------------------------------------------
// Y[n][HID] = X[n][K] * WT[K][HID]   (WT row stride ldw; K = 6 (padded rows of W1 read as [n][f]) or 128)
template <bool W_IS_NF>
__global__ __launch_bounds__(256) void graph_linear_kernel(const float* __restrict__ X, int K, int num_nodes,
                                                           const float* __restrict__ W, float* __restrict__ Y) {
    __shared__ float xs[32][HID + 1];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * 32;
    for (int i = tid; i < 32 * K; i += 256) {
        const int r = i / K, k = i % K;
        xs[r][k] = (n0 + r < num_nodes) ? X[(size_t)(n0 + r) * K + k] : 0.f;
    }
    __syncthreads();
    const int col = tid & 127, half = tid >> 7;   // 16 nodes per thread
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k = 0; k < K; ++k) {
        const float w = W_IS_NF ? W[col * FPAD + k] : W[(size_t)k * HID + col];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fmaf(xs[16 * half + i][k], w, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = n0 + 16 * half + i;
        if (n < num_nodes) Y[(size_t)n * HID + col] = acc[i];
    }
}

// ---------------------------------------------------------------------------------------------
// boards of ANY size (3x3 .. 9x9) on plain kernels: the fused trunks (gcn_trunk_split.hip, gcn_trunk_exact.hip) are specialised
// for the 9x9 board of the benchmark; smaller boards (the reference's constants.py:5-20 debugging sizes) go records -> node features + normalised
// adjacency in ELL form (<= 5 entries per node) -> 3 x (linear, ELL gather + bias + ReLU) -> mean pool -> exact heads.
// Correctness-first, fp32 throughout.  Workspace (caller-owned): 272 floats per node.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ell_gather_kernel(const float* __restrict__ Y, int num_nodes, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= num_nodes) return;
    float a0 = bias[2 * lane], a1 = bias[2 * lane + 1];
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        const int j = idx[(size_t)n * 5 + e];
        if (j >= 0) {
            const float we = w[(size_t)n * 5 + e];
            const float2 y = *reinterpret_cast<const float2*>(Y + (size_t)j * HID + 2 * lane);
            a0 = fmaf(we, y.x, a0);
            a1 = fmaf(we, y.y, a1);
        }
    }
    *reinterpret_cast<float2*>(out + (size_t)n * HID + 2 * lane) = make_float2(fmaxf(a0, 0.f), fmaxf(a1, 0.f));
}

// (`active`: the engine's leaf mask, as in the heads -- a masked-out board's pooled row is left as it was)
__global__ __launch_bounds__(128) void board_pool_kernel(const float* __restrict__ Hn, int V, const uint8_t* __restrict__ active,
                                                         float* __restrict__ pooled) {
    const int b = blockIdx.x;
    if (active && !active[b]) return;
    float s = 0.f;
    for (int i = 0; i < V; ++i) s += Hn[((size_t)b * V + i) * HID + threadIdx.x];
    pooled[(size_t)b * HID + threadIdx.x] = s / (float)V;
}

size_t boards_any_workspace_floats(int N, int B) { return (size_t)B * N * N * 272; }

int launch_gcn_forward_boards_any(int N, const void* states, int fmt, int B, const float* packed, float* workspace,
                                  size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre,
                                  float* value, const uint8_t* active, int flags, int32_t* saturated, hipStream_t st,
                                  const int32_t* list, const int32_t* list_count) {
    // (`list`: see gcn_trunk_boards_mm_kernel; honoured by the 9x9 split trunk only -- every other path walks the mask, which must agree)
    if (N == 9) return launch_gcn_forward_boards(N, states, fmt, B, packed, pooled, logits, policy, value_pre, value, active, flags, saturated, st, list, list_count);
    if (!(N == 3 || N == 5 || N == 7)) return fail("board_size must be 3, 5, 7 or 9");
    if (B <= 0) return 0;
    if (!pooled) return fail("pooled workspace is required");
    if (!workspace || workspace_floats < boards_any_workspace_floats(N, B)) return fail("workspace too small (272 floats per node)");
    const int V = N * N, R = B * V, A = V + 2 * (N - 1) * (N - 1);
    float* x0 = workspace;
    float* ell_w = x0 + (size_t)R * 6;
    int32_t* ell_idx = reinterpret_cast<int32_t*>(ell_w + (size_t)R * 5);
    float* work0 = reinterpret_cast<float*>(ell_idx + (size_t)R * 5);
    float* work1 = work0 + (size_t)R * HID;
    const dim3 lg((R + 31) / 32), gg((R + 3) / 4), blk(256);
    if (int r = launch_gcn_boards_graph(N, states, fmt, B, x0, ell_idx, ell_w, st)) return r;
    hipLaunchKernelGGL(graph_linear_kernel<true>, lg, blk, 0, st, (const float*)x0, 6, R, packed + PackedLayout::W1, work0);
    hipLaunchKernelGGL(ell_gather_kernel, gg, blk, 0, st, (const float*)work0, R, (const int32_t*)ell_idx, (const float*)ell_w, packed + PackedLayout::B1, work1);
    hipLaunchKernelGGL(graph_linear_kernel<false>, lg, blk, 0, st, (const float*)work1, HID, R, packed + PackedLayout::W2T, work0);
    hipLaunchKernelGGL(ell_gather_kernel, gg, blk, 0, st, (const float*)work0, R, (const int32_t*)ell_idx, (const float*)ell_w, packed + PackedLayout::B2, work1);
    hipLaunchKernelGGL(graph_linear_kernel<false>, lg, blk, 0, st, (const float*)work1, HID, R, packed + PackedLayout::W3T, work0);
    hipLaunchKernelGGL(ell_gather_kernel, gg, blk, 0, st, (const float*)work0, R, (const int32_t*)ell_idx, (const float*)ell_w, packed + PackedLayout::B3, work1);
    hipLaunchKernelGGL(board_pool_kernel, dim3(B), dim3(128), 0, st, (const float*)work1, V, active, pooled);
    if (int r = check_launch("generic board kernels")) return r;
    if (!logits && !policy && !value_pre && !value) return 0;
    return launch_gcn_heads_exact(pooled, B, A, packed, logits, policy, value_pre, value, active, st);
}

}  // namespace aqg
