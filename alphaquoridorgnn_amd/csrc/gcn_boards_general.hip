// gcn_boards_general.hip -- GraphPolicyValueNetwork of ANY shape on board records (include/aqgnn.h, aqg_gcn_forward_boards_general):
// the forward the engine's prior_mode 3 enqueues per simulation, and forward_states of a non-default shape.
//
//   featuriser   boards_prep_kernel (board_featuriser.hip): x0 [B*V, 6] + the normalised wall-cut grid as ELL rows of 5
//   L layers     board_gcn_layer_kernel: H_out = relu(A_hat (H_in W^T) + b), one launch per layer; the last one writes the mean pool
//   heads        gen_linear x 4 and gen_heads (gcn_general.hip)
//
// Every number equals the width-generic composition gen_linear -> gen_aggregate (-> gen_pool) bit for bit: the linear map runs the
// same f32-input MFMA over the same zero-padded K slabs of 32 (a k-ordered fmaf chain), the stencil starts from the bias and takes
// the ELL entries in stored order with fmaf, and the pool sums the rows in ascending order before one division by V.  What the
// fusion removes is the [B*V, N] round trip of Y through HBM between the two launches.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"

namespace aqg {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int S = 36;      // LDS row stride of the K slabs (gen_linear's: the 16 rows x 4 k of a fragment fall on 64 distinct banks)
constexpr int YS = 68;     // LDS row stride of the Y tile: an MFMA result's 4 rows x 16 columns fall on 64 distinct banks

// One workgroup (4 waves) per (board b, 64 output columns n0 ..).  The board's V rows (padded to RT tiles of 16) and the 64 weight
// rows are staged in K slabs of 32; wave w owns output columns [16 w, 16 w + 16) for all RT row tiles.  Y = X W^T stays in LDS;
// then lane l of wave w applies the 5-point stencil to column l for rows w, w + 4, ...  With `pooled` the layer's output is not
// stored: its rows go back to LDS (over the dead K slabs) and pooled[b] = (sum of the V rows in order) / V.
// A board with active[b] != 1 is skipped whole (no loads, no stores).
template <int N, bool VEC>
__global__ __launch_bounds__(256) void board_gcn_layer_kernel(int K, int Nout, const float* __restrict__ X, const float* __restrict__ W,
                                                              const float* __restrict__ bias, const int32_t* __restrict__ ell_idx,
                                                              const float* __restrict__ ell_w, const uint8_t* __restrict__ active,
                                                              float* __restrict__ H, float* __restrict__ pooled) {
    constexpr int V = N * N, RT = (V + 15) / 16, RP = 16 * RT;
    static_assert((RP + 64) * S >= V * 64, "the pooled rows must fit over the K slabs");
    __shared__ alignas(16) float slab[(RP + 64) * S];   // xs [RP][S] then ws [64][S]; after the K loop: the output rows [V][64]
    __shared__ alignas(16) float ys[RP * YS];
    __shared__ int32_t li[V * 5];
    __shared__ float lw[V * 5];
    float* const xs = slab;
    float* const ws = slab + RP * S;
    const int b = blockIdx.x, n0 = blockIdx.y * 64;
    if (active && active[b] != 1) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const size_t r0 = (size_t)b * V;
    // this board's ELL rows with board-local ids (the featuriser only links tiles of the same board; anything else is skipped)
    for (int i = tid; i < V * 5; i += 256) {
        const int s = ell_idx[r0 * 5 + i];
        const int l = s - b * V;
        li[i] = (s >= 0 && l >= 0 && l < V) ? l : -1;
        lw[i] = ell_w[r0 * 5 + i];
    }
    f32x4 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 32) {
        __syncthreads();
        if constexpr (VEC) {            // K % 4 == 0, X and W 16-byte aligned: a 4-float group is wholly inside or outside K
            for (int idx = tid; idx < RP * 8; idx += 256) {
                const int r = idx >> 3, k = 4 * (idx & 7);
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (r < V && k0 + k < K) v = *reinterpret_cast<const f32x4*>(X + (r0 + r) * K + k0 + k);
                *reinterpret_cast<f32x4*>(xs + r * S + k) = v;
            }
            for (int idx = tid; idx < 64 * 8; idx += 256) {
                const int j = idx >> 3, k = 4 * (idx & 7);
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (n0 + j < Nout && k0 + k < K) v = *reinterpret_cast<const f32x4*>(W + (size_t)(n0 + j) * K + k0 + k);
                *reinterpret_cast<f32x4*>(ws + j * S + k) = v;
            }
        } else {
            for (int idx = tid; idx < RP * 32; idx += 256) {
                const int r = idx >> 5, k = idx & 31;
                xs[r * S + k] = (r < V && k0 + k < K) ? X[(r0 + r) * K + k0 + k] : 0.f;
            }
            for (int idx = tid; idx < 64 * 32; idx += 256) {
                const int j = idx >> 5, k = idx & 31;
                ws[j * S + k] = (n0 + j < Nout && k0 + k < K) ? W[(size_t)(n0 + j) * K + k0 + k] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < 32; kk += 4) {
            const float bw = ws[(16 * w + c) * S + kk + q];
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[t] = mfma4(xs[(16 * t + c) * S + kk + q], bw, acc[t]);
        }
    }
    // Y = X W^T + 0 (gen_linear adds its absent bias as +0.f, which turns a -0 into +0: so does this)
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) ys[(16 * t + 4 * q + i) * YS + 16 * w + c] = acc[t][i] + 0.f;   // C/D: row 4 q + i, col c
    __syncthreads();
    const int n = n0 + lane;
    const bool nok = n < Nout;
    const float bn = (bias && nok) ? bias[n] : 0.f;
    float* const hs = slab;                       // pooled layer: the output rows [V][64] over the dead K slabs
    for (int r = w; r < V; r += 4) {
        float a = bn;
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            const int s = li[r * 5 + e];
            if (s < 0) continue;
            a = fmaf(lw[r * 5 + e], ys[s * YS + lane], a);
        }
        a = fmaxf(a, 0.f);
        if (pooled) hs[r * 64 + lane] = a;
        else if (nok) H[(r0 + r) * Nout + n] = a;
    }
    if (!pooled) return;
    __syncthreads();
    if (w == 0 && nok) {
        float s = 0.f;
        for (int r = 0; r < V; ++r) s += hs[r * 64 + lane];
        pooled[(size_t)b * Nout + n] = s / (float)V;
    }
}

inline size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }

struct GeneralWorkspace {
    float* x0; float* ell_w; int32_t* ell_idx; float* h[2]; float* pooled; float* hp; float* hv; float* logits; float* vpre;
};

// floats of each region, every one rounded up to 64 (256 bytes: the vector loads need 16-byte alignment)
inline size_t general_layout(int N, int hidden, int A, int B, GeneralWorkspace* ws, float* base) {
    const size_t R = (size_t)B * N * N, Hh = (size_t)(hidden / 2);
    const size_t sz[10] = {R * 6, R * 5, R * 5, R * hidden, R * hidden, (size_t)B * hidden, (size_t)B * Hh, (size_t)B * Hh,
                           (size_t)B * A, (size_t)B};
    size_t off[10], total = 0;
    for (int i = 0; i < 10; ++i) { off[i] = total; total += round64(sz[i]); }
    if (ws && base) {
        ws->x0 = base + off[0]; ws->ell_w = base + off[1]; ws->ell_idx = reinterpret_cast<int32_t*>(base + off[2]);
        ws->h[0] = base + off[3]; ws->h[1] = base + off[4]; ws->pooled = base + off[5]; ws->hp = base + off[6]; ws->hv = base + off[7];
        ws->logits = base + off[8]; ws->vpre = base + off[9];
    }
    return total;
}

template <int N>
int launch_layer_n(int B, int K, int Nout, const float* X, const float* W, const float* bias, const int32_t* ell_idx,
                   const float* ell_w, const uint8_t* active, float* H, float* pooled, hipStream_t st) {
    const dim3 grid(B, (Nout + 63) / 64), blk(256);
    const bool vec = K % 4 == 0 && (((uintptr_t)X | (uintptr_t)W) & 15) == 0;
    if (vec) hipLaunchKernelGGL((board_gcn_layer_kernel<N, true>), grid, blk, 0, st, K, Nout, X, W, bias, ell_idx, ell_w, active, H, pooled);
    else hipLaunchKernelGGL((board_gcn_layer_kernel<N, false>), grid, blk, 0, st, K, Nout, X, W, bias, ell_idx, ell_w, active, H, pooled);
    return check_launch("board_gcn_layer_kernel");
}

}  // namespace

// One fused GCNConv + bias + ReLU over B boards (ELL rows from the featuriser); `pooled` non-NULL: write the mean pool instead of H.
int launch_board_gcn_layer(int N, int B, int K, int Nout, const float* X, const float* W, const float* bias, const int32_t* ell_idx,
                           const float* ell_w, const uint8_t* active, float* H, float* pooled, hipStream_t st) {
    if (B <= 0 || Nout <= 0) return 0;
    return for_board_size(N, [&](auto n) { return launch_layer_n<decltype(n)::value>(B, K, Nout, X, W, bias, ell_idx, ell_w, active, H, pooled, st); });
}

size_t boards_general_workspace_floats(int N, int hidden, int A, int B) {
    if (B <= 0 || hidden <= 0 || A <= 0) return 0;
    return general_layout(N, hidden, A, B, nullptr, nullptr);
}

int check_general_net(const aqg_gcn_general_net* net, const char** why) {
    if (!net) { *why = "null network descriptor"; return -1; }
    if (net->num_features != 6) { *why = "board records have 6 feature planes: num_features must be 6"; return -1; }
    if (net->hidden < 2 || net->hidden > 1024) { *why = "hidden must be 2..1024"; return -1; }
    if (net->num_layers < 1 || net->num_layers > AQG_GENERAL_MAX_LAYERS) { *why = "num_layers must be 1..32"; return -1; }
    if (net->policy_size < 1 || net->policy_size > 4096) { *why = "policy_size must be 1..4096"; return -1; }
    for (int i = 0; i < 2 * net->num_layers + 8; ++i)
        if (!net->params[i]) { *why = "a parameter pointer is NULL"; return -1; }
    return 0;
}

int launch_gcn_forward_boards_general(int N, const void* states, int fmt, int B, const aqg_gcn_general_net* net,
                                      const uint8_t* active, float* workspace, size_t workspace_floats, float* pooled, float* logits,
                                      float* policy, float* value_pre, float* value, hipStream_t st) {
    const char* why = "";
    if (!board_size_supported(N)) return fail("aqg_gcn_forward_boards_general: board_size must be 3, 5, 7 or 9");
    if (fmt != 0 && fmt != 1) return fail("aqg_gcn_forward_boards_general: state_fmt must be 0 or 1");
    if (B < 0) return fail("aqg_gcn_forward_boards_general: negative size");
    if (check_general_net(net, &why)) return fail("aqg_gcn_forward_boards_general", why);
    if (B == 0) return 0;
    if (!states || !policy) return fail("aqg_gcn_forward_boards_general: states and policy are required");
    const int Hd = net->hidden, L = net->num_layers, A = net->policy_size;
    if (!workspace || workspace_floats < boards_general_workspace_floats(N, Hd, A, B))
        return fail("aqg_gcn_forward_boards_general: workspace too small (aqg_gcn_boards_general_workspace_floats)");
    GeneralWorkspace ws;
    general_layout(N, Hd, A, B, &ws, workspace);
    if (!pooled) pooled = ws.pooled;
    if (!logits) logits = ws.logits;
    if (!value_pre) value_pre = ws.vpre;
    if (int r = launch_gcn_boards_graph(N, states, fmt, B, ws.x0, ws.ell_idx, ws.ell_w, st)) return r;
    const float* const* p = net->params;
    const float* X = ws.x0;
    int K = net->num_features;
    for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        float* H = last ? nullptr : ws.h[l & 1];
        if (int r = launch_board_gcn_layer(N, B, K, Hd, X, p[2 * l], p[2 * l + 1], ws.ell_idx, ws.ell_w, active, H,
                                           last ? pooled : nullptr, st))
            return r;
        X = H;
        K = Hd;
    }
    // heads (pv_network_gnn.py:37-47): the width-generic linear maps over every row (a skipped board's rows are garbage in, garbage
    // out, never read), then softmax / tanh for the active boards only -- an inactive board's policy / value rows are left as they were
    const int Hh = Hd / 2, o = 2 * L;
    if (int r = launch_gen_linear(B, Hd, Hh, pooled, p[o], p[o + 1], nullptr, AQG_LIN_RELU, ws.hp, st)) return r;
    if (int r = launch_gen_linear(B, Hh, A, ws.hp, p[o + 2], p[o + 3], nullptr, 0, logits, st)) return r;
    if (int r = launch_gen_linear(B, Hd, Hh, pooled, p[o + 4], p[o + 5], nullptr, AQG_LIN_RELU, ws.hv, st)) return r;
    if (int r = launch_gen_linear(B, Hh, 1, ws.hv, p[o + 6], p[o + 7], nullptr, 0, value_pre, st)) return r;
    return launch_gen_heads(B, A, logits, value_pre, policy, value, st, active);
}

}  // namespace aqg
