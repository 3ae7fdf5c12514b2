// gcn_graph_grad.hip -- backward of forward(x, edge_index, batch) (the generic graph path of gcn_forward.hip), fp32.
//
// Notation: A_hat = the gcn_norm adjacency (CSR by destination in the forward, CSR by SOURCE here = A_hat^T),
// P_l = A_hat (H_{l-1} W_l^T) + b_l, H_l = relu(P_l), H_0 = x; pooled[g] = mean of H_3 over graph g; heads as in
// gcn_heads_kernel.  The forward saved H_1, H_2, H_3 and pooled; the heads' hidden layer is recomputed in the forward's
// own summation order, so its ReLU masks are the forward's.
//
//   heads   : one workgroup per graph -> dlogits, dvpre, d(hidden), dpooled; weight gradients of the heads by a
//             fixed-order sum over graphs (head_outer_kernel)
//   pool    : dP_3[i] = (H_3[i] > 0) * dpooled[graph(i)] / |graph(i)|
//   layer l : dZ_l = A_hat^T dP_l                            (gather over the CSR by source, one wave per node)
//             dW_l = dZ_l^T H_{l-1}, db_l = sum_i dP_l[i]     (f32-input MFMA over row chunks -> partial tiles -> fixed-order reduce)
//             dP_{l-1} = (H_{l-1} > 0) * (dZ_l W_l)           (f32-input MFMA, W_l's fragments held in registers)
//             dx = dZ_1 W_1 for l = 1 when asked for          (VALU, 6 outputs per node)
// No atomics anywhere: every sum runs in an order fixed by the sizes alone, so two backward passes are bit-identical.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"

namespace aqg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HID = 128;
constexpr int HH = HID / 2;        // hidden units of each head
constexpr int APAD = 256;          // dlogits row stride in the workspace
constexpr int FEAT = 6;
constexpr int MAX_CHUNKS = 512;    // row chunks of the dW split (partial tiles in the workspace)
constexpr int PART = HID * HID + HID;   // one chunk's partial: dW [128][128] (or [128][6] in its first floats) + db [128]

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows of the dW split: a multiple of 32, at most MAX_CHUNKS chunks
inline int chunk_rows(int n) {
    const int per = (n + MAX_CHUNKS - 1) / MAX_CHUNKS;
    return ((per + 31) / 32) * 32;
}
inline int num_chunks(int n) { const int r = chunk_rows(n); return (n + r - 1) / r; }

// ------------------------------------------------------------------------------------------- heads
// One workgroup (256 threads) per graph.  params: the 14 state_dict tensors ([out, in] weights).
__global__ __launch_bounds__(256) void head_backward_kernel(int G, int A, const float* __restrict__ pooled,
                                                            const float* __restrict__ policy, const float* __restrict__ value,
                                                            const float* __restrict__ dpolicy, const float* __restrict__ dvalue,
                                                            const float* __restrict__ pw1, const float* __restrict__ pb1,
                                                            const float* __restrict__ pw2, const float* __restrict__ vw1,
                                                            const float* __restrict__ vb1, const float* __restrict__ vw2,
                                                            float* __restrict__ hid_out, float* __restrict__ dhid_out,
                                                            float* __restrict__ dlogits_out, float* __restrict__ dvpre_out,
                                                            float* __restrict__ dpooled) {
    __shared__ float g[HID];
    __shared__ float hid[HID];        // 0..63 policy hidden, 64..127 value hidden (post-ReLU)
    __shared__ float dl[APAD];
    __shared__ float dh[HID];
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b >= G) return;
    if (tid < HID) g[tid] = pooled[(size_t)b * HID + tid];
    __syncthreads();
    if (tid < HID) {   // gcn_heads_kernel's order: two k halves summed from 0 each, then (part0 + part1) + bias
        const float* w = tid < HH ? pw1 + (size_t)tid * HID : vw1 + (size_t)(tid - HH) * HID;
        float p0 = 0.f, p1 = 0.f;
        for (int k = 0; k < HH; ++k) p0 = fmaf(g[k], w[k], p0);
        for (int k = HH; k < HID; ++k) p1 = fmaf(g[k], w[k], p1);
        const float h = fmaxf(p0 + p1 + (tid < HH ? pb1[tid] : vb1[tid - HH]), 0.f);
        hid[tid] = h;
        hid_out[(size_t)b * HID + tid] = h;
    }
    // softmax backward: dlogits = p * (dp - sum(dp * p)), the sum as a fixed shuffle tree + 4-wave sum
    float pa = 0.f, dpa = 0.f;
    if (dpolicy && tid < A) { pa = policy[(size_t)b * A + tid]; dpa = dpolicy[(size_t)b * A + tid]; }
    float s = dpa * pa;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const float tot = (red[0] + red[1]) + (red[2] + red[3]);
    dl[tid] = (dpolicy && tid < A) ? pa * (dpa - tot) : 0.f;
    if (tid < A) dlogits_out[(size_t)b * APAD + tid] = dl[tid];
    float dvp = 0.f;
    if (dvalue) { const float v = value[b]; dvp = dvalue[b] * (1.f - v * v); }
    if (tid == 0) dvpre_out[b] = dvp;
    __syncthreads();
    if (tid < HH) {           // policy hidden: sum_a dlogits[a] W2[a][u]
        float acc = 0.f;
        for (int a = 0; a < A; ++a) acc = fmaf(dl[a], pw2[(size_t)a * HH + tid], acc);
        dh[tid] = hid[tid] > 0.f ? acc : 0.f;
    } else if (tid < HID) {   // value hidden
        dh[tid] = hid[tid] > 0.f ? dvp * vw2[tid - HH] : 0.f;
    }
    __syncthreads();
    if (tid < HID) {
        dhid_out[(size_t)b * HID + tid] = dh[tid];
        float acc = 0.f;
        for (int u = 0; u < HH; ++u) acc = fmaf(dh[u], pw1[(size_t)u * HID + tid], acc);
        for (int u = 0; u < HH; ++u) acc = fmaf(dh[HH + u], vw1[(size_t)u * HID + tid], acc);
        dpooled[(size_t)b * HID + tid] = acc;
    }
}

// outW[o][i] = sum_r dY[r][o] X[r][i] (r = 0 .. R-1 in order), outB[o] = sum_r dY[r][o]; one thread per output
// (i == I is the bias column).  The heads' reductions over graphs.
__global__ __launch_bounds__(256) void head_outer_kernel(int R, const float* __restrict__ dY, int ldy, int O,
                                                         const float* __restrict__ X, int ldx, int I,
                                                         float* __restrict__ outW, float* __restrict__ outB) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= O * (I + 1)) return;
    const int o = t / (I + 1), i = t % (I + 1);
    float acc = 0.f;
    if (i < I) {
        for (int r = 0; r < R; ++r) acc = fmaf(dY[(size_t)r * ldy + o], X[(size_t)r * ldx + i], acc);
        outW[(size_t)o * I + i] = acc;
    } else {
        for (int r = 0; r < R; ++r) acc += dY[(size_t)r * ldy + o];
        outB[o] = acc;
    }
}

// ------------------------------------------------------------------------------------------- pool / gather
// dP3[i][c] = (H3[i][c] > 0) * dpooled[g][c] / |g|, g = the graph holding node i (binary search in graph_ptr)
__global__ __launch_bounds__(256) void pool_backward_kernel(int n, const int32_t* __restrict__ gptr, int G,
                                                            const float* __restrict__ dpooled, const float* __restrict__ H3,
                                                            float* __restrict__ dP) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    int lo = 0, hi = G;                       // largest g with gptr[g] <= i
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (gptr[m] <= i) lo = m; else hi = m; }
    const float cnt = (float)(gptr[lo + 1] - gptr[lo]);
    const float2 d = *reinterpret_cast<const float2*>(dpooled + (size_t)lo * HID + 2 * lane);
    const float2 h = *reinterpret_cast<const float2*>(H3 + (size_t)i * HID + 2 * lane);
    *reinterpret_cast<float2*>(dP + (size_t)i * HID + 2 * lane) =
        make_float2(h.x > 0.f ? d.x / cnt : 0.f, h.y > 0.f ? d.y / cnt : 0.f);
}

// dZ[j] = sum_{e in tcsr[j]} w_e dP[dst_e]: one wave per node, lane = 2 columns, edges in the CSR's (stable) order
__global__ __launch_bounds__(256) void gather_t_kernel(const float* __restrict__ dP, int n, const int32_t* __restrict__ tptr,
                                                       const int32_t* __restrict__ tdst, const float* __restrict__ tw,
                                                       float* __restrict__ dZ) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    float a0 = 0.f, a1 = 0.f;
    for (int e = tptr[j]; e < tptr[j + 1]; ++e) {
        const float we = tw[e];
        const float2 y = *reinterpret_cast<const float2*>(dP + (size_t)tdst[e] * HID + 2 * lane);
        a0 = fmaf(we, y.x, a0);
        a1 = fmaf(we, y.y, a1);
    }
    *reinterpret_cast<float2*>(dZ + (size_t)j * HID + 2 * lane) = make_float2(a0, a1);
}

// ------------------------------------------------------------------------------------------- dW_l, db_l
// One workgroup (4 waves) per row chunk.  part[chunk] = { dW [128][K] = sum_i dZ[i][o] Hp[i][k],  db [128] = sum_i dP[i][o] }
// over the chunk's rows.  MFMA 16x16x4 f32: A = dZ^T (m = o, k = row), B = Hp (k = row, n = feature column); wave w owns
// o in [32w, 32w + 32) (2 o-tiles) x KT feature tiles.  32 rows at a time are staged in LDS (row stride 144: the 4 rows of a
// fragment fall on distinct banks).
template <int KT>   // 8: K = 128;  1: K = 6 (layer 1, H_0 = x, columns 6..15 zero)
__global__ __launch_bounds__(256) void dw_partial_kernel(int n, int rows_per_chunk, const float* __restrict__ dZ,
                                                         const float* __restrict__ Hp, const float* __restrict__ dP,
                                                         float* __restrict__ part) {
    constexpr int K = KT == 8 ? HID : FEAT;
    constexpr int S = 144;
    constexpr int HC = 16 * KT;            // staged feature columns
    __shared__ alignas(16) float zs[32 * S];
    __shared__ alignas(16) float hs[32 * S];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const size_t r0 = (size_t)blockIdx.x * rows_per_chunk;
    const size_t r1 = r0 + rows_per_chunk < (size_t)n ? r0 + rows_per_chunk : (size_t)n;
    f32x4 acc[2][KT];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < KT; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (size_t rb = r0; rb < r1; rb += 32) {
        __syncthreads();
        for (int idx = tid; idx < 32 * 32; idx += 256) {      // dZ rows as float4
            const int r = idx >> 5, c4 = idx & 31;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (rb + r < r1) v = *reinterpret_cast<const f32x4*>(dZ + (rb + r) * HID + 4 * c4);
            *reinterpret_cast<f32x4*>(zs + r * S + 4 * c4) = v;
        }
        if (KT == 8) {
            for (int idx = tid; idx < 32 * 32; idx += 256) {
                const int r = idx >> 5, c4 = idx & 31;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (rb + r < r1) v = *reinterpret_cast<const f32x4*>(Hp + (rb + r) * HID + 4 * c4);
                *reinterpret_cast<f32x4*>(hs + r * S + 4 * c4) = v;
            }
        } else {
            for (int idx = tid; idx < 32 * HC; idx += 256) {
                const int r = idx / HC, k = idx % HC;
                hs[r * S + k] = (k < K && rb + r < r1) ? Hp[(rb + r) * K + k] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < 32; kk += 4) {
            const float a0 = zs[(kk + q) * S + 32 * w + c];
            const float a1 = zs[(kk + q) * S + 32 * w + 16 + c];
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const float bv = hs[(kk + q) * S + 16 * t + c];
                acc[0][t] = mfma4(a0, bv, acc[0][t]);
                acc[1][t] = mfma4(a1, bv, acc[1][t]);
            }
        }
    }
    float* out = part + (size_t)blockIdx.x * PART;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 32 * w + 16 * a + 4 * q + i, k = 16 * t + c;   // C/D: row = 4 (lane >> 4) + reg, col = lane & 15
                if (k < K) out[(size_t)o * K + k] = acc[a][t][i];
            }
    if (tid < HID) {          // db over the chunk's rows, in row order
        float s = 0.f;
        for (size_t r = r0; r < r1; ++r) s += dP[r * HID + tid];
        out[HID * HID + tid] = s;
    }
}

// dW[j] = sum_c part[c][j] (c in order) for j < 128 K;  db likewise
__global__ __launch_bounds__(256) void dw_reduce_kernel(int chunks, int K, const float* __restrict__ part,
                                                        float* __restrict__ dW, float* __restrict__ db) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int nw = HID * K;
    if (j >= nw + HID) return;
    const int src = j < nw ? j : HID * HID + (j - nw);
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * PART + src];
    if (j < nw) dW[j] = s; else db[j - nw] = s;
}

// ------------------------------------------------------------------------------------------- dP_{l-1}, dx
// dP_prev[i][k] = (Hp[i][k] > 0) * sum_o dZ[i][o] W[o][k]   (W = the layer's [out 128][in 128] weight).
// MFMA 16x16x4 f32: A = dZ (m = row, k = o), B = W (k = o, n = k).  Wave w owns columns [32w, 32w + 32); its W slice is
// 64 VGPRs of B fragments for the whole kernel.  K order is permuted so that each lane's A values are one ds_read_b128:
// at step s of o-group gi, k-slot q stands for o = 16 gi + 4 q + s.  Workgroups stride over 32-row tiles staged in LDS.
__global__ __launch_bounds__(256) void dh_kernel(int n, const float* __restrict__ dZ, const float* __restrict__ W,
                                                 const float* __restrict__ Hp, float* __restrict__ dPp) {
    constexpr int S = 132;
    __shared__ alignas(16) float zs[32 * S];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    float bf[8][4][2];
#pragma unroll
    for (int gi = 0; gi < 8; ++gi)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t) bf[gi][s][t] = W[(size_t)(16 * gi + 4 * q + s) * HID + 32 * w + 16 * t + c];
    const size_t tiles = ((size_t)n + 31) / 32;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t rb = tile * 32;
        __syncthreads();
        for (int idx = tid; idx < 32 * 32; idx += 256) {
            const int r = idx >> 5, c4 = idx & 31;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (rb + r < (size_t)n) v = *reinterpret_cast<const f32x4*>(dZ + (rb + r) * HID + 4 * c4);
            *reinterpret_cast<f32x4*>(zs + r * S + 4 * c4) = v;
        }
        __syncthreads();
        f32x4 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int gi = 0; gi < 8; ++gi) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(zs + c * S + 16 * gi + 4 * q);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(zs + (16 + c) * S + 16 * gi + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    acc[0][t] = mfma4(a0[s], bf[gi][s][t], acc[0][t]);
                    acc[1][t] = mfma4(a1[s], bf[gi][s][t], acc[1][t]);
                }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const size_t r = rb + 16 * a + 4 * q + i;
                    const int k = 32 * w + 16 * t + c;
                    if (r < (size_t)n) dPp[r * HID + k] = Hp[r * HID + k] > 0.f ? acc[a][t][i] : 0.f;
                }
    }
}

// dx[i][f] = sum_o dZ[i][o] W1[o][f]: one thread per (node, feature)
__global__ __launch_bounds__(256) void dx_kernel(int n, const float* __restrict__ dZ, const float* __restrict__ W1,
                                                 float* __restrict__ dx) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * FEAT) return;
    const size_t i = t / FEAT;
    const int f = (int)(t % FEAT);
    float acc = 0.f;
    for (int o = 0; o < HID; ++o) acc = fmaf(dZ[i * HID + o], W1[o * FEAT + f], acc);
    dx[t] = acc;
}

}  // namespace

size_t graph_backward_workspace_floats(int n, int G) {
    if (n <= 0 || G <= 0) return 0;
    return 2 * (size_t)n * HID + (size_t)num_chunks(n) * PART + (size_t)G * (3 * HID + APAD + 1);
}

// params[14]: state_dict order (include/aqgnn.h); grads[14] likewise.
int launch_gcn_backward_graph(int F, int A, const float* x, int n, const float* h1, const float* h2, const float* h3,
                              const int32_t* tptr, const int32_t* tdst, const float* tw, const int32_t* gptr, int G,
                              const float* pooled, const float* policy, const float* value, const float* dpolicy,
                              const float* dvalue, const float* const* params, float* workspace, size_t workspace_floats,
                              float* const* grads, float* dx, hipStream_t st) {
    if (F != FEAT) return fail("num_features must be 6 (NUM_FEATURES pv_network_gnn.py:17)");
    if (A <= 0 || A > 248) return fail("policy size must be 1..248");
    if (n <= 0 || G <= 0) {
        const size_t sz[14] = {HID * FEAT, HID, HID * HID, HID, HID * HID, HID, HH * HID, HH, (size_t)A * HH, (size_t)A,
                               HH * HID, HH, HH, 1};
        for (int i = 0; i < 14; ++i)
            if (hipMemsetAsync(grads[i], 0, sz[i] * sizeof(float), st) != hipSuccess) return fail("hipMemsetAsync");
        return 0;
    }
    if (workspace_floats < graph_backward_workspace_floats(n, G)) return fail("aqg_gcn_backward_graph: workspace too small");
    float* dP = workspace;
    float* dZ = dP + (size_t)n * HID;
    float* part = dZ + (size_t)n * HID;
    float* hid = part + (size_t)num_chunks(n) * PART;
    float* dhid = hid + (size_t)G * HID;
    float* dpooled = dhid + (size_t)G * HID;
    float* dlog = dpooled + (size_t)G * HID;
    float* dvpre = dlog + (size_t)G * APAD;
    const float* const* p = params;
    hipLaunchKernelGGL(head_backward_kernel, dim3(G), dim3(256), 0, st, G, A, pooled, policy, value, dpolicy, dvalue,
                       p[6], p[7], p[8], p[10], p[11], p[12], hid, dhid, dlog, dvpre, dpooled);
    auto outer = [&](const float* dY, int ldy, int O, const float* X, int ldx, int I, float* oW, float* oB) {
        const int T = O * (I + 1);
        hipLaunchKernelGGL(head_outer_kernel, dim3((T + 255) / 256), dim3(256), 0, st, G, dY, ldy, O, X, ldx, I, oW, oB);
    };
    outer(dhid, HID, HH, pooled, HID, HID, grads[6], grads[7]);             // policy_head.0
    outer(dlog, APAD, A, hid, HID, HH, grads[8], grads[9]);                 // policy_head.2
    outer(dhid + HH, HID, HH, pooled, HID, HID, grads[10], grads[11]);      // value_head.0
    outer(dvpre, 1, 1, hid + HH, HID, HH, grads[12], grads[13]);            // value_head.2
    if (int r = check_launch("graph backward: heads")) return r;
    const dim3 rows((n + 3) / 4);
    hipLaunchKernelGGL(pool_backward_kernel, rows, dim3(256), 0, st, n, gptr, G, (const float*)dpooled, h3, dP);
    const int rpc = chunk_rows(n), nch = num_chunks(n);
    int dh_grid = (n + 31) / 32;
    if (dh_grid > 2048) dh_grid = 2048;
    const float* Hs[4] = {x, h1, h2, h3};
    for (int l = 3; l >= 1; --l) {
        hipLaunchKernelGGL(gather_t_kernel, rows, dim3(256), 0, st, (const float*)dP, n, tptr, tdst, tw, dZ);
        const int K = l == 1 ? FEAT : HID;
        if (l == 1)
            hipLaunchKernelGGL(dw_partial_kernel<1>, dim3(nch), dim3(256), 0, st, n, rpc, (const float*)dZ, Hs[0], (const float*)dP, part);
        else
            hipLaunchKernelGGL(dw_partial_kernel<8>, dim3(nch), dim3(256), 0, st, n, rpc, (const float*)dZ, Hs[l - 1], (const float*)dP, part);
        hipLaunchKernelGGL(dw_reduce_kernel, dim3((HID * K + HID + 255) / 256), dim3(256), 0, st, nch, K, (const float*)part,
                           grads[2 * (l - 1)], grads[2 * (l - 1) + 1]);
        if (l > 1)
            hipLaunchKernelGGL(dh_kernel, dim3(dh_grid), dim3(256), 0, st, n, (const float*)dZ, p[2 * (l - 1)], Hs[l - 1], dP);
        else if (dx)
            hipLaunchKernelGGL(dx_kernel, dim3(((size_t)n * FEAT + 255) / 256), dim3(256), 0, st, n, (const float*)dZ, p[0], dx);
        if (int r = check_launch("graph backward: layer")) return r;
    }
    return 0;
}

}  // namespace aqg
