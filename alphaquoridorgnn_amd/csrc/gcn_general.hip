// gcn_general.hip -- width-generic graph primitives, fp32: the GraphPolicyValueNetwork of any shape, the stand-alone GCNConv,
// global_mean_pool and their backward passes are composed from these by pv_network_gnn.py (include/aqgnn.h, "graph primitives").
//
//   linear        Y[M,N] = X[M,K] W^T (+ b) (ReLU) (x mask)          f32-input MFMA 16x16x4, 64x64 tiles, runtime M, K, N
//                 (W [N,K] as PyTorch stores it, or [K,N]: the backward's dX = dY W with the same kernel)
//   linear_grad   dW[N,K] = dY^T X,  db[N] = sum_m dYb[m]             MFMA over row chunks -> partial tiles -> fixed-order reduce
//   aggregate     out[i] = sum_{e in csr(i)} w_e Y[src_e] (+ b) (ReLU)  one wave per node, lanes across columns
//   mean pool     pooled[g] = mean of H over graph g (0 for an empty graph), and its backward (optionally ReLU-masked)
//   heads         softmax over each row of the logits, tanh of the value, and their backward
//
// Tails of M, K and N are zero-padded in LDS or masked at the store; the caller's buffers are never padded.  The f32-input MFMA
// is bit-for-bit a k-ordered fmaf chain, and no kernel here uses atomics: every sum runs in an order fixed by the sizes alone,
// so every result is a deterministic function of the inputs.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"

namespace aqg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int GEN_MAX_CHUNKS = 512;           // row chunks of linear_grad
constexpr size_t GEN_PART_BUDGET = 1u << 24;  // floats of partial tiles linear_grad aims to stay under

// ------------------------------------------------------------------------------------------- linear
// One workgroup (4 waves) per 64x64 output tile; K in slabs of 32 staged in LDS (row stride 36: the 16 rows x 4 k of a fragment
// fall on 64 distinct banks).  Wave w owns rows [16w, 16w + 16) of the tile and its 4 column tiles.
// MFMA 16x16x4: A[m][k] = X[row][k], B[k][j] = W[col][k] (flags & AQG_LIN_W_KN: W[k][col]).
__global__ __launch_bounds__(256) void gen_linear_kernel(int M, int K, int N, const float* __restrict__ X,
                                                         const float* __restrict__ W, const float* __restrict__ bias,
                                                         const float* __restrict__ mask, int flags, float* __restrict__ Y) {
    constexpr int S = 36;
    __shared__ alignas(16) float xs[64 * S];
    __shared__ alignas(16) float ws[64 * S];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const size_t m0 = (size_t)blockIdx.x * 64;
    const int n0 = blockIdx.y * 64;
    const bool kn = flags & AQG_LIN_W_KN;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 32) {
        __syncthreads();
        for (int idx = tid; idx < 64 * 32; idx += 256) {
            const int r = idx >> 5, k = idx & 31;
            xs[r * S + k] = (m0 + r < (size_t)M && k0 + k < K) ? X[(m0 + r) * K + k0 + k] : 0.f;
        }
        if (!kn) {
            for (int idx = tid; idx < 64 * 32; idx += 256) {
                const int j = idx >> 5, k = idx & 31;
                ws[j * S + k] = (n0 + j < N && k0 + k < K) ? W[(size_t)(n0 + j) * K + k0 + k] : 0.f;
            }
        } else {
            for (int idx = tid; idx < 64 * 32; idx += 256) {
                const int k = idx >> 6, j = idx & 63;
                ws[j * S + k] = (n0 + j < N && k0 + k < K) ? W[(size_t)(k0 + k) * N + n0 + j] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < 32; kk += 4) {
            const float a = xs[(16 * w + c) * S + kk + q];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mfma4(a, ws[(16 * t + c) * S + kk + q], acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * t + c;
        if (n >= N) continue;
        const float bn = bias ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {              // C/D: row = 4 (lane >> 4) + reg, col = lane & 15
            const size_t m = m0 + 16 * w + 4 * q + i;
            if (m >= (size_t)M) continue;
            const size_t o = m * N + n;
            float v = acc[t][i] + bn;
            if (flags & AQG_LIN_ACCUMULATE) v = Y[o] + v;
            if (flags & AQG_LIN_RELU) v = fmaxf(v, 0.f);
            if (mask && !(mask[o] > 0.f)) v = 0.f;
            Y[o] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------- linear_grad
// rows of one chunk: a multiple of 32; at most GEN_MAX_CHUNKS chunks and about GEN_PART_BUDGET floats of partials
inline int grad_chunk_rows(long long M, int N, int K) {
    const size_t part = (size_t)N * K + N;
    size_t cmax = GEN_PART_BUDGET / part;
    if (cmax < 1) cmax = 1;
    if (cmax > GEN_MAX_CHUNKS) cmax = GEN_MAX_CHUNKS;
    const long long per = (M + (long long)cmax - 1) / (long long)cmax;
    return (int)(((per + 31) / 32) * 32);
}
inline int grad_chunks(long long M, int N, int K) { const int r = grad_chunk_rows(M, N, K); return (int)((M + r - 1) / r); }

// One workgroup per (row chunk, 64 n, 64 k): part[chunk] = { dW [N][K] = sum_r dY[r][n] X[r][k],  db [N] = sum_r dYb[r][n] } over
// the chunk's rows in order.  32 rows at a time in LDS (row stride 80: a fragment's 4 rows x 16 columns hit 64 distinct banks).
// MFMA 16x16x4: A[m = n][k = row] = dY[row][n], B[k = row][j = k] = X[row][k]; wave w owns n in [16w, 16w + 16) x 4 k tiles.
// The workgroups of the first k tile also sum db from the staged rows (dYb staged separately when it is not dY).
__global__ __launch_bounds__(256) void gen_grad_partial_kernel(int M, int N, int K, int rows_per_chunk, const float* __restrict__ dY,
                                                               const float* __restrict__ X, const float* __restrict__ dYb,
                                                               float* __restrict__ part) {
    constexpr int S = 80;
    __shared__ alignas(16) float ys[32 * S];
    __shared__ alignas(16) float xs[32 * S];
    __shared__ alignas(16) float bs[32 * S];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const size_t r0 = (size_t)blockIdx.x * rows_per_chunk;
    const size_t r1 = r0 + rows_per_chunk < (size_t)M ? r0 + rows_per_chunk : (size_t)M;
    const int n0 = blockIdx.y * 64, k0 = blockIdx.z * 64;
    const bool do_db = blockIdx.z == 0;
    const bool sep_b = do_db && dYb != dY;
    const float* bsrc = sep_b ? bs : ys;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;
    for (size_t rb = r0; rb < r1; rb += 32) {
        __syncthreads();
        for (int idx = tid; idx < 32 * 64; idx += 256) {
            const int r = idx >> 6, j = idx & 63;
            const bool rok = rb + r < r1;
            ys[r * S + j] = (rok && n0 + j < N) ? dY[(rb + r) * N + n0 + j] : 0.f;
            xs[r * S + j] = (rok && k0 + j < K) ? X[(rb + r) * K + k0 + j] : 0.f;
            if (sep_b) bs[r * S + j] = (rok && n0 + j < N) ? dYb[(rb + r) * N + n0 + j] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < 32; kk += 4) {
            const float a = ys[(kk + q) * S + 16 * w + c];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mfma4(a, xs[(kk + q) * S + 16 * t + c], acc[t]);
        }
        if (do_db && tid < 64) {
            const int nr = r1 - rb < 32 ? (int)(r1 - rb) : 32;
            for (int r = 0; r < nr; ++r) dbs += bsrc[r * S + tid];
        }
    }
    float* out = part + (size_t)blockIdx.x * ((size_t)N * K + N);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + 16 * w + 4 * q + i, k = k0 + 16 * t + c;
            if (n < N && k < K) out[(size_t)n * K + k] = acc[t][i];
        }
    if (do_db && tid < 64 && n0 + tid < N) out[(size_t)N * K + n0 + tid] = dbs;
}

// dW[j] = sum_c part[c][j] (c in order) for j < N K;  db likewise (db may be NULL)
__global__ __launch_bounds__(256) void gen_grad_reduce_kernel(int chunks, int N, int K, const float* __restrict__ part,
                                                              float* __restrict__ dW, float* __restrict__ db) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nw = (size_t)N * K, stride = nw + N;
    if (j >= stride || (j >= nw && !db)) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * stride + j];
    if (j < nw) dW[j] = s; else db[j - nw] = s;
}

// ------------------------------------------------------------------------------------------- aggregate
template <int V> struct vec;
template <> struct vec<1> { typedef float t; };
template <> struct vec<2> { typedef float2 t; };
template <> struct vec<4> { typedef f32x4 t; };

template <int V> __device__ __forceinline__ void vfma(float w, const float* y, float* a) {
    const typename vec<V>::t v = *reinterpret_cast<const typename vec<V>::t*>(y);
    if constexpr (V == 1) a[0] = fmaf(w, v, a[0]);
    else if constexpr (V == 2) { a[0] = fmaf(w, v.x, a[0]); a[1] = fmaf(w, v.y, a[1]); }
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = fmaf(w, v[i], a[i]);
    }
}

// out[i][c] = (relu) (bias[c] + sum_{e = ptr[i] .. ptr[i+1]) w_e Y[src_e][c]), the edges in CSR order; an entry with src < 0 is
// skipped.  One wave per node; lane l holds columns V (l + 64 j) .. + V - 1 (V = 4 / 2 / 1 when N is a multiple of 4 / 2 / neither).
template <int V>
__global__ __launch_bounds__(256) void gen_aggregate_kernel(int n, int N, const float* __restrict__ Y, const int32_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ src, const float* __restrict__ wt,
                                                            const float* __restrict__ bias, int relu, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int e0 = ptr[i], e1 = ptr[i + 1];
    for (int c = V * lane; c < N; c += 64 * V) {
        float a[V];
#pragma unroll
        for (int v = 0; v < V; ++v) a[v] = bias ? bias[c + v] : 0.f;
        for (int e = e0; e < e1; ++e) {
            const int s = src[e];
            if (s < 0) continue;
            vfma<V>(wt[e], Y + (size_t)s * N + c, a);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) out[(size_t)i * N + c + v] = relu ? fmaxf(a[v], 0.f) : a[v];
    }
}

// ------------------------------------------------------------------------------------------- mean pool
// pooled[g][c] = sum of H[i][c] over i = gptr[g] .. gptr[g+1] (in order) / count; 0 for an empty graph.  One workgroup per graph.
__global__ __launch_bounds__(256) void gen_pool_kernel(const float* __restrict__ H, int N, const int32_t* __restrict__ gptr, int G,
                                                       float* __restrict__ pooled) {
    const int g = blockIdx.x;
    if (g >= G) return;
    const int a = gptr[g], b = gptr[g + 1];
    for (int c = threadIdx.x; c < N; c += 256) {
        float s = 0.f;
        for (int i = a; i < b; ++i) s += H[(size_t)i * N + c];
        pooled[(size_t)g * N + c] = b > a ? s / (float)(b - a) : 0.f;
    }
}

// dH[i][c] = dpooled[g][c] / |g| (g = the graph holding node i: binary search in gptr), x (mask[i][c] > 0) when mask is given.
// One wave per node.
__global__ __launch_bounds__(256) void gen_pool_backward_kernel(int n, int N, const float* __restrict__ dpooled,
                                                                const int32_t* __restrict__ gptr, int G, const float* __restrict__ mask,
                                                                float* __restrict__ dH) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    int lo = 0, hi = G;                       // largest g with gptr[g] <= i
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (gptr[m] <= i) lo = m; else hi = m; }
    const float cnt = (float)(gptr[lo + 1] - gptr[lo]);
    for (int c = lane; c < N; c += 64) {
        const size_t o = (size_t)i * N + c;
        const float d = dpooled[(size_t)lo * N + c] / cnt;
        dH[o] = (mask && !(mask[o] > 0.f)) ? 0.f : d;
    }
}

// ------------------------------------------------------------------------------------------- heads
// sum / max over a 256-thread workgroup: per-thread strided values -> fixed shuffle tree -> the 4 waves in order
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off);
        v = is_max ? fmaxf(v, o) : v + o;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// policy[g] = softmax(logits[g]) over A; value[g] = tanh(vpre[g]).  One workgroup per row; a row with active[g] != 1 is skipped
// (active may be NULL: every row).
__global__ __launch_bounds__(256) void gen_heads_kernel(int G, int A, const float* __restrict__ logits, const float* __restrict__ vpre,
                                                        float* __restrict__ policy, float* __restrict__ value,
                                                        const uint8_t* __restrict__ active) {
    __shared__ float red[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g >= G || (active && active[g] != 1)) return;
    const float* l = logits + (size_t)g * A;
    float m = -INFINITY;
    for (int a = tid; a < A; a += 256) m = fmaxf(m, l[a]);
    m = block_reduce(m, true, red);
    float s = 0.f;
    for (int a = tid; a < A; a += 256) s += expf(l[a] - m);
    s = block_reduce(s, false, red);
    for (int a = tid; a < A; a += 256) policy[(size_t)g * A + a] = expf(l[a] - m) / s;
    if (tid == 0 && vpre && value) value[g] = tanhf(vpre[g]);
}

// dlogits[g] = p (dp - sum_a dp_a p_a) (0 without dpolicy); dvpre[g] = dvalue (1 - value^2) (0 without dvalue).
__global__ __launch_bounds__(256) void gen_heads_backward_kernel(int G, int A, const float* __restrict__ policy,
                                                                 const float* __restrict__ dpolicy, const float* __restrict__ value,
                                                                 const float* __restrict__ dvalue, float* __restrict__ dlogits,
                                                                 float* __restrict__ dvpre) {
    __shared__ float red[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g >= G) return;
    const size_t row = (size_t)g * A;
    if (dlogits) {
        if (dpolicy) {
            float s = 0.f;
            for (int a = tid; a < A; a += 256) s = fmaf(dpolicy[row + a], policy[row + a], s);
            s = block_reduce(s, false, red);
            for (int a = tid; a < A; a += 256) dlogits[row + a] = policy[row + a] * (dpolicy[row + a] - s);
        } else {
            for (int a = tid; a < A; a += 256) dlogits[row + a] = 0.f;
        }
    }
    if (tid == 0 && dvpre) {
        float d = 0.f;
        if (dvalue) { const float v = value[g]; d = dvalue[g] * (1.f - v * v); }
        dvpre[g] = d;
    }
}

inline unsigned blocks_of(long long items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

int launch_gen_linear(int M, int K, int N, const float* X, const float* W, const float* bias, const float* mask, int flags,
                      float* Y, hipStream_t st) {
    if (M <= 0 || N <= 0) return 0;
    hipLaunchKernelGGL(gen_linear_kernel, dim3(blocks_of(M, 64), blocks_of(N, 64)), dim3(256), 0, st, M, K, N, X, W, bias, mask,
                       flags, Y);
    return check_launch("gen_linear_kernel");
}

size_t gen_linear_grad_workspace_floats(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return (size_t)grad_chunks(M, N, K) * ((size_t)N * K + N);
}

// An upper bound of gen_linear_grad_workspace_floats(M, N, K) over every M <= max_rows, in closed form: a chunk holds at least 32
// rows and there are at most the budget's chunk count, so chunks <= min(cmax, ceil(max_rows / 32)) -- monotone in max_rows.
size_t gen_linear_grad_workspace_floats_bound(long long max_rows, int N, int K) {
    if (max_rows <= 0 || N <= 0 || K <= 0) return 0;
    const size_t part = (size_t)N * K + N;
    size_t cmax = GEN_PART_BUDGET / part;
    if (cmax < 1) cmax = 1;
    if (cmax > GEN_MAX_CHUNKS) cmax = GEN_MAX_CHUNKS;
    const size_t by_rows = (size_t)((max_rows + 31) / 32);
    return (by_rows < cmax ? by_rows : cmax) * part;
}

int launch_gen_linear_grad(int M, int K, int N, const float* dY, const float* X, const float* dYb, float* workspace,
                           size_t workspace_floats, float* dW, float* db, hipStream_t st) {
    if (N <= 0 || K <= 0) return 0;
    if (M <= 0) {         // no rows: zero gradients
        if (hipMemsetAsync(dW, 0, (size_t)N * K * sizeof(float), st) != hipSuccess) return fail("hipMemsetAsync");
        if (db && hipMemsetAsync(db, 0, (size_t)N * sizeof(float), st) != hipSuccess) return fail("hipMemsetAsync");
        return 0;
    }
    if (workspace_floats < gen_linear_grad_workspace_floats(M, N, K)) return fail("aqg_graph_linear_grad: workspace too small");
    const int rpc = grad_chunk_rows(M, N, K), nch = grad_chunks(M, N, K);
    hipLaunchKernelGGL(gen_grad_partial_kernel, dim3(nch, blocks_of(N, 64), blocks_of(K, 64)), dim3(256), 0, st, M, N, K, rpc, dY, X,
                       dYb ? dYb : dY, workspace);
    hipLaunchKernelGGL(gen_grad_reduce_kernel, dim3(blocks_of((long long)N * K + N, 256)), dim3(256), 0, st, nch, N, K,
                       (const float*)workspace, dW, db);
    return check_launch("gen_grad kernels");
}

int launch_gen_aggregate(int n, int N, const float* Y, const int32_t* ptr, const int32_t* src, const float* w, const float* bias,
                         int relu, float* out, hipStream_t st) {
    if (n <= 0 || N <= 0) return 0;
    const dim3 grid(blocks_of(n, 4)), blk(256);
    const bool a16 = ((uintptr_t)Y & 15) == 0, a8 = ((uintptr_t)Y & 7) == 0;
    if (N % 4 == 0 && a16)
        hipLaunchKernelGGL(gen_aggregate_kernel<4>, grid, blk, 0, st, n, N, Y, ptr, src, w, bias, relu, out);
    else if (N % 2 == 0 && a8)
        hipLaunchKernelGGL(gen_aggregate_kernel<2>, grid, blk, 0, st, n, N, Y, ptr, src, w, bias, relu, out);
    else
        hipLaunchKernelGGL(gen_aggregate_kernel<1>, grid, blk, 0, st, n, N, Y, ptr, src, w, bias, relu, out);
    return check_launch("gen_aggregate_kernel");
}

int launch_gen_mean_pool(int N, const float* H, const int32_t* gptr, int G, float* pooled, hipStream_t st) {
    if (G <= 0 || N <= 0) return 0;
    hipLaunchKernelGGL(gen_pool_kernel, dim3(G), dim3(256), 0, st, H, N, gptr, G, pooled);
    return check_launch("gen_pool_kernel");
}

int launch_gen_mean_pool_backward(int n, int N, const float* dpooled, const int32_t* gptr, int G, const float* mask, float* dH,
                                  hipStream_t st) {
    if (n <= 0 || N <= 0) return 0;
    hipLaunchKernelGGL(gen_pool_backward_kernel, dim3(blocks_of(n, 4)), dim3(256), 0, st, n, N, dpooled, gptr, G, mask, dH);
    return check_launch("gen_pool_backward_kernel");
}

int launch_gen_heads(int G, int A, const float* logits, const float* vpre, float* policy, float* value, hipStream_t st,
                     const uint8_t* active) {
    if (G <= 0) return 0;
    hipLaunchKernelGGL(gen_heads_kernel, dim3(G), dim3(256), 0, st, G, A, logits, vpre, policy, value, active);
    return check_launch("gen_heads_kernel");
}

int launch_gen_heads_backward(int G, int A, const float* policy, const float* dpolicy, const float* value, const float* dvalue,
                              float* dlogits, float* dvpre, hipStream_t st) {
    if (G <= 0) return 0;
    hipLaunchKernelGGL(gen_heads_backward_kernel, dim3(G), dim3(256), 0, st, G, A, policy, dpolicy, value, dvalue, dlogits, dvpre);
    return check_launch("gen_heads_backward_kernel");
}

}  // namespace aqg
