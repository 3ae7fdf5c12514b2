// gcn_train_general.hip -- one optimisation step of GraphPolicyValueNetwork at ANY shape on board records (include/aqgnn.h,
// aqg_gcn_train_step_general): the arithmetic of the fused 6/128/3 step (gcn_train.hip, whose header states the losses), composed
// from the any-shape forward kernels and the width-generic primitives, with three kernels of its own.
//
//   prep       train_general_prep_kernel: the mean pool's graph pointer (and, with an order, this step's records gathered)
//   forward    featuriser, board_gcn_layer_kernel per layer with H_l kept, gen_mean_pool, gen_linear x 4, gen_heads: the policy and
//              value are bit for bit those of aqg_gcn_forward_boards_general (the same kernels; the pool sums in the same order)
//   loss       train_general_loss_kernel: both loss terms of each position, d loss / d policy and d loss / d value; with the
//              cross-entropy form (include/aqgnn.h "loss form") policy_value_loss_kernel, which also does gen_heads_backward's work
//   heads      gen_heads_backward, gen_linear (W [K,N], ReLU mask) and gen_linear_grad for the four head layers
//   trunk      gen_mean_pool_backward (mask H_L > 0) -> dP_L; per layer l = L .. 1 ONE launch of board_gcn_layer_backward_kernel:
//              dZ_l = A_hat dP_l (A_hat is symmetric on the board graph) and dP_{l-1} = (dZ_l W_l) x [H_{l-1} > 0], then
//              gen_linear_grad for dW_l = dZ_l^T H_{l-1} and db_l = colsum dP_l
//   finish     train_general_finish_kernel: torch.optim.Adam over all 2 L + 8 tensors in one launch, and the two batch-mean losses
//
// No atomics: every sum runs in an order fixed by the sizes, so two runs give bit-identical parameters.  No allocation and no host
// synchronisation: the caller owns one workspace of aqg_gcn_train_general_workspace_floats floats.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "wave_ops.hpp"
#include "train_adam.hpp"
#include "train_driver.hpp"
#include <type_traits>

namespace aqg {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int S = 36;                                    // LDS row stride of the slabs of 32 (board_gcn_layer_kernel's)
constexpr int MAXT = 2 * AQG_GENERAL_MAX_LAYERS + 8;     // parameter tensors of the largest network

__device__ __forceinline__ size_t row_of(const int64_t* order, int first, int b) {
    return order ? (size_t)order[first + b] : (size_t)(first + b);
}

// gptr[g] = g V for g = 0 .. B; with an order, this step's B records are copied to `gathered` (the featuriser reads them in place)
__global__ __launch_bounds__(256) void train_general_prep_kernel(int V, int B, const uint8_t* __restrict__ states72,
                                                                 const int64_t* __restrict__ order, int first, int32_t* __restrict__ gptr,
                                                                 uint8_t* __restrict__ gathered) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= B) gptr[i] = i * V;
    if (order && i < B * 72) {
        const int b = i / 72, k = i - 72 * b;
        gathered[i] = states72[(size_t)order[first + b] * 72 + k];
    }
}

// sum over the workgroup's 256 threads in a fixed order (a shuffle tree in each wave, then the 4 waves in order)
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_xor_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per position b, train_network.py:54-55,85-86 as in gcn_train_heads.hpp:
//   loss[b] = { -sum_a t_a log_softmax(p)_a,  (v - z)^2 },  dpol[b][a] = (softmax(p)_a sum_a t_a - t_a) / B,  dval[b] = 2 (v - z) / B
// with p = the network's (already softmaxed) policy, v its tanh value; the targets are rows order[first + b] (or first + b).
__global__ __launch_bounds__(256) void train_general_loss_kernel(int B, int A, const float* __restrict__ policy,
                                                                 const float* __restrict__ value, const float* __restrict__ pi,
                                                                 const float* __restrict__ z, const int64_t* __restrict__ order, int first,
                                                                 float* __restrict__ loss, float* __restrict__ dpol,
                                                                 float* __restrict__ dval) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t src = row_of(order, first, b);
    const float* p = policy + (size_t)b * A;
    const float* t = pi + src * A;
    float ts = 0.f, s2 = 0.f;
    for (int a = tid; a < A; a += 256) { ts += t[a]; s2 += expf(p[a]); }     // p in [0, 1]: the second softmax needs no shift
    ts = block_sum(ts, red);
    s2 = block_sum(s2, red);
    const float ls2 = logf(s2), inv_b = 1.f / (float)B;
    float lp = 0.f;
    for (int a = tid; a < A; a += 256) {
        const float pa = p[a], ta = t[a];
        dpol[(size_t)b * A + a] = ((expf(pa) / s2) * ts - ta) * inv_b;
        lp += -ta * (pa - ls2);
    }
    lp = block_sum(lp, red);
    if (tid == 0) {
        const float dv = value[b] - z[src];
        loss[2 * b] = lp;
        loss[2 * b + 1] = dv * dv;
        dval[b] = 2.f * dv * inv_b;
    }
}

// max over the workgroup's 256 threads (block_sum's shape)
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The cross-entropy form of the loss (include/aqgnn.h "loss form", policy_form 1) in ONE launch, in place of train_general_loss_kernel
// + gen_heads_backward_kernel: one workgroup per position b, from the LOGITS x = logits[b] (never from ln p: exp(x_a - m) may
// underflow, (m - x_a) + ln se does not), the tanh value v and the targets of row order[first + b] (or first + b):
//   loss[b] = { sum_a t_a ((m - x_a) + ln se),  (v - z)^2 },  dlogits[b][a] = (exp(x_a - m) / se  T - t_a) / B,
//   dvpre[b] = w 2 (v - z) / B (1 - v^2)                      with m = max x, se = sum_a exp(x_a - m), T = sum_a t_a.
// Three passes over the row, every loop bounded by A (any A >= 1); the sums in block_sum's fixed order, no atomics.
__global__ __launch_bounds__(256) void policy_value_loss_kernel(int B, int A, const float* __restrict__ logits,
                                                                const float* __restrict__ value, const float* __restrict__ pi,
                                                                const float* __restrict__ z, const int64_t* __restrict__ order, int first,
                                                                float vw, float* __restrict__ loss, float* __restrict__ dlogits,
                                                                float* __restrict__ dvpre) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t src = row_of(order, first, b);
    const float* x = logits + (size_t)b * A;
    const float* t = pi + src * A;
    float mx = -INFINITY, ts = 0.f;
    for (int a = tid; a < A; a += 256) { mx = fmaxf(mx, x[a]); ts += t[a]; }
    const float m = block_max(mx, red);
    ts = block_sum(ts, red);
    float se = 0.f;
    for (int a = tid; a < A; a += 256) se += expf(x[a] - m);
    se = block_sum(se, red);
    const float lse = logf(se), inv_b = 1.f / (float)B;
    float lp = 0.f;
    for (int a = tid; a < A; a += 256) {
        const float xa = x[a], ta = t[a];
        dlogits[(size_t)b * A + a] = ((expf(xa - m) / se) * ts - ta) * inv_b;
        lp += ta * ((m - xa) + lse);
    }
    lp = block_sum(lp, red);
    if (tid == 0) {
        const float v = value[b], dv = v - z[src];
        loss[2 * b] = lp;
        loss[2 * b + 1] = dv * dv;
        dvpre[b] = vw * (2.f * dv * inv_b) * (1.f - v * v);
    }
}

// form 0 with a value weight: d loss / d value of train_general_loss_kernel scaled in place, between the two launches
__global__ __launch_bounds__(256) void scale_dval_kernel(int B, float vw, float* __restrict__ dval) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) dval[i] *= vw;
}

// The layer backward of P_l = A_hat (H_{l-1} W_l^T) + b_l, H_l = relu(P_l), given dP_l [B V, Hd] (ReLU already applied):
//   dZ_l = A_hat dP_l  (written once, by the workgroups of column block 0: gen_linear_grad forms dW_l from it)
//   dP_{l-1} = (dZ_l W_l) x [H_{l-1} > 0]   (when dPprev is non-NULL; W_l is [Hd, K] as PyTorch stores it)
// One workgroup (4 waves) per (board b, 64 columns k0 .. of dP_{l-1}); the contraction over Hd runs in slabs of 32: the slab of dP_l
// is staged in LDS, the 5-point stencil turns it into the slab of dZ_l there, and wave w accumulates the columns [16 w, 16 w + 16)
// of all RT row tiles on the f32-input MFMA (a k-ordered fmaf chain, as the forward's).  The structure of board_gcn_layer_kernel,
// in reverse.
template <int N>
__global__ __launch_bounds__(256) void board_gcn_layer_backward_kernel(int Hd, int K, const float* __restrict__ dP, const float* __restrict__ W,
                                                                       const float* __restrict__ Hprev, const int32_t* __restrict__ ell_idx,
                                                                       const float* __restrict__ ell_w, float* __restrict__ dZ,
                                                                       float* __restrict__ dPprev) {
    constexpr int V = N * N, RT = (V + 15) / 16, RP = 16 * RT;
    __shared__ alignas(16) float ps[V * S];      // dP_l slab [V][32]
    __shared__ alignas(16) float zs[RP * S];     // dZ_l slab [RP][32], rows V .. RP zero
    __shared__ alignas(16) float ws[64 * S];     // W_l^T slab [64 k][32 n]
    __shared__ int32_t li[V * 5];
    __shared__ float lw[V * 5];
    const int b = blockIdx.x, k0 = blockIdx.y * 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const size_t r0 = (size_t)b * V;
    const bool mm = dPprev != nullptr, wz = blockIdx.y == 0;
    for (int i = tid; i < V * 5; i += 256) {
        const int s = ell_idx[r0 * 5 + i];
        const int l = s - b * V;
        li[i] = (s >= 0 && l >= 0 && l < V) ? l : -1;
        lw[i] = ell_w[r0 * 5 + i];
    }
    for (int i = V * S + tid; i < RP * S; i += 256) zs[i] = 0.f;
    f32x4 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < Hd; n0 += 32) {
        __syncthreads();
        for (int idx = tid; idx < V * 32; idx += 256) {
            const int r = idx >> 5, j = idx & 31;
            ps[r * S + j] = n0 + j < Hd ? dP[(r0 + r) * Hd + n0 + j] : 0.f;
        }
        if (mm) {
            for (int idx = tid; idx < 64 * 32; idx += 256) {
                const int j = idx & 63, n = idx >> 6;
                ws[j * S + n] = (k0 + j < K && n0 + n < Hd) ? W[(size_t)(n0 + n) * K + k0 + j] : 0.f;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < V * 32; idx += 256) {
            const int r = idx >> 5, j = idx & 31;
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                const int s = li[r * 5 + e];
                if (s < 0) continue;
                a = fmaf(lw[r * 5 + e], ps[s * S + j], a);
            }
            zs[r * S + j] = a;
            if (wz && n0 + j < Hd) dZ[(r0 + r) * Hd + n0 + j] = a;
        }
        if (!mm) continue;
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < 32; kk += 4) {
            const float bw = ws[(16 * w + c) * S + kk + q];
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[t] = mfma4(zs[(16 * t + c) * S + kk + q], bw, acc[t]);
        }
    }
    if (!mm) return;
    const int k = k0 + 16 * w + c;
    if (k >= K) return;
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {                  // C/D: row 4 q + i of tile t, column c of wave w's 16
            const int r = 16 * t + 4 * q + i;
            if (r >= V) continue;
            const size_t o = (r0 + r) * K + k;
            dPprev[o] = Hprev[o] > 0.f ? acc[t][i] : 0.f;
        }
}

// torch.optim.Adam over every parameter element of the network (train_adam.hpp); and, in the workgroup after the last
// element's (when `loss` is set), its loss_means.
struct AdamJobs {
    float* p[MAXT]; const float* g[MAXT]; float* m[MAXT]; float* v[MAXT];
    unsigned int end[MAXT];          // running element count after tensor i
    int tensors, update, B;
    AdamStep adam;
    LossMeans means;
};

// Two instantiations: <AdamJobs>, the launch as it has always been (the same instructions and registers as before the template), and
// <AdamOptimJobs>, with the optimiser controls of train_adam.hpp: every Adam workgroup first adds up the norm's partials and derives
// the clip coefficient.
struct AdamOptimJobs : AdamJobs { OptimArgs<MAXT> op; };
template <class Jobs>
__global__ __launch_bounds__(256) void train_general_finish_kernel(Jobs jb, unsigned int adam_blocks) {
    constexpr bool OPT = std::is_same_v<Jobs, AdamOptimJobs>;
    if (blockIdx.x == adam_blocks) {
        loss_means(jb.means, jb.B);
        return;
    }
    float coef = 1.f;
    if constexpr (OPT) {
        __shared__ float norm_red[4];
        coef = optim_prologue(jb.op.s, norm_red);
    }
    const unsigned int e0 = blockIdx.x * 256 + threadIdx.x;
    if (e0 >= jb.end[jb.tensors - 1]) return;
    int lo = 0, hi = jb.tensors - 1;               // the first tensor i with e0 < end[i]
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (e0 < jb.end[mid]) hi = mid; else lo = mid + 1; }
    const int i = lo;
    const unsigned int e = e0 - (i ? jb.end[i - 1] : 0u);
    float gr = jb.g[i][e], opar = jb.p[i][e];
    const float om = jb.m[i][e], ov = jb.v[i][e];
    if constexpr (OPT) {
        const GradParam gp = optim_apply(coef, jb.op.wd[i], jb.op.s.decoupled, jb.adam.lr, gr, opar);
        gr = gp.g; opar = gp.p;
    }
    const AdamMoments n = adam_moments(jb.adam, gr, om, ov);
    jb.m[i][e] = n.m; jb.v[i][e] = n.v;
    jb.p[i][e] = adam_param(jb.adam, opar, n);
}

inline size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }
inline unsigned blocks_of(long long items, int per) { return (unsigned)((items + per - 1) / per); }

struct TrainWorkspace {
    float* x0; float* ell_w; int32_t* ell_idx; int32_t* gptr; uint8_t* states; float* h; size_t h_stride;
    float* pooled; float* hp; float* hv; float* logits; float* vpre; float* policy; float* value; float* loss; float* loss_mean;
    float* dpol; float* dval; float* dlogits; float* dvpre; float* dhp; float* dhv; float* dpooled; float* dp[2]; float* dz;
    float* part; size_t part_floats;
};

// the partial tiles of the largest gen_linear_grad of a step with up to B positions (a closed-form bound, monotone in B: the
// exact need of gen_linear_grad is not monotone in its row count, so every region of train_layout grows with B and the layout of
// max_batch serves every smaller batch)
inline size_t part_floats(int N, int Hd, int L, int A, int B) {
    const long long R = (long long)B * N * N;
    const int Hh = Hd / 2;
    size_t m = 0;
    const size_t c[5] = {gen_linear_grad_workspace_floats_bound(B, A, Hh), gen_linear_grad_workspace_floats_bound(B, 1, Hh),
                         gen_linear_grad_workspace_floats_bound(B, Hh, Hd), gen_linear_grad_workspace_floats_bound(R, Hd, 6),
                         L > 1 ? gen_linear_grad_workspace_floats_bound(R, Hd, Hd) : 0};
    for (size_t x : c) m = x > m ? x : m;
    return m;
}

// floats of each region, every one rounded up to 64 (256 bytes: the vector loads need 16-byte alignment); the partial tiles last
inline size_t train_layout(int N, int Hd, int L, int A, int B, TrainWorkspace* ws, float* base) {
    const size_t R = (size_t)B * N * N, Hh = (size_t)(Hd / 2), RH = round64(R * Hd);
    const size_t sz[26] = {R * 6, R * 5, R * 5, (size_t)B + 1, (size_t)B * 18, RH * L,
                           (size_t)B * Hd, (size_t)B * Hh, (size_t)B * Hh, (size_t)B * A, (size_t)B, (size_t)B * A, (size_t)B,
                           (size_t)B * 2, 2, (size_t)B * A, (size_t)B, (size_t)B * A, (size_t)B, (size_t)B * Hh, (size_t)B * Hh,
                           (size_t)B * Hd, RH, RH, RH, part_floats(N, Hd, L, A, B)};
    size_t off[26], total = 0;
    for (int i = 0; i < 26; ++i) { off[i] = total; total += round64(sz[i]); }
    if (ws && base) {
        ws->x0 = base + off[0]; ws->ell_w = base + off[1]; ws->ell_idx = reinterpret_cast<int32_t*>(base + off[2]);
        ws->gptr = reinterpret_cast<int32_t*>(base + off[3]); ws->states = reinterpret_cast<uint8_t*>(base + off[4]);
        ws->h = base + off[5]; ws->h_stride = RH;
        ws->pooled = base + off[6]; ws->hp = base + off[7]; ws->hv = base + off[8]; ws->logits = base + off[9]; ws->vpre = base + off[10];
        ws->policy = base + off[11]; ws->value = base + off[12]; ws->loss = base + off[13]; ws->loss_mean = base + off[14];
        ws->dpol = base + off[15]; ws->dval = base + off[16]; ws->dlogits = base + off[17]; ws->dvpre = base + off[18];
        ws->dhp = base + off[19]; ws->dhv = base + off[20]; ws->dpooled = base + off[21]; ws->dp[0] = base + off[22];
        ws->dp[1] = base + off[23]; ws->dz = base + off[24]; ws->part = base + off[25]; ws->part_floats = sz[25];
    }
    return total;
}

template <int N>
int launch_layer_backward_n(int B, int Hd, int K, const float* dP, const float* W, const float* Hprev, const int32_t* ell_idx,
                            const float* ell_w, float* dZ, float* dPprev, hipStream_t st) {
    const dim3 grid(B, dPprev ? (K + 63) / 64 : 1), blk(256);
    hipLaunchKernelGGL((board_gcn_layer_backward_kernel<N>), grid, blk, 0, st, Hd, K, dP, W, Hprev, ell_idx, ell_w, dZ, dPprev);
    return check_launch("board_gcn_layer_backward_kernel");
}

int launch_layer_backward(int N, int B, int Hd, int K, const float* dP, const float* W, const float* Hprev, const int32_t* ell_idx,
                          const float* ell_w, float* dZ, float* dPprev, hipStream_t st) {
    return for_board_size(N, [&](auto n) { return launch_layer_backward_n<decltype(n)::value>(B, Hd, K, dP, W, Hprev, ell_idx, ell_w, dZ, dPprev, st); });
}

// forward, losses and backward of B positions (rows order[first ..] or first ..): gradients into t.grads, per-position losses
int forward_backward(const aqg_train_general& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first,
                     int B, const TrainWorkspace& ws, float* policy, float* value, float* loss, hipStream_t st, const aqg_loss* lf) {
    const int N = t.board_size, V = N * N, Hd = t.hidden, L = t.num_layers, A = t.policy_size, Hh = Hd / 2, R = B * V;
    float* const* p = t.params;
    float* const* g = t.grads;
    if (int r = launch_train_general_prep(V, B, states72, order, first, ws.gptr, ws.states, st)) return r;
    const uint8_t* recs = order ? ws.states : states72 + (size_t)first * 72;
    if (int r = launch_gcn_boards_graph(N, recs, 0, B, ws.x0, ws.ell_idx, ws.ell_w, st)) return r;
    // forward: every layer's output kept (H_l = ws.h + (l - 1) h_stride), then the pool and the heads of the any-shape forward
    auto H = [&](int l) -> float* { return l == 0 ? ws.x0 : ws.h + (size_t)(l - 1) * ws.h_stride; };
    for (int l = 1; l <= L; ++l)
        if (int r = launch_board_gcn_layer(N, B, l == 1 ? 6 : Hd, Hd, H(l - 1), p[2 * l - 2], p[2 * l - 1], ws.ell_idx, ws.ell_w,
                                           nullptr, H(l), nullptr, st))
            return r;
    if (int r = launch_gen_mean_pool(Hd, H(L), ws.gptr, B, ws.pooled, st)) return r;
    const int o = 2 * L;
    if (int r = launch_gen_linear(B, Hd, Hh, ws.pooled, p[o], p[o + 1], nullptr, AQG_LIN_RELU, ws.hp, st)) return r;
    if (int r = launch_gen_linear(B, Hh, A, ws.hp, p[o + 2], p[o + 3], nullptr, 0, ws.logits, st)) return r;
    if (int r = launch_gen_linear(B, Hd, Hh, ws.pooled, p[o + 4], p[o + 5], nullptr, AQG_LIN_RELU, ws.hv, st)) return r;
    if (int r = launch_gen_linear(B, Hh, 1, ws.hv, p[o + 6], p[o + 7], nullptr, 0, ws.vpre, st)) return r;
    if (int r = launch_gen_heads(B, A, ws.logits, ws.vpre, policy, value, st, nullptr)) return r;
    // losses and the way back to the logits / the pre-tanh value
    if (int r = launch_train_losses(B, A, ws.logits, policy, value, pi, z, order, first, lf, loss, ws.dpol, ws.dval, ws.dlogits,
                                    ws.dvpre, st))
        return r;
    // heads: second layers, the hidden layers' gradients (ReLU mask = the saved activations), first layers, d loss / d pooled
    float* part = ws.part;
    const size_t pf = ws.part_floats;
    if (int r = launch_gen_linear_grad(B, Hh, A, ws.dlogits, ws.hp, nullptr, part, pf, g[o + 2], g[o + 3], st)) return r;
    if (int r = launch_gen_linear_grad(B, Hh, 1, ws.dvpre, ws.hv, nullptr, part, pf, g[o + 6], g[o + 7], st)) return r;
    if (int r = launch_gen_linear(B, A, Hh, ws.dlogits, p[o + 2], nullptr, ws.hp, AQG_LIN_W_KN, ws.dhp, st)) return r;
    if (int r = launch_gen_linear(B, 1, Hh, ws.dvpre, p[o + 6], nullptr, ws.hv, AQG_LIN_W_KN, ws.dhv, st)) return r;
    if (int r = launch_gen_linear_grad(B, Hd, Hh, ws.dhp, ws.pooled, nullptr, part, pf, g[o], g[o + 1], st)) return r;
    if (int r = launch_gen_linear_grad(B, Hd, Hh, ws.dhv, ws.pooled, nullptr, part, pf, g[o + 4], g[o + 5], st)) return r;
    if (int r = launch_gen_linear(B, Hh, Hd, ws.dhp, p[o], nullptr, nullptr, AQG_LIN_W_KN, ws.dpooled, st)) return r;
    if (int r = launch_gen_linear(B, Hh, Hd, ws.dhv, p[o + 4], nullptr, nullptr, AQG_LIN_W_KN | AQG_LIN_ACCUMULATE, ws.dpooled, st))
        return r;
    // trunk: dP_L = d pooled / V x [H_L > 0], then one fused launch and one weight gradient per layer
    if (int r = launch_gen_mean_pool_backward(R, Hd, ws.dpooled, ws.gptr, B, H(L), ws.dp[L & 1], st)) return r;
    for (int l = L; l >= 1; --l) {
        const int K = l == 1 ? 6 : Hd;
        float* dP = ws.dp[l & 1];
        if (int r = launch_layer_backward(N, B, Hd, K, dP, p[2 * l - 2], H(l - 1), ws.ell_idx, ws.ell_w, ws.dz,
                                          l == 1 ? nullptr : ws.dp[(l - 1) & 1], st))
            return r;
        if (int r = launch_gen_linear_grad(R, K, Hd, ws.dz, H(l - 1), dP, part, pf, g[2 * l - 2], g[2 * l - 1], st)) return r;
    }
    return 0;
}

int launch_finish(const aqg_train_general& t, int B, bool update, int step, const float* loss, float* loss_mean, float* loss_sums,
                  hipStream_t st, const OptimLaunch* ol = nullptr) {
    const int T = 2 * t.num_layers + 8;
    AdamJobs jb{};
    unsigned int run = 0;
    size_t numel[MAXT];
    train_general_tensor_sizes(t, numel);
    for (int i = 0; i < T; ++i) {
        run += (unsigned int)numel[i];
        jb.end[i] = run;
        jb.p[i] = t.params[i]; jb.g[i] = t.grads[i]; jb.m[i] = t.adam_m[i]; jb.v[i] = t.adam_v[i];
    }
    jb.tensors = T; jb.update = update; jb.B = B;
    jb.adam = adam_step(t.lr, t.beta1, t.beta2, t.eps, step);
    jb.means = LossMeans{loss, loss_mean, loss_sums};
    const unsigned int adam_blocks = update ? blocks_of(run, 256) : 0u;
    const unsigned int grid = adam_blocks + (loss && B > 0 ? 1u : 0u);
    if (grid == 0) return 0;
    if (ol && update) {
        AdamOptimJobs jo{};
        static_cast<AdamJobs&>(jo) = jb;
        fill_optim(*ol, T, &jo.op.s, jo.op.wd);
        hipLaunchKernelGGL(train_general_finish_kernel<AdamOptimJobs>, dim3(grid), dim3(256), 0, st, jo, adam_blocks);
        return check_launch("train_general_finish_kernel<AdamOptimJobs>");
    }
    hipLaunchKernelGGL(train_general_finish_kernel<AdamJobs>, dim3(grid), dim3(256), 0, st, jb, adam_blocks);
    return check_launch("train_general_finish_kernel");
}

int validate(const aqg_train_general& t, const char* what) {
    if (!board_size_supported(t.board_size)) return fail(what, "board_size must be 3, 5, 7 or 9");
    aqg_gcn_general_net net{};
    net.num_features = t.num_features; net.hidden = t.hidden; net.num_layers = t.num_layers; net.policy_size = t.policy_size;
    const char* why = "";
    if (t.num_layers >= 1 && t.num_layers <= AQG_GENERAL_MAX_LAYERS)
        for (int i = 0; i < 2 * t.num_layers + 8; ++i) net.params[i] = t.params[i];
    if (check_general_net(&net, &why)) return fail(what, why);
    return 0;
}

}  // namespace

// elements of each of the 2 L + 8 tensors, in parameter order
void train_general_tensor_sizes(const aqg_train_general& t, size_t* numel) {
    const int L = t.num_layers, Hd = t.hidden, Hh = Hd / 2, A = t.policy_size;
    const size_t hs[8] = {(size_t)Hh * Hd, (size_t)Hh, (size_t)A * Hh, (size_t)A, (size_t)Hh * Hd, (size_t)Hh, (size_t)Hh, 1};
    for (int i = 0; i < 2 * L + 8; ++i)
        numel[i] = i >= 2 * L ? hs[i - 2 * L] : (i & 1) ? (size_t)Hd : (size_t)Hd * (i == 0 ? 6 : Hd);
}

// the prep and loss kernels, shared with the residual CNN's step (cnn_train.hip): the same graph pointer / gathered records and the
// same two loss terms and their gradients
int launch_train_general_prep(int V, int B, const uint8_t* states72, const int64_t* order, int first, int32_t* gptr, uint8_t* gathered,
                              hipStream_t st) {
    hipLaunchKernelGGL(train_general_prep_kernel, dim3(blocks_of(order ? (long long)B * 72 : (long long)B + 1, 256)), dim3(256), 0, st,
                       V, B, states72, order, first, gptr, gathered);
    return check_launch("train_general_prep_kernel");
}

int launch_train_general_loss(int B, int A, const float* policy, const float* value, const float* pi, const float* z,
                              const int64_t* order, int first, float* loss, float* dpol, float* dval, hipStream_t st) {
    hipLaunchKernelGGL(train_general_loss_kernel, dim3(B), dim3(256), 0, st, B, A, policy, value, pi, z, order, first, loss, dpol, dval);
    return check_launch("train_general_loss_kernel");
}

int launch_policy_value_loss(int B, int A, const float* logits, const float* value, const float* pi, const float* z, const int64_t* order,
                             int first, float value_weight, float* loss, float* dlogits, float* dvpre, hipStream_t st) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(policy_value_loss_kernel, dim3(B), dim3(256), 0, st, B, A, logits, value, pi, z, order, first, value_weight, loss,
                       dlogits, dvpre);
    return check_launch("policy_value_loss_kernel");
}

// both loss terms of B positions and the way back to the logits / the pre-tanh value, in the form lf asks for (null = the
// reference's, weight 1: the two launches there have always been)
int launch_train_losses(int B, int A, const float* logits, const float* policy, const float* value, const float* pi, const float* z,
                        const int64_t* order, int first, const aqg_loss* lf, float* loss, float* dpol, float* dval, float* dlogits,
                        float* dvpre, hipStream_t st) {
    if (lf && lf->policy_form == 1)
        return launch_policy_value_loss(B, A, logits, value, pi, z, order, first, lf->value_weight, loss, dlogits, dvpre, st);
    if (int r = launch_train_general_loss(B, A, policy, value, pi, z, order, first, loss, dpol, dval, st)) return r;
    if (lf && lf->value_weight != 1.f) {
        hipLaunchKernelGGL(scale_dval_kernel, dim3(blocks_of(B, 256)), dim3(256), 0, st, B, lf->value_weight, dval);
        if (int r = check_launch("scale_dval_kernel")) return r;
    }
    return launch_gen_heads_backward(B, A, policy, dpol, value, dval, dlogits, dvpre, st);
}

size_t train_general_workspace_floats(int N, int hidden, int num_layers, int policy_size, int max_batch) {
    if (!board_size_supported(N) || hidden < 2 || hidden > 1024 || num_layers < 1 || num_layers > AQG_GENERAL_MAX_LAYERS ||
        policy_size < 1 || policy_size > 4096 || max_batch < 1)
        return 0;
    return train_layout(N, hidden, num_layers, policy_size, max_batch, nullptr, nullptr);   // monotone in the batch: O(1) host work
}

// the any-shape GNN as a kind of train_driver.hpp
struct GeneralKind {
    using Workspace = TrainWorkspace;
    static constexpr const char *step_name = "aqg_gcn_train_step_general", *steps_name = "aqg_gcn_train_steps_general";
    static constexpr const char* workspace_refusal = "workspace too small (aqg_gcn_train_general_workspace_floats)";
    static constexpr bool empty_batch_mode1_updates = true;     // batch 0, mode 1: Adam still runs, on whatever grads holds
    static constexpr auto validate = aqg::validate;
    static constexpr auto forward_backward = aqg::forward_backward;
    static constexpr auto launch_finish = aqg::launch_finish;
    static size_t layout(const aqg_train_general& t, int B, TrainWorkspace* ws) {
        return train_layout(t.board_size, t.hidden, t.num_layers, t.policy_size, B, ws, ws ? t.workspace : nullptr);
    }
};

int train_step_general(const aqg_train_general& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
                       const OptimPlan* plan, const aqg_weight_average* avg, const aqg_loss* lf) {
    return train_driver_step<GeneralKind>(t, states72, pi, z, mode, st, plan, avg, lf);
}
int train_steps_general(const aqg_train_general& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                        long long positions, float* loss_sums, hipStream_t st, const OptimPlan* plan,
                        const aqg_weight_average* avg, const aqg_loss* lf) {
    return train_driver_steps<GeneralKind>(t, states72, pi, z, order, positions, loss_sums, st, plan, avg, lf);
}

}  // namespace aqg
