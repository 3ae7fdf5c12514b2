// gcn_train_exact.hpp -- the exact-f32 body of the fused training step: forward, heads + losses and backward of one position on
// the f32-input matrix pipe.  A header because two units inline it: train_board_kernel<N> (gcn_train_exact.hip) and the in-launch
// fallback of train_board_split_kernel (gcn_train_split.hip).
#pragma once
#include "gcn_train_heads.hpp"

namespace aqg {

// One board's graph in LDS: PyG gcn_norm weights in ELL form (self, U, D, L, R; a closed side has weight 0 and points at
// the node itself) and the six node features (pv_network_cnn.py:88-114; edges = open tile adjacencies, game_logic.py:145-167).
struct BoardGraph {
    float w[96 * 5];
    float x0[96 * 8];          // features, zero-padded to 8 columns and to whole row tiles
    unsigned char nb[96 * 4];
};

template <int N>
__device__ __forceinline__ void board_graph(BoardGraph& gr, const uint8_t* __restrict__ rec, int t) {
    constexpr int V = N * N, S = N - 1, VP = (V + 15) / 16 * 16;
    if (t < VP) {
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        st4(gr.x0 + t * 8, z);
        st4(gr.x0 + t * 8 + 4, z);
    }
    if (t < V) {
        const QState s = unpack72(rec);
        const int x = t / N, y = t % N;
        const bool slot_ok = x < S && y < S;
        const int slot = x * S + y;
        float* f = gr.x0 + t * 8;
        f[0] = (t == s.ppos) ? 1.f : 0.f;
        f[1] = (float)s.pwl;
        f[2] = (t == s.epos) ? 1.f : 0.f;
        f[3] = (float)s.ewl;
        f[4] = (slot_ok && ((s.hw >> slot) & 1)) ? 1.f : 0.f;
        f[5] = (slot_ok && ((s.vw >> slot) & 1)) ? 1.f : 0.f;
        const int ob = tile_open_bits<N>(s.hw, s.vw, t);
        const float di = 1.0f / sqrtf((float)(1 + __popc(ob)));
        const int nbr[4] = {t - N, t + N, t - 1, t + 1};
        gr.w[t * 5] = di * di;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const bool open = (ob >> d) & 1;
            float w = 0.f;
            int j = t;
            if (open) {
                const int obn = tile_open_bits<N>(s.hw, s.vw, nbr[d]);
                w = di * (1.0f / sqrtf((float)(1 + __popc(obn))));
                j = nbr[d];
            }
            gr.w[t * 5 + 1 + d] = w;
            gr.nb[t * 4 + d] = (unsigned char)j;
        }
    }
}

// (A_hat Z)[n][c4 .. c4+3] from an LDS image of Z with row stride ZS
template <int ZS>
__device__ __forceinline__ f32x4 agg_row(const float* Zs, const BoardGraph& gr, int n, int c4) {
    const float* w = gr.w + n * 5;
    const unsigned char* nb = gr.nb + n * 4;
    f32x4 a = w[0] * ld4(Zs + n * ZS + c4);
#pragma unroll
    for (int d = 0; d < 4; ++d) a += w[1 + d] * ld4(Zs + (int)nb[d] * ZS + c4);
    return a;
}

// acc[rt] += A[16 rt + r16][k] * B[k][col]  over k = 0..127; A an LDS image with row stride SA, B held in registers (the per-board
// kernel's LDS is full of activations): bw[ks] = W[(4 ks + q) * sk + col * sc], 32 strided dwords per lane, requested one phase
// ahead of their use.
__device__ __forceinline__ void load_bfrag(float (&bw)[32], const float* __restrict__ W, int sk, int sc, int col, int q) {
    const float* p = W + (size_t)col * sc + (size_t)q * sk;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) bw[ks] = p[(size_t)4 * ks * sk];
}
// Forward form (B[k][c] = W[c][k], a row of W per output column): 16-byte loads, lane (c, q) holds W[c][16 j + 4 q .. + 3], so the
// contraction index is enumerated as k = 16 j + 4 q + e and the A operand comes by ds_read_b128 (4 k values per lane; with
// the 132-float row stride the 16 rows of a quarter wave fall into 16 different 16-byte bank groups).  A quarter of the
// address-unit work of the dword form (16 segments per instruction either way, 8 instructions instead of 32).
__device__ __forceinline__ void load_bfrag4(f32x4 (&bv)[8], const float* __restrict__ W, int col, int q) {
    const float* p = W + (size_t)col * TH + 4 * q;
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = ld4(p + 16 * j);
}
template <int RT>
__device__ __forceinline__ void mfma_rows_reg4(f32x4 (&acc)[RT], const float* As, const f32x4 (&bv)[8], int r16, int q) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        f32x4 a[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) a[rt] = ld4(As + (16 * rt + r16) * SA + 16 * j + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = mfma4(a[rt][e], bv[j][e], acc[rt]);
        }
    }
}
template <int RT>
__device__ __forceinline__ void mfma_rows_reg(f32x4 (&acc)[RT], const float* As, const float (&bw)[32], int r16, int q) {
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = mfma4(As[(16 * rt + r16) * SA + 4 * ks + q], bw[ks], acc[rt]);
    }
}

// rows [0, V) x 128 floats of a global [.][128] array -> LDS image with row stride S, rows [V, VZ) zero-filled.  Two
// halves so that a caller can put other work between the issue of the loads and the LDS writes.
template <int V, int VZ, int NT> struct RowTile {
    static constexpr int IT = (VZ * 32 + NT - 1) / NT;
    f32x4 v[IT];
    __device__ __forceinline__ void issue(const float* __restrict__ src, int t) {
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = t + NT * k, n = i >> 5, c4 = (i & 31) * 4;
            v[k] = n < V ? ld4(src + (size_t)n * TH + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    template <int S> __device__ __forceinline__ void land(float* dst, int t) const {
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = t + NT * k, n = i >> 5, c4 = (i & 31) * 4;
            if (n < VZ) st4(dst + n * S + c4, v[k]);
        }
    }
};

// ---------------------------------------------------------------------------------------------
// The whole forward + backward of ONE position in one workgroup (8 wavefronts; wave w owns feature columns 16 w .. 16 w + 15,
// and rows 16 w .. of the weight gradients).  Nothing but the per-board partial gradients leaves the CU: the activations H1,
// H2 go to memory once and come back through the L2 of the same XCD, H3 never leaves LDS.  grid = B.
// LDS: Hs (A operand: H_l, then dZ_l), Zs (accumulator images; the heads' scratch), Hb (H_{l-1} as the B operand of the
// weight gradient and as the ReLU mask of the next layer down).
// ---------------------------------------------------------------------------------------------
struct TrunkParams { const float* p[6]; };       // state_dict tensors 0..5
// (the body is a device function over ONE raw LDS block so that the split-precision kernel (gcn_train_split.hip) can fall back to it for a board
//  whose values leave fp16 range without owning two sets of static LDS arrays; `hrows` = rows per board of the h1 / h2 buffers)
constexpr int F32_BODY_SMEM = (int)(sizeof(float) * (2 * 96 * SA + 84 * SB + 4 * TH) + sizeof(BoardGraph));
// LF, vw: the loss form and value weight of heads_board (gcn_train_heads.hpp), handed through
template <int N, int LF = LOSS_PLAIN>
__device__ __forceinline__ void train_board_f32_body(unsigned char* __restrict__ smem, const uint8_t* __restrict__ states72,
                                                     const int64_t* __restrict__ order, int first,
                                                     const TrunkParams& tp, const HeadParams& hpm, const float* __restrict__ pi_all,
                                                     const float* __restrict__ z_all, int A, int B, int hrows,
                                                     float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ g_out,
                                                     float* __restrict__ hp, float* __restrict__ hv, float* __restrict__ lg,
                                                     float* __restrict__ pol, float* __restrict__ vp, float* __restrict__ val,
                                                     float* __restrict__ loss, float* __restrict__ dhp, float* __restrict__ dhv,
                                                     float* __restrict__ part_dW3, float* __restrict__ part_dW2,
                                                     float* __restrict__ part_dW1, float* __restrict__ part_db, float vw = 1.f) {
    constexpr int V = N * N, RT = (V + 15) / 16, VK = (V + 3) / 4 * 4, NIT = (V + 15) / 16;
    float* const Hs = reinterpret_cast<float*>(smem);
    float* const Zs = Hs + 96 * SA;
    float* const Hb = Zs + 96 * SA;
    float* const cs = Hb + 84 * SB;
    BoardGraph& gr = *reinterpret_cast<BoardGraph*>(cs + 4 * TH);
    TrainHeadsSmem& hsm = *reinterpret_cast<TrainHeadsSmem*>(Zs);
    static_assert(sizeof(TrainHeadsSmem) <= sizeof(float) * 96 * SA && 16 * TH <= 84 * SB, "scratch aliases");
    const int b = blockIdx.x, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6, q = lane >> 4, r16 = lane & 15;
    const int col = 16 * wave + r16;
    const int c4 = (t & 31) * 4, rg = t >> 5;                       // aggregation mapping: 32 float4 per row x 16 row groups
    const float *W1 = tp.p[0], *b1 = tp.p[1], *W2 = tp.p[2], *b2 = tp.p[3], *W3 = tp.p[4], *b3 = tp.p[5];
    float bw[32];
    f32x4 bv4[8];
    f32x4 acc[RT];
    const f32x4 bias1 = ld4(b1 + c4), bias2 = ld4(b2 + c4), bias3 = ld4(b3 + c4);   // (ahead of the weight fragments in the load queue)
    auto zero_acc = [&]() {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto acc_to_Zs = [&]() {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) Zs[(16 * rt + 4 * q + i) * SA + col] = acc[rt][i];
        }
    };
    TS_DECL
    board_graph<N>(gr, states72 + record_of(order, first, b) * STATE72, t);
    load_bfrag4(bv4, W2, col, q);
    // Every weight this kernel will read was rewritten by the previous step's Adam update and is cold in this XCD's L2.  One
    // load per 64-byte line pulls W3 and the heads' matrices in now, under the graph setup and layer 1, instead of in front
    // of the phases that need them (the values are summed into `warm_sink`, which is never equal to its magic number).
    float warm[6];
    {
        const int l16 = t * 16;
        warm[0] = W3[l16]; warm[1] = W3[l16 + 512 * 16];
        warm[2] = hpm.p[0][l16]; warm[3] = hpm.p[4][l16];
        warm[4] = l16 < A * HH ? hpm.p[2][l16] : 0.f; warm[5] = l16 + 512 * 16 < A * HH ? hpm.p[2][l16 + 512 * 16] : 0.f;
    }
    for (int i = t; i < (96 - V) * 32; i += 512) st4(Hs + (V + (i >> 5)) * SA + (i & 31) * 4, f32x4{0.f, 0.f, 0.f, 0.f});   // rows V..95: zero for good
                                                                     // (the padding rows of every contraction over the nodes)
    __syncthreads();
    TS(2, 0)
    // ---- forward, layer 1 (K = 6 padded to 8)
    {
        const float w_lo = W1[col * TF + q];
        const float w_hi = (q < 2) ? W1[col * TF + 4 + q] : 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            a = mfma4(gr.x0[(16 * rt + r16) * 8 + q], w_lo, a);
            a = mfma4(gr.x0[(16 * rt + r16) * 8 + 4 + q], w_hi, a);
            acc[rt] = a;
        }
        acc_to_Zs();
    }
    __syncthreads();
    auto aggregate_relu = [&](const f32x4 bv, float* __restrict__ hglob) {          // Zs -> Hs (+ memory)
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int n = rg + 16 * it;
            if (n < V) {
                const f32x4 a = relu4(agg_row<SA>(Zs, gr, n, c4) + bv);
                st4(Hs + n * SA + c4, a);
                if (hglob) st4(hglob + ((size_t)b * hrows + n) * TH + c4, a);
            }
        }
    };
    aggregate_relu(bias1, h1);
    const float warm_sink = ((warm[0] + warm[1]) + (warm[2] + warm[3])) + (warm[4] + warm[5]);
    __syncthreads();
    TS(2, 1)
    // ---- layer 2
    zero_acc();
    mfma_rows_reg4<RT>(acc, Hs, bv4, r16, q);
    TS(2, 2)
    load_bfrag4(bv4, W3, col, q);
    acc_to_Zs();
    __syncthreads();
    aggregate_relu(bias2, h2);
    __syncthreads();
    TS(2, 3)
    // ---- layer 3 + mean pool (H3 stays in LDS: the backward needs only its sign)
    zero_acc();
    mfma_rows_reg4<RT>(acc, Hs, bv4, r16, q);
    TS(2, 4)
    acc_to_Zs();
    __syncthreads();
    {
        const f32x4 bv = bias3;
        f32x4 colsum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int n = rg + 16 * it;
            if (n < V) {
                const f32x4 a = relu4(agg_row<SA>(Zs, gr, n, c4) + bv);
                st4(Hs + n * SA + c4, a);
                colsum += a;
            }
        }
        st4(Hb + rg * TH + c4, colsum);                              // (Hb is free until the backward loads H2 into it)
    }
    __syncthreads();
    if (t < TH) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += Hb[r * TH + t];
        s /= (float)V;                                               // global_mean_pool
        hsm.gs[t] = s;
        g_out[(size_t)b * TH + t] = s;                               // (the head weight gradients are batch dot products with it)
    }
    TS(2, 5)
    // ---- heads, losses, head gradients (its first barrier publishes gs)
    heads_board<LF>(hsm, b, hpm, pi_all, z_all, order, first, A, B, hp, hv, lg, pol, vp, val, loss, dhp, dhv, vw);
    TS(2, 6)
    load_bfrag(bw, W3, TH, 1, col, q);                               // the data gradient's fragments of W3 (B[j][k] = W3[j][k]): land under layer 3's backward
    // ---- backward.  One layer: dP (accumulator layout) -> Zs;  dZ = A_hat dP -> Hs;  dW partial = dZ^T H_{l-1} (Hb)
    RowTile<V, VK, 512> hin;
    auto mask_and_bias_grad = [&](const float* M, int stride) -> float {   // acc (.)= [M > 0]; returns this lane's column sum
        float dbp = 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = 16 * rt + 4 * q + i;
                if (!(n < V && M[n * stride + col] > 0.f)) acc[rt][i] = 0.f;
                dbp += acc[rt][i];
            }
        }
        return dbp;
    };
    auto finish_layer = [&](float dbp, const float* __restrict__ hprev, float* __restrict__ pdb) {
        // callers have passed a barrier since the last read of Zs / of Hs as an A operand / of Hb as a mask
        acc_to_Zs();
        cs[q * TH + col] = dbp;
        if (hprev) hin.issue(hprev + (size_t)b * hrows * TH, t);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int n = rg + 16 * it;
            if (n < V) st4(Hs + n * SA + c4, agg_row<SA>(Zs, gr, n, c4));                 // dZ = A_hat dP (A_hat is symmetric)
        }
        if (t < TH) pdb[(size_t)b * TH + t] = (cs[t] + cs[TH + t]) + (cs[2 * TH + t] + cs[3 * TH + t]);
        if (hprev) hin.template land<SB>(Hb, t);
        __syncthreads();
    };
    auto weight_grad = [&](float* __restrict__ pdW) {                  // rows 16 wave .. of W_l, all 128 columns
        f32x4 wacc[8];
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) wacc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < VK / 4; ++ks) {
            const float a = Hs[(4 * ks + q) * SA + 16 * wave + r16];
#pragma unroll
            for (int ct = 0; ct < 8; ++ct) wacc[ct] = mfma4(a, Hb[(4 * ks + q) * SB + 16 * ct + r16], wacc[ct]);
        }
        float* dst = pdW + (size_t)b * TH * TH + (size_t)(16 * wave + 4 * q) * TH + r16;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[(size_t)i * TH + 16 * ct] = wacc[ct][i];
        }
    };
    // layer 3: dH3 = dg / V on every node (global_mean_pool backward); the mask is H3, still in Hs
    {
        const float v = hsm.dgv[col] / (float)V;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{v, v, v, v};
        const float dbp = mask_and_bias_grad(Hs, SA);
        __syncthreads();                                             // everybody has read dg (in Zs) and H3 (in Hs)
        finish_layer(dbp, h2, part_db + (size_t)2 * B * TH);
        TS(2, 7)
        weight_grad(part_dW3);
        TS(2, 8)
    }
    // layer 2: dH2 = dZ3 W3, mask H2 (in Hb)
    {
        zero_acc();
        mfma_rows_reg<RT>(acc, Hs, bw, r16, q);
        TS(2, 9)
        load_bfrag(bw, W2, TH, 1, col, q);
#ifdef AQG_TRAIN_DEBUG
        for (int rt = 0; rt < RT; ++rt) for (int i = 0; i < 4; ++i) if (16 * rt + 4 * q + i < V) DBG_PUT(1, B, b, 16 * rt + 4 * q + i, col, acc[rt][i])
        for (int i = t; i < V * TH; i += 512) DBG_PUT(2, B, b, i / TH, i % TH, Hs[(i / TH) * SA + (i % TH)])
#endif
        const float dbp = mask_and_bias_grad(Hb, SB);
#ifdef AQG_TRAIN_DEBUG
        for (int rt = 0; rt < RT; ++rt) for (int i = 0; i < 4; ++i) if (16 * rt + 4 * q + i < V) DBG_PUT(0, B, b, 16 * rt + 4 * q + i, col, acc[rt][i])
#endif
        __syncthreads();                                             // dZ3 (Hs) and H2 (Hb) are dead
        finish_layer(dbp, h1, part_db + (size_t)B * TH);
        TS(2, 10)
        weight_grad(part_dW2);
        TS(2, 11)
    }
    // layer 1: dH1 = dZ2 W2, mask H1 (in Hb); dW1 = dZ1^T X0 (six feature columns of one padded tile)
    {
        zero_acc();
        mfma_rows_reg<RT>(acc, Hs, bw, r16, q);
        TS(2, 12)
        const float dbp = mask_and_bias_grad(Hb, SB);
        __syncthreads();
        finish_layer(dbp, nullptr, part_db);
        TS(2, 13)
        f32x4 wacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < VK / 4; ++ks)
            wacc = mfma4(Hs[(4 * ks + q) * SA + 16 * wave + r16], r16 < 8 ? gr.x0[(4 * ks + q) * 8 + r16] : 0.f, wacc);
        if (r16 < TF) {
            float* dst = part_dW1 + (size_t)b * TH * TF + (size_t)(16 * wave + 4 * q) * TF + r16;
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[i * TF] = wacc[i];
        }
        TS(2, 14)
    }
    if (warm_sink == -1.2345678e-31f) part_db[0] = warm_sink;          // (keeps the warm-up loads alive; never taken)
}

}  // namespace aqg
