// gcn_train_heads.hpp -- the heads of the fused training step: one position's policy / value heads, both losses and the head
// gradients inside the per-board kernels.  Inlined into the exact-f32 body (gcn_train_exact.hpp) and a real callee of the split
// body (heads_board_call, gcn_train_split.hip).
#pragma once
#include "gcn_train_common.hpp"

namespace aqg {

// ---------------------------------------------------------------------------------------------
// heads, losses and the way back to the pooled features, inside the per-board kernels.
//   train_network.py:54,85: CrossEntropyLoss(policy_pred, policy_target) with policy_pred ALREADY softmaxed
//   (pv_network_gnn.py:42,62) and probability targets: l_b = -sum_a t_a log_softmax(pol)_a, mean over the batch
//   train_network.py:55,86: MSELoss(value_pred.squeeze(), value_target), mean over the batch
// Leaves: pol, val, loss terms; hp, hv (hidden layers); lg = d loss / d logits, vp = d loss / d pre-tanh value;
// dhp, dhv (gradients at the hidden layers, ReLU applied); dg = d loss / d pooled features.
// ---------------------------------------------------------------------------------------------
struct HeadParams { const float* p[8]; };        // state_dict tensors 6..13
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_f(float old, float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float x) {              // fixed order: quads, 8, 16, 32, 64 lanes
    x += dpp_f<0xB1, 0xf>(0.f, x);     // quad_perm [1,0,3,2]
    x += dpp_f<0x4E, 0xf>(0.f, x);     // quad_perm [2,3,0,1]
    x += dpp_f<0x141, 0xf>(0.f, x);    // row_half_mirror
    x += dpp_f<0x140, 0xf>(0.f, x);    // row_mirror: 16 lanes agree
    x += dpp_f<0x142, 0xa>(0.f, x);    // row_bcast15 -> rows 1, 3
    x += dpp_f<0x143, 0xc>(0.f, x);    // row_bcast31 -> rows 2, 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
struct TrainHeadsSmem {
    float gs[TH], hs[TH], dhs[TH], dl[256], red[2][8][2];
    float dgv[TH];                       // d loss / d pooled features: the result the backward pass starts from
    alignas(16) float part[32][TH];      // per (wave, row group): partial sums over that group's weight rows
};
__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]))); }
// One position's heads, losses and head gradients by a workgroup of NW = 8 wavefronts (all of them load and multiply; the softmax /
// loss reductions run on wave 0).  The caller has put the pooled features into sm.gs (published by the first barrier in here); on
// return sm.dgv = dg.
//
// Weight access.  Every matrix is read ONCE, by 16-byte loads, into registers that serve its forward product AND its transposed
// product on the way back: a quarter wave (16 lanes = one DPP row) owns a weight row, lane l of it holds columns 4 l .. 4 l + 3 (and
// 64 + 4 l .. for the 128-wide first layers), so
//   forward    y[row]  = sum_k W[row][k] x[k]     = 4 or 8 FMAs per lane + four DPP row rotations
//   backward   dx[k]  += dy[row] W[row][k]          = FMAs into the lane's own columns, no reduction until the rows of the 4 NW
//                                                     quarter waves are added up through LDS in a fixed order.
// (Before: one row per wave instruction with a 64-lane reduction per row, policy_head.2 and both first layers read twice, the
//  second time with 4-byte strided loads -- 180 vector-memory instructions and ~100 weight registers per lane; now 15 and 60.)
//
// LF, the loss form (include/aqgnn.h "loss form"): LOSS_PLAIN = the reference's, as this body has always been (vw is not looked at);
// LOSS_CE = the cross-entropy taken from the logits wave 0 already holds -- no second exponential round, no s2 / ls2, no dot
// reduction -- with the value weight vw; LOSS_REF_W = the reference's policy term with the value weight.  Everything behind dl[]
// and dvp is the same in all three.
constexpr int LOSS_PLAIN = 0, LOSS_CE = 1, LOSS_REF_W = 2;
template <int LF = LOSS_PLAIN>
__device__ __forceinline__ void heads_board(TrainHeadsSmem& sm, int b, const HeadParams& Pm,
                                            const float* __restrict__ pi_all, const float* __restrict__ z_all,
                                            const int64_t* __restrict__ order, int first, int A, int B,
                                            float* __restrict__ hp, float* __restrict__ hv, float* __restrict__ lg,
                                            float* __restrict__ pol, float* __restrict__ vp, float* __restrict__ val,
                                            float* __restrict__ loss, float* __restrict__ dhp, float* __restrict__ dhv,
                                            float vw = 1.f) {
    float (&gs)[TH] = sm.gs; float (&hs)[TH] = sm.hs; float (&dhs)[TH] = sm.dhs; float (&dl)[256] = sm.dl;
    float (&red)[2][8][2] = sm.red;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rg = lane >> 4, l = lane & 15;
    const bool feat = t < TH;                                       // threads 0..127: one pooled feature / hidden unit each
    const float *Wp1 = Pm.p[0], *bp1 = Pm.p[1], *Wp2 = Pm.p[2], *bp2 = Pm.p[3], *Wv1 = Pm.p[4], *bv1 = Pm.p[5], *Wv2 = Pm.p[6], *bv2 = Pm.p[7];
    const size_t rec = record_of(order, first, b);
    TS_DECL
    constexpr int NW = 8;
    constexpr int HG = TH / (4 * NW);                               // first-layer row groups per wave (4 rows each)
    constexpr int LG = 64 / NW;                                     // policy_head.2 row groups per wave: 64 groups = 256 rows >= A
    f32x4 w1a[HG], w1b[HG], w2[LG];
    float hb[HG];
#pragma unroll
    for (int i = 0; i < HG; ++i) {
        const int o = 4 * (wave + NW * i) + rg;                     // hidden unit: 0..63 policy head, 64..127 value head
        const float* wr = (o < HH ? Wp1 + (size_t)o * TH : Wv1 + (size_t)(o - HH) * TH) + 4 * l;
        w1a[i] = ld4(wr); w1b[i] = ld4(wr + 64);
        hb[i] = o < HH ? bp1[o] : bv1[o - HH];
    }
#pragma unroll
    for (int i = 0; i < LG; ++i) {
        const int a = 4 * (wave + NW * i) + rg;
        w2[i] = a < A ? ld4(Wp2 + (size_t)a * HH + 4 * l) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // wave 0's inputs of the softmax / loss section, requested up front with everything else: targets and logit biases of its four
    // logits per lane, the value head's second layer
    float tgq[4], lbq[4], wv2q = 0.f, bvq = 0.f, ztq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int a = lane + 64 * j;
        const bool ok = wave == 0 && a < A;
        tgq[j] = ok ? pi_all[rec * A + a] : 0.f;
        lbq[j] = ok ? bp2[a] : 0.f;
    }
    if (wave == 0) { wv2q = Wv2[lane]; bvq = bv2[0]; ztq = z_all[rec]; }
    __syncthreads();
    TS(1, 0)
    {   // hidden layers: hs[0..63] policy, hs[64..127] value
        const f32x4 g0 = ld4(gs + 4 * l), g1 = ld4(gs + 64 + 4 * l);
#pragma unroll
        for (int i = 0; i < HG; ++i) {
            const int o = 4 * (wave + NW * i) + rg;
            const float s = fmaxf(row16_sum(dot4(w1a[i], g0) + dot4(w1b[i], g1)) + hb[i], 0.f);
            if (l == 0) {
                hs[o] = s;
                (o < HH ? hp : hv)[(size_t)b * HH + (o & 63)] = s;
            }
        }
    }
    __syncthreads();
    TS(1, 1)
    {
        const f32x4 h4 = ld4(hs + 4 * l);
#pragma unroll
        for (int i = 0; i < LG; ++i) {
            const int a = 4 * (wave + NW * i) + rg;
            const float s = row16_sum(dot4(w2[i], h4));
            if (l == 0 && a < A) dl[a] = s;                          // (dl is reused for d loss / d logits below)
        }
    }
    __syncthreads();
    TS(1, 2)
    // softmax, the reference's second softmax inside CrossEntropyLoss, both losses and the way back to the logits: ONE wavefront
    // holds all A <= 256 logits (four per lane) and every reduction is a wave reduction -- no barrier until the results are out
    // (four workgroup-wide reductions with a barrier each took 3.9 k cycles of the 12 k the heads need).
    if (wave == 0) {
        float lgv[4], tg[4], pv[4], dp[4];
        float mxl = -INFINITY, ts = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = lane + 64 * j;
            const bool ok = a < A;
            lgv[j] = ok ? dl[a] + lbq[j] : -INFINITY;
            tg[j] = tgq[j];
            mxl = fmaxf(mxl, lgv[j]);
            ts += tg[j];
        }
        const float m = wave_max(mxl);
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { pv[j] = lane + 64 * j < A ? expf(lgv[j] - m) : 0.f; se += pv[j]; }
        se = wave_sum(se);
        const float tsum = wave_sum(ts);
        float lp = 0.f;
        if constexpr (LF == LOSS_CE) {
            const float lse0 = logf(se);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = lane + 64 * j < A;
                pv[j] = pv[j] / se;                                  // the network's softmax (pv_network_gnn.py:42)
                dp[j] = ok ? (pv[j] * tsum - tg[j]) / (float)B : 0.f;    // d(mean_b l_b) / d logit
                lp += ok ? tg[j] * ((m - lgv[j]) + lse0) : 0.f;          // t (lse - x), from the logits: finite where pv underflows
            }
            lp = wave_sum(lp);
        }
        float dot = 0.f;
        if constexpr (LF != LOSS_CE) {
            float s2 = 0.f, e2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pv[j] = pv[j] / se;                                  // first softmax (the network's own, pv_network_gnn.py:42)
                e2[j] = lane + 64 * j < A ? expf(pv[j]) : 0.f;       // second softmax inside CrossEntropyLoss; p in [0,1]: no shift needed
                s2 += e2[j];
            }
            s2 = wave_sum(s2);
            const float ls2 = logf(s2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = lane + 64 * j < A;
                dp[j] = ok ? ((e2[j] / s2) * tsum - tg[j]) / (float)B : 0.f;   // d(mean_b l_b) / d pol
                lp += ok ? -tg[j] * (pv[j] - ls2) : 0.f;
                dot += dp[j] * pv[j];
            }
            lp = wave_sum(lp);
            dot = wave_sum(dot);
        }
        const float vsum = wave_sum(wv2q * hs[HH + lane]);       // the value head's 64-term dot product
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = lane + 64 * j;
            float dlogit;
            if constexpr (LF == LOSS_CE) dlogit = dp[j];
            else dlogit = a < A ? pv[j] * (dp[j] - dot) : 0.f;          // back through the first softmax
            dl[a] = dlogit;                                             // (zero for the rows A..255 of the padded row groups)
            if (a < A) {
                pol[(size_t)b * A + a] = pv[j];
                lg[(size_t)b * A + a] = dlogit;
            }
        }
        const float v = tanhf(vsum + bvq);
        const float dv = v - ztq;
        float dvp0 = (2.f * dv / (float)B) * (1.f - v * v);
        if constexpr (LF != LOSS_PLAIN) dvp0 *= vw;
        if (lane == 0) {
            red[0][0][0] = dvp0;
            val[b] = v;
            vp[b] = dvp0;
            loss[2 * b] = lp;
            loss[2 * b + 1] = dv * dv;
        }
    }
    __syncthreads();
    const float dvp = red[0][0][0];
    TS(1, 3)
    {   // d loss / d policy hidden layer: this quarter wave's rows of policy_head.2, transposed product
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < LG; ++i) acc += dl[4 * (wave + NW * i) + rg] * w2[i];
        st4(&sm.part[4 * wave + rg][4 * l], acc);
    }
    __syncthreads();
    TS(1, 4)
    if (feat) {
        const int j = t & 63;
        float s;
        if (t < HH) {
            s = 0.f;
#pragma unroll
            for (int r = 0; r < 4 * NW; ++r) s += sm.part[r][j];
        } else s = dvp * Wv2[j];
        if (!(hs[t] > 0.f)) s = 0.f;
        dhs[t] = s;
        (t < HH ? dhp : dhv)[(size_t)b * HH + j] = s;
    }
    __syncthreads();
    TS(1, 5)
    {   // dg = dhp W_p1 + dhv W_v1: this quarter wave's rows of the two first layers, transposed product
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < HG; ++i) {
            const float d = dhs[4 * (wave + NW * i) + rg];
            a0 += d * w1a[i]; a1 += d * w1b[i];
        }
        st4(&sm.part[4 * wave + rg][4 * l], a0);
        st4(&sm.part[4 * wave + rg][64 + 4 * l], a1);
    }
    __syncthreads();
    TS(1, 6)
    if (feat) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 4 * NW; ++r) s += sm.part[r][t];
        sm.dgv[t] = s;
    }
    __syncthreads();
}

}  // namespace aqg
