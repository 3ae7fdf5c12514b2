// gcn_trunk_exact.hip -- the exact-f32 trunk and heads of GraphPolicyValueNetwork.forward (pv_network_gnn.py:53-64) on 9x9 boards:
// what AQG_GNN_EXACT_F32 and trunk_variant 0 / 1 run, what serves a weight set or a board the split trunk's fp16 range guard
// reports (gcn_trunk_split.hip), and -- the heads -- what finishes the plain 3x3 / 5x5 / 7x7 path (gcn_boards_plain.hip).
//
// trunk kernel (boards): one 256-thread workgroup walks boards; per board the whole 3-layer GCN trunk runs
// out of ONE in-place LDS image H[81][132] f32 (HBM traffic: 72/24 B in, 512 B out per board):
//   setup   : wall masks -> per-node degree / sym-norm coefficients + the 6 node features (pv_network_cnn.py:88-114)
//   layer 1 : aggregate the 6-wide features over the <=5-point wall-cut stencil, then 6->128 on VALU
//   layer 2,3: dense 128x128 contraction on f32-input MFMA (v_mfma_f32_16x16x4_f32; rows 0..79 as five
//             16-row tiles, row 80 on VALU -> no padded MFMA work), accumulators staged in registers and
//             written back in place; then the normalised neighbour gather (= PyG's scatter-add on this
//             fixed-degree graph) + bias + ReLU, again register-staged in place
//   pool    : global_mean_pool fused into the layer-3 gather
// Each wave owns 32 output columns and keeps its slice of W2^T and W3^T in registers for the whole kernel
// (128 VGPRs), so weights cost no LDS/L2 traffic per board.  K is permuted (lane quarter q covers
// k in [kbase[q], kbase[q]+32)) so every A fragment is 8 contiguous ds_read_b128 and the padded row stride
// (132 floats) keeps each 16-lane ds_read_b128 group on 16 distinct 16-byte bank slots.
//
// heads kernel (gcn_heads_kernel): policy MLP 128->64->209 (+Softmax) and value MLP 128->64->1 (+Tanh), 8 boards per workgroup.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "wave_ops.hpp"
#include "gcn_packed.hpp"

namespace aqg {

struct alignas(16) TrunkSmem {
    alignas(16) float H[81 * LD];      // in-place activation image, [node][channel]
    alignas(16) float X0[81 * FPAD];   // node features
    alignas(16) float AX[81 * FPAD];   // A_hat * X0 (layer-1 input after the 6-wide gather)
    alignas(16) float coef[96][8];     // per node: self, U, D, L, R gather coefficients (0 when the edge is cut), 3 pad
    int obits[96];                     // per node: open-edge bits (U,D,L,R) -- setup step 1 -> step 2
};

// Stripe row schedule shared by layer 1 and the stripe gathers: lane -> 4 columns (cg = lane & 7) of one row
// per iteration (rs = lane >> 3).  Iterations 0..7 take rows it + 8*rs (0..63): with the 132-float row stride
// the 16-lane ds_read_b128 groups then hit 16 distinct 16-byte bank slots.  Iterations 8..10 take rows
// 64 + 8*(it-8) + rs (64..80; the last one only row 80).
__device__ __forceinline__ int stripe_row(int it, int rs) { return it < 8 ? it + 8 * rs : 64 + 8 * (it - 8) + rs; }
constexpr int STRIPE_ITERS = 11;

// B fragments of W^T for this wave from the fragment-ordered copy: Wf[j][s] = W^T[kb + s][32*wave + 16*j + c].
// 16 fully coalesced dwordx4 loads (1 KiB per wave-instruction) off one scalar base + one lane offset.
__device__ __forceinline__ void load_wfrag(float (&Wf)[2][32], const float* __restrict__ WF, int wave, int lane) {
    const float* base = WF + (size_t)__builtin_amdgcn_readfirstlane(wave) * (2 * 8 * 256) + lane * 4;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(base + (j * 8 + s4) * 256);
            Wf[j][4 * s4 + 0] = v[0]; Wf[j][4 * s4 + 1] = v[1]; Wf[j][4 * s4 + 2] = v[2]; Wf[j][4 * s4 + 3] = v[3];
        }
}

// ---- MFMA phase of one GCN layer: XW[0..79][stripe] = H[0..79][:] x W[:, stripe]  (PyG order: linear first).
// Wave `wave` owns the 32-column stripe [32*wave, 32*wave+32) for ALL rows; its A operand is the whole image,
// read as plain ds_read_b128 (no VALU in the MFMA stream).  Node 80 is done on VALU by the same lanes.
// Half tiles (16 k-steps = 4 x ds_read_b128) are double-buffered; sched_barrier pins the read/MFMA order.
__device__ __forceinline__ void stripe_matmul(const float* __restrict__ H, const float (&Wf)[2][32], int lane,
                                              f32x4 (&acc)[5][2], float& r0, float& r1) {
    const int c = lane & 15, q = lane >> 4;
    const int kb = (q & 1) * 64 + (q >> 1) * 32;  // kbase = {0, 64, 32, 96}
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        acc[m][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc[m][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const float* arow = H + c * LD + kb;
    f32x4 cur[4], nxt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cur[j] = *reinterpret_cast<const f32x4*>(arow + 4 * j);
#pragma unroll
    for (int ht = 0; ht < 10; ++ht) {          // half tile ht: rows 16*(ht/2).., k-steps 16*(ht&1)..
        const int m = ht >> 1, h = ht & 1;
        const float* nsrc = (ht < 9) ? arow + 16 * ((ht + 1) >> 1) * LD + 16 * ((ht + 1) & 1) : H + 80 * LD + kb;
#pragma unroll
        for (int j = 0; j < 4; ++j) nxt[j] = *reinterpret_cast<const f32x4*>(nsrc + 4 * j);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float av = cur[s >> 2][s & 3];
            acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Wf[0][16 * h + s], acc[m][0], 0, 0, 0);
            acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Wf[1][16 * h + s], acc[m][1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    // node 80: each lane covers its quarter of K for its two columns, quarters combined by xor-shuffles
    r0 = 0.f; r1 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) nxt[j] = *reinterpret_cast<const f32x4*>(H + 80 * LD + kb + 16 + 4 * j);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r0 = fmaf(cur[j][i], Wf[0][4 * j + i], r0);
            r1 = fmaf(cur[j][i], Wf[1][4 * j + i], r1);
        }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r0 = fmaf(nxt[j][i], Wf[0][16 + 4 * j + i], r0);
            r1 = fmaf(nxt[j][i], Wf[1][16 + 4 * j + i], r1);
        }
    r0 += __shfl_xor(r0, 16); r0 += __shfl_xor(r0, 32);
    r1 += __shfl_xor(r1, 16); r1 += __shfl_xor(r1, 32);
}

// ---- stripe epilogue: the wave parks its XW stripe in its own columns of H (the image is dead after the
// barrier), then gathers it back with the normalised neighbour coefficients (= PyG's scatter-add on this
// fixed-degree graph), + bias, ReLU.  Only this wave touches these columns, so ordering is wave-local.
// LAST: mean-pool instead of writing back.
template <bool LAST>
__device__ __forceinline__ void stripe_gather(TrunkSmem& sm, const f32x4 (&acc)[5][2], float r0, float r1,
                                              const float* __restrict__ bias_g, int wave, int lane,
                                              float* __restrict__ pooled_out) {
    {
        const int c = lane & 15, q = lane >> 4;
        float* w = sm.H + (4 * q) * LD + 32 * wave + c;
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[(16 * m + i) * LD] = acc[m][0][i];
                w[(16 * m + i) * LD + 16] = acc[m][1][i];
            }
        if (q == 0) {
            sm.H[80 * LD + 32 * wave + c] = r0;
            sm.H[80 * LD + 32 * wave + 16 + c] = r1;
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int cg = lane & 7, rs = lane >> 3;
    const int colb = 32 * wave + 4 * cg;
    const f32x4 bias = *reinterpret_cast<const f32x4*>(bias_g + colb);
    f32x4 out[STRIPE_ITERS];
    // Row r's neighbours sit at fixed row offsets (-9, +9, -1, +1); off-board ones are clamped to r itself (their
    // coefficient is 0 -- but the clamp is REQUIRED: 0 x NaN garbage is NaN, which the ReLU would silently turn into 0).  With the schedule of stripe_row() every clamp is known at compile time except
    // "up" in iterations 0..7 (only the rs == 0 lanes have r < 9), which is one per-lane offset.
    const float* p1 = sm.H + colb + rs * 8 * LD;          // iteration it < 8: row it + 8*rs
    const float* p2 = sm.H + colb + (64 + rs) * LD;       // iteration 8, 9: rows 64+rs, 72+rs
    const float* k1 = &sm.coef[8 * rs][0];
    const float* k2 = &sm.coef[64 + rs][0];
    const int offU1 = rs == 0 ? 0 : -9 * LD;
#pragma unroll
    for (int it = 0; it < STRIPE_ITERS; ++it) {
        const float *ps, *pu, *pd, *pl, *pr, *pk;
        if (it < 8) {
            ps = p1 + it * LD; pk = k1 + it * 8;
            pu = (it == 0) ? (rs <= 1 ? ps : ps - 9 * LD) : ps + offU1;   // rows it + 8*rs < 9: rs == 0, and row 8 (it 0, rs 1)
            pd = ps + 9 * LD; pr = ps + LD;
            pl = (it == 0) ? (rs == 0 ? ps : ps - LD) : ps - LD;
        } else if (it == 8) {
            ps = p2; pk = k2; pu = ps - 9 * LD; pd = ps + 9 * LD; pl = ps - LD; pr = ps + LD;
        } else if (it == 9) {
            ps = p2 + 8 * LD; pk = k2 + 64; pu = ps - 9 * LD; pd = ps; pl = ps - LD; pr = ps + LD;
        } else {                                             // row 80 (every lane computes it; only rs == 0 is used)
            ps = sm.H + colb + 80 * LD; pk = &sm.coef[80][0]; pu = ps - 9 * LD; pd = ps; pl = ps - LD; pr = ps;
        }
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(pk);
        const float kr = pk[4];
        const f32x4 hs = *reinterpret_cast<const f32x4*>(ps);
        const f32x4 hu = *reinterpret_cast<const f32x4*>(pu);
        const f32x4 hd = *reinterpret_cast<const f32x4*>(pd);
        const f32x4 hl = *reinterpret_cast<const f32x4*>(pl);
        const f32x4 hr = *reinterpret_cast<const f32x4*>(pr);
        f32x4 v = bias + k4[0] * hs + k4[1] * hu + k4[2] * hd + k4[3] * hl + kr * hr;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        out[it] = v;
        if (it & 1) __builtin_amdgcn_sched_barrier(0);   // two iterations' reads (14) in flight, not all 77
    }
    if (!LAST) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < STRIPE_ITERS; ++it) {
            const int r = stripe_row(it, rs);
            if (r < 81) *reinterpret_cast<f32x4*>(sm.H + r * LD + colb) = out[it];
        }
    } else {
        f32x4 sum = out[0];
#pragma unroll
        for (int it = 1; it < STRIPE_ITERS - 1; ++it) sum += out[it];
        if (rs == 0) sum += out[STRIPE_ITERS - 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = sum[e];
            x += __shfl_xor(x, 8); x += __shfl_xor(x, 16); x += __shfl_xor(x, 32);
            sum[e] = x * (1.0f / 81.0f);
        }
        if (rs == 0) *reinterpret_cast<f32x4*>(pooled_out + colb) = sum;
    }
}

// RESIDENT = true : one workgroup per CU (512-VGPR budget), both layers' fragments live in registers for the
//                   whole kernel -> zero per-board weight traffic, but no cross-workgroup phase overlap.
// RESIDENT = false: two workgroups per CU (256 VGPRs); each layer's fragments are re-fetched per board from
//                   L2 (128 KB per board per workgroup), issued one phase ahead of use.
template <bool RESIDENT, int WGS_PER_CU>
__global__ __launch_bounds__(256, WGS_PER_CU) void gcn_trunk_boards_kernel(const void* __restrict__ states, int fmt,
                                                                                   int B, const float* __restrict__ pk,
                                                                                   float* __restrict__ pooled,
                                                                                   const uint8_t* __restrict__ active) {
    constexpr int N = 9, V = 81, S = 8;
    __shared__ TrunkSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    float W2f[2][32], W3f[2][32];
    if (RESIDENT) {
        load_wfrag(W2f, pk + PackedLayout::WF2, wave, lane);
        load_wfrag(W3f, pk + PackedLayout::WF3, wave, lane);
    }
    // Raw state prefetch: the record's dwords are loaded one board ahead and only unpacked at setup time, so
    // the global-load latency hides under the previous board's layers (18 dwords for state72, 6 for QState).
    const int ndw = fmt == 0 ? 18 : 6;
    auto fetch_raw = [&](uint32_t (&raw)[18], int bb) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(states) + (size_t)bb * ndw;
#pragma unroll
        for (int i = 0; i < 18; ++i) raw[i] = (i < ndw) ? src[i] : 0u;
    };
    auto unpack_raw = [&](const uint32_t (&raw)[18]) -> QState {
        QState s;
        if (fmt == 0) {
            uint64_t h = 0, v = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                h |= (uint64_t)gather_bit0_x4(raw[1 + i]) << (4 * i);
                v |= (uint64_t)gather_bit0_x4(raw[1 + i] >> 1) << (4 * i);
            }
            s.hw = h; s.vw = v;
            s.ppos = (uint8_t)(raw[0] & 0xff); s.pwl = (uint8_t)((raw[0] >> 8) & 0xff);
            s.epos = (uint8_t)((raw[0] >> 16) & 0xff); s.ewl = (uint8_t)(raw[0] >> 24);
            s.plies = (uint16_t)(raw[17] & 0xffff);
        } else {
            s.hw = (uint64_t)raw[0] | ((uint64_t)raw[1] << 32);
            s.vw = (uint64_t)raw[2] | ((uint64_t)raw[3] << 32);
            s.ppos = (uint8_t)(raw[4] & 0xff); s.pwl = (uint8_t)((raw[4] >> 8) & 0xff);
            s.epos = (uint8_t)((raw[4] >> 16) & 0xff); s.ewl = (uint8_t)(raw[4] >> 24);
            s.plies = (uint16_t)(raw[5] & 0xffff);
        }
        s.pad = 0;
        return s;
    };
    int b = blockIdx.x;
    while (b < B && active && !active[b]) b += gridDim.x;
    uint32_t raw[18];
    if (b < B && tid < V) fetch_raw(raw, b);

    AQG_STAMP_DECL
    while (b < B) {
        AQG_STAMP_AT(7)
        // ---- setup step 1: node features + this tile's open-edge bits
        if (tid < V) {
            const QState s = unpack_raw(raw);
            const int t = tid, x = t / N, y = t % N;
            sm.obits[t] = tile_open_bits<N>(s.hw, s.vw, t);
            const bool slot_ok = (x < S) && (y < S);
            const int slot = x * S + y;
            f32x4 xa, xb;
            xa[0] = (t == s.ppos) ? 1.f : 0.f;
            xa[1] = (float)s.pwl;
            xa[2] = (t == s.epos) ? 1.f : 0.f;      // enemy's own frame (pv_network_cnn.py:101)
            xa[3] = (float)s.ewl;
            xb[0] = (slot_ok && ((s.hw >> slot) & 1)) ? 1.f : 0.f;
            xb[1] = (slot_ok && ((s.vw >> slot) & 1)) ? 1.f : 0.f;
            xb[2] = 0.f; xb[3] = 0.f;
            *reinterpret_cast<f32x4*>(sm.X0 + t * FPAD) = xa;
            *reinterpret_cast<f32x4*>(sm.X0 + t * FPAD + 4) = xb;
        }
        // prefetch the next board's raw record (lands under this board's layers)
        int bn = b + gridDim.x;
        while (bn < B && active && !active[bn]) bn += gridDim.x;
        if (bn < B && tid < V) fetch_raw(raw, bn);
        if (!RESIDENT) load_wfrag(W2f, pk + PackedLayout::WF2, wave, lane);   // lands under layer 1
        __syncthreads();
        AQG_STAMP_AT(0)
        // ---- setup step 2 + layer 1a: sym-norm coefficients from the neighbours' degrees, AX = A_hat * X0
        if (tid < V) {
            const int t = tid;
            const int ob = sm.obits[t];
            const int tu = t >= 9 ? t - 9 : t, td = t < 72 ? t + 9 : t, tl = t > 0 ? t - 1 : t, tr = t < 80 ? t + 1 : t;
            const float di = dinv_of_bits(ob);
            f32x4 k4;
            k4[0] = di * di;
            k4[1] = (ob & 1) ? di * dinv_of_bits(sm.obits[tu]) : 0.f;
            k4[2] = (ob & 2) ? di * dinv_of_bits(sm.obits[td]) : 0.f;
            k4[3] = (ob & 4) ? di * dinv_of_bits(sm.obits[tl]) : 0.f;
            const float kr = (ob & 8) ? di * dinv_of_bits(sm.obits[tr]) : 0.f;
            *reinterpret_cast<f32x4*>(&sm.coef[t][0]) = k4;
            sm.coef[t][4] = kr;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 v = k4[0] * *reinterpret_cast<const f32x4*>(sm.X0 + t * FPAD + 4 * h) +
                                k4[1] * *reinterpret_cast<const f32x4*>(sm.X0 + tu * FPAD + 4 * h) +
                                k4[2] * *reinterpret_cast<const f32x4*>(sm.X0 + td * FPAD + 4 * h) +
                                k4[3] * *reinterpret_cast<const f32x4*>(sm.X0 + tl * FPAD + 4 * h) +
                                kr * *reinterpret_cast<const f32x4*>(sm.X0 + tr * FPAD + 4 * h);
                *reinterpret_cast<f32x4*>(sm.AX + t * FPAD + 4 * h) = v;
            }
        }
        __syncthreads();
        AQG_STAMP_AT(1)
        // ---- layer 1b: H1[r][cols] = ReLU(b1 + AX[r] . W1[cols]) on this wave's stripe (4 columns x 1 row per lane-iteration)
        {
            const int cg = lane & 7, rs = lane >> 3;
            const int colb = 32 * wave + 4 * cg;
            float w1[4][6];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(pk + PackedLayout::W1 + (colb + e) * FPAD);
                const float2 hi = *reinterpret_cast<const float2*>(pk + PackedLayout::W1 + (colb + e) * FPAD + 4);
                w1[e][0] = lo[0]; w1[e][1] = lo[1]; w1[e][2] = lo[2]; w1[e][3] = lo[3]; w1[e][4] = hi.x; w1[e][5] = hi.y;
            }
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(pk + PackedLayout::B1 + colb);
#pragma unroll
            for (int it = 0; it < STRIPE_ITERS; ++it) {
                const int r = stripe_row(it, rs);
                if (r < V) {
                    const f32x4 xa = *reinterpret_cast<const f32x4*>(sm.AX + r * FPAD);
                    const float2 xb = *reinterpret_cast<const float2*>(sm.AX + r * FPAD + 4);
                    f32x4 v = b1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float a = v[e];
                        a = fmaf(xa[0], w1[e][0], a); a = fmaf(xa[1], w1[e][1], a); a = fmaf(xa[2], w1[e][2], a);
                        a = fmaf(xa[3], w1[e][3], a); a = fmaf(xb.x, w1[e][4], a); a = fmaf(xb.y, w1[e][5], a);
                        v[e] = fmaxf(a, 0.f);
                    }
                    *reinterpret_cast<f32x4*>(sm.H + r * LD + colb) = v;
                }
                if ((it & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        AQG_STAMP_AT(2)
        // ---- layer 2
        f32x4 acc[5][2];
        float r0, r1;
        stripe_matmul(sm.H, W2f, lane, acc, r0, r1);
        if (!RESIDENT) load_wfrag(W3f, pk + PackedLayout::WF3, wave, lane);   // lands under the layer-2 epilogue
        __syncthreads();                       // every wave has finished reading the image
        AQG_STAMP_AT(3)
        stripe_gather<false>(sm, acc, r0, r1, pk + PackedLayout::B2, wave, lane, nullptr);
        __syncthreads();
        AQG_STAMP_AT(4)
        // ---- layer 3 + mean pool
        stripe_matmul(sm.H, W3f, lane, acc, r0, r1);
        __syncthreads();
        AQG_STAMP_AT(5)
        stripe_gather<true>(sm, acc, r0, r1, pk + PackedLayout::B3, wave, lane, pooled + (size_t)b * HID);
        __syncthreads();                       // coef / image are rewritten by the next board's setup
        AQG_STAMP_AT(6)
#ifdef AQG_STAMP
        ++st_n;
#endif
        b = bn;
    }
#ifdef AQG_STAMP
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(pooled + (size_t)B * HID);
        for (int i = 0; i < 16; ++i) o[i] = st_sum[i];
        o[16] = (unsigned long long)st_n;
    }
#endif
}


// ---------------------------------------------------------------------------------------------
// heads: 16 boards per workgroup
// ---------------------------------------------------------------------------------------------
constexpr int HB = 8;   // boards per workgroup: B = 2048 -> 256 workgroups, one per CU

// Latency-bound small GEMMs: the weights stream from L2 (118 KB, shared by every workgroup), so the loop is built
// for memory-level parallelism -- 16 independent coalesced weight loads in flight per thread -- and the 8 boards
// of a workgroup sit transposed in LDS ([k][board]) so one k-step reads them with two broadcast ds_read_b128.
__global__ __launch_bounds__(256) void gcn_heads_kernel(const float* __restrict__ pooled, int B, int A,
                                                        const float* __restrict__ pk, float* __restrict__ logits,
                                                        float* __restrict__ policy, float* __restrict__ value_pre,
                                                        float* __restrict__ value, const uint8_t* __restrict__ active) {
    __shared__ alignas(16) float gT[HID][HB];          // pooled features, transposed
    __shared__ alignas(16) float part[2][HID][HB];     // hidden-layer partial sums of the two k halves
    __shared__ alignas(16) float hidT[HID][HB];        // hidden activations (0..63 policy, 64..127 value), transposed
    __shared__ float lg[HB][APAD];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * HB;
    const int nb = min(HB, B - b0);
    for (int i = tid; i < HB * HID; i += 256) {
        const int r = i / HID, k = i % HID;
        gT[k][r] = (r < nb) ? pooled[(size_t)(b0 + r) * HID + k] : 0.f;
    }
    __syncthreads();
    {   // hidden layer of both heads: unit u, k half kh (64 k each), all 8 boards
        const int u = tid & 127, kh = tid >> 7;
        float acc[HB];
#pragma unroll
        for (int i = 0; i < HB; ++i) acc[i] = 0.f;
        const float* w = pk + PackedLayout::HW1T + (size_t)(64 * kh) * HID + u;
#pragma unroll
        for (int k0 = 0; k0 < 64; k0 += 16) {
            float wk[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) wk[j] = w[(size_t)(k0 + j) * HID];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const f32x4 ga = *reinterpret_cast<const f32x4*>(&gT[64 * kh + k0 + j][0]);
                const f32x4 gb = *reinterpret_cast<const f32x4*>(&gT[64 * kh + k0 + j][4]);
#pragma unroll
                for (int i = 0; i < 4; ++i) { acc[i] = fmaf(ga[i], wk[j], acc[i]); acc[4 + i] = fmaf(gb[i], wk[j], acc[4 + i]); }
            }
        }
        *reinterpret_cast<f32x4*>(&part[kh][u][0]) = (f32x4){acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4*>(&part[kh][u][4]) = (f32x4){acc[4], acc[5], acc[6], acc[7]};
    }
    __syncthreads();
    for (int i = tid; i < HID * HB; i += 256) {
        const int u = i / HB, r = i % HB;
        hidT[u][r] = fmaxf(part[0][u][r] + part[1][u][r] + pk[PackedLayout::HB1 + u], 0.f);
    }
    __syncthreads();
    if (tid < A) {
        float acc[HB];
        const float bias = pk[PackedLayout::PB2 + tid];
#pragma unroll
        for (int i = 0; i < HB; ++i) acc[i] = bias;
        const float* w = pk + PackedLayout::PW2T + tid;
#pragma unroll
        for (int k0 = 0; k0 < HID / 2; k0 += 16) {
            float wk[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) wk[j] = w[(size_t)(k0 + j) * APAD];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const f32x4 ha = *reinterpret_cast<const f32x4*>(&hidT[k0 + j][0]);
                const f32x4 hb = *reinterpret_cast<const f32x4*>(&hidT[k0 + j][4]);
#pragma unroll
                for (int i = 0; i < 4; ++i) { acc[i] = fmaf(ha[i], wk[j], acc[i]); acc[4 + i] = fmaf(hb[i], wk[j], acc[4 + i]); }
            }
        }
#pragma unroll
        for (int i = 0; i < HB; ++i) lg[i][tid] = acc[i];
    } else if (tid >= 248) {   // value head: one thread per board
        const int i = tid - 248;
        float acc = pk[PackedLayout::VB2];
        for (int k = 0; k < HID / 2; ++k) acc = fmaf(hidT[HID / 2 + k][i], pk[PackedLayout::VW2 + k], acc);
        if (i < nb && !(active && !active[b0 + i])) {
            if (value_pre) value_pre[b0 + i] = acc;
            if (value) value[b0 + i] = tanhf(acc);
        }
    }
    __syncthreads();
    // softmax: wave w handles boards 2w, 2w+1
    const int lane = tid & 63, wave = tid >> 6;
    for (int r = 2 * wave; r < 2 * wave + 2; ++r) {
        if (r >= nb) break;
        if (active && !active[b0 + r]) continue;
        float m = -INFINITY;
        for (int a = lane; a < A; a += 64) m = fmaxf(m, lg[r][a]);
        m = wave_xor_max(m);
        float e[4];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = lane + 64 * j;
            e[j] = (a < A) ? expf(lg[r][a] - m) : 0.f;
            s += e[j];
        }
        s = wave_xor_sum(s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = lane + 64 * j;
            if (a < A) {
                if (logits) logits[(size_t)(b0 + r) * A + a] = lg[r][a];
                if (policy) policy[(size_t)(b0 + r) * A + a] = e[j] / s;
            }
        }
    }
}

// variant 0: weights resident, one workgroup per CU; otherwise two workgroups per CU.  Enqueue only: the caller checks the launch.
void launch_gcn_trunk_exact(int variant, const void* states, int fmt, int B, const float* packed, float* pooled,
                            const uint8_t* active, hipStream_t st) {
    // persistent grid: 256 CUs x resident workgroups per CU, grid-stride over boards
    if (variant == 0) {
        int grid = B < 256 ? B : 256;
        hipLaunchKernelGGL((gcn_trunk_boards_kernel<true, 1>), dim3(grid), dim3(256), 0, st, states, fmt, B, packed, pooled, active);
    } else {
        int grid = B < 512 ? B : 512;
        hipLaunchKernelGGL((gcn_trunk_boards_kernel<false, 2>), dim3(grid), dim3(256), 0, st, states, fmt, B, packed, pooled, active);
    }
}

int launch_gcn_heads_exact(const float* pooled, int B, int A, const float* packed, float* logits, float* policy, float* value_pre,
                           float* value, const uint8_t* active, hipStream_t st) {
    hipLaunchKernelGGL(gcn_heads_kernel, dim3((B + HB - 1) / HB), dim3(256), 0, st, pooled, B, A, packed,
                       logits, policy, value_pre, value, active);
    return check_launch("gcn_heads_kernel");
}

}  // namespace aqg
