// gcn_heads_split.hpp -- the heads of GraphPolicyValueNetwork.forward (pv_network_gnn.py:60-64) on the split matrix pipe, as a workgroup-wide
// device function: heads_body and what it needs (HeadsSmem, the DPP row reductions, the packed buffer's fragment loads, the fp16-range
// guard's report).  Two kernels run it: gcn_heads_mm_kernel (gcn_trunk_split.hip: 16 boards per workgroup, results to global memory) and
// the MCTS step kernel (mcts_step.hip: the leaves of a step workgroup's own eight games, results to LDS).  __forceinline__ device code only.
#pragma once
#include "gcn_packed.hpp"
#include <cmath>

namespace aqg {

// (row16_sum, the sum over the 16 lanes of a DPP row, is in split_mfma.hpp: the training heads use it too.)

// Weight fragments are fetched with buffer loads: one SGPR resource for the packed buffer, one shared VGPR (lane * 16)
// and a scalar offset per load -- no 64-bit address VGPRs (they were the first thing the allocator spilled, and a
// spilled address is reloaded behind an s_waitcnt vmcnt(0) that serialises the whole prefetch).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t packed_rsrc(const float* pk) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pk), 0, (int)(PackedLayout::TOTAL * sizeof(float)), 0x00020000);
}
__device__ __forceinline__ u32x4 load_frag16(__amdgpu_buffer_rsrc_t rs, int lane16, int byte_off) {
    return __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, byte_off, 0);
}

// Runtime fp16-range guard.  The split kernels are fp32-equivalent only while every value they store as fp16 pairs stays inside
// fp16 range: the post-ReLU activations (clamped at 65504 instead of overflowing) and the linear maps' outputs (converted as they
// are split).  Where a static bound over all inputs proves that (AQG_GNN_RANGE_PROVEN) only the records' wall counts are checked;
// otherwise layer 1's pre-clamp outputs are bounded by a float maximum, the linear maps' outputs U by a float maximum of |U| against
// PackedLayout::GUARD (layer 2's aggregate is then bounded analytically; layer 3's lands in the pooled row, which the heads kernel
// checks).  A launch that met such a value ORs 1 into the caller's `saturated` word: the host then serves the weight set with the exact
// f32-input kernels (pv_network_gnn / engine).  The reference's fp32 has no such cliff (pv_network_gnn.py:53-64).
// tests/test_gpu_parity.py::test_gnn_runtime_saturation_signal / test_gnn_range_guard_watches_every_feature drive it.
// (__builtin_bit_cast applied to a vector ELEMENT expression -- bit_cast(int, v[1]) -- read element 0 for every index with hipcc 7.2:
//  the first, per-value form of this guard watched one value in four.  Take the element into a scalar first.)
__device__ __forceinline__ void report_saturation(bool lane_saw_it, int32_t* __restrict__ saturated) {
    if (saturated && __builtin_amdgcn_ballot_w64(lane_saw_it) != 0) {            // wave-uniform, practically never taken
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        if (l == 0) atomicOr(saturated, 1);
    }
}

// ---------------------------------------------------------------------------------------------
// heads on the split matrix pipe: EIGHT waves per 16 boards.  (Round 4 also ran this body inside the trunk launch -- by the workgroup
// that pools the last board of a 16-board group, agent-scope stores + one atomic per workgroup, nobody waiting for anybody: correct,
// and slower, 25.7 against 23.4 us per 480-board evaluation; profiles/r04_heads_by_last_finisher_*.log, commit d13f38b in the history.)
//   layer 1 (transposed):  hid^T[u][board] = HW1[u][k] pooled^T[k][board]   A = host-split weight fragments (wave w: unit tile w),
//                          B = this lane's 8 consecutive pooled features of board (lane & 15), split in registers
//   layer 2:               logits[board][a] = hid[board][u] PW2^T[u][a]     A = the layer-1 accumulators of waves 0..3 (lane = board,
//                          4 consecutive units per tile -> k-slot order of WHP2) through 4 KB of LDS, B = host-split weight
//                          fragments (wave w: action tiles w and w + 8)
//   softmax in the accumulator layout (lane = action column, 4 boards per lane): per wave over its action tiles, DPP row
//   reductions over the 16 lanes of a row, the eight waves' (max, sum) combined through LDS in a fixed order;
//   value head: waves 4..7 hold its hidden units, wave 4 sums them in a fixed order.
// Same split precision as the trunk (3 fp16 terms per product, f32 accumulate).  Every wave requests ALL its weight fragments
// (16 x 16 B per lane) and its pooled features before anything else: 96 registers of operands, inside the trunk's 128-register cap.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void split8(const f32x4 x0, const f32x4 x1, u32x4& hi, u32x4& lo) {
    hi = (u32x4){cvt_pk_f16(x0[0], x0[1]), cvt_pk_f16(x0[2], x0[3]), cvt_pk_f16(x1[0], x1[1]), cvt_pk_f16(x1[2], x1[3])};
    const f32x4 r0 = x0 - f16_pairs_to_f32(hi[0], hi[1]), r1 = x1 - f16_pairs_to_f32(hi[2], hi[3]);
    lo = (u32x4){cvt_pk_f16(r0[0], r0[1]), cvt_pk_f16(r0[2], r0[3]), cvt_pk_f16(r1[0], r1[1]), cvt_pk_f16(r1[2], r1[3])};
}
__device__ __forceinline__ float row16_max(float x) {
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x128, 0xf, 0xf, false)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x124, 0xf, 0xf, false)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x122, 0xf, 0xf, false)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x121, 0xf, 0xf, false)));
    return x;
}

constexpr int HEADS_WAVES = 8;
struct alignas(16) HeadsSmem {
    unsigned int hfrag[2][2][64][4];     // layer-2 A fragments [kb2][plane][lane][unit tile parity x 2 dwords]: written by waves 0..3, read by all
    float vlane[4][64];                  // value head: per-lane partial dot products of waves 4..7 (unit tiles 4..7)
    float wmax[HEADS_WAVES][16], wsum[HEADS_WAVES][16];   // per-wave softmax partials per board
};

// All 512 threads of a workgroup call this for the 16 boards b0 .. b0 + 15 (two internal barriers).  `prs` = buffer resource of the
// pooled rows [B][128] f32.
// STEP (the MCTS step kernel, mcts_step.hip): the same arithmetic for the leaves of the workgroup's own games, with three differences
// in where things come from and go to -- a board is live where its `active` byte is 1 (the engine's leaf_flag: 2 marks a leaf whose
// priors are in memory already); the softmax row of board b0 + i goes to lds_policy[i][action] and tanh(value) to lds_value[i]
// instead of global memory (the caller puts a barrier in front of their readers); and mid() is called once the hidden layer's
// MFMAs are issued: the caller requests its own first load round there, in the registers the hidden layer's operands have left.
struct HeadsNoMid { __device__ __forceinline__ void operator()() const {} };
template <bool STEP = false, class Mid = HeadsNoMid>
__device__ __forceinline__ void heads_body(HeadsSmem& sm, __amdgpu_buffer_rsrc_t prs, int b0, int B, int A, __amdgpu_buffer_rsrc_t rs,
                                           const float* __restrict__ pk, float* __restrict__ logits, float* __restrict__ policy,
                                           float* __restrict__ value_pre, float* __restrict__ value, const uint8_t* __restrict__ active,
                                           int32_t* __restrict__ saturated, int wave, int lane, float (*lds_policy)[256] = nullptr,
                                           float* lds_value = nullptr, Mid mid = Mid()) {
    const int c = lane & 15, q = lane >> 4;
    constexpr int H1 = (int)(PackedLayout::WHH1 * sizeof(float)), P2 = (int)(PackedLayout::WHP2 * sizeof(float));
    const int ntiles = (A + 15) >> 4;
    const bool want_policy = STEP || logits || policy;
    // this wave's weight fragments of layer 1: hidden-unit tile `wave`
    u32x4 af[2][4];                                            // [plane][kb]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) af[pl][kb] = load_frag16(rs, lane * 16, H1 + ((pl * 8 + wave) * 4 + kb) * (64 * 16));
    // B operand of layer 1: 32 pooled features of board (b0 + c) -- requested now, split below
    const bool okc = b0 + c < B;
    f32x4 x0[4], x1[4];
    {
        const int row = (okc ? b0 + c : B - 1) * (HID * 4);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            x0[kb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, row + (32 * kb + 8 * q) * 4, 0, 0));
            x1[kb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, row + (32 * kb + 8 * q + 4) * 4, 0, 0));
        }
    }
    // every small operand of the later phases is requested here too, behind the fragments and the pooled rows: behind a barrier each
    // of them (layer-1 bias, value weights, action biases, the boards' active flags) was a memory round trip of its own in this chain
    const f32x4 bias = *reinterpret_cast<const f32x4*>(pk + PackedLayout::HB1 + 16 * wave + 4 * q);
    const f32x4 vw = *reinterpret_cast<const f32x4*>(pk + PackedLayout::VW2 + 16 * (wave & 3) + 4 * q);
    float pb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int a = 16 * (wave + 8 * j) + c; pb[j] = pk[PackedLayout::PB2 + (a < A ? a : 0)]; }
    const float vb2 = pk[PackedLayout::VB2];
    // the boards' active flags: five unconditional byte loads (clamped indices, through a pointer that is never null), all in flight
    // with everything else -- written as `brd < B && !(active && !active[brd])` each became a branch around a load with its own
    // s_waitcnt vmcnt(0): five serial round trips
    const uint8_t* __restrict__ ap = active ? active : reinterpret_cast<const uint8_t*>(pk);
    unsigned int af4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) af4[i] = ap[active ? min(b0 + 4 * q + i, B - 1) : 0];
    const unsigned int afc = ap[active ? min(b0 + c, B - 1) : 0];
    u32x4 ph[4], pl_[4];
    bool counted;
    {
        float xmax = 0.f;                                              // fp16-range guard (see report_saturation)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            if (!okc) { x0[kb] = (f32x4){0.f, 0.f, 0.f, 0.f}; x1[kb] = x0[kb]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) xmax = fmaxf(fmaxf(fabsf(x0[kb][e]), fabsf(x1[kb][e])), xmax);
            split8(x0[kb], x1[kb], ph[kb], pl_[kb]);
        }
        counted = okc && (!active || (STEP ? afc == 1 : afc != 0));                        // (fp16-range guard) a masked-out board's pooled row is whatever the buffer held
        if (wave == 0) report_saturation(counted && !(xmax <= 65504.0f), saturated);  // (!(<=) also catches a NaN row; every wave sees the same rows)
    }
    int live4 = 0;                                             // bit i: board b0 + 4 q + i exists and is not masked out
#pragma unroll
    for (int i = 0; i < 4; ++i) live4 |= (b0 + 4 * q + i < B && (!active || (STEP ? af4[i] == 1 : af4[i] != 0))) ? (1 << i) : 0;
    // layer-2 fragments: requested only now, in the registers the raw pooled rows have left (the kernel has to stay inside 128
    // registers -- eight such waves then fit on a CU beside one trunk workgroup; at 140 registers they did not, and the self-play loop
    // lost 15 %: 1,468 against 1,720 games/s); they land under layer 1 and the barrier
    // (STEP: the step kernel keeps more than this body alive -- there the fragments of (j, kb2) are requested behind the hidden layer's
    //  k block 2 j + kb2, in the registers that block's operands have just left, and land under the rest of layer 1 and the barrier)
    u32x4 bq[2][2][2];                                         // [action tile wave + 8 j][plane][kb2]
    auto request_bq = [&](int j, int kb) {
        const int at = wave + 8 * j;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            bq[j][pl][kb] = (want_policy && at < ntiles) ? load_frag16(rs, lane * 16, P2 + ((pl * 14 + at) * 2 + kb) * (64 * 16)) : (u32x4){0u, 0u, 0u, 0u};
    };
    if (!STEP) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) request_bq(j, kb);
    }
    // ---- phase 1: hidden units 16 wave + 4 q + e of board b0 + c
    {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            acc = mfma_f16(af[1][kb], ph[kb], acc);
            acc = mfma_f16(af[0][kb], pl_[kb], acc);
            acc = mfma_f16(af[0][kb], ph[kb], acc);
            if (STEP) {
                __builtin_amdgcn_sched_barrier(0);
                request_bq(kb >> 1, kb & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (STEP) {
            __builtin_amdgcn_sched_barrier(0);
            mid();
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 h = acc + bias;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = fmaxf(h[e], 0.f);
        if (wave < 4) {
            // (stored as fp16 pairs for the policy head's second layer: same range guard)
            report_saturation(counted && !(fmaxf(fmaxf(h[0], h[1]), fmaxf(h[2], h[3])) <= 65504.0f), saturated);
            const unsigned int h01 = cvt_pk_f16(h[0], h[1]), h23 = cvt_pk_f16(h[2], h[3]);
            const f32x4 r = h - f16_pairs_to_f32(h01, h23);
            const int kb2 = wave >> 1, t = wave & 1;
            *reinterpret_cast<u32x2*>(&sm.hfrag[kb2][0][lane][2 * t]) = (u32x2){h01, h23};
            *reinterpret_cast<u32x2*>(&sm.hfrag[kb2][1][lane][2 * t]) = (u32x2){cvt_pk_f16(r[0], r[1]), cvt_pk_f16(r[2], r[3])};
        } else {
            sm.vlane[wave - 4][lane] = h[0] * vw[0] + h[1] * vw[1] + h[2] * vw[2] + h[3] * vw[3];
        }
    }
    __syncthreads();
    if (wave == 4) {                                           // value head: fixed-order sum of the four unit tiles, then of the four lane quarters
        float v = (sm.vlane[0][lane] + sm.vlane[1][lane]) + (sm.vlane[2][lane] + sm.vlane[3][lane]);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (counted && lane < 16) {                            // (lane < 16: c == lane, board b0 + lane)
            v += vb2;
            if (STEP) lds_value[lane] = tanhf(v);
            else {
                if (value_pre) value_pre[b0 + lane] = v;
                if (value) value[b0 + lane] = tanhf(v);
            }
        }
    }
    if (!want_policy) return;
    // ---- phase 2: this wave's action tiles, lane = action 16 at + c, rows = boards 4 q .. 4 q + 3
    u32x4 hh[2], hl[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        hh[kb] = *reinterpret_cast<const u32x4*>(&sm.hfrag[kb][0][lane][0]);
        hl[kb] = *reinterpret_cast<const u32x4*>(&sm.hfrag[kb][1][lane][0]);
    }
    f32x4 lg[2];
    f32x4 m = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int at = wave + 8 * j, a = 16 * at + c;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            acc = mfma_f16(hl[kb], bq[j][0][kb], acc);
            acc = mfma_f16(hh[kb], bq[j][1][kb], acc);
            acc = mfma_f16(hh[kb], bq[j][0][kb], acc);
        }
        const bool ok = a < A;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lg[j][i] = ok ? acc[i] + pb[j] : -INFINITY;
            m[i] = fmaxf(m[i], lg[j][i]);
        }
    }
    f32x4 ssum = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 ex[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = row16_max(m[i]);          // this wave's maximum per board (finite: every wave owns tile w < 14)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ex[j][i] = __expf(lg[j][i] - m[i]);                // exp(-inf) = 0 for padded columns; ~2 ulp, far inside the tolerance
            ssum[i] += ex[j][i];
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) ssum[i] = row16_sum(ssum[i]);
    if (c == 0) {
        *reinterpret_cast<f32x4*>(&sm.wmax[wave][4 * q]) = m;
        *reinterpret_cast<f32x4*>(&sm.wsum[wave][4 * q]) = ssum;
    }
    __syncthreads();
    // common maximum M, total S = sum_w s_w exp(m_w - M) in wave order; this wave's exponentials are rescaled by exp(m_w - M) / S
    f32x4 scale;
    {
        // (STEP: the partials come in three LDS rounds of 32 registers -- the maxima, then (m_w, s_w) of four waves at a time, each
        //  round's offset made to depend on the previous round's result -- where the stand-alone kernel has all 64 in flight at once:
        //  the step kernel's own first load round is alive beside them.  Same values, same order of additions.)
        int qo = 4 * q;
        f32x4 M = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int w = 0; w < HEADS_WAVES; ++w) {
            const f32x4 mw = *reinterpret_cast<const f32x4*>(&sm.wmax[w][qo]);
#pragma unroll
            for (int i = 0; i < 4; ++i) M[i] = fmaxf(M[i], mw[i]);
        }
        f32x4 S = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < HEADS_WAVES; ++w) {
            if (STEP && (w & 3) == 0) {
                const float d0 = w ? S[0] : M[0], d1 = w ? S[1] : M[1], d2 = w ? S[2] : M[2], d3 = w ? S[3] : M[3];
                asm volatile("" : "+v"(qo) : "v"(d0), "v"(d1), "v"(d2), "v"(d3));
            }
            const f32x4 mw = *reinterpret_cast<const f32x4*>(&sm.wmax[w][qo]);
            const f32x4 sw = *reinterpret_cast<const f32x4*>(&sm.wsum[w][qo]);
#pragma unroll
            for (int i = 0; i < 4; ++i) S[i] += sw[i] * __expf(mw[i] - M[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) scale[i] = __expf(m[i] - M[i]) / S[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int brd = b0 + 4 * q + i;
        if (!((live4 >> i) & 1)) continue;
        if (STEP) {
            float* p = &lds_policy[4 * q + i][16 * wave + c];
#pragma unroll
            for (int j = 0; j < 2; ++j) if (16 * (wave + 8 * j) + c < A) p[128 * j] = ex[j][i] * scale[i];
            continue;
        }
        const size_t row = (size_t)brd * A + 16 * wave + c;     // one 64-bit address per board row, this wave's tiles at +512 B steps
        if (policy) {
            float* __restrict__ p = policy + row;
#pragma unroll
            for (int j = 0; j < 2; ++j) if (16 * (wave + 8 * j) + c < A) p[128 * j] = ex[j][i] * scale[i];
        }
        if (logits) {
            float* __restrict__ l = logits + row;
#pragma unroll
            for (int j = 0; j < 2; ++j) if (16 * (wave + 8 * j) + c < A) l[128 * j] = lg[j][i];
        }
    }
}

// heads_half (the step kernel's two kinds of workgroup, option "policy_beside_step"): heads_body<STEP> cut into its two halves, each exactly
// what the whole body computes for its outputs -- the same fragments, the same MFMA sequence per output, the same order of every sum.
// A function of its own, so that the whole body above and the kernels built from it stay instruction for instruction what they were.
// (Serving the whole body from these pieces too was built and measured, profiles/heads_one_body.log: the stand-alone kernel keeps its
//  speed, the three older fused step forms lose half a per cent in every order of the pieces tried -- so the two functions stay.)
// The phases are written once, as pieces, and put in order at the end: the hidden tile's pieces run as ONE region of the waves that
// have a tile (separate regions made the allocator carry 64 registers of operands through their joins, and spill).
//   HEADS_VALUE   waves 4..7 run their hidden tiles; behind the one barrier EVERY wave forms the fixed-order sum wave 4 forms in the
//                 whole body and the function returns tanh(value) of board b0 + wave (nothing goes through lds_value, no board mask is
//                 read: the caller uses the value of a live board only, and the range guard is the policy half's); mid() is called at
//                 entry, behind the requests of the operands -- one hidden tile per wave leaves the registers for it;
//   HEADS_POLICY  waves 0..3 run their hidden tiles, all eight the policy layer and the softmax; the pooled rows' and the hidden units'
//                 range guards report here.  A board is live where head_live(active, board) is 1: the caller's own record type.
enum HeadsPart { HEADS_VALUE = 1, HEADS_POLICY = 2 };
__device__ __forceinline__ unsigned int head_live(const uint8_t* flags, int i) { return flags[i]; }
template <int PART, class Act = uint8_t, class Mid = HeadsNoMid>
__device__ __forceinline__ float heads_half(HeadsSmem& sm, __amdgpu_buffer_rsrc_t prs, int b0, int B, int A, __amdgpu_buffer_rsrc_t rs,
                                           const float* __restrict__ pk, float* __restrict__ logits, float* __restrict__ policy,
                                           float* __restrict__ value_pre, float* __restrict__ value, const Act* __restrict__ active,
                                           int32_t* __restrict__ saturated, int wave, int lane, float (*lds_policy)[256] = nullptr,
                                           float* lds_value = nullptr, Mid mid = Mid()) {
    const int c = lane & 15, q = lane >> 4;
    constexpr int H1 = (int)(PackedLayout::WHH1 * sizeof(float)), P2 = (int)(PackedLayout::WHP2 * sizeof(float));
    const int ntiles = (A + 15) >> 4;
    static_assert(PART == HEADS_VALUE || PART == HEADS_POLICY, "a half");
    constexpr bool STEP = true;
    constexpr bool DO_VALUE = PART != HEADS_POLICY, DO_POLICY = PART != HEADS_VALUE;
    const bool want_policy = DO_POLICY && (STEP || logits || policy);
    const bool tile = PART == HEADS_VALUE ? wave >= 4 : wave < 4;      // (wave-uniform) this wave runs a hidden tile
    // this wave's weight fragments of layer 1: hidden-unit tile `wave`
    u32x4 af[2][4];                                            // [plane][kb]
    // B operand of layer 1: 32 pooled features of board (b0 + c) -- requested first, split below
    const bool okc = b0 + c < B;
    f32x4 x0[4], x1[4];
    auto request_tile = [&]() {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) af[pl][kb] = load_frag16(rs, lane * 16, H1 + ((pl * 8 + wave) * 4 + kb) * (64 * 16));
        const int row = (okc ? b0 + c : B - 1) * (HID * 4);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            x0[kb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, row + (32 * kb + 8 * q) * 4, 0, 0));
            x1[kb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, row + (32 * kb + 8 * q + 4) * 4, 0, 0));
        }
    };
    // every small operand of the later phases is requested at the start too, with the fragments and the pooled rows: behind a barrier each
    // of them (layer-1 bias, value weights, action biases, the boards' active flags) was a memory round trip of its own in this chain
    f32x4 bias, vw;
    float pb[2] = {0.f, 0.f}, vb2;
    // the boards' active flags: five unconditional byte loads (clamped indices, through a pointer that is never null), all in flight
    // with everything else -- written as `brd < B && !(active && !active[brd])` each became a branch around a load with its own
    // s_waitcnt vmcnt(0): five serial round trips
    const Act* __restrict__ ap = active ? active : reinterpret_cast<const Act*>(pk);
    unsigned int af4[4], afc;
    auto request_small = [&]() {
        bias = *reinterpret_cast<const f32x4*>(pk + PackedLayout::HB1 + 16 * wave + 4 * q);
        vw = *reinterpret_cast<const f32x4*>(pk + PackedLayout::VW2 + 16 * (wave & 3) + 4 * q);
        if (DO_POLICY) {
#pragma unroll
            for (int j = 0; j < 2; ++j) { const int a = 16 * (wave + 8 * j) + c; pb[j] = pk[PackedLayout::PB2 + (a < A ? a : 0)]; }
        }
        vb2 = pk[PackedLayout::VB2];
        if constexpr (DO_POLICY) {
#pragma unroll
            for (int i = 0; i < 4; ++i) af4[i] = head_live(ap, active ? min(b0 + 4 * q + i, B - 1) : 0);
            afc = head_live(ap, active ? min(b0 + c, B - 1) : 0);
        } else {
            af4[0] = af4[1] = af4[2] = af4[3] = afc = 1u;
        }
    };
    u32x4 ph[4], pl_[4];
    bool counted = false;
    auto split_tile = [&]() {
        float xmax = 0.f;                                              // fp16-range guard (see report_saturation)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            if (!okc) { x0[kb] = (f32x4){0.f, 0.f, 0.f, 0.f}; x1[kb] = x0[kb]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) xmax = fmaxf(fmaxf(fabsf(x0[kb][e]), fabsf(x1[kb][e])), xmax);
            split8(x0[kb], x1[kb], ph[kb], pl_[kb]);
        }
        counted = okc && (!active || (STEP ? afc == 1 : afc != 0));                        // (fp16-range guard) a masked-out board's pooled row is whatever the buffer held
        if (DO_POLICY && wave == 0) report_saturation(counted && !(xmax <= 65504.0f), saturated);  // (!(<=) also catches a NaN row; every wave sees the same rows)
    };
    int live4 = 0;                                             // bit i: board b0 + 4 q + i exists and is not masked out
    auto mask_boards = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) live4 |= (b0 + 4 * q + i < B && (!active || (STEP ? af4[i] == 1 : af4[i] != 0))) ? (1 << i) : 0;
    };
    // layer-2 fragments: requested only behind the split, in the registers the raw pooled rows have left (the kernel has to stay inside 128
    // registers -- eight such waves then fit on a CU beside one trunk workgroup; at 140 registers they did not, and the self-play loop
    // lost 15 %: 1,468 against 1,720 games/s); they land under layer 1 and the barrier
    // (STEP: the step kernel keeps more than this body alive -- there the fragments of (j, kb2) are requested behind the hidden layer's
    //  k block 2 j + kb2, in the registers that block's operands have just left, and land under the rest of layer 1 and the barrier)
    u32x4 bq[2][2][2];                                         // [action tile wave + 8 j][plane][kb2]
    auto request_bq = [&](int j, int kb) {
        const int at = wave + 8 * j;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            bq[j][pl][kb] = (want_policy && at < ntiles) ? load_frag16(rs, lane * 16, P2 + ((pl * 14 + at) * 2 + kb) * (64 * 16)) : (u32x4){0u, 0u, 0u, 0u};
    };
    auto request_bq_all = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) request_bq(j, kb);
    };
    // ---- phase 1: hidden units 16 wave + 4 q + e of board b0 + c
    auto run_tile = [&]() {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            acc = mfma_f16(af[1][kb], ph[kb], acc);
            acc = mfma_f16(af[0][kb], pl_[kb], acc);
            acc = mfma_f16(af[0][kb], ph[kb], acc);
            if (STEP && DO_POLICY) {
                __builtin_amdgcn_sched_barrier(0);
                request_bq(kb >> 1, kb & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (STEP && PART != HEADS_VALUE) {
            __builtin_amdgcn_sched_barrier(0);
            mid();
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 h = acc + bias;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = fmaxf(h[e], 0.f);
        if (DO_POLICY && (!DO_VALUE || wave < 4)) {
            // (stored as fp16 pairs for the policy head's second layer: same range guard)
            report_saturation(counted && !(fmaxf(fmaxf(h[0], h[1]), fmaxf(h[2], h[3])) <= 65504.0f), saturated);
            const unsigned int h01 = cvt_pk_f16(h[0], h[1]), h23 = cvt_pk_f16(h[2], h[3]);
            const f32x4 r = h - f16_pairs_to_f32(h01, h23);
            const int kb2 = wave >> 1, t = wave & 1;
            *reinterpret_cast<u32x2*>(&sm.hfrag[kb2][0][lane][2 * t]) = (u32x2){h01, h23};
            *reinterpret_cast<u32x2*>(&sm.hfrag[kb2][1][lane][2 * t]) = (u32x2){cvt_pk_f16(r[0], r[1]), cvt_pk_f16(r[2], r[3])};
        } else {
            sm.vlane[wave - 4][lane] = h[0] * vw[0] + h[1] * vw[1] + h[2] * vw[2] + h[3] * vw[3];
        }
    };
    {
        request_small();
        if (tile) {
            request_tile();
            if (PART == HEADS_VALUE) mid();
            split_tile();
            run_tile();
        } else {
            if (PART == HEADS_VALUE) mid();
            else request_bq_all();                             // (no hidden tile: the layer-2 fragments land under the barrier)
        }
        if (DO_POLICY) mask_boards();
    }
    __syncthreads();
    if (PART == HEADS_VALUE) {                                 // (every wave: the sum below, for the caller's own board)
        float v = (sm.vlane[0][lane] + sm.vlane[1][lane]) + (sm.vlane[2][lane] + sm.vlane[3][lane]);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        v = tanhf(v + vb2);
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), wave));
    }
    if (DO_VALUE && wave == 4) {                               // value head: fixed-order sum of the four unit tiles, then of the four lane quarters
        float v = (sm.vlane[0][lane] + sm.vlane[1][lane]) + (sm.vlane[2][lane] + sm.vlane[3][lane]);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (counted && lane < 16) {                            // (lane < 16: c == lane, board b0 + lane)
            v += vb2;
            if (STEP) lds_value[lane] = tanhf(v);
            else {
                if (value_pre) value_pre[b0 + lane] = v;
                if (value) value[b0 + lane] = tanhf(v);
            }
        }
    }
    if (!want_policy) return 0.f;
    // ---- phase 2: this wave's action tiles, lane = action 16 at + c, rows = boards 4 q .. 4 q + 3
    u32x4 hh[2], hl[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        hh[kb] = *reinterpret_cast<const u32x4*>(&sm.hfrag[kb][0][lane][0]);
        hl[kb] = *reinterpret_cast<const u32x4*>(&sm.hfrag[kb][1][lane][0]);
    }
    f32x4 lg[2];
    f32x4 m = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int at = wave + 8 * j, a = 16 * at + c;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            acc = mfma_f16(hl[kb], bq[j][0][kb], acc);
            acc = mfma_f16(hh[kb], bq[j][1][kb], acc);
            acc = mfma_f16(hh[kb], bq[j][0][kb], acc);
        }
        const bool ok = a < A;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lg[j][i] = ok ? acc[i] + pb[j] : -INFINITY;
            m[i] = fmaxf(m[i], lg[j][i]);
        }
    }
    f32x4 ssum = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 ex[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = row16_max(m[i]);          // this wave's maximum per board (finite: every wave owns tile w < 14)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ex[j][i] = __expf(lg[j][i] - m[i]);                // exp(-inf) = 0 for padded columns; ~2 ulp, far inside the tolerance
            ssum[i] += ex[j][i];
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) ssum[i] = row16_sum(ssum[i]);
    if (c == 0) {
        *reinterpret_cast<f32x4*>(&sm.wmax[wave][4 * q]) = m;
        *reinterpret_cast<f32x4*>(&sm.wsum[wave][4 * q]) = ssum;
    }
    __syncthreads();
    // common maximum M, total S = sum_w s_w exp(m_w - M) in wave order; this wave's exponentials are rescaled by exp(m_w - M) / S
    f32x4 scale;
    {
        // (STEP: the partials come in three LDS rounds of 32 registers -- the maxima, then (m_w, s_w) of four waves at a time, each
        //  round's offset made to depend on the previous round's result -- where the stand-alone kernel has all 64 in flight at once:
        //  the step kernel's own first load round is alive beside them.  Same values, same order of additions.)
        int qo = 4 * q;
        f32x4 M = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int w = 0; w < HEADS_WAVES; ++w) {
            const f32x4 mw = *reinterpret_cast<const f32x4*>(&sm.wmax[w][qo]);
#pragma unroll
            for (int i = 0; i < 4; ++i) M[i] = fmaxf(M[i], mw[i]);
        }
        f32x4 S = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < HEADS_WAVES; ++w) {
            if (STEP && (w & 3) == 0) {
                const float d0 = w ? S[0] : M[0], d1 = w ? S[1] : M[1], d2 = w ? S[2] : M[2], d3 = w ? S[3] : M[3];
                asm volatile("" : "+v"(qo) : "v"(d0), "v"(d1), "v"(d2), "v"(d3));
            }
            const f32x4 mw = *reinterpret_cast<const f32x4*>(&sm.wmax[w][qo]);
            const f32x4 sw = *reinterpret_cast<const f32x4*>(&sm.wsum[w][qo]);
#pragma unroll
            for (int i = 0; i < 4; ++i) S[i] += sw[i] * __expf(mw[i] - M[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) scale[i] = __expf(m[i] - M[i]) / S[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int brd = b0 + 4 * q + i;
        if (!((live4 >> i) & 1)) continue;
        if (STEP) {
            float* p = &lds_policy[4 * q + i][16 * wave + c];
#pragma unroll
            for (int j = 0; j < 2; ++j) if (16 * (wave + 8 * j) + c < A) p[128 * j] = ex[j][i] * scale[i];
            continue;
        }
        const size_t row = (size_t)brd * A + 16 * wave + c;     // one 64-bit address per board row, this wave's tiles at +512 B steps
        if (policy) {
            float* __restrict__ p = policy + row;
#pragma unroll
            for (int j = 0; j < 2; ++j) if (16 * (wave + 8 * j) + c < A) p[128 * j] = ex[j][i] * scale[i];
        }
        if (logits) {
            float* __restrict__ l = logits + row;
#pragma unroll
            for (int j = 0; j < 2; ++j) if (16 * (wave + 8 * j) + c < A) l[128 * j] = lg[j][i];
        }
    }
    return 0.f;
}

}  // namespace aqg
