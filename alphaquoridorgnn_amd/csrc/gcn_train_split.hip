// gcn_train_split.hip -- train_board_split_kernel: the fp16-split form of the fused training step's board launch (option
// "train_fused" 2, the default on 9x9; 3 forces its fallback).  The fallback inlines the exact-f32 body (gcn_train_exact.hpp); the
// heads (gcn_train_heads.hpp) are a real callee here, heads_board_call.
#define AQG_TRAIN_TU split
#include "gcn_train_exact.hpp"

namespace aqg {

// ---------------------------------------------------------------------------------------------
// The same step of ONE 9x9 position with every contraction on the 16-bit matrix pipe in split precision (split_mfma.hpp): the
// default on the 9x9 board.  v_mfma_f32_16x16x32_f16 runs at 16x the rate of the f32-input MFMA the exact body (gcn_train_exact.hpp) uses; with three
// fp16 terms per f32 product the contractions cost a fifth, and the neighbourhood aggregation -- a VALU gather over LDS there,
// 38 % of that kernel -- becomes 30 MFMAs on the board's banded A_hat (ten 32x16 blocks, f32 entries split hi / lo).
//
// Layouts.  Wave w owns feature columns 16 w .. 16 w + 15 everywhere.  A 16x16 accumulator tile has lane = column c (lane & 15)
// and rows 4 q + r (q = lane >> 4) in its four registers; two consecutive row tiles of NODES are therefore an operand fragment of
// any product contracted over the nodes (k-slot order of split_mfma.hpp), with no data movement:
//   linear map      U = X W^T        A = fp16 planes of X in LDS [node][feature] (ds_read_b128), B = this wave's rows of W, split on
//                                    the fly from the f32 master weights  ->  U: lane = feature, registers = nodes
//   aggregation, T  V^T = U^T A_hat  A = U (registers), B = A_hat block  ->  lane = node, registers = 4 consecutive features:
//                                    relu, split, 8-byte plane stores: the next linear map's A operand
//   aggregation, R  V = A_hat U      A = A_hat block (the SAME fragment: A_hat is symmetric), B = U (registers)  ->  lane = feature,
//                                    registers = nodes: an operand of the weight gradient dW = dZ^T H, which contracts over nodes
//   weight gradient dW[all j][k in the wave's 16] = sum_n dZ[n][j] H[n][k]: B = the wave's OWN H fragments (form R of the forward
//                                    pass, parked in memory lane-linearly and read back), A = the dZ fragments of all eight waves
//                                    through 48 KB of LDS, lane-linear (form R of the backward pass)
// so a layer costs 72 (linear) + 30 + 30 (both forms) MFMAs per wave going forward, and 72 (data gradient) + 60 + 72 (weight
// gradient) going back; nothing is ever transposed.  ReLU masks are 24 bits per lane and layer, kept in registers.
// Range: the backward pass is scaled per board by a power of two that puts max |dg| at 128..256 (the gradients of a mean loss over
// 128 positions would otherwise sit in fp16's subnormals) and unscaled, exactly, at the stores of the partial sums.  Forward values
// are NOT scaled: they are O(1) for weights of ordinary scale only.  Two checks send a board to the exact-f32 body in the same launch
// (counted in g_train_fallbacks) -- the reference's fp32 has neither cliff:
//   high side  every f32 value is range-checked before it is split; a board that meets |x| > 65504 anywhere is redone;
//   low side   a block of a GCN weight matrix -- the 16 output features of one wave -- that is not all zero and whose largest entry
//              is below SPLIT_MIN_TRAIN_SCALE (split_mfma.hpp: its lo halves are subnormal, it is carried to 2^-25 absolute
//              whatever its own scale, and the ReLU masks of those features are decided by that error) counts as a value out of
//              range -- a static test on the weights, so it redoes every board of the step.  Activations that are small under
//              weights of ordinary scale are not tested.
// ---------------------------------------------------------------------------------------------
struct alignas(16) SplitSmem {
    alignas(16) unsigned char P[2][PPLANE];                 // fp16 hi / lo planes [node][feature]: H_l going forward, dZ_l going back
    alignas(16) unsigned int AF[2][AF_BLOCKS][64][4];       // hi / lo fragments of the ten non-zero blocks of A_hat
    alignas(16) unsigned int FR[8][3][2][64][4];            // [wave][k block][hi / lo]: dZ_l as A fragments of the weight gradient (the heads' scratch before)
    alignas(16) unsigned short X0A[96][8];                  // the six input features per node (fp16, exact), rows of the layer-1 A operand
    alignas(16) unsigned short X0T[16][96];                 // ... and feature-major: B operand of layer 1's weight gradient
    alignas(16) float dinv[96];                             // deg^-1/2 (self loop included), 0 for the padding nodes
    unsigned char ob[96];                                   // open sides of a tile: bit 0 up (n - 9), 1 down, 2 left, 3 right
};
static_assert(sizeof(TrainHeadsSmem) <= sizeof(unsigned int) * 8 * 3 * 2 * 64 * 4, "heads scratch aliases FR");
constexpr int SPLIT_KERNEL_SMEM = (int)sizeof(SplitSmem) > F32_BODY_SMEM ? (int)sizeof(SplitSmem) : F32_BODY_SMEM;
static_assert(SPLIT_KERNEL_SMEM <= 160 * 1024, "one workgroup per CU");
__device__ unsigned int g_train_fallbacks = 0;
constexpr int BWD_SCALE_LOG2 = 7;       // max |dg| s in [128, 256): dP3 = dg s / 81 <= 3.2, 2^14 of headroom, every lo half a normal fp16

// Range guard: the largest |x| this lane has split.  (The bit-pattern form of the inference trunk -- one signed and one unsigned
// integer maximum, one v_max3 per two values each, no canonicalising v_max per operand -- saves 400 of this body's 3,300 vector
// instructions and was 7 % SLOWER here, 0.0610 against 0.0571 ms per step in a same-box A/B; retired.)
struct Rng { float m = 0.f; };
__device__ __forceinline__ void trk(Rng& m, float a, float b) { m.m = fmaxf(m.m, fmaxf(fabsf(a), fabsf(b))); }
__device__ __forceinline__ bool out_of_fp16_range(const Rng& m) { return !(m.m <= 65504.0f); }
// relu on the bit pattern: one v_max_i32, no canonicalising v_max on top as fmaxf(x, 0.f) has (that form was the ablation; retired).
// (through a scalar parameter: __builtin_bit_cast applied to a vector ELEMENT expression read element 0 for all four -- hipcc 7.2)
__device__ __forceinline__ float relu1i(float x) { return __builtin_bit_cast(float, max(__builtin_bit_cast(int, x), 0)); }
// 1 if x > 0 else 0, on the bit pattern (a positive float is a positive integer): one v_med3_i32
__device__ __forceinline__ unsigned int positive_bit(float x) { return (unsigned int)min(max(__builtin_bit_cast(int, x), 0), 1); }
__device__ __forceinline__ void trk(Rng& m, const f32x4 v) { trk(m, v[0], v[1]); trk(m, v[2], v[3]); }
__device__ __forceinline__ f32x4 relu4i(const f32x4 v) { return f32x4{relu1i(v[0]), relu1i(v[1]), relu1i(v[2]), relu1i(v[3])}; }
__device__ __forceinline__ void mfma_fence(u32x4& a) { asm volatile("s_nop 3" : "+v"(a)); }
// tile m of a [nodes][16] accumulator image -> dwords 2 (m & 1), + 1 of k block m >> 1 of its hi / lo node-contraction fragments
// The range check of two values that are being split: ONE v_max3_f32 with |.| modifiers (fmaxf(|a|, |b|) costs the compiler a
// canonicalising v_max per operand on top).  As an asm statement it must not be the first reader of a matrix-pipe result (hipcc pads
// nothing for asm): `dep` is the packed fp16 pair the compiler-visible v_cvt_pk has just made of the same two values, so the check
// sits behind that instruction, the way lo_pair() does.
__device__ __forceinline__ void trk_after(Rng& m, unsigned int dep, float a, float b) {
    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m.m) : "v"(a), "v"(b), "v"(dep));
}
__device__ __forceinline__ void split_tile(const f32x4 z, int m, u32x4 (&zh)[3], u32x4 (&zl)[3], Rng* rng = nullptr) {
    const int kb = m >> 1, d = 2 * (m & 1);
    zh[kb][d] = cvt_pk_f16(z[0], z[1]); zh[kb][d + 1] = cvt_pk_f16(z[2], z[3]);
    if (rng) { trk_after(*rng, zh[kb][d], z[0], z[1]); trk_after(*rng, zh[kb][d + 1], z[2], z[3]); }
    zl[kb][d] = lo_pair(zh[kb][d], z[0], z[1]); zl[kb][d + 1] = lo_pair(zh[kb][d + 1], z[2], z[3]);
}
__device__ __forceinline__ void plane_store4(unsigned char (&P)[2][PPLANE], int off, const f32x4 v, Rng* rng = nullptr) {
    const unsigned int h01 = cvt_pk_f16(v[0], v[1]), h23 = cvt_pk_f16(v[2], v[3]);
    if (rng) { trk_after(*rng, h01, v[0], v[1]); trk_after(*rng, h23, v[2], v[3]); }
    *reinterpret_cast<u32x2*>(&P[0][off]) = (u32x2){h01, h23};
    *reinterpret_cast<u32x2*>(&P[1][off]) = (u32x2){lo_pair(h01, v[0], v[1]), lo_pair(h23, v[2], v[3])};
}
__device__ __forceinline__ bool live_row(int nt, int q, int r) { return nt < 5 || (q == 0 && r == 0); }      // node 16 nt + 4 q + r < 81

// U = X W^T for this wave's 16 columns from the planes (six 16-row tiles, tile 5 = row 80 repeated, x four 32-deep k blocks, three
// fp16 terms, smallest first); post(m, tile) sees every finished tile before it is split into the node-contraction fragments.
template <class Post>
__device__ __forceinline__ void linear_split_post(const unsigned char (&P)[2][PPLANE], const u32x4 (&Bh)[4], const u32x4 (&Bl)[4], int lane,
                                                  u32x4 (&zh)[3], u32x4 (&zl)[3], Rng& rng, Post post) {
    const int c = lane & 15, q = lane >> 4;
    // The fragments of step s + D are requested while step s multiplies (a ring of that many register pairs).  One step ahead is
    // enough: 2 / 3 / 5 steps measured 0.0568 / 0.0572 / 0.0613 ms per step against 0.0565 -- the phase is not waiting for LDS.
    constexpr int D = 1;
    u32x4 ring[D + 1][2];
    auto frag_off = [&](int step) -> int {
        const int m = step >> 2, kb = step & 3;
        return plane_off(m < 5 ? 16 * m + c : 80, 4 * kb + q);
    };
    auto request = [&](int step) {
        const int o = frag_off(step);
        ring[step % (D + 1)][0] = *reinterpret_cast<const u32x4*>(&P[0][o]);
        ring[step % (D + 1)][1] = *reinterpret_cast<const u32x4*>(&P[1][o]);
    };
#pragma unroll
    for (int i = 0; i < D; ++i) request(i);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, done = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int step = 0; step < 24; ++step) {
        const int m = step >> 2, kb = step & 3;
        if (step + D < 24) request(step + D);
        __builtin_amdgcn_sched_barrier(0);                              // (keeps the 48 fragment reads from being hoisted in a body: 192 registers)
        const u32x4 hi = ring[step % (D + 1)][0], lo = ring[step % (D + 1)][1];
        f32x4 a = kb == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc;
        a = mfma_f16(lo, Bh[kb], a);
        a = mfma_f16(hi, Bl[kb], a);
        a = mfma_f16(hi, Bh[kb], a);
        acc = a;
        // the finished tile m - 1 is masked / checked and split under tile m's first MFMA group
        if (m > 0 && kb == 0) { post(m - 1, done); split_tile(done, m - 1, zh, zl, &rng); }
        __builtin_amdgcn_sched_barrier(0);
        if (kb == 3) done = acc;
    }
    post(5, done);
    split_tile(done, 5, zh, zl, &rng);
}

// Both forms of the aggregation over the ten blocks (header of this section), node tile by node tile: the blocks of a tile are
// consecutive, and epi(nt, oT, oR) gets the finished tile (started from the presets pT / pR: bias rows or zero) while the next
// tile's MFMAs are issued -- only one tile's accumulators are alive at a time.
template <bool DO_T, bool DO_R, class Epi>
__device__ __forceinline__ void aggregate_tr(const unsigned int (&AF)[2][AF_BLOCKS][64][4], const u32x4 (&zh)[3], const u32x4 (&zl)[3],
                                             const f32x4 pT, const f32x4 pR, int lane, Epi epi) {
    f32x4 oT = pT, oR = pR;
#pragma unroll
    for (int blk = 0; blk < AF_BLOCKS; ++blk) {
        const int kb = af_kb(blk), nt = af_nt(blk);
        const u32x4 ah = *reinterpret_cast<const u32x4*>(&AF[0][blk][lane][0]);
        const u32x4 al = *reinterpret_cast<const u32x4*>(&AF[1][blk][lane][0]);
        if (DO_T) {
            oT = mfma_f16(zl[kb], ah, oT);
            oT = mfma_f16(zh[kb], al, oT);
            oT = mfma_f16(zh[kb], ah, oT);
        }
        if (DO_R) {
            oR = mfma_f16(ah, zl[kb], oR);
            oR = mfma_f16(al, zh[kb], oR);
            oR = mfma_f16(ah, zh[kb], oR);
        }
        if (blk + 1 == AF_BLOCKS || af_nt(blk + 1) != nt) {
            epi(nt, oT, oR);
            oT = pT; oR = pR;
        }
    }
}

// (a real call: inlined into the split body, the heads' ~130 registers on top of the trunk's state spill -- 300 registers, and the
//  heads alone then take 124 k cycles instead of 25 k; as a callee they get a register allocation of their own)
//  (the scratch travels as its LDS byte offset and is cast back from the LDS address space inside, so that the callee's accesses are
//  ds_ instructions, not flat ones)
typedef __attribute__((address_space(3))) TrainHeadsSmem TrainHeadsSmemLds;
typedef const __attribute__((address_space(1))) float* gcf;           // pointer arguments in the global address space: global_, not flat_
typedef __attribute__((address_space(1))) float* gf;
//  (LF: the loss form of heads_board; the plain form's arguments are what they have always been, any other form's value weight
//  travels as one more register argument)
template <int LF = LOSS_PLAIN, class... VW>
__device__ __attribute__((noinline)) void heads_board_call(unsigned int sm_lds, int b, gcf w0, gcf w1, gcf w2, gcf w3, gcf w4, gcf w5, gcf w6, gcf w7,
                                                           gcf pi_all, gcf z_all, const __attribute__((address_space(1))) int64_t* order, int first,
                                                           int A, int B, gf hp, gf hv, gf lg, gf pol, gf vp, gf val, gf loss, gf dhp, gf dhv, VW... vw) {
    static_assert(sizeof...(VW) == (LF == LOSS_PLAIN ? 0 : 1), "a value weight with every form but the plain one");
    TrainHeadsSmem& sm = *(TrainHeadsSmem*)reinterpret_cast<TrainHeadsSmemLds*>((size_t)sm_lds);
    HeadParams Pg;
    Pg.p[0] = (const float*)w0; Pg.p[1] = (const float*)w1; Pg.p[2] = (const float*)w2; Pg.p[3] = (const float*)w3;
    Pg.p[4] = (const float*)w4; Pg.p[5] = (const float*)w5; Pg.p[6] = (const float*)w6; Pg.p[7] = (const float*)w7;
    heads_board<LF>(sm, b, Pg, (const float*)pi_all, (const float*)z_all, (const int64_t*)order, first, A, B, (float*)hp, (float*)hv,
                    (float*)lg, (float*)pol, (float*)vp, (float*)val, (float*)loss, (float*)dhp, (float*)dhv, vw...);
}

// returns false (to every thread of the workgroup) if a value left fp16 range or a block of weights sits below the split's scale
// (header): the caller redoes the board with the f32 body
template <int LF = LOSS_PLAIN, class... VW>
__device__ __forceinline__ bool train_board_split_body(unsigned char* __restrict__ smem, const uint8_t* __restrict__ states72,
                                                       const int64_t* __restrict__ order, int first,
                                                       const TrunkParams& tp, const HeadParams& hpm, const float* __restrict__ pi_all,
                                                       const float* __restrict__ z_all, int A, int B,
                                                       float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ g_out,
                                                       float* __restrict__ hp, float* __restrict__ hv, float* __restrict__ lg,
                                                       float* __restrict__ pol, float* __restrict__ vp, float* __restrict__ val,
                                                       float* __restrict__ loss, float* __restrict__ dhp, float* __restrict__ dhv,
                                                       float* __restrict__ part_dW3, float* __restrict__ part_dW2,
                                                       float* __restrict__ part_dW1, float* __restrict__ part_db, VW... vw) {
    constexpr int N = 9, V = 81;
    SplitSmem& sm = *reinterpret_cast<SplitSmem*>(smem);
    TrainHeadsSmem& hsm = *reinterpret_cast<TrainHeadsSmem*>(&sm.FR[0][0][0][0][0]);
    const int b = blockIdx.x, t = threadIdx.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), q = lane >> 4, c = lane & 15;
    const int col = 16 * wave + c;
    const float *W1 = tp.p[0], *b1 = tp.p[1], *W2 = tp.p[2], *b2 = tp.p[3], *W3 = tp.p[4], *b3 = tp.p[5];
    Rng mx;                                                            // range guard over everything this lane splits
    // low side (header): m = the largest |entry| this lane holds of its wave's 16 rows of a GCN weight matrix.  Two ballots, nothing
    // kept, no branch (one would end the block the weight loads are scheduled in): a block below the scale poisons the range
    // guard's maximum, which also takes in m itself
    auto weight_block_scale = [&](float m) {
        const unsigned int none_at_scale = __builtin_amdgcn_ballot_w64(m >= SPLIT_MIN_TRAIN_SCALE) == 0 ? 1u : 0u;
        const unsigned int some_nonzero = __builtin_amdgcn_ballot_w64(m > 0.f) != 0 ? 1u : 0u;
        mx.m = fmaxf(mx.m, __builtin_bit_cast(float, (none_at_scale & some_nonzero) * 0x7f800000u) + m);      // + inf, or m itself
    };
    TS_DECL
    // ---- loads that do not depend on the board: biases (both layouts), W1, W2 rows of this wave's columns
    const f32x4 bT1 = ld4(b1 + 16 * wave + 4 * q), bT2 = ld4(b2 + 16 * wave + 4 * q);
    const float bR1 = b1[col], bR2 = b2[col], bR3 = b3[col];
    float w1v[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) w1v[e] = q == 0 ? W1[col * TF + e] : 0.f;
    f32x4 wf[8];                                                       // W_l[col][32 kb + 8 q + 0..7]: B fragments of the forward linear maps
    auto request_w = [&](const float* __restrict__ W) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) { wf[2 * kb] = ld4(W + (size_t)col * TH + 32 * kb + 8 * q); wf[2 * kb + 1] = ld4(W + (size_t)col * TH + 32 * kb + 8 * q + 4); }
    };
    u32x4 Bh[4], Bl[4];
    auto split_w = [&]() {
        Rng wm;                                                         // the block's own maximum: the low-side test (header)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const f32x4 a = wf[2 * kb], bb = wf[2 * kb + 1];
            Bh[kb] = (u32x4){cvt_pk_f16(a[0], a[1]), cvt_pk_f16(a[2], a[3]), cvt_pk_f16(bb[0], bb[1]), cvt_pk_f16(bb[2], bb[3])};
            trk_after(wm, Bh[kb][0], a[0], a[1]); trk_after(wm, Bh[kb][1], a[2], a[3]);
            trk_after(wm, Bh[kb][2], bb[0], bb[1]); trk_after(wm, Bh[kb][3], bb[2], bb[3]);
            Bl[kb] = (u32x4){lo_pair(Bh[kb][0], a[0], a[1]), lo_pair(Bh[kb][1], a[2], a[3]), lo_pair(Bh[kb][2], bb[0], bb[1]), lo_pair(Bh[kb][3], bb[2], bb[3])};
            mfma_fence(Bl[kb]);
        }
        weight_block_scale(wm.m);
    };
    request_w(W2);
    // (warming the heads' matrices into this XCD's L2 from here -- one load per 64-byte line, as the f32 body does -- measured 6 % SLOWER
    //  for this body: 0.0607 against 0.0572 ms per step, tools/ab_train.sh)
    // ---- the board: features, open sides, deg^-1/2
    const uint8_t* rec = states72 + record_of(order, first, b) * STATE72;
    if (t < 96) {
        unsigned short xa[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        float di = 0.f;
        int ob = 0;
        if (t < V) {
            const QState s = unpack72(rec);
            const int x = t / N, y = t % N;
            const bool slot_ok = x < N - 1 && y < N - 1;
            const int slot = x * (N - 1) + y;
            const unsigned short one = 0x3C00;
            xa[0] = t == s.ppos ? one : 0;
            xa[1] = __builtin_bit_cast(unsigned short, (_Float16)(float)s.pwl);
            xa[2] = t == s.epos ? one : 0;
            xa[3] = __builtin_bit_cast(unsigned short, (_Float16)(float)s.ewl);
            xa[4] = (slot_ok && ((s.hw >> slot) & 1)) ? one : 0;
            xa[5] = (slot_ok && ((s.vw >> slot) & 1)) ? one : 0;
            ob = tile_open_bits<N>(s.hw, s.vw, t);
            di = 1.0f / sqrtf((float)(1 + __popc(ob)));
        }
        *reinterpret_cast<u32x4*>(&sm.X0A[t][0]) = (u32x4){xa[0] | ((unsigned)xa[1] << 16), xa[2] | ((unsigned)xa[3] << 16), xa[4] | ((unsigned)xa[5] << 16), 0u};
#pragma unroll
        for (int k = 0; k < 8; ++k) sm.X0T[k][t] = xa[k];
        sm.dinv[t] = di;
        sm.ob[t] = (unsigned char)ob;
    } else if (t < 96 + 8 * 96 / 2) {
        reinterpret_cast<unsigned int*>(&sm.X0T[8][0])[t - 96] = 0u;                     // feature rows 8..15 of the padded tile
    }
    __syncthreads();
    TS(3, 0)
    // ---- A_hat fragments: entry (k-slot e of lane (c, q), block (kb, nt)) = dinv[n] dinv[k] where k is in the closed neighbourhood of n = 16 nt + c
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int blk = wave + 8 * it;                                                   // wave-uniform
        if (blk < AF_BLOCKS) {
            const int kb = (AF_KB_PACK >> (2 * blk)) & 3, nt = (AF_NT_PACK >> (3 * blk)) & 7;
            const int n = 16 * nt + c;
            const int obn = sm.ob[n];
            const float dn = sm.dinv[n];
            float v[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k0 = 32 * kb + 16 * h + 4 * q;
                const f32x4 dk = *reinterpret_cast<const f32x4*>(&sm.dinv[k0]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = k0 + i - n;
                    const bool adj = d == 0 || (d == -N && (obn & 1)) || (d == N && (obn & 2)) || (d == -1 && (obn & 4)) || (d == 1 && (obn & 8));
                    v[4 * h + i] = adj ? dn * dk[i] : 0.f;
                }
            }
            u32x4 fh, fl;
#pragma unroll
            for (int p = 0; p < 4; ++p) { fh[p] = cvt_pk_f16(v[2 * p], v[2 * p + 1]); fl[p] = lo_pair(fh[p], v[2 * p], v[2 * p + 1]); }
            *reinterpret_cast<u32x4*>(&sm.AF[0][blk][lane][0]) = fh;
            *reinterpret_cast<u32x4*>(&sm.AF[1][blk][lane][0]) = fl;
        }
    }
    // ---- layer 1, linear: Z1 = X0 W1^T (K = 6 in one 32-deep block; X0 is exact in fp16: two terms)
    u32x4 zh[3], zl[3];
    {
        u32x4 w1h = {cvt_pk_f16(w1v[0], w1v[1]), cvt_pk_f16(w1v[2], w1v[3]), cvt_pk_f16(w1v[4], w1v[5]), 0u};
        u32x4 w1l = {lo_pair(w1h[0], w1v[0], w1v[1]), lo_pair(w1h[1], w1v[2], w1v[3]), lo_pair(w1h[2], w1v[4], w1v[5]), 0u};
        mfma_fence(w1l);
        Rng w1m;
        trk_after(w1m, w1h[0], w1v[0], w1v[1]); trk_after(w1m, w1h[1], w1v[2], w1v[3]); trk_after(w1m, w1h[2], w1v[4], w1v[5]);
        weight_block_scale(w1m.m);
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            u32x4 xa = *reinterpret_cast<const u32x4*>(&sm.X0A[m < 5 ? 16 * m + c : 80][0]);
            if (q != 0) xa = (u32x4){0u, 0u, 0u, 0u};
            f32x4 z = mfma_f16(xa, w1l, (f32x4){0.f, 0.f, 0.f, 0.f});
            z = mfma_f16(xa, w1h, z);
            split_tile(z, m, zh, zl, &mx);
        }
    }
    __syncthreads();                                                   // A_hat fragments complete
    TS(3, 1)
    // ---- forward epilogues
    const int poff = (2 * wave + (q >> 1)) /* 16-byte slot of features 16 w + 4 q .. */, pbyte = 8 * (q & 1);
    auto store_plane_tile = [&](int nt, f32x4 v, bool relu) {          // T form: lane = node c of tile nt, features 16 w + 4 q + r
        if (relu) v = relu4i(v);                                        // (what is split is range-checked: a pre-activation below -65504 is a zero)
        if (nt < 5 || c == 0) plane_store4(sm.P, plane_off(16 * nt + c, poff) + pbyte, v, &mx);
    };
    unsigned int msk[3] = {0u, 0u, 0u};                                 // ReLU masks of the three layers: bit 4 nt + r, R layout
    u32x4 hh[3], hl[3];                                                 // R form of H_l (lane = feature c, nodes 16 nt + 4 q + r) as fragments
    auto park_tile = [&](int nt, f32x4 v, unsigned int& m) {       // (the same values as the T form, which store_plane_tile has range-checked)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                  // (a NaN would count as positive: the range guard has long fired then)
            const float x = v[r];
            if (nt < 5) m |= positive_bit(x) << (4 * nt + r);
            else if (live_row(nt, q, r)) m |= positive_bit(x) << (4 * nt + r);
        }
        v = relu4i(v);
        split_tile(v, nt, hh, hl);
    };
    auto park_store = [&](float* __restrict__ hpark) {
        u32x4* dst = reinterpret_cast<u32x4*>(hpark + (size_t)b * 96 * TH) + (size_t)wave * 6 * 64 + lane;
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) { dst[(2 * kb) * 64] = hh[kb]; dst[(2 * kb + 1) * 64] = hl[kb]; }
    };
    // ---- layer 1: aggregation, planes of H1, parked fragments of H1
#pragma unroll
    for (int kb = 0; kb < 3; ++kb) mfma_fence(zl[kb]);
    aggregate_tr<true, true>(sm.AF, zh, zl, bT1, (f32x4){bR1, bR1, bR1, bR1}, lane, [&](int nt, const f32x4& oT, const f32x4& oR) {
        store_plane_tile(nt, oT, true);
        park_tile(nt, oR, msk[0]);
    });
    TS(3, 14)
    park_store(h1);
    split_w();                                                          // W2 fragments
    request_w(W3);
    TS(3, 15)
    __syncthreads();                                                    // planes of H1 complete
    TS(3, 2)
    // ---- layer 2
    linear_split_post(sm.P, Bh, Bl, lane, zh, zl, mx, [&](int, f32x4&) {});
#pragma unroll
    for (int kb = 0; kb < 3; ++kb) mfma_fence(zl[kb]);
    __syncthreads();                                                    // everybody has read the planes of H1
    TS(3, 3)
    aggregate_tr<true, true>(sm.AF, zh, zl, bT2, (f32x4){bR2, bR2, bR2, bR2}, lane, [&](int nt, const f32x4& oT, const f32x4& oR) {
        store_plane_tile(nt, oT, true);
        park_tile(nt, oR, msk[1]);
    });
    park_store(h2);
    split_w();                                                          // W3 fragments
    __syncthreads();                                                    // planes of H2 complete
    TS(3, 4)
    // ---- layer 3 (R form only: its ReLU mask and the mean pool; H3 itself is not needed again)
    linear_split_post(sm.P, Bh, Bl, lane, zh, zl, mx, [&](int, f32x4&) {});
#pragma unroll
    for (int kb = 0; kb < 3; ++kb) mfma_fence(zl[kb]);
    {
        float s = 0.f;
        aggregate_tr<false, true>(sm.AF, zh, zl, bT2, (f32x4){bR3, bR3, bR3, bR3}, lane, [&](int nt, const f32x4&, const f32x4& oR) {
            // (H3 is not split: only its signs and its f32 column sums are used)
#pragma unroll
            for (int r = 0; r < 4; ++r) if (oR[r] > 0.f && live_row(nt, q, r)) { msk[2] |= 1u << (4 * nt + r); s += oR[r]; }
        });
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        s /= (float)V;                                                  // global_mean_pool
        // (FR, which the heads' scratch aliases, is first written in the backward pass)
        if (q == 0) { hsm.gs[col] = s; g_out[(size_t)b * TH + col] = s; }
    }
    // the backward pass's own operands: W_{l+1}^T fragments of the data gradients and this wave's parked H_{l-1} (requested a phase ahead)
    float wt[32];                                                       // W_l[32 kb + 8 q + e][col]: B fragments of the data gradients
    auto request_wt = [&](const float* __restrict__ W) {
#pragma unroll
        for (int i = 0; i < 32; ++i) wt[i] = W[(size_t)(32 * (i >> 3) + 8 * q + (i & 7)) * TH + col];
    };
    auto split_wt = [&]() {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float a0 = wt[8 * kb + 2 * p], a1 = wt[8 * kb + 2 * p + 1];
                Bh[kb][p] = cvt_pk_f16(a0, a1);                 // (range-checked as W_l's rows by split_w: the eight waves' rows are the whole matrix)
                Bl[kb][p] = lo_pair(Bh[kb][p], a0, a1);
            }
            mfma_fence(Bl[kb]);
        }
    };
    auto request_h = [&](const float* __restrict__ hpark) {
        const u32x4* src = reinterpret_cast<const u32x4*>(hpark + (size_t)b * 96 * TH) + (size_t)wave * 6 * 64 + lane;
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) { hh[kb] = src[(2 * kb) * 64]; hl[kb] = src[(2 * kb + 1) * 64]; }
    };
    TS(3, 5)
    // ---- heads, losses, head gradients (its first barrier publishes gs)
    heads_board_call<LF>((unsigned int)(size_t)(TrainHeadsSmemLds*)&hsm, b, (gcf)hpm.p[0], (gcf)hpm.p[1], (gcf)hpm.p[2], (gcf)hpm.p[3], (gcf)hpm.p[4], (gcf)hpm.p[5],
                     (gcf)hpm.p[6], (gcf)hpm.p[7], (gcf)pi_all, (gcf)z_all, (const __attribute__((address_space(1))) int64_t*)order, first, A, B,
                     (gf)hp, (gf)hv, (gf)lg, (gf)pol, (gf)vp, (gf)val, (gf)loss, (gf)dhp, (gf)dhv, vw...);
    TS(3, 6)
    {
        // (requested BEHIND the call: hoisted above it -- which the compiler does unless the base pointers pass through this empty
        //  asm statement -- the 56 registers would be loaded, waited for, spilled around the call and reloaded)
        const float* W3b = W3;
        const float* h2b = h2;
        asm volatile("" : "+s"(W3b), "+s"(h2b));
        request_wt(W3b);
        request_h(h2b);
    }
    // ---- backward.  dg = hsm.dgv; scaled by a power of two s with max |dg| s in [128, 256)
    float dgs, inv_s;
    {
        const float d0 = hsm.dgv[lane], d1 = hsm.dgv[64 + lane];
        const float m = wave_max(fmaxf(fabsf(d0), fabsf(d1)));
        const int e = (__builtin_bit_cast(int, m) >> 23) & 0xFF;
        int es = 254 + BWD_SCALE_LOG2 - e;                              // biased exponent of s = 2^(BWD_SCALE_LOG2 - (e - 127))
        es = (e == 0 || e == 255) ? 127 : min(max(es, 1), 254);
        const float s = __builtin_bit_cast(float, es << 23);
        inv_s = 1.0f / s;
        dgs = hsm.dgv[col] * s / (float)V;                              // global_mean_pool backward, this lane's column
    }
    __syncthreads();                                                    // the heads' scratch is dead: FR may be written
    auto store_db = [&](float sdb, int layer) {
        sdb += __shfl_xor(sdb, 16);
        sdb += __shfl_xor(sdb, 32);
        if (q == 0) part_db[((size_t)layer * B + b) * TH + col] = sdb * inv_s;
    };
    u32x4 ah[3], al[3];                                                 // R form of dZ_l: A fragments of dW_l
    auto publish_dz = [&]() {
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) {
            *reinterpret_cast<u32x4*>(&sm.FR[wave][kb][0][lane][0]) = ah[kb];
            *reinterpret_cast<u32x4*>(&sm.FR[wave][kb][1][lane][0]) = al[kb];
        }
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto aggregate_back = [&](bool planes) {
        if (planes)
            aggregate_tr<true, true>(sm.AF, zh, zl, zero4, zero4, lane, [&](int nt, const f32x4& oT, const f32x4& oR) {
                store_plane_tile(nt, oT, false);                        // dZ_l: A operand of the next data gradient (range-checked there; oR repeats it)
                split_tile(oR, nt, ah, al);
            });
        else
            aggregate_tr<false, true>(sm.AF, zh, zl, zero4, zero4, lane, [&](int nt, const f32x4&, const f32x4& oR) {
                split_tile(oR, nt, ah, al, &mx);
            });
    };
    auto weight_grad = [&](float* __restrict__ pdW) {                   // dW_l[all j][this wave's k]: A = parked H_{l-1}, B = FR (all waves)
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) mfma_fence(hl[kb]);              // (loaded, not computed: harmless)
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) {
            // the TRANSPOSED tile dW^T[k][j] = sum_n H[n][k] dZ[n][j]: lane = row j = 16 jt + c of dW, registers = 4 consecutive
            // columns k = 16 w + 4 q + r -- one 16-byte store per tile and lane (the other operand order needs four 4-byte ones)
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 3; ++kb) {
                const u32x4 zh_ = *reinterpret_cast<const u32x4*>(&sm.FR[jt][kb][0][lane][0]);
                const u32x4 zl_ = *reinterpret_cast<const u32x4*>(&sm.FR[jt][kb][1][lane][0]);
                o = mfma_f16(hl[kb], zh_, o);
                o = mfma_f16(hh[kb], zl_, o);
                o = mfma_f16(hh[kb], zh_, o);
            }
            st4(pdW + (size_t)b * TH * TH + (size_t)(16 * jt + c) * TH + 16 * wave + 4 * q, o * inv_s);
        }
    };
    // layer 3: dP3 = dg / V on the nodes whose H3 is positive
    {
        float sdb = 0.f;
#pragma unroll
        for (int nt = 0; nt < 6; ++nt) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = ((msk[2] >> (4 * nt + r)) & 1u) ? dgs : 0.f; sdb += v[r]; }
            split_tile(v, nt, zh, zl);
        }
        trk(mx, dgs, dgs);
        store_db(sdb, 2);
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) mfma_fence(zl[kb]);
        aggregate_back(true);                                           // (every wave left the planes of H2 long ago)
        publish_dz();
        split_wt();                                                     // W3^T fragments
        request_wt(W2);
        __syncthreads();                                                // planes and fragments of dZ3 complete
        TS(3, 7)
        weight_grad(part_dW3);
        request_h(h1);
        TS(3, 8)
    }
    // layers 2 and 1: dH_l = dZ_{l+1} W_{l+1}, masked by H_l > 0
    auto masked_linear = [&](unsigned int m, int layer) {
        float sdb = 0.f;
#ifdef AQG_TRAIN_DEBUG
        if (layer == 1)            // the planes hold dZ3 / s: dense dump of hi + lo
            for (int i = t; i < V * TH; i += 512) {
                const int n = i / TH, f = i % TH, o = plane_off(n, f >> 3) + 2 * (f & 7);
                DBG_PUT(2, B, b, n, f, ((float)*reinterpret_cast<const _Float16*>(&sm.P[0][o]) + (float)*reinterpret_cast<const _Float16*>(&sm.P[1][o])) * inv_s)
            }
#endif
        linear_split_post(sm.P, Bh, Bl, lane, zh, zl, mx, [&](int mt, f32x4& z) {
#ifdef AQG_TRAIN_DEBUG
            if (layer == 1) for (int r = 0; r < 4; ++r) if (live_row(mt, q, r)) DBG_PUT(1, B, b, 16 * mt + 4 * q + r, col, z[r] * inv_s)
#endif
#pragma unroll
            for (int r = 0; r < 4; ++r) { if (!((m >> (4 * mt + r)) & 1u)) z[r] = 0.f; sdb += z[r]; }
#ifdef AQG_TRAIN_DEBUG
            if (layer == 1) for (int r = 0; r < 4; ++r) if (live_row(mt, q, r)) DBG_PUT(0, B, b, 16 * mt + 4 * q + r, col, z[r] * inv_s)
#endif
        });
        store_db(sdb, layer);
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) mfma_fence(zl[kb]);
    };
    {
        masked_linear(msk[1], 1);
        TS(3, 9)
        __syncthreads();                                                // everybody has read the planes of dZ3 (and FR: weight_grad is behind)
        aggregate_back(true);
        publish_dz();
        split_wt();                                                     // W2^T fragments
        __syncthreads();
        TS(3, 10)
        weight_grad(part_dW2);
        TS(3, 11)
    }
    {
        masked_linear(msk[0], 0);
        TS(3, 12)
        aggregate_back(false);
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) mfma_fence(al[kb]);
        // dW1[this wave's j][k < 6] = sum_n dZ1[n][j] X0[n][k]: A = own fragments, B = the feature-major X0 image (exact: two terms)
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) {
            const u32x2 x0 = *reinterpret_cast<const u32x2*>(&sm.X0T[c][32 * kb + 4 * q]);
            const u32x2 x1 = *reinterpret_cast<const u32x2*>(&sm.X0T[c][32 * kb + 16 + 4 * q]);
            const u32x4 xb = {x0[0], x0[1], x1[0], x1[1]};
            o = mfma_f16(al[kb], xb, o);
            o = mfma_f16(ah[kb], xb, o);
        }
        if (c < TF) {
            float* dst = part_dW1 + (size_t)b * TH * TF + (size_t)(16 * wave + 4 * q) * TF + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[r * TF] = o[r] * inv_s;
        }
        TS(3, 13)
    }
    return !__syncthreads_or(out_of_fp16_range(mx));
}

// option "train_fused" = 3 forces the fallback for every board (tests)
// (LF, vw: as train_board_kernel's -- the plain form takes no further argument)
template <int LF = LOSS_PLAIN, class... VW>
__global__ __launch_bounds__(512) void train_board_split_kernel(const uint8_t* __restrict__ states72, const int64_t* __restrict__ order, int first,
                                                                TrunkParams tp, HeadParams hpm, const float* __restrict__ pi_all,
                                                                const float* __restrict__ z_all, int A, int B, int force_fallback,
                                                                float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ g_out,
                                                                float* __restrict__ hp, float* __restrict__ hv, float* __restrict__ lg,
                                                                float* __restrict__ pol, float* __restrict__ vp, float* __restrict__ val,
                                                                float* __restrict__ loss, float* __restrict__ dhp, float* __restrict__ dhv,
                                                                float* __restrict__ part_dW3, float* __restrict__ part_dW2,
                                                                float* __restrict__ part_dW1, float* __restrict__ part_db, VW... vw) {
    __shared__ __align__(16) unsigned char smem[SPLIT_KERNEL_SMEM];
    const bool ok = train_board_split_body<LF>(smem, states72, order, first, tp, hpm, pi_all, z_all, A, B, h1, h2, g_out, hp, hv, lg, pol, vp,
                                               val, loss, dhp, dhv, part_dW3, part_dW2, part_dW1, part_db, vw...);
    if (ok && !force_fallback) return;
    if (threadIdx.x == 0) atomicAdd(&g_train_fallbacks, 1u);
    __syncthreads();
    train_board_f32_body<9, LF>(smem, states72, order, first, tp, hpm, pi_all, z_all, A, B, 96, h1, h2, g_out, hp, hv, lg, pol, vp, val, loss,
                                dhp, dhv, part_dW3, part_dW2, part_dW1, part_db, vw...);
}

long long train_fallbacks(int reset) {
    unsigned int v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_train_fallbacks), sizeof(v)) != hipSuccess) return -1;
    if (reset) { const unsigned int z = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(g_train_fallbacks), &z, sizeof(z)) != hipSuccess) return -1; }
    return (long long)v;
}
AQG_TRAIN_STAMP_READER(train_stamps_split)
AQG_TRAIN_DEBUG_SETTER(train_debug_buf_split)

// 9x9 only; h1 / h2 hold 96 rows per board here: the parked fragments (and the fallback's rows)
int launch_train_board_split(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first,
                             int B, int force_fallback, hipStream_t st, const aqg_loss* lf) {
    TrunkParams tp;
    for (int i = 0; i < 6; ++i) tp.p[i] = t.params[i];
    HeadParams hp;
    for (int i = 0; i < 8; ++i) hp.p[i] = t.params[6 + i];
    float *pdW3 = t.part, *pdW2 = pdW3 + (size_t)B * TH * TH, *pdW1 = pdW2 + (size_t)B * TH * TH, *pdb = pdW1 + (size_t)B * TH * TF;
    if (lf && lf->policy_form == 1)
        hipLaunchKernelGGL((train_board_split_kernel<LOSS_CE, float>), dim3(B), dim3(512), 0, st, states72, order, first, tp, hp, pi, z,
                           t.policy_size, B, force_fallback, t.h1, t.h2, t.g, t.hp, t.hv, t.lg, t.pol, t.vp, t.val, t.loss, t.dhp, t.dhv, pdW3,
                           pdW2, pdW1, pdb, lf->value_weight);
    else if (lf)
        hipLaunchKernelGGL((train_board_split_kernel<LOSS_REF_W, float>), dim3(B), dim3(512), 0, st, states72, order, first, tp, hp, pi, z,
                           t.policy_size, B, force_fallback, t.h1, t.h2, t.g, t.hp, t.hv, t.lg, t.pol, t.vp, t.val, t.loss, t.dhp, t.dhv, pdW3,
                           pdW2, pdW1, pdb, lf->value_weight);
    else
        hipLaunchKernelGGL(train_board_split_kernel<>, dim3(B), dim3(512), 0, st, states72, order, first, tp, hp, pi, z, t.policy_size, B,
                           force_fallback, t.h1, t.h2, t.g, t.hp, t.hv, t.lg, t.pol, t.vp, t.val, t.loss, t.dhp, t.dhv, pdW3, pdW2, pdW1, pdb);
    return check_launch("training forward/backward kernels");
}

}  // namespace aqg
