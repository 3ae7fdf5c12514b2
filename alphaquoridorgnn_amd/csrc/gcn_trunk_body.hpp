// gcn_trunk_body.hpp -- the device code of the default 9x9 trunk (trunk_variant 3): its LDS image, the fp16-split linear map, the
// banded aggregation, the per-board input build, and trunk_boards_body, the board loop of one 8-wave workgroup.  Two kernels run the
// body: gcn_trunk_boards_mm_kernel (gcn_trunk_split.hip; every forward path) and the engine's evaluation launch, which puts the
// leaves' legal-move searches in front of the board workgroups (engine_eval_kernel, mcts_eval.hip).  __forceinline__ device code only.
#pragma once
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "gcn_packed.hpp"
#include "gcn_heads_split.hpp"
#include <cmath>

namespace aqg {

// =============================================================================================
// all-MFMA trunk (default): linear maps AND neighbourhood aggregation on the 16-bit matrix pipe, fp32-equivalent.
//   GCNConv:  H' = relu( D^-1/2 (A + I) D^-1/2 (H W) + b )          (pv_network_gnn.py:55-57 + PyG gcn_norm)
// Split precision: every f32 operand x is held as two fp16 numbers, hi = RNE16(x), lo = RNE16(x - hi) (11 + 11
// mantissa bits), and a product is rebuilt as hi*hi + hi*lo + lo*hi, accumulated in f32 by
// v_mfma_f32_16x16x32_f16 (16x the f32-input MFMA rate).  The dropped lo*lo term is ~2^-22 |ab|: logits land within
// 1e-7 of the exact-f32 kernel, i.e. at the distance the exact-f32 kernel itself has from the fp64 oracle.
// Activations are O(1) after ReLU / normalised aggregation and |W| < 1: far inside fp16 range.
// 1. Z = H W per wave column stripe: A fragments = fp16 hi/lo planes of H in LDS ([plane][node][feature], read with
//    ds_read_b128), B fragments = host-split W in registers, 3 terms per 16x16x32 block.
// 2. Z' = dinv (.) Z in f32, split into fp16 hi/lo IN REGISTERS.  The accumulator layout of a 16x16 tile (lane =
//    column c, 4 consecutive rows per lane) is also a legal A-operand layout (lane = row of A, 8 consecutive k per
//    lane) for the TRANSPOSED product  Y^T = Z'^T (A + I): the k index (= node) is simply enumerated in the order
//    the accumulators hold it, k-slot (q, e) <-> node 32 kb + 16 (e >> 2) + 4 q + (e & 3), and the adjacency B
//    fragments are built in that same order.  (A + I) is 0/1 -- exact in fp16 -- so the product needs two terms
//    (hi, lo), and it is banded (|k - n| in {0, 1, 9}): 10 of the 18 (k-block, node-tile) blocks are non-zero.
// 3. The transposed result has lane = node, 4 consecutive features per lane: exactly the 8-byte packed store of
//    the plane image (or, for the last layer, the per-lane partial of the mean pool).  No parking of f32 tiles in
//    LDS, no VALU gather, no separate layer-1 gather: layer 1 is  X0 W1  (one MFMA per tile: the six features and
//    the hi/lo split of W1 share one 32-deep k block, X0 is exact in fp16) followed by the same aggregation.
// Per wave and board: 6 + 2 x 72 MFMAs for layer 1 and the linear maps + 2 x 20 for the aggregations.
// =============================================================================================
// One 8-wave workgroup walks boards (persistent grid, two workgroups per CU); a wave owns one 16-column feature tile for all 81 nodes.
// Per board: record decode + bias offsets, the layer-1 input rows G' (built at the top), layer 1, the adjacency fragments (built behind
// layer 1), linear map / aggregation of layers 2 and 3, mean pool -- four workgroup barriers.  (Forms measured slower and removed in
// round 4 -- a 4-wave form, a one-workgroup-per-CU pair form, per-board VALU heads, next-board prefetch under layer 3 -- and the
// timing-only ablation switches that priced this kernel's parts are in the history: git show 8ccbea1:alphaquoridorgnn_amd/csrc/gcn_forward.hip,
// results in profiles/r03_trunk_ablation.log / r03_trunk_ab_runs.log.)
constexpr int NWV = 8;                                 // waves per trunk workgroup
#define AQG_BOARD_BARRIER() __syncthreads()
struct alignas(16) TrunkSmemM {
    alignas(16) unsigned char P[2][PPLANE];            // fp16 hi / lo planes of the activation image [node][feature] (scale CQ / D^-1/2)
    alignas(16) unsigned int AF[AF_BLOCKS][64][4];     // B fragments of (A + I) diag(CQ / deg) of the board (fp16, exact)
    // layer-1 input, aggregated FIRST: G'[n][f] = sum over the closed neighbourhood k of n of X0[k][f] / sqrt(deg k), as fp16
    // hi[0..7] | lo[8..15] per node (6 features used, slots 6, 7 stay zero)
    alignas(16) unsigned short G16[81][16];
    alignas(16) float Y[NWV][96];                      // per-wave scratch of the setup: X0[k][f] / sqrt(deg k) of the wave's feature
    alignas(16) unsigned short degv[NWV][2][32];       // per wave and block slot: fp16 CQ / deg of the 32 nodes of a k block
    alignas(16) float dinvtab[8];                      // 1 / (81 CQ sqrt(deg)), deg = 1..5: the mean pool's weights, read by (deg - 1) * 4 (set once per workgroup)
    alignas(16) float dinv1[NWV][8];                   // 1 / sqrt(deg): the layer-1 input rows' weights, one copy per wave (written and
                                                       // read by the same wave: no barrier between kernel start and the first board's setup)
    // the aggregation's bias rows, PackedLayout::TB regrouped per wave (set once per workgroup): a wave only ever reads its own 64 bytes
    // of a row, so its five degrees' rows lie 64 bytes apart -- 320 bytes span 80 banks: degree 5 meets degree 1, every other pair of
    // rows sits on banks of its own, and lanes of one (deg, q) read one address.  At most two-way conflicts for any mix of degrees
    // (TB's own stride of 512 bytes would put all five rows on the same banks).
    alignas(16) float BR[3][NWV][5][16];
};
static_assert(2 * sizeof(TrunkSmemM) <= 160 * 1024, "two 8-wave workgroups per CU");

// (row16_sum, the sum over the 16 lanes of a DPP row, is in split_mfma.hpp.)
// The same for four values at once, as sixteen v_add_f32 with a DPP operand: the four chains are interleaved, so each add's DPP
// source was written four instructions earlier (a DPP read needs two wait states behind the VALU write of its source; hipcc
// pads nothing inside an asm statement).  hipcc turns the builtin form into v_mov_b32_dpp + packed adds: 24 instructions.
__device__ __forceinline__ f32x4 row16_sum4(f32x4 v) {
    float a = v[0], b = v[1], c = v[2], d = v[3];
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %3, %3, %3 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %3, %3, %3 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %3, %3, %3 row_ror:1 row_mask:0xf bank_mask:0xf"
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    return (f32x4){a, b, c, d};
}

// (The packed buffer's fragment loads -- packed_rsrc, load_frag16 -- and the fp16-range guard's report_saturation are in
//  gcn_heads_split.hpp: the heads use them too, and the MCTS step kernel runs the heads.)

// relu on the BIT PATTERN: max(int(x), 0) -- negative floats (sign bit set) are negative integers, non-negative floats order
// like their bit patterns -- optionally saturating at the largest finite fp16 (0x477FE000 = 65504.0f).  One v_max_i32 /
// v_med3_i32, and unlike fmaxf() on an MFMA result no canonicalising v_max on top; unlike an asm v_max_f32 the compiler SEES
// it, so the matrix pipe's write-back latency in front of this first reader is padded by the compiler, wherever it schedules it.
__device__ __forceinline__ float relu_sat16(float x) {
    const int i = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, min(max(i, 0), 0x477FE000));
}
__device__ __forceinline__ float relu_f(float x) { return __builtin_bit_cast(float, max(__builtin_bit_cast(int, x), 0)); }
// (The opposite direction -- an MFMA result first read INSIDE an asm statement -- has the same blind spot: the first version of
// this kernel did its relu in asm and was wrong by different amounts in each of its three forms, depending on what the scheduler
// happened to put between the last MFMA and the asm.  Every first reader of an accumulator is compiler-visible code now.)

// fp16 planes of four consecutive features of one node: hi (11 bits) + lo (next 11 bits) = 22 mantissa bits
__device__ __forceinline__ void store_split4(TrunkSmemM& sm, int off, const f32x4 v) {
    const unsigned int h01 = cvt_pk_f16(v[0], v[1]), h23 = cvt_pk_f16(v[2], v[3]);
    *reinterpret_cast<u32x2*>(&sm.P[0][off]) = (u32x2){h01, h23};
    *reinterpret_cast<u32x2*>(&sm.P[1][off]) = (u32x2){lo_pair(h01, v[0], v[1]), lo_pair(h23, v[2], v[3])};
}

__device__ __forceinline__ void load_bfrag_mm(u32x4 (&Bf)[2][4], __amdgpu_buffer_rsrc_t rs, size_t region, int wave, int lane) {
    const int base = (int)(region * sizeof(float)) + wave * (4 * 64 * 16);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) Bf[pl][kb] = load_frag16(rs, lane * 16, base + (pl * (8 * 4 * 64) + kb * 64) * 16);
}

// fp16 hi / lo aggregation fragments of one finished 16-node tile m of U (accumulator layout: lane = feature column, 4
// consecutive nodes): dwords 2 (m & 1), 2 (m & 1) + 1 of k block m >> 1.  `piece` 0 = the two hi dwords, 1 / 2 = one lo dword each,
// so that the three pieces can be spread over the MFMA groups of the NEXT tile.
// largest |x| of two values that are being split: ONE v_max3_f32 with |.| modifiers, as an asm statement ordered behind the
// compiler-visible v_cvt_pk of the same two values by `dep` (hipcc pads nothing for asm: it must not be the first reader of a
// matrix-pipe result -- the way lo_pair() is ordered)
__device__ __forceinline__ void absmax_after(float& m, unsigned int dep, float a, float b) {
    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(a), "v"(b), "v"(dep));
}
// the signed form for values that are about to be ReLU-ed (a negative excursion becomes a zero: nothing to report), ordered behind the
// two compiler-visible instructions that have read a and b (their results d0, d1)
__device__ __forceinline__ void max_after2(float& m, float d0, float d1, float a, float b) {
    asm("v_max3_f32 %0, %1, %2, %0" : "+v"(m) : "v"(a), "v"(b), "v"(d0), "v"(d1));
}
__device__ __forceinline__ void split_tile_piece(const f32x4 z, int m, int piece, u32x4 (&zh)[3], u32x4 (&zl)[3], float* zmax = nullptr) {
    const int kb = m >> 1, d = 2 * (m & 1);
    if (piece == 0) {
        zh[kb][d] = cvt_pk_f16(z[0], z[1]); zh[kb][d + 1] = cvt_pk_f16(z[2], z[3]);
        if (zmax) { absmax_after(*zmax, zh[kb][d], z[0], z[1]); absmax_after(*zmax, zh[kb][d + 1], z[2], z[3]); }
    }
    else if (piece == 1) zl[kb][d] = lo_pair(zh[kb][d], z[0], z[1]);
    else zl[kb][d + 1] = lo_pair(zh[kb][d + 1], z[2], z[3]);
}

// U = Q W~ for this wave's columns: six 16-row tiles (tile 5 = row 80 repeated) x four 32-deep k blocks, A fragments
// double-buffered from the planes, three fp16 terms per block (smallest first).  The fp16 split of tile m - 1 (six vector
// instructions per feature tile) is issued between the MFMA groups of tile m: it costs no time of its own.
__device__ __forceinline__ void linear_split(const TrunkSmemM& sm, const u32x4 (&Bf)[2][4], int lane, u32x4 (&zh)[3], u32x4 (&zl)[3],
                                             float* zmax = nullptr) {
    const int c = lane & 15, q = lane >> 4;
    // the fragments of step s + 1 are requested while step s multiplies (two register pairs).  One step ahead is enough with four
    // waves per SIMD: rings 2 / 3 steps deep measured 48.0 / 45.4 M boards/s against 48.4 at 4,096 boards (round 3).
    u32x4 ring[2][2];
    auto frag_off = [&](int step) -> int {                  // step = m*4 + kb
        const int m = step >> 2, kb = step & 3;
        const int row = (m < 5) ? 16 * m + c : 80;
        return plane_off(row, 4 * kb + q);
    };
    auto request = [&](int step) {
        const int o = frag_off(step);
        ring[step & 1][0] = *reinterpret_cast<const u32x4*>(&sm.P[0][o]);
        ring[step & 1][1] = *reinterpret_cast<const u32x4*>(&sm.P[1][o]);
    };
    request(0);
    f32x4 acc, done;
#pragma unroll
    for (int step = 0; step < 24; ++step) {
        const int m = step >> 2, kb = step & 3;
        if (step + 1 < 24) request(step + 1);
        __builtin_amdgcn_sched_barrier(0);
        const u32x4 hi = ring[step & 1][0], lo = ring[step & 1][1];
        f32x4 a = kb == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc;
        a = mfma_f16(lo, Bf[0][kb], a);
        a = mfma_f16(hi, Bf[1][kb], a);
        a = mfma_f16(hi, Bf[0][kb], a);
        acc = a;
        if (m > 0 && kb < 3) split_tile_piece(done, m - 1, kb, zh, zl, zmax);
        __builtin_amdgcn_sched_barrier(0);
        if (kb == 3) done = acc;
    }
#pragma unroll
    for (int piece = 0; piece < 3; ++piece) split_tile_piece(done, 5, piece, zh, zl, zmax);
}

// The aggregation accumulators start from the bias: out[nt] = TB[layer][deg(node) - 1][this lane's 4 features] = CQ b sqrt(deg),
// so that relu(out) IS the next plane image -- no multiply, no add on the vector unit.  `toff` packs (deg - 1) * 512 + 16 q per
// node tile of this lane, 16 bits each.  The rows come from the workgroup's LDS image (TrunkSmemM::BR, rows 64 bytes apart: the row
// offset moves from bit 9 to bit 6, for both tiles of a register at once), one ds_read_b128 per node tile: requested right in front
// of the MFMAs that accumulate on them -- an LDS latency ahead, not a phase ahead, so `out` is not live across a linear map.
__device__ __forceinline__ void request_bias(f32x4 (&out)[6], const TrunkSmemM& sm, int layer, const int (&toff)[3], int wave) {
    const unsigned char* rows = reinterpret_cast<const unsigned char*>(&sm.BR[layer][wave][0][0]);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const uint32_t t = (uint32_t)toff[p];
        const uint32_t r = ((t >> 3) & 0x01C001C0u) | (t & 0x00300030u);          // (deg - 1) * 64 + 16 q, twice
        out[2 * p] = *reinterpret_cast<const f32x4*>(rows + (r & 0xFFFFu));
        out[2 * p + 1] = *reinterpret_cast<const f32x4*>(rows + (r >> 16));
    }
}

// Aggregation + epilogue, node tile by node tile:  V^T = U^T (A + I) diag(CQ / deg) on top of the bias rows, then
// Q = relu(V) -> split planes (lane = node, 4 consecutive features), or the mean pool of D^-1/2 Q / CQ for the last layer.
// The blocks of a node tile are consecutive (a dependent 16x16x32 chain issues at the full rate), so tile nt is complete while
// tile nt + 1 is still on the matrix pipe: its relu / split / stores are vector and LDS work issued under those MFMAs.
// (No plane byte is read here: the caller has passed the barrier behind the linear map, the stores are free to go.)
// No range check here: the caller has bounded layer 2's aggregate by its linear map's output (or the weight set's range is proven),
// layer 3's aggregate is never split (the heads check the pooled row).
template <bool LAST>
__device__ __forceinline__ void aggregate_store(TrunkSmemM& sm, const unsigned int (&AF)[AF_BLOCKS][64][4], u32x4 (&zh)[3], u32x4 (&zl)[3], f32x4 (&out)[6], int wave, int lane,
                                                const int (&toff)[3], __amdgpu_buffer_rsrc_t pooled_rs, int pooled_soff) {
    constexpr int AHEAD = 3;                                   // adjacency fragments in flight (4 registers each)
    const int c = lane & 15, q = lane >> 4;
    const int col0 = 16 * wave + 4 * q;
    u32x4 af[AF_BLOCKS];
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) af[i] = *reinterpret_cast<const u32x4*>(&AF[i][lane][0]);
    split_fence(zl[0], zl[1], zl[2]);
    f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto epilogue = [&](int nt) {
        const int node = 16 * nt + c;
        const bool live = (nt < 5) || (c == 0);                              // node < 81
        float dn = 0.f;
        // deg - 1 sits above the row offset's 9 bits (and the 16 q below them leave bits 7, 8 clear): bits 7..11 = (deg - 1) * 4, the byte
        // offset into the 1 / sqrt(deg) table -- one v_bfe + one ds_read where the select chain took nine instructions per node tile
        if (LAST) dn = *reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(sm.dinvtab) + (((unsigned)toff[nt >> 1] >> (7 + 16 * (nt & 1))) & 0x1Cu));
        f32x4 v = out[nt];
        if (LAST) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = relu_f(v[e]);
            if (live) sum += v * dn;
        } else {
            // relu, saturating at the largest finite fp16: an overflowing activation stays a (wrong) finite number instead of
            // becoming inf - inf = NaN that the next relu would silently turn into 0 (it has been REPORTED by the caller's bound on
            // the linear map's output: the host then serves the weight set with the exact-f32 kernels)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = relu_sat16(v[e]);
            if (live) store_split4(sm, plane_off(node, col0 >> 3) + ((2 * col0) & 15), v);
        }
    };
    // blocks are numbered in node-tile order already: kb = {0,0,1,0,1,1,2,1,2,2}, nt = {0,1,1,2,2,3,3,4,4,5}
#pragma unroll
    for (int blk = 0; blk < AF_BLOCKS; ++blk) {
        const int kb = af_kb(blk), nt = af_nt(blk);
        if (blk + AHEAD < AF_BLOCKS) af[blk + AHEAD] = *reinterpret_cast<const u32x4*>(&AF[blk + AHEAD][lane][0]);
        out[nt] = mfma_f16(zl[kb], af[blk], out[nt]);
        out[nt] = mfma_f16(zh[kb], af[blk], out[nt]);
        // tile nt - 1 was finished by the previous block(s): its epilogue goes out under this tile's MFMAs
        if (nt > 0 && (blk + 1 == AF_BLOCKS || af_nt(blk + 1) != nt)) epilogue(nt - 1);
    }
    epilogue(5);
    if (LAST) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int col0 = 16 * wave + 4 * (ln >> 4);
        const f32x4 t = row16_sum4(sum);                                  // (the table's entries carry the 1 / (81 CQ) of the mean)
        // (buffer store off an SGPR descriptor + scalar row offset: no 64-bit address registers alive across the board loop)
        if (c == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t), pooled_rs, col0 * 4, pooled_soff, 0);
    }
}

// Bit `lane` of a wave-uniform 64-bit mask, as 0 / 1 or as 0 / a: ONE v_cndmask with the scalar pair as its lane condition
// (what `(m >> lane) & 1` means, minus the 64-bit vector shift).  The masks are SALU results: no VALU-SGPR hazard to pad.
// (readfirstlane: the register allocator must see a scalar pair even where it chose vector registers for a uniform value; it
// folds away when the value already is one.)
__device__ __forceinline__ uint64_t uniform64(uint64_t m) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32);
}
__device__ __forceinline__ uint32_t lane_bit(uint64_t m) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(uniform64(m)));
    return r;
}
template <int IMM> __device__ __forceinline__ uint32_t lane_val(uint64_t m) {     // bit `lane` of m ? IMM : 0  (IMM an inline constant)
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, %2, %1" : "=v"(r) : "s"(uniform64(m)), "n"(IMM));
    return r;
}
__device__ __forceinline__ float lane_sel(uint64_t m, float a) {
    float r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(a), "s"(uniform64(m)));
    return r;
}

// Layer 1, aggregate-first:  Q1^T = relu( (c W1) G'^T + c sqrt(deg) b )  -- ONE MFMA per node tile and feature tile.  A = the wave's
// W1 fragment (rows = its 16 output features; k = the six input features three times: hi.hi, hi.lo, lo.hi), B = the node tile's
// rows of G' (lane = node; k-slots of q = 0 / 2 read the hi half, q = 1 the lo half, q = 3 meets zero weight slots), accumulated on
// the bias rows.  The result already has the store layout (lane = node, 4 consecutive features): relu, fp16 split, plane stores.
// 6 MFMAs per wave and feature tile where the linear-first form needed 6 + 20 (X0 W1, then the 128-wide banded aggregation).
template <int TRACK>
__device__ __forceinline__ void layer1_store(TrunkSmemM& sm, const unsigned short (&G)[81][16], const u32x4 &w1f, f32x4 (&out)[6],
                                             int wave, int lane, int32_t* __restrict__ saturated) {
    const int c = lane & 15, q = lane >> 4;
    float fmx = 0.f;
    const int col0 = 16 * wave + 4 * q;
    u32x4 gf[6];
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) gf[nt] = *reinterpret_cast<const u32x4*>(&G[nt < 5 ? 16 * nt + c : 80][8 * (q & 1)]);
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) out[nt] = mfma_f16(w1f, gf[nt], out[nt]);
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) {
        const int node = 16 * nt + c;
        const bool live = (nt < 5) || (c == 0);                              // node < 81
        f32x4 v = out[nt];
        // mode 2: the pre-clamp values are finite here (finite weights times bounded layer-1 rows: no inf, no NaN) and only a
        // POSITIVE excursion is clamped, so the largest value is all there is to watch -- a plain float maximum, two values per
        // instruction (the first reader of these matrix-pipe results is the compiler-visible v_med3 below: the maxima sit behind it)
        f32x4 w = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = relu_sat16(v[e]);
        if (TRACK == 2 && live) { max_after2(fmx, v[0], v[1], w[0], w[1]); max_after2(fmx, v[2], v[3], w[2], w[3]); }
        if (live) store_split4(sm, plane_off(node, col0 >> 3) + ((2 * col0) & 15), v);
    }
    if (TRACK == 2) report_saturation(!(fmx <= 65504.0f), saturated);
}

__device__ __forceinline__ uint32_t bit_of64(uint64_t m, int s) {             // bit s of a wave-uniform 64-bit mask
    const uint32_t w = (s & 32) ? (uint32_t)(m >> 32) : (uint32_t)m;
    return (w >> (s & 31)) & 1u;
}

// The lane index, re-derived from the execution mask (two v_mbcnt) wherever it is needed instead of being kept in a register across
// the board loop (at the 128-register cap the allocator spilled it and reloaded it behind an s_waitcnt vmcnt(0)).
__device__ __forceinline__ int fresh_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// ---- per-board inputs.  decode: the record becomes wave-uniform scalars (the wall masks by ballot over the 64 wall bytes).
__device__ __forceinline__ void trunk_decode(int fmt, uint32_t r0, uint32_t r1, uint64_t& hw, uint64_t& vw, uint32_t& hd) {
    if (fmt == 0) {
        hw = __ballot((r0 & 1u) != 0);                               // wall byte: bit0 H, bit1 V
        vw = __ballot((r0 & 2u) != 0);
        hd = __builtin_amdgcn_readfirstlane(r1);
    } else {
        // (readlane returns a SIGNED int: without the uint32_t cast a wall in slot 31 sign-extends into slots 32..63 --
        //  a round-1 bug that only the in-engine evaluation path could hit; tests/test_gpu_parity.py pins it now)
        hw = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(r0, 0) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(r0, 1) << 32);
        vw = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(r0, 2) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(r0, 3) << 32);
        hd = (uint32_t)__builtin_amdgcn_readlane(r0, 4);
    }
}
// deg - 1 = U + D + L + R of every node as three bit planes (bit-sliced adder on the scalar unit; c1 excludes c3, so
// c1 + c2 + c3 <= 2 and b2 = c1 & c2), lo = nodes 0..63, hi = nodes 64..80
struct Planes { uint64_t b0l, b1l, b2l, b0h, b1h, b2h; };
__device__ __forceinline__ Planes degree_planes(const Open& op) {
    Planes p;
    {
        const uint64_t x = op.U.lo ^ op.D.lo, c1 = op.U.lo & op.D.lo, y = op.L.lo ^ op.R.lo, c2 = op.L.lo & op.R.lo, c3 = x & y;
        p.b0l = x ^ y; p.b1l = c1 ^ c2 ^ c3; p.b2l = c1 & c2;
    }
    {
        const uint64_t x = op.U.hi ^ op.D.hi, c1 = op.U.hi & op.D.hi, y = op.L.hi ^ op.R.hi, c2 = op.L.hi & op.R.hi, c3 = x & y;
        p.b0h = x ^ y; p.b1h = c1 ^ c2 ^ c3; p.b2h = c1 & c2;
    }
    return p;
}
// build_inputs: everything a board's layers read from LDS besides the planes --
//  (1) layer-1 input, aggregated first (GCNConv is linear before its ReLU: A_hat (X W) = (A_hat X) W, and X has 6 columns where
//      X W has 128):  G'[n][f] = sum_{k in N[n]} X0[k][f] / sqrt(deg k)  (the 1 / sqrt(deg n) half of the symmetric norm cancels
//      against the sqrt(deg) scale of the plane image).  Wave f < 6 owns feature f for all 81 nodes (lane = node `lane`, lanes
//      < 17 also node 64 + lane): the feature is a wave-uniform bitboard times a scalar (pv_network_cnn.py:88-114: pawn tile,
//      walls in hand, enemy pawn tile in the enemy's frame, its walls, horizontal / vertical wall at the tile's slot), so x = one
//      v_cndmask; x / sqrt(deg) goes through 384 bytes of the wave's own LDS scratch to reach the four neighbours (no other
//      wave is involved: no barrier), the sum is split into fp16 hi / lo and stored as the B operand rows of layer 1;
//  (2) the banded adjacency fragments of layers 2 and 3.
// `what` & 1: the G' rows (top of a board), & 2: the adjacency fragments (behind layer 1).
__device__ __forceinline__ void trunk_build_inputs(unsigned short (&G16)[81][16], unsigned int (&AF)[AF_BLOCKS][64][4], float* __restrict__ Yw,
                                               unsigned short (&degv)[2][32], const float (&dtab)[8], int wave, uint64_t hw, uint64_t vw, uint32_t hd, int what) {
    constexpr int N = 9, V = 81, NSLOT = 2;
    const Open op = make_open<N>(hw, vw);
    const Planes pl = degree_planes(op);
    if (what & 1) {
        const int ppos = hd & 0xff, pwl = (hd >> 8) & 0xff, epos = (hd >> 16) & 0xff, ewl = hd >> 24;
        const BB shb = spread_slots<N>(hw), svb = spread_slots<N>(vw);
        const int f = __builtin_amdgcn_readfirstlane(wave);        // wave-uniform, and known to be: the masks below stay scalar
        if (f < 6) {
            BB m = mask_all<N>();
            float sc = 1.f;
            if (f == 0) m = bb_bit(ppos);
            else if (f == 1) sc = (float)pwl;
            else if (f == 2) m = bb_bit(epos);
            else if (f == 3) sc = (float)ewl;
            else if (f == 4) m = shb;
            else m = svb;
            const int ln = fresh_lane(), l1 = min(ln, 16);
            // 1 / sqrt(deg) of this lane's two nodes from the table: byte offset (deg - 1) * 4 assembled from the three degree bit planes
            const float dnv0 = *reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(dtab) + (lane_val<4>(pl.b0l) | lane_val<8>(pl.b1l) | lane_val<16>(pl.b2l)));
            const float dnv1 = *reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(dtab) + (lane_val<4>(pl.b0h) | lane_val<8>(pl.b1h) | lane_val<16>(pl.b2h)));
            const float y0 = lane_sel(m.lo, sc) * dnv0, y1 = lane_sel(m.hi, sc) * dnv1;
                            Yw[ln] = y0;
            if (ln < 17) Yw[64 + ln] = y1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // (an edge that is open leads to a node of the board: clamped addresses are only ever read by lanes that discard them)
            const float nu0 = Yw[max(ln - 9, 0)], nd0 = Yw[ln + 9], nl0 = Yw[max(ln - 1, 0)], nr0 = Yw[ln + 1];
            const float nu1 = Yw[55 + l1], nd1 = Yw[73 + l1], nl1 = Yw[63 + l1], nr1 = Yw[65 + l1];
            const float g0 = (((y0 + lane_sel(op.U.lo, nu0)) + lane_sel(op.D.lo, nd0)) + lane_sel(op.L.lo, nl0)) + lane_sel(op.R.lo, nr0);
            const float g1 = (((y1 + lane_sel(op.U.hi, nu1)) + lane_sel(op.D.hi, nd1)) + lane_sel(op.L.hi, nl1)) + lane_sel(op.R.hi, nr1);
            const _Float16 h0 = (_Float16)g0, h1 = (_Float16)g1;
            const _Float16 e0 = (_Float16)(g0 - (float)h0), e1 = (_Float16)(g1 - (float)h1);
            G16[ln][f] = __builtin_bit_cast(unsigned short, h0);
            G16[ln][8 + f] = __builtin_bit_cast(unsigned short, e0);
            if (ln < 17) {
                G16[64 + ln][f] = __builtin_bit_cast(unsigned short, h1);
                G16[64 + ln][8 + f] = __builtin_bit_cast(unsigned short, e1);
            }
        }
    }
    if (what & 2) {
        const int lane = fresh_lane();
        // the four open-edge boards as 3 x 32-bit words each (word w = nodes 32 w .. 32 w + 31), selected arithmetically
        // (scalars, not an array: an indexed local array would live in scratch memory)
        const uint32_t u0 = (uint32_t)op.U.lo, u1 = (uint32_t)(op.U.lo >> 32), u2 = (uint32_t)op.U.hi;
        const uint32_t d0w = (uint32_t)op.D.lo, d1w = (uint32_t)(op.D.lo >> 32), d2w = (uint32_t)op.D.hi;
        const uint32_t l0 = (uint32_t)op.L.lo, l1 = (uint32_t)(op.L.lo >> 32), l2 = (uint32_t)op.L.hi;
        const uint32_t r0w = (uint32_t)op.R.lo, r1w = (uint32_t)(op.R.lo >> 32), r2w = (uint32_t)op.R.hi;
        auto sel3 = [](uint32_t a0, uint32_t a1, uint32_t a2, int w) -> uint32_t { const uint32_t a = w == 0 ? a0 : a1; return w == 2 ? a2 : a; };
        auto open_word = [&](int dir, int w) -> uint32_t {
            return dir == 0 ? sel3(u0, u1, u2, w) : dir == 1 ? sel3(d0w, d1w, d2w, w) : dir == 2 ? sel3(l0, l1, l2, w) : sel3(r0w, r1w, r2w, w);
        };
        // ten adjacency blocks over the eight waves:   w0 {8}  w1 {9}  w2 {0,6}  w3 {1,7}  w4..7 {2..5}
        auto slot_block = [&](int it) -> int {                           // wave-uniform
            return it == 0 ? (wave >= 2 ? wave - 2 : wave + 8) : ((wave == 2 || wave == 3) ? wave + 4 : AF_BLOCKS);
        };
        // step 1: the fp16 values CQ / deg(k) of the 32 source nodes of each block's k range, through this wave's own LDS
        //         scratch (lane l < 32 = node 32 kb + l; the word of the open-edge boards is wave-uniform)
#pragma unroll
        for (int it = 0; it < NSLOT; ++it) {
            const int blk = slot_block(it);
            if (blk < AF_BLOCKS && lane < 32) {
                const int kb = (AF_KB_PACK >> (2 * blk)) & 3;
                const int l = lane;
                const uint32_t deg = 1u + ((open_word(0, kb) >> l) & 1u) + ((open_word(1, kb) >> l) & 1u) +
                                     ((open_word(2, kb) >> l) & 1u) + ((open_word(3, kb) >> l) & 1u);
                // fp16 of CQ / deg = 0.9375, 0.46875, 0.3125, 0.234375, 0.1875 (all exact)
                const uint32_t val = deg == 1u ? 0x3B80u : deg == 2u ? 0x3780u : deg == 3u ? 0x3500u : deg == 4u ? 0x3380u : 0x3200u;
                degv[it][l] = (unsigned short)((32 * kb + l < V) ? val : 0u);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // step 2: the fragments.  k-slot e of lane (c, q) is node 32 kb + 16 (e >> 2) + 4 q + (e & 3); entry = CQ / deg(k) where
        //         node n = 16 nt + c has k in its closed neighbourhood, else 0
#pragma unroll
        for (int it = 0; it < NSLOT; ++it) {
            const int blk = slot_block(it);
            if (blk < AF_BLOCKS) {
                const int kb = (AF_KB_PACK >> (2 * blk)) & 3, nt = (AF_NT_PACK >> (3 * blk)) & 7;
                const int ln = lane;
                const int n = 16 * nt + (ln & 15), q = ln >> 4;
                u32x4 fr = (u32x4){0u, 0u, 0u, 0u};
                if (n < V) {
                    const int w = nt >> 1, sft = n & 31;                 // n >> 5 == nt >> 1: the word is wave-uniform
                    // window of row n of (A + I) around the diagonal: bit (k - n + 9), k = n-9 (U), n-1 (L), n, n+1 (R), n+9 (D)
                    // (kept four bits up: the four slots of a half then are bits s .. s + 3 of it for s = window position + 4, and a
                    //  position left of the window (s < 0) or right of it (s > 31) reads zeros once s is clamped to 0..31 -- the low four
                    //  bits and everything above bit 22 are clear)
                    const uint32_t win4 = (1u << 13) | (((open_word(0, w) >> sft) & 1u) << 4) | (((open_word(2, w) >> sft) & 1u) << 12) |
                                          (((open_word(3, w) >> sft) & 1u) << 14) | (((open_word(1, w) >> sft) & 1u) << 22);
                    const int d0 = 32 * kb + 4 * q - n + 9 + 4;          // window bit of k-slot e = 0 (+ 4); e = 4 sits 16 higher
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const u32x2 dv = *reinterpret_cast<const u32x2*>(&degv[it][16 * h + 4 * q]);   // nodes 32 kb + 16 h + 4 q + 0..3
                        const uint32_t nib = (win4 >> (uint32_t)min(max(d0 + 16 * h, 0), 31)) & 0xFu;
                        const uint32_t t2 = nib | (nib << 15);           // b0 -> bit 0, b1 -> bit 16, b2 -> bit 2, b3 -> bit 18
                        // a packed 16-bit multiply by the 0 / 1 of each half keeps or clears the half (v_pk_mul_lo_u16)
                        // (scalars first: __builtin_bit_cast of a vector ELEMENT reads element 0 whatever the index -- hipcc 7.2, see the range-guard comment)
                        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
                        const uint32_t dv0 = dv[0], dv1 = dv[1], s0 = t2 & 0x00010001u, s1 = (t2 >> 2) & 0x00010001u;
                        fr[2 * h] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, s0) * __builtin_bit_cast(u16x2, dv0));
                        fr[2 * h + 1] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, s1) * __builtin_bit_cast(u16x2, dv1));
                    }
                }
                *reinterpret_cast<u32x4*>(&AF[blk][ln][0]) = fr;
            }
        }
    }
}


// Byte offset of a lane's rows in a bias table, (deg - 1) * 512 + 16 q, for its node 16 nt + c of every node tile (first row for
// the padding nodes 81..95: their plane bits are zero), two node tiles per register; deg - 1 stays readable above bit 9 (the mean
// pool's 1 / sqrt(deg)).  Straight from the record's degree bit planes: nothing here waits for a barrier.
__device__ __forceinline__ void trunk_bias_offsets(uint64_t hw, uint64_t vw, int c, int q, int (&toff)[3]) {
    const Planes pl = degree_planes(make_open<9>(hw, vw));
    const uint32_t qq = (uint32_t)(16 * q) * 0x00010001u;
    // two node tiles per 32-bit plane word (nodes 32 p + c and 32 p + 16 + c are bits c and 16 + c): one shift + one mask per plane
    // serves both tiles of a register
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const uint32_t w0 = p < 2 ? (uint32_t)(pl.b0l >> (32 * p)) : (uint32_t)pl.b0h;
        const uint32_t w1 = p < 2 ? (uint32_t)(pl.b1l >> (32 * p)) : (uint32_t)pl.b1h;
        const uint32_t w2 = p < 2 ? (uint32_t)(pl.b2l >> (32 * p)) : (uint32_t)pl.b2h;
        const uint32_t x0 = (w0 >> c) & 0x00010001u, x1 = (w1 >> c) & 0x00010001u, x2 = (w2 >> c) & 0x00010001u;
        const uint32_t dm2 = x0 | (x1 << 1) | (x2 << 2);                 // deg - 1 of the even tile in bits 0..2, of the odd tile in bits 16..18
        toff[p] = (int)((dm2 << 9) + qq);                                // (deg - 1) * HID * 4 + 16 q, twice
    }
}

// (hipcc's second launch-bound argument is waves per SIMD: workgroups per CU x waves per workgroup / 4 SIMDs)
// TRACK (the range guard's mode): 0 = the caller has PROVEN that no value of this weight set can leave fp16 range on any record with at
// most AQG_GNN_PROVEN_MAX_WALLS walls in hand (AQG_GNN_RANGE_PROVEN, include/aqgnn.h): nothing is tracked, each record's two wall counts
// are checked instead, on the scalar unit.  2 (every other weight set) = the values are bounded where that is cheapest: layer 1's
// pre-clamp outputs by a float maximum; the linear maps' outputs U (which are split themselves) by a float maximum of |U| against the
// thresholds of PackedLayout::GUARD -- layer 2's aggregate is then below 65504 by  |V| <= 2.0625 max|U| + max|TB|,  layer 3's is not
// split at all (the heads check the pooled row): one vector instruction per TWO values at three places.
// LIST: the boards come as a compact list (below); the mask-walking instantiation carries none of that code
// blk / nblk: this workgroup's index among the launch's board workgroups and their number (blockIdx.x / gridDim.x of the plain kernel;
// the engine's evaluation launch counts from behind its legal-move workgroups): first board, stride, start offset and priorities
// all follow from them.  BESIDE: the body shares its kernel with the legal-move workgroups (see the board loop's top).
template <int TRACK, bool LIST, bool BESIDE = false>
__device__ __forceinline__ void trunk_boards_body(TrunkSmemM& sm, const unsigned int blk, const unsigned int nblk, const void* __restrict__ states, int fmt,
                                                  int B, const float* __restrict__ pk, float* __restrict__ pooled, const uint8_t* __restrict__ active,
                                                  int phase_delay, int32_t* __restrict__ saturated, const int32_t* __restrict__ list_arg,
                                                  const int32_t* __restrict__ list_count) {
    const int32_t* __restrict__ const list = LIST ? list_arg : nullptr;
    // The two workgroups resident on a CU run identical phase sequences; a start offset for the second-resident ones
    // (phase_delay x 64 cycles) keeps one on the matrix pipe while the other does vector work.
    const int prio_mode = phase_delay >> 16;     // static wave priorities (aqg_set_option("trunk_prio"); chosen by launch size on the host)
    phase_delay &= 0xFFFF;
    for (int i = 0; i < (int)(blk >> 8) * phase_delay; ++i) __builtin_amdgcn_s_sleep(1);   // 2nd / 3rd resident: 1x / 2x
    {
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const bool up = ((prio_mode & 1) && wv >= 4) || ((prio_mode & 2) && blk >= 256) || ((prio_mode & 4) && blk < 256);
        if (up) __builtin_amdgcn_s_setprio(1);
    }
    // trunk_prio bit 3: the two workgroups of a CU take turns at priority 1, phase by phase, instead of the older one winning
    // every arbitration (otherwise the younger one's chain is 25 % longer)
    const int prio_sel0 = (prio_mode & 8) ? (int)((blk >> 8) & 1) : -1;
    int prio_sel = prio_sel0;
    auto phase_prio = [&](int kph) {
        if (prio_sel >= 0) { if ((kph + prio_sel) & 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
    };
    // The thread index is NOT kept in a register across the board loop (at the 128-register cap the allocator spilled it and
    // reloaded it behind an s_waitcnt vmcnt(0) that drained the weight prefetches): the wave index is a scalar, the lane index
    // is re-derived from the execution mask (two v_mbcnt) wherever it is needed.
    const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int wave = wave0;

    // `list` (optional): the launch's boards as a COMPACT list of indices, *list_count long -- workgroup w takes entries w, w + grid, ...
    // The MCTS with its evaluation cache on hands over the ~quarter of a set's leaves that miss the cache this way: walking the
    // mask instead, a workgroup's share of a 4,096-slot set is Binomial(8, 1/4) boards and the launch lasts as long as the
    // unluckiest workgroup (38 us against ~22 for the same boards spread evenly).
    int j = blk;
    const int nlist = list ? __builtin_amdgcn_readfirstlane(*list_count) : 0;
    int b = list ? (j < nlist ? __builtin_amdgcn_readfirstlane(list[j]) : B) : (int)blk;
    // A board's record lives in two VGPRs of EVERY wave (each wave fetches it itself: 24-72 bytes), one board ahead:
    //   fmt 0 (state72): rec0 = wall byte of slot `lane`, rec1 = header dword;  fmt 1 (QState): rec0 = dword `lane` (< 5)
    uint32_t rec0 = 0, rec1 = 0;
    // buffer loads off one SGPR descriptor + a scalar record offset: no 64-bit address registers to keep alive across the loop
    const __amdgpu_buffer_rsrc_t rst = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(states), 0, B * (fmt == 0 ? 72 : 24), 0x00020000);
    auto fetch_record = [&](int bb, uint32_t& r0, uint32_t& r1) {
        const int ln = fresh_lane();          // offsets are recomputed per fetch, not kept (spilled) across the board loop
        if (fmt == 0) {
            r0 = __builtin_amdgcn_raw_buffer_load_b8(rst, 4 + ln, bb * 72, 0);
            r1 = __builtin_amdgcn_raw_buffer_load_b32(rst, 0, bb * 72, 0);
        } else {
            r0 = __builtin_amdgcn_raw_buffer_load_b32(rst, (ln < 5 ? ln : 4) * 4, bb * 24, 0);
        }
    };
    // The first board's record is requested BEFORE its `active` flag is known: the two loads are in flight together instead of
    // one behind the other (one memory latency off every launch -- the MCTS's launches are one board per workgroup, ~94 % active).
    if (b < B) {
        fetch_record(b, rec0, rec1);
        if (!list && active && !active[b]) {          // (workgroup-uniform) inactive slot: walk on to the next active board
            do { b += nblk; } while (b < B && !active[b]);
            if (b < B) fetch_record(b, rec0, rec1);
        }
    }
    const __amdgpu_buffer_rsrc_t rs = packed_rsrc(pk);
    // once per workgroup: the k-slots 6, 7 of the hi and lo halves of every G' row, which no board ever writes, and the bias rows of
    // the three layers (one coalesced pass over the 7,680 bytes of PackedLayout::TB, 16 bytes per thread, into the per-wave grouping
    // of TrunkSmemM::BR).  No barrier here: their first reader sits behind the first board's setup barrier.
    {
        const int t0 = (int)threadIdx.x;
        constexpr int TB_WORDS = 3 * 5 * HID / 4;                        // 16-byte words of the table: [layer][deg - 1][wave][4]
        if (t0 < TB_WORDS) {
            const u32x4 row = load_frag16(rs, t0 * 16, (int)(PackedLayout::TB * sizeof(float)));
            const int layer = t0 / (5 * HID / 4), r = t0 % (5 * HID / 4);
            *reinterpret_cast<u32x4*>(&sm.BR[layer][(r >> 2) & (NWV - 1)][r >> 5][4 * (r & 3)]) = row;
        }
        for (int i = t0; i < 81 * 2; i += 64 * NWV)
            *reinterpret_cast<unsigned int*>(&sm.G16[0][0] + 16 * (i >> 1) + 6 + 8 * (i & 1)) = 0u;
        if (t0 < 8) sm.dinvtab[t0] = dinv_of_dm((uint32_t)t0) * (float)(1.0 / (81.0 * CQ));      // (first read behind the layer-3 barriers)
        if ((t0 & 63) < 8) sm.dinv1[t0 >> 6][t0 & 63] = dinv_of_dm((uint32_t)(t0 & 63));           // each wave its own copy: no barrier here
    }
    u32x4 Bf[2][4];
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pooled, 0, B * (HID * 4), 0x00020000);

    auto build_inputs = [&](uint64_t hw, uint64_t vw, uint32_t hd, int what) {
        trunk_build_inputs(sm.G16, sm.AF, sm.Y[wave], sm.degv[wave], sm.dinv1[wave], wave, hw, vw, hd, what);
    };

    AQG_STAMP_DECL
    while (b < B) {
        AQG_STAMP_AT(7)
        wave = wave0;
        asm volatile("" : "+s"(wave));         // opaque per board: wave-derived predicates are recomputed (2-3 scalar ops), not
                                               // hoisted out of the loop into registers that then spill
        // (the same for the priority mode's predicate in the engine's evaluation kernel, whose search workgroups spill scalars into a vector
        //  register that the whole kernel then lacks: hoisted, the predicate was kept in a VECTOR register and spilled to scratch)
        if (BESIDE) { prio_sel = prio_sel0; asm volatile("" : "+s"(prio_sel)); }
        const int lane = fresh_lane(), c = lane & 15, q = lane >> 4;
        // the small layer-1 weight fragment goes out first
        const u32x4 w1f = load_frag16(rs, lane * 16, (int)(PackedLayout::WH1 * sizeof(float)) + wave * (64 * 16));
        __builtin_amdgcn_sched_barrier(0);
        int toff[3];
        uint64_t hw, vw;
        uint32_t hd;
        trunk_decode(fmt, rec0, rec1, hw, vw, hd);
        trunk_bias_offsets(hw, vw, c, q, toff);
        f32x4 out[6];
        u32x4 zh[3], zl[3];
        AQG_STAMP_AT(6)
        build_inputs(hw, vw, hd, 1);                                     // the layer-1 input rows G'
        int bn;
        if (list) { j += nblk; bn = j < nlist ? __builtin_amdgcn_readfirstlane(list[j]) : B; }
        else { bn = b + nblk; while (bn < B && active && !active[bn]) bn += nblk; }
        AQG_BOARD_BARRIER();                     // this board's G' rows are complete; the previous board is done
        AQG_STAMP_AT(0)
        phase_prio(1);
        // ---- layer 1: one MFMA per node tile on top of the bias rows, relu, planes
        request_bias(out, sm, 0, toff, wave);
        if (TRACK == 0 && (((hd >> 8) & 0xffu) > AQG_GNN_PROVEN_MAX_WALLS || (hd >> 24) > AQG_GNN_PROVEN_MAX_WALLS)) report_saturation(true, saturated);
        layer1_store<TRACK>(sm, sm.G16, w1f, out, wave, lane, saturated);
        AQG_STAMP_AT(8)
        __builtin_amdgcn_sched_barrier(0);
        load_bfrag_mm(Bf, rs, PackedLayout::WH2, wave, lane);             // layer-2 weights: land under the barrier
        __builtin_amdgcn_sched_barrier(0);
        phase_prio(2);
        build_inputs(hw, vw, hd, 2);                                     // the adjacency fragments of layers 2 and 3
        AQG_STAMP_AT(9)
        AQG_BOARD_BARRIER();
        AQG_STAMP_AT(1)
        // ---- layer 2
        phase_prio(3);
        {
            float zmax = 0.f;
            linear_split(sm, Bf, lane, zh, zl, TRACK == 2 ? &zmax : nullptr);
            if (TRACK == 2) report_saturation(!(zmax <= pk[PackedLayout::GUARD + 0]), saturated);
        }
        AQG_STAMP_AT(2)
        AQG_STAMP_AT(11)
        __builtin_amdgcn_sched_barrier(0);
        load_bfrag_mm(Bf, rs, PackedLayout::WH3, wave, lane);             // lands under the barrier + aggregation
        uint32_t nrec0 = 0, nrec1 = 0;
        if (bn < B) fetch_record(bn, nrec0, nrec1);                         // the next board's record rides behind it
        __builtin_amdgcn_sched_barrier(0);
        AQG_STAMP_AT(12)
        AQG_BOARD_BARRIER();                                                    // every wave is done reading the planes
        AQG_STAMP_AT(13)
        phase_prio(4);
        request_bias(out, sm, 1, toff, wave);
        aggregate_store<false>(sm, sm.AF, zh, zl, out, wave, lane, toff, prs, 0);
        AQG_STAMP_AT(14)
        AQG_BOARD_BARRIER();
        AQG_STAMP_AT(3)
        // ---- layer 3 + mean pool
        phase_prio(5);
        AQG_STAMP_AT(10)
        {
            float zmax = 0.f;
            linear_split(sm, Bf, lane, zh, zl, TRACK == 2 ? &zmax : nullptr);
            if (TRACK == 2) report_saturation(!(zmax <= pk[PackedLayout::GUARD + 1]), saturated);
        }
        AQG_STAMP_AT(4)
        AQG_STAMP_AT(15)
        phase_prio(6);
        request_bias(out, sm, 2, toff, wave);
        aggregate_store<true>(sm, sm.AF, zh, zl, out, wave, lane, toff, prs, b * (HID * 4));
        rec0 = nrec0; rec1 = nrec1;
        // (No barrier at the end of a board: what the next board writes in front of its top barrier -- the G' rows, wave-private
        //  scratch -- was last read in layer 1 of this board, three barriers back; its planes and adjacency fragments are written
        //  behind that barrier, which no wave passes before every wave has finished this board's layer 3.)
        AQG_STAMP_AT(5)
#ifdef AQG_STAMP
        ++st_n;
#endif
        b = bn;
    }
#ifdef AQG_STAMP
    if (blk == 0 && threadIdx.x == 0) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(pooled + (size_t)B * HID);
        for (int i = 0; i < 16; ++i) o[i] = st_sum[i];
        o[16] = (unsigned long long)st_n;
    }
#endif
}

}  // namespace aqg
