// gcn_packed.hpp -- what every kernel family of the fixed-shape GraphPolicyValueNetwork (hidden width 128) shares: the network's
// constants, the layout of the packed weight buffer (filled by gcn_pack.hip, documented in include/aqgnn.h), the scale CQ of the
// split trunk's activation image, the D^-1/2 table and the phase-stamp macros of the diagnostic build.  Declarations and
// __forceinline__ device helpers only.
#pragma once
#include "split_mfma.hpp"

namespace aqg {

constexpr int HID = 128;          // HIDDEN_DIM pv_network_gnn.py:18
constexpr int FPAD = 8;           // NUM_FEATURES (6) padded
constexpr int LD = 132;           // LDS row stride in floats (528 B: 33 x 16-B slots, odd -> conflict-free)
constexpr int APAD = 256;         // policy outputs padded

// packed weight offsets (floats) -- documented in include/aqgnn.h
struct PackedLayout {
    static constexpr size_t W1 = 0;                       // [HID][FPAD]
    static constexpr size_t B1 = W1 + HID * FPAD;         // [HID]
    static constexpr size_t W2T = B1 + HID;               // [HID k][HID n]
    static constexpr size_t B2 = W2T + HID * HID;
    static constexpr size_t W3T = B2 + HID;
    static constexpr size_t B3 = W3T + HID * HID;
    static constexpr size_t HW1T = B3 + HID;              // [HID k][HID unit]
    static constexpr size_t HB1 = HW1T + HID * HID;
    static constexpr size_t PW2T = HB1 + HID;             // [HID/2 k][APAD]
    static constexpr size_t PB2 = PW2T + (HID / 2) * APAD;
    static constexpr size_t VW2 = PB2 + APAD;             // [HID/2]
    static constexpr size_t VB2 = VW2 + HID / 2;          // [4]
    // MFMA B-fragment order of W2^T / W3^T: [wave 4][ntile 2][s4 8][lane 64][4]  (see load_wfrag)
    static constexpr size_t WF2 = VB2 + 4;
    static constexpr size_t WF3 = WF2 + HID * HID;
    // fp16 2-way split (hi, lo) of W2^T / W3^T in 16x16x32 MFMA B-fragment order, stored as raw dwords:
    // [plane 2][tile 8 (16 columns each)][kblock 4][lane 64][4 dwords = 8 fp16]   (see load_bfrag_mm)
    static constexpr size_t WH2 = WF3 + HID * HID;
    static constexpr size_t WH3 = WH2 + 2 * HID * HID / 2;
    // layer-1 weight (times CQ) as fp16 A fragments, rows = output features, the split folded into the k dimension: per lane 8
    // halves, k-slots 0..7 and 8..15 = hi(c W1[n][0..5]),0,0   16..23 = lo(c W1[n][0..5]),0,0   24..31 = 0:  [tile 8][lane 64][4 dwords]
    static constexpr size_t WH1 = WH3 + 2 * HID * HID / 2;
    // heads on the split matrix pipe (gcn_heads_mm_kernel): hidden layer of both heads as A fragments
    // [plane 2][unit tile 8][kblock 4][lane 64][4 dwords]  (lane = unit 16*ut + c, k = 32*kb + 8*q + 0..7), and
    // policy_head.2 as B fragments [plane 2][action tile 14][kblock 2][lane 64][4 dwords] (lane = action 16*at + c,
    // k-slot (q, e) <-> hidden unit 32*kb + 16*(e >> 2) + 4*q + (e & 3): the order the layer-1 accumulators hold them)
    static constexpr size_t WHH1 = WH1 + 4 * 2 * 64 * 4;
    static constexpr size_t WHP2 = WHH1 + 2 * 8 * 4 * 64 * 4;
    // aggregation accumulator init of the default trunk: TB[layer 3][deg-1 5][HID] = CQ * b_layer[f] * sqrt(deg)
    // (the bias of a node with `deg` neighbours incl. itself, pre-divided by its D^-1/2 factor; see the trunk comment)
    static constexpr size_t TB = WHP2 + 2 * 14 * 2 * 64 * 4;
    // range-guard thresholds of the tracking trunk build (GUARD_MODE 2): [0] = largest |U| of layer 2's linear map for which layer 2's
    // aggregate provably stays below 65504, (65504 - max |TB_2|) / 2.07;  [1] = 65504 (layer 3's U is only split itself);  both are -1
    // (no maximum satisfies them: every board is reported) for a set the split kernels cannot serve -- a weight outside fp16 range, or
    // a split weight matrix below SPLIT_MIN_PLANE_SCALE;  [2..3] spare
    static constexpr size_t GUARD = TB + 3 * 5 * HID;
    static constexpr size_t TOTAL = GUARD + 4;
};

// Scale of the activation image of the default trunk: the planes hold Q = CQ * relu(...) / D^-1/2.  CQ = 15/16 makes
// CQ / deg exact in fp16 for every degree 1..5 (0.9375, 0.46875, 0.3125, 0.234375, 0.1875): the normalised adjacency
// becomes an EXACT fp16 matrix and no activation is ever multiplied by an irrational D^-1/2 factor on the vector unit.
constexpr double CQ = 15.0 / 16.0;

// deg^-1/2 for deg 1..5 (self loop + <=4 open neighbours), correctly rounded f32
__device__ __forceinline__ float dinv_of(int deg) {
    switch (deg) {
        case 1: return 1.0f;
        case 2: return 0.70710678118654752f;
        case 3: return 0.57735026918962576f;
        case 4: return 0.5f;
        default: return 0.44721359549995794f;
    }
}

__device__ __forceinline__ float dinv_of_bits(int bits) { return dinv_of(1 + __popc(bits)); }
// the same as straight selects on deg - 1 (a switch on a per-lane value can compile to divergent branches)
__device__ __forceinline__ float dinv_of_dm(uint32_t dm) {
    const float a = dm == 0u ? 1.0f : 0.70710678118654752f, b = dm == 2u ? 0.57735026918962576f : 0.5f;
    const float ab = dm < 2u ? a : b;
    return dm < 4u ? ab : 0.44721359549995794f;
}

// Diagnostic build only (-DAQG_STAMP, never shipped): per-phase s_memtime sums of workgroup 0 / wave 0 are
// written behind the pooled rows (pooled + B*128, as 16 x u64).  In the real kernel no stamp executes.
#ifdef AQG_STAMP
#define AQG_STAMP_DECL unsigned long long st_prev = __builtin_readcyclecounter(), st_sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; int st_n = 0;
#define AQG_STAMP_VMWAIT(i) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); AQG_STAMP_AT(i) }
#define AQG_STAMP_AT(i) { unsigned long long st_now = __builtin_readcyclecounter(); st_sum[i] += st_now - st_prev; st_prev = st_now; }
#else
#define AQG_STAMP_DECL
#define AQG_STAMP_AT(i)
#define AQG_STAMP_VMWAIT(i)
#endif

}  // namespace aqg
