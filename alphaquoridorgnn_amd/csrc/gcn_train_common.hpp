// gcn_train_common.hpp -- what every unit of the fused 6/128/3 training step (gcn_train.hip is the map) shares: the sizes, the
// small f32x4 helpers (f32x4 itself is split_mfma.hpp's), record_of, and the two diagnostic builds' marks.
#pragma once
#include "aqg_common.hpp"
#include "split_mfma.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"

namespace aqg {

constexpr int TH = 128;    // HIDDEN_DIM
constexpr int TF = 6;      // NUM_FEATURES
constexpr int HH = 64;     // width of each head's hidden layer
constexpr int SA = 132;    // LDS row stride of a [rows][128] A operand  (132 = 4 mod 64: 16 rows x 4 k-lanes hit 64 banks)
constexpr int SB = 144;    // LDS row stride of H [nodes][128] as its B operand (144 = 16 mod 64)

// Diagnostic build only (-DAQG_STAMP, tools/stamp_train.py; never shipped): thread 0 of workgroup 0 adds the cycles between
// consecutive phase marks of section k to g_train_stamp[k][phase]; k = 0 train_final_kernel, 1 the heads, 2 the f32 body,
// 3 the split body.  One array per unit, under the unit's own name (AQG_TRAIN_TU, defined in front of this header; the note at
// AQG_TRACE_TU in aqg_common.hpp says why); the unit's AQG_TRAIN_STAMP_READER adds its counters to out[64] and clears them on
// reset, and aqg_debug_train_stamps (gcn_train.hip) calls every unit's.
#ifdef AQG_STAMP
#define g_train_stamp AQG_CAT(g_train_stamp_, AQG_TRAIN_TU)
static __device__ unsigned long long g_train_stamp[4][16];
#define TS_DECL unsigned long long ts_prev = __builtin_readcyclecounter();
#define TS(k, i) { const unsigned long long ts_now = __builtin_readcyclecounter(); if (blockIdx.x == 0 && threadIdx.x == 0) g_train_stamp[k][i] += ts_now - ts_prev; ts_prev = ts_now; }
#define AQG_TRAIN_STAMP_READER(name) int name(unsigned long long* out, int reset) { unsigned long long v[64]; \
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_train_stamp), sizeof(v)) != hipSuccess) return -1; \
    for (int i = 0; i < 64; ++i) out[i] += v[i]; \
    if (reset) { memset(v, 0, sizeof(v)); if (hipMemcpyToSymbol(HIP_SYMBOL(g_train_stamp), v, sizeof(v)) != hipSuccess) return -1; } \
    return 0; }
#else
#define TS_DECL
#define TS(k, i)
#define AQG_TRAIN_STAMP_READER(name)
#endif

// developer build only (-DAQG_TRAIN_DEBUG, tools/train_debug.py): dense dumps of intermediate gradients, [slot][b][96][128]; one
// pointer per unit with a DBG_PUT, set through the unit's AQG_TRAIN_DEBUG_SETTER by aqg_debug_train_buf (gcn_train.hip)
#ifdef AQG_TRAIN_DEBUG
#define g_train_dbg AQG_CAT(g_train_dbg_, AQG_TRAIN_TU)
static __device__ float* g_train_dbg = nullptr;
#define DBG_PUT(slot, B_, b_, n_, col_, v_) { if (g_train_dbg) g_train_dbg[(((size_t)(slot) * (B_) + (b_)) * 96 + (n_)) * 128 + (col_)] = (v_); }
#define AQG_TRAIN_DEBUG_SETTER(name) int name(float* buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_train_dbg), &buf, sizeof(buf)) == hipSuccess ? 0 : -1; }
#else
#define DBG_PUT(slot, B_, b_, n_, col_, v_)
#define AQG_TRAIN_DEBUG_SETTER(name)
#endif

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)}; }

__device__ __forceinline__ size_t record_of(const int64_t* __restrict__ order, int first, int b) {
    return order ? (size_t)order[first + b] : (size_t)(first + b);
}

}  // namespace aqg
