// weight_average.hip -- the exponential moving average of the parameters (struct aqg_weight_average, include/aqgnn.h "weight
// averaging"): e' = f32(d e) + f32(w p) over every tensor of a device table in ONE launch, beside the three trainers' steps.
//
//   table     4 T + 1 int64 words on the device: average pointers | source pointers | element counts | prefix of the chunk counts.
//   chunk     WA_CHUNK = 4,096 floats of ONE tensor, cut on the 16-byte grid the average's base sits in, as grad_sumsq_kernel
//             (grad_norm.hip) cuts its buffer: with `mis` = the floats between that grid and the base (0..3), element j of the tensor
//             is float mis + j of the grid and chunk c holds the grid's floats [c C, (c + 1) C).
//   workgroup b finds its tensor i = the number of prefix[1..T] <= b -- every wave counts for itself, 64 entries per round with a
//             ballot (no LDS, no barrier; the loop ends at the argument T) -- and its chunk b - prefix[i].  Lane t takes the 16-byte
//             words t, t + 256, t + 512, t + 768 of the chunk, all loads of both tensors issued before the first store.  A word wholly
//             inside the tensor, with the source sitting on the grid as the average does, is one 16-byte load of each and one 16-byte
//             store; every other float is loaded and stored alone, each access guarded by the range: nothing outside [e, e + n) or
//             [p, p + n) is touched, any 4-byte-aligned bases and any n >= 1 work.  The source is only read.  No atomics.
//
// The update is written once (wa_update) with contraction off: two rounded products and a rounded sum, what
// train_network.weight_average_reference states in numpy and torch.optim.swa_utils.get_ema_avg_fn computes on the CPU.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include <algorithm>
#include <cmath>

namespace aqg {

namespace {

constexpr int WA_THREADS = 256;
constexpr int WA_WORDS = 4;                                   // 16-byte words per lane
constexpr int WA_CHUNK = WA_THREADS * WA_WORDS * 4;           // floats per workgroup
static_assert(WA_CHUNK == AQG_WEIGHT_AVERAGE_CHUNK, "the header states the chunk the table's prefix is built on");
typedef float wa_f32x4 __attribute__((ext_vector_type(4)));

// the table's pointer words are read AS pointers: hipcc takes a pointer loaded from a kernel argument's memory for a global one
// (global_ loads and stores), an integer turned into a pointer for a generic one (flat_)
struct WaArgs { float* const* table; int T; float d, w; };

__device__ __forceinline__ float wa_update(float d, float w, float e, float p) {
#pragma clang fp contract(off)       // every product and the sum rounded, as train_network.weight_average_reference states them
    const float de = d * e;
    const float wp = w * p;
    return de + wp;
}

__global__ __launch_bounds__(WA_THREADS) void weight_average_kernel(WaArgs a) {
    const WaArgs l = a;                         // (a copy, not a reference into `a`: train_adam.hpp says why)
    const int T = l.T, t = threadIdx.x, lane = t & 63;
    const long long b = blockIdx.x;
    const long long* words = reinterpret_cast<const long long*>(l.table);
    const long long* prefix = words + 3 * (long long)T;
    int i = 0;                                  // wave-uniform: the ballot is a scalar
    for (int j0 = 0; j0 < T; j0 += 64) {
        const int j = j0 + lane;
        const bool behind = j < T && prefix[j + 1] <= b;
        i += __popcll(__ballot(behind));
    }
    if (i >= T) return;                         // (a grid larger than the prefix says: the host checks refuse it)
    float* e = l.table[i];
    const float* p = l.table[T + i];
    const long long n = words[2 * (long long)T + i];
    const long long c = b - prefix[i];
    const int mis = (int)((reinterpret_cast<uintptr_t>(e) >> 2) & 3);
    const bool alike = mis == (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
    const long long nv = n + mis;
    const float d = l.d, w = l.w;

    wa_f32x4 x[WA_WORDS], y[WA_WORDS];
#pragma unroll
    for (int k = 0; k < WA_WORDS; ++k) {
        const long long f = (c * (WA_CHUNK / 4) + (long long)k * WA_THREADS + t) * 4;      // first float of the word, on the grid
        if (alike && f >= mis && f + 4 <= nv) {
            x[k] = *reinterpret_cast<const wa_f32x4*>(e + (f - mis));
            y[k] = *reinterpret_cast<const wa_f32x4*>(p + (f - mis));
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = f + q >= mis && f + q < nv;
                x[k][q] = in ? e[f + q - mis] : 0.f;
                y[k][q] = in ? p[f + q - mis] : 0.f;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < WA_WORDS; ++k) {
        const long long f = (c * (WA_CHUNK / 4) + (long long)k * WA_THREADS + t) * 4;
        wa_f32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = wa_update(d, w, x[k][q], y[k][q]);
        if (alike && f >= mis && f + 4 <= nv) {
            *reinterpret_cast<wa_f32x4*>(e + (f - mis)) = r;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (f + q >= mis && f + q < nv) e[f + q - mis] = r[q];
        }
    }
}

struct Range { uintptr_t lo, hi; bool average; };

}  // namespace

// every refusal of include/aqgnn.h "weight averaging", on the host table; nothing is launched
int check_weight_average(const aqg_weight_average* a, const char* what) {
    if (!a) return fail(what, "aqg_weight_average is NULL");
    if (!a->table || !a->host_table) return fail(what, "aqg_weight_average.table is NULL");
    const int T = a->num_tensors;
    if (T < 1 || T > AQG_WEIGHT_AVERAGE_MAX_TENSORS) return fail(what, "aqg_weight_average.num_tensors must be 1..1024");
    if (!(a->decay >= 0.f && a->decay < 1.f)) return fail(what, "aqg_weight_average.decay must be in [0, 1)");
    if (a->every < 1) return fail(what, "aqg_weight_average.every must be >= 1");
    const int64_t* h = a->host_table;
    Range r[2 * AQG_WEIGHT_AVERAGE_MAX_TENSORS];
    long long chunks = 0;
    if (h[3 * T] != 0) return fail(what, "the weight average's chunk prefix does not start at 0");
    for (int i = 0; i < T; ++i) {
        const uintptr_t e = (uintptr_t)h[i], p = (uintptr_t)h[T + i];
        const long long n = h[2 * T + i];
        if (!e || !p) return fail(what, "null tensor in the weight average's table");
        if ((e & 3) || (p & 3)) return fail(what, "the weight average's tensors must be 4-byte aligned");
        if (n < 1) return fail(what, "a tensor of the weight average has fewer than 1 element");
        if (n > 0x1fffffffffffLL) return fail(what, "a tensor of the weight average is too large");
        chunks += (n + (long long)((e >> 2) & 3) + WA_CHUNK - 1) / WA_CHUNK;
        if (h[3 * T + i + 1] != chunks) return fail(what, "the weight average's chunk prefix does not match its tensors");
        r[2 * i] = Range{e, e + (uintptr_t)n * 4, true};
        r[2 * i + 1] = Range{p, p + (uintptr_t)n * 4, false};
    }
    if (a->total_chunks != chunks) return fail(what, "aqg_weight_average.total_chunks does not match its tensors");
    if (chunks > 0x7fffffffLL) return fail(what, "the weight average has more than 2^31 - 1 chunks");
    // a sweep over the ranges by start: an average must begin behind everything seen, a source behind every average seen
    std::sort(r, r + 2 * T, [](const Range& u, const Range& v) { return u.lo < v.lo; });
    uintptr_t end_any = 0, end_average = 0;
    for (int k = 0; k < 2 * T; ++k) {
        if (r[k].lo < (r[k].average ? end_any : end_average))
            return fail(what, "an average tensor overlaps a source tensor or another average tensor");
        end_any = std::max(end_any, r[k].hi);
        if (r[k].average) end_average = std::max(end_average, r[k].hi);
    }
    return 0;
}

// the launch of a CHECKED struct
int launch_weight_average(const aqg_weight_average& a, hipStream_t st) {
    const WaArgs args{reinterpret_cast<float* const*>(a.table), a.num_tensors, a.decay, (float)(1.0 - (double)a.decay)};
    hipLaunchKernelGGL(weight_average_kernel, dim3((unsigned)a.total_chunks), dim3(WA_THREADS), 0, st, args);
    return check_launch("weight_average_kernel");
}

}  // namespace aqg
