// wave_ops.hpp -- what the 64 lanes of one wavefront do together: the xor-butterfly sum and maximum (offsets 32, 16, ..., 1; every
// lane ends with the same bits) and the wavefront-scope LDS hand-over.  __forceinline__ device code only; a unit that needs its
// arithmetic uncontracted sets `#pragma clang fp contract(off)` itself (an addition or a maximum has nothing to contract).
// Two fixed orders exist: wave_sum of gcn_train_heads.hpp adds quads first (DPP row operations, the trainers' pinned bits), these add
// halves first (what the engine's and the replay window's numpy statements restate); a float sum differs between them in its last bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace aqg {

template <class T>      // int, float, double, long long
__device__ __forceinline__ T wave_xor_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// uint64_t as two 32-bit shuffles of its halves (mod 2^64)
__device__ __forceinline__ uint64_t wave_xor_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ int wave_xor_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float wave_xor_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_xor_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// orders a wavefront's LDS writes in front of its own later LDS reads: release fence, wave barrier, acquire fence, all of wavefront
// scope.  Every lane must reach it.  Not for rows shared between wavefronts (those hand over at workgroup scope).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace aqg
