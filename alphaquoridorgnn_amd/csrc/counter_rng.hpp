// counter_rng.hpp -- the counter-based generator documented in include/aqgnn.h, shared by the baseline agents (agents.hip) and the
// root exploration noise (mcts_move.hip): stateless, so a draw depends on (key, index) alone and never on launch geometry.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace aqg {

constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {       // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the key of sub-stream b of `seed`
__host__ __device__ __forceinline__ uint64_t stream_key(uint64_t seed, uint64_t b) { return mix64(seed + GOLDEN * (b + 1)); }
// draw i of the stream `key`: a float64 in [0, 1)
__host__ __device__ __forceinline__ double counter_uniform(uint64_t key, uint64_t i) {
    return (double)(mix64(key + GOLDEN * (i + 1)) >> 11) * 0x1.0p-53;
}

}  // namespace aqg
