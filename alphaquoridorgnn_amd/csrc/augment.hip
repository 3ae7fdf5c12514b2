// augment.hip -- mirror-symmetry training augmentation: the epoch's shuffle (a row gather) and the left-right mirror of the rows it
// flips, in ONE launch over (state72, pi, z) rows (include/aqgnn.h, "training augmentation").
//
// A bandwidth-bound permuting copy, ~912 B per row at 9x9 (72 + 4 * 209 + 4).  A workgroup owns AUG_ROWS consecutive OUTPUT rows:
// its first lanes read their order[] entries in one coalesced load, decide each row's flip (table or counter generator, keyed by
// the SOURCE row) and copy z, one lane per row; then every wavefront copies whole rows, four rows' loads in flight before a store.
// Stores are contiguous across lanes -- out[j] = in[perm(j)] -- and perm is arithmetic (a mirror inside a line of N or N - 1 cells),
// so the permuted reads stay inside the source row's own cache lines.  No record byte is ever used as an address: a position byte
// is a VALUE that is rewritten (or copied through when it is no tile of the board).  No atomics, no scratch; every loop ends on n.
#include "aqg_common.hpp"
#include "counter_rng.hpp"
#include "launchers.hpp"

namespace aqg {

constexpr int AUG_WAVES = 4;
constexpr int AUG_GROUP = 4;    // rows a wavefront loads before it stores any
// output rows of one workgroup: one group per wavefront.  Measured on an MI355X against 32 and 64 (2 and 4 groups per wavefront in
// turn): 16 is the fastest at 1,000, 4,000 and 163,840 rows -- a short epoch needs the workgroups, a long one loses nothing
constexpr int AUG_ROWS = AUG_WAVES * AUG_GROUP;

// cell i of a grid of lines of W cells, mirrored inside its line: (i / W) * W + (W - 1 - i % W)
template <int W>
__device__ __forceinline__ int mirror_cell(int i) { return i + (W - 1) - 2 * (i % W); }

// the action a mirrored policy row reads for its action j (the map is an involution: out[mirror(a)] = in[a])
template <int N>
__device__ __forceinline__ int mirror_action(int j) {
    constexpr int V = Geo<N>::V, S = Geo<N>::S, NW = Geo<N>::NW;
    if (j < V) return mirror_cell<N>(j);
    if (j < V + NW) return V + mirror_cell<S>(j - V);
    return V + NW + mirror_cell<S>(j - V - NW);
}

// byte k of the output record of source record `in` (k < STATE72)
template <int N>
__device__ __forceinline__ uint8_t record_byte(const uint8_t* __restrict__ in, int k, bool flip) {
    constexpr int V = Geo<N>::V, S = Geo<N>::S, NW = Geo<N>::NW;
    const bool wall = k >= 4 && k < 4 + NW;
    const uint8_t v = in[flip && wall ? 4 + mirror_cell<S>(k - 4) : k];
    if (flip && (k == 0 || k == 2) && v < V) return (uint8_t)mirror_cell<N>(v);     // a pawn; a byte that is no tile has no image
    return v;
}

template <int N>
__global__ __launch_bounds__(AUG_WAVES * WAVE) void augment_gather_kernel(
        const uint8_t* __restrict__ states72, const float* __restrict__ pi, const float* __restrict__ z,
        const int64_t* __restrict__ order, const uint8_t* __restrict__ flips, int use_seed, uint64_t key, int n,
        uint8_t* __restrict__ out72, float* __restrict__ out_pi, float* __restrict__ out_z) {
    constexpr int A = Geo<N>::A;
    constexpr int PI_PASSES = (A + WAVE - 1) / WAVE;           // 1, 1, 2, 4 at 3x3 .. 9x9
    __shared__ int64_t src_row[AUG_ROWS];
    __shared__ uint8_t src_flip[AUG_ROWS];
    const int first = blockIdx.x * AUG_ROWS;                    // < n: the grid is ceil(n / AUG_ROWS)
    const int rows = min(AUG_ROWS, n - first);
    const int t = threadIdx.x;
    if (t < rows) {
        const int64_t r = order ? order[first + t] : (int64_t)(first + t);
        src_row[t] = r;
        src_flip[t] = flips ? (uint8_t)(flips[r] != 0) : (uint8_t)(use_seed && counter_uniform(key, (uint64_t)r) < 0.5);
        if (z) out_z[first + t] = z[r];
    }
    __syncthreads();
    const int wave = t >> 6, lane = t & 63;
    for (int q0 = wave * AUG_GROUP; q0 < rows; q0 += AUG_WAVES * AUG_GROUP) {
        float pv[AUG_GROUP][PI_PASSES];
        uint8_t sv[AUG_GROUP][2];
#pragma unroll
        for (int g = 0; g < AUG_GROUP; ++g) {
            const int q = q0 + g;
            if (q >= rows) continue;
            const size_t r = (size_t)src_row[q];
            const bool flip = src_flip[q] != 0;
            if (pi) {
                const float* __restrict__ in = pi + r * A;
#pragma unroll
                for (int p = 0; p < PI_PASSES; ++p) {
                    const int j = p * WAVE + lane;
                    if (j < A) pv[g][p] = in[flip ? mirror_action<N>(j) : j];
                }
            }
            if (states72) {
                const uint8_t* __restrict__ in = states72 + r * STATE72;
                sv[g][0] = record_byte<N>(in, lane, flip);
                if (lane < STATE72 - WAVE) sv[g][1] = record_byte<N>(in, WAVE + lane, flip);
            }
        }
#pragma unroll
        for (int g = 0; g < AUG_GROUP; ++g) {
            const int q = q0 + g;
            if (q >= rows) continue;
            const size_t i = (size_t)(first + q);
            if (pi) {
#pragma unroll
                for (int p = 0; p < PI_PASSES; ++p) {
                    const int j = p * WAVE + lane;
                    if (j < A) out_pi[i * A + j] = pv[g][p];
                }
            }
            if (states72) {
                out72[i * STATE72 + lane] = sv[g][0];
                if (lane < STATE72 - WAVE) out72[i * STATE72 + WAVE + lane] = sv[g][1];
            }
        }
    }
}

int launch_augment_gather(int N, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                          const uint8_t* flips, int use_seed, uint64_t seed, uint64_t epoch, int n, uint8_t* out72, float* out_pi,
                          float* out_z, hipStream_t st) {
    if (!board_size_supported(N)) return fail("aqg_augment_gather: unsupported board_size (odd 3..9)");
    const int A = action_count(N);
    if (policy_size != A) return fail("aqg_augment_gather: policy_size is not the board's action count N^2 + 2 (N - 1)^2");
    if (n < 0) return fail("aqg_augment_gather: negative row count");
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at (an empty array's may be NULL)
    if (!states72 != !out72 || !pi != !out_pi || !z != !out_z)
        return fail("aqg_augment_gather: an input and its output must both be given or both be NULL");
    if (!states72 && !pi && !z) return 0;
    // An output that overlaps an input would be read by one workgroup after another has written it.  The outputs have n rows; of a
    // source only what is certain is assumed: n rows without order, one row with it (its row count is not an argument) -- never a
    // refusal of a legitimate call, and an output inside the rest of a gathered source is the caller's to avoid.
    const size_t in_rows = order ? 1 : (size_t)n;
    const size_t row_bytes[3] = {STATE72, (size_t)A * sizeof(float), sizeof(float)};
    const void* ins[3] = {states72, pi, z};
    const void* outs[3] = {out72, out_pi, out_z};
    for (int o = 0; o < 3; ++o)
        for (int i = 0; i < 3; ++i)
            if (overlap(outs[o], (size_t)n * row_bytes[o], ins[i], in_rows * row_bytes[i]))
                return fail("aqg_augment_gather: an output overlaps an input");
    const uint64_t key = stream_key(seed, epoch);
    const dim3 grid((unsigned)(((size_t)n + AUG_ROWS - 1) / AUG_ROWS)), block(AUG_WAVES * WAVE);
    return for_board_size(N, [&](auto nn) {
        hipLaunchKernelGGL(augment_gather_kernel<decltype(nn)::value>, grid, block, 0, st, states72, pi, z, order, flips,
                           (flips || !use_seed) ? 0 : 1, key, n, out72, out_pi, out_z);
        return check_launch("augment_gather_kernel");
    });
}

}  // namespace aqg
