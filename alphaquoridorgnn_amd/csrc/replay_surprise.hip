// replay_surprise.hip -- replay window: which rows an update trains on, drawn by policy surprise (include/aqgnn.h, "policy surprise
// weighting").  Two launches: the surprise of every row against the network the update starts from, and each row's number of copies.
//
// aqg_replay_surprise_rows: k = f32(KL(row's policy target || the network's policy of the row's record)) and q = floor(k 2^20), for
// one chunk of n rows whose network policy the caller has just computed ([n, A], row i of the chunk) -- the target is row index[offset
// + i] of the ring (index NULL: row offset + i), the results go to k[offset + i] and q[offset + i].  A streaming read of 8A bytes
// a row with two float64 logarithms per positive target entry.  The geometry is replay.hip's and augment.hip's: a workgroup owns
// SPR_ROWS = 16 consecutive rows of the chunk, every one of its SPR_WAVES = 4 wavefronts takes SPR_GROUP = 4 rows whole, the four ring
// rows first, then all the rows' loads of both arrays in flight before the first use.  No LDS, no atomics, no workgroup barrier, no
// scratch; every loop is bounded by a constant and every row by n.
//
// The sum is float64, evaluated exactly as written (no contraction: t * (ln t - ln p) is a product of a difference, then one sum),
// in a FIXED order that replay.surprise_reference repeats: lane l adds its own entries a = l, l + 64, ... in ascending order to +0.0,
// then the xor-shuffle wave reduction 32, 16, ..., 1 (v += shfl_xor(v, off): a sum of two operands commutes, so every lane ends with
// the same bits).  An entry with t <= 0 adds nothing.  The row predicates -- any non-finite entry of t or p, any negative target
// entry, any positive target entry -- are pure, and made wave-uniform by ballot as in replay_refresh_kernel; a row they reject, and a
// row whose index entry is outside the ring (it is then not read), gets k = 0, q = 0.
//
// aqg_replay_surprise_counts: one lane per row.  f = (E U) / m + ((E (1 - U)) q) / S in float64 in that order (S from a device
// int64; S <= 0: f = E / m), count = min(floor(f) + [u < f - floor(f)], C) with u = counter_uniform(stream_key(seed, update), r), r
// the row's place in the arrays (the ring slot): a row's draw does not depend on m, on the chunking or on the rank.
#include "aqg_common.hpp"
#include "counter_rng.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"
#include <cfloat>
#include <cmath>

#ifdef __FAST_MATH__
#error "replay_surprise.hip: the float64 sum, its logarithms and the divisions must be the IEEE ones (no fast-math)"
#endif
// t * (ln t - ln p), acc + term, (E U) / m + ...: every operation rounded on its own (replay.surprise_reference is the same in numpy)
#pragma clang fp contract(off)

namespace aqg {

constexpr int SPR_WAVES = 4;
constexpr int SPR_GROUP = 4;    // rows a wavefront loads before it uses any
constexpr int SPR_ROWS = SPR_WAVES * SPR_GROUP;     // rows of one workgroup
constexpr int SPR_LANES = 256;  // rows of one workgroup of the counts launch
constexpr int SPR_MAX_ROWS = 1 << 24;      // m at most: S = sum q < 2^24 * 2^27
constexpr float SPR_TINY = 0x1.0p-126f;    // the least p a logarithm is taken of
constexpr double SPR_K_MAX = 88.0;         // > 126 ln 2, the most a row whose target sums to 1 can reach: q < 2^27 whatever the row holds
constexpr double SPR_Q_SCALE = 0x1.0p20;

template <int N>
__global__ __launch_bounds__(SPR_WAVES * WAVE) void replay_surprise_rows_kernel(
        const float* __restrict__ net_policy, const float* __restrict__ ring_pi, const int64_t* __restrict__ index, int rows, int offset,
        int n, float* __restrict__ k, int32_t* __restrict__ q) {
    constexpr int A = Geo<N>::A;
    constexpr int PASSES = (A + WAVE - 1) / WAVE;              // 1, 1, 2, 4 at 3x3 .. 9x9
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = blockIdx.x * SPR_ROWS + wave * SPR_GROUP;        // this wavefront's first row of the chunk
    int64_t r[SPR_GROUP];
    float t[SPR_GROUP][PASSES], p[SPR_GROUP][PASSES];
    // ---- the ring rows of the group, then every load of both arrays, none waiting for another
#pragma unroll
    for (int g = 0; g < SPR_GROUP; ++g) {
        const int i = first + g;
        r[g] = i >= n ? (int64_t)-1 : index ? index[(size_t)offset + i] : (int64_t)offset + i;      // wave-uniform
    }
#pragma unroll
    for (int g = 0; g < SPR_GROUP; ++g) {
        const bool live = r[g] >= 0 && r[g] < (int64_t)rows;           // first + g < n, and a row the ring has
#pragma unroll
        for (int s = 0; s < PASSES; ++s) {
            const int a = s * WAVE + lane;
            const bool in = live && a < A;
            t[g][s] = in ? ring_pi[(size_t)r[g] * A + a] : 0.f;        // past the row: neither negative, nor positive, nor non-finite
            p[g][s] = in ? net_policy[(size_t)(first + g) * A + a] : 1.f;
        }
    }
#pragma unroll
    for (int g = 0; g < SPR_GROUP; ++g) {
        if (first + g >= n) continue;                                   // wave-uniform: the reduction below runs on whole wavefronts
        bool bad = false, some = false;
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < PASSES; ++s) {
            const float tt = t[g][s], pp = p[g][s];
            bad = bad || !(tt >= 0.f && tt <= FLT_MAX) || !(fabsf(pp) <= FLT_MAX);       // negative, infinite or NaN
            some = some || tt > 0.f;
            if (tt > 0.f) {
                const float pc = pp > SPR_TINY ? pp : SPR_TINY;
                const double d = log((double)tt) - log((double)pc);
                const double term = (double)tt * d;
                acc = acc + term;
            }
        }
        const double kl = wave_xor_sum(acc);
        const bool ok = r[g] >= 0 && r[g] < (int64_t)rows && __ballot(bad) == 0 && __ballot(some) != 0;
        const float kk = ok ? (float)fmin(fmax(kl, 0.0), SPR_K_MAX) : 0.f;
        if (lane == 0) {
            k[(size_t)offset + first + g] = kk;
            q[(size_t)offset + first + g] = (int32_t)((double)kk * SPR_Q_SCALE);      // exact product, < 2^27: the conversion is the floor
        }
    }
}

__global__ __launch_bounds__(SPR_LANES) void replay_surprise_counts_kernel(
        const int32_t* __restrict__ q, const int64_t* __restrict__ index, const int64_t* __restrict__ total, int m, double expected,
        double share, int max_copies, uint64_t key, int32_t* __restrict__ count) {
    const size_t j = (size_t)blockIdx.x * SPR_LANES + threadIdx.x;
    if (j >= (size_t)m) return;
    const int64_t S = *total;
    const int64_t r = index ? index[j] : (int64_t)j;
    double f;
    if (S > 0) {
        const double uniform = (expected * share) / (double)m;
        const double rest = expected * (1.0 - share);
        const double surprised = (rest * (double)q[j]) / (double)S;
        f = uniform + surprised;
    } else {
        f = expected / (double)m;
    }
    const double whole = floor(f);
    const double u = counter_uniform(key, (uint64_t)r);
    const double c = whole + (u < f - whole ? 1.0 : 0.0);
    count[j] = (int32_t)fmin(c, (double)max_copies);
}

int launch_replay_surprise_rows(int N, int policy_size, const float* net_policy, const float* ring_pi, const int64_t* index, int rows,
                                int m, int offset, int n, float* k, int32_t* q, hipStream_t st) {
    const char* what = "aqg_replay_surprise_rows";
    if (!board_size_supported(N)) return fail(what, "unsupported board_size (odd 3..9)");
    const int A = action_count(N);
    if (policy_size != A) return fail(what, "policy_size is not the board's action count N^2 + 2 (N - 1)^2");
    if (m < 0 || m > SPR_MAX_ROWS) return fail(what, "m out of range (0 .. 2^24 rows)");
    if (rows < 0) return fail(what, "negative row count of the ring");
    if (!index && m > rows) return fail(what, "m out of range (without an index, m <= rows)");
    if (offset < 0 || n < 0 || n > m - offset) return fail(what, "the chunk is not inside the m rows (0 <= offset, 0 <= n, offset + n <= m)");
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at
    if (!net_policy || !ring_pi || !k || !q) return fail(what, "net_policy, ring_pi, k and q must be given");
    const void* outs[2] = {k, q};
    const void* srcs[3] = {net_policy, ring_pi, index};
    const size_t src_bytes[3] = {(size_t)n * A * sizeof(float), (size_t)(index ? 1 : rows) * A * sizeof(float), (size_t)m * sizeof(int64_t)};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 3; ++i)
            if (overlap(outs[o], (size_t)m * 4, srcs[i], src_bytes[i])) return fail(what, "an output overlaps a source");
    if (overlap(k, (size_t)m * 4, q, (size_t)m * 4)) return fail(what, "k overlaps q");
    const dim3 grid((unsigned)(((size_t)n + SPR_ROWS - 1) / SPR_ROWS)), block(SPR_WAVES * WAVE);
    return for_board_size(N, [&](auto nn) {
        hipLaunchKernelGGL((replay_surprise_rows_kernel<decltype(nn)::value>), grid, block, 0, st, net_policy, ring_pi, index, rows, offset, n,
                           k, q);
        return check_launch("replay_surprise_rows_kernel");
    });
}

int launch_replay_surprise_counts(const int32_t* q, const int64_t* index, const int64_t* total, int m, long long expected_rows,
                                  double uniform_share, int max_copies, uint64_t seed, uint64_t update, int32_t* count, hipStream_t st) {
    const char* what = "aqg_replay_surprise_counts";
    if (m < 0 || m > SPR_MAX_ROWS) return fail(what, "m out of range (0 .. 2^24 rows)");
    if (!(uniform_share >= 0.0 && uniform_share <= 1.0)) return fail(what, "uniform_share must be in [0, 1]");      // NaN fails both
    if (max_copies < 1 || max_copies > 255) return fail(what, "max_copies must be in 1 .. 255");
    if (expected_rows < 1 || expected_rows > (1ll << 40)) return fail(what, "expected_rows must be in 1 .. 2^40");
    if (m == 0) return 0;                   // nothing to write: the pointers are not looked at
    if (!q || !total || !count) return fail(what, "q, total and count must be given");
    const void* srcs[3] = {q, index, total};
    const size_t src_bytes[3] = {(size_t)m * sizeof(int32_t), (size_t)m * sizeof(int64_t), sizeof(int64_t)};
    for (int i = 0; i < 3; ++i)
        if (overlap(count, (size_t)m * sizeof(int32_t), srcs[i], src_bytes[i])) return fail(what, "count overlaps a source");
    const dim3 grid((unsigned)(((size_t)m + SPR_LANES - 1) / SPR_LANES)), block(SPR_LANES);
    hipLaunchKernelGGL(replay_surprise_counts_kernel, grid, block, 0, st, q, index, total, m, (double)expected_rows, uniform_share,
                       max_copies, stream_key(seed, update), count);
    return check_launch("replay_surprise_counts_kernel");
}

}  // namespace aqg
