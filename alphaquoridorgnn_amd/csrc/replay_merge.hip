// replay_merge.hip -- replay window: repeated positions merged into one row with averaged targets (include/aqgnn.h, "position
// merge").  Three entry points; torch sorts and does the prefix plumbing between them (replay.merge_positions), every row is touched
// here.  replay.merge_reference / replay.position_keys are the same statements in numpy, bit for bit.
//
//   keys   position_keys_kernel: one 64-bit hash of a record's KEY BYTES (0..67 and 70; 68-69 are the ply counter, 71 is spare) per
//          row.  Lanes across the record's bytes, a coalesced 72-byte read per row; the hash is a SUM over the bytes,
//          sum_k (b_k + 1) * M_k mod 2^64 with M_k an odd constant of the byte's place, then one bijective mixing step -- integer
//          sums are exact in any order, so the wave reduction needs none.  A single changed key byte changes the sum by
//          (b' - b) * M_k, which is never 0 mod 2^64 (M_k odd, |b' - b| < 256).  The hash only GROUPS rows: nothing is merged on it.
//   heads  run_heads_kernel: heads[i] = 1 iff i == 0 or the key bytes of row perm[i] differ from those of row perm[i - 1] -- a full
//          compare, lanes across the bytes, one wave vote per row.
//   merge  merge_runs_kernel, the hot path: output row o is the run perm[starts[o] .. starts[o + 1]) (starts[u] = n); its record is
//          row perm[starts[o]]'s 72 bytes verbatim, its targets the run's mean.  A gathering copy of ~4A + 76 bytes per input row
//          (912 at 9x9) in augment.hip's geometry: a workgroup owns MRG_ROWS = 16 consecutive OUTPUT rows, its first lanes read the
//          runs' bounds (and copy z and write count), then each of the 4 wavefronts takes MRG_GROUP = 4 rows whole, lanes across the
//          policy row, the four first rows' loads in flight before the first store.  A run of length 1 -- almost every run -- ends there,
//          bit for bit.  A longer run adds its other rows onto the first, MRG_ADD = 8 rows' loads in flight at a time, z as column A of the
//          row; the lanes fetch the run's perm entries in one coalesced load, so a row's address is a shuffle away.
//
// Summation order -- a function of the run's length L and the rows' order within the run alone:
//     chunk c = rows [64 c, min(64 c + 64, L)) of the run, summed left to right starting FROM its first row: ((x0 + x1) + x2) + ...
//     total   = the chunk sums, summed left to right starting from chunk 0's;   mean = total / f32(L), the correctly rounded quotient.
// Depth: a term passes through at most d(L) = min(L, 64) - 1 + ceil(L / 64) - 1 additions (63 + L / 64 for a long run;
// replay.merge_depth).  A run of L <= MRG_CHUNK = 64 rows is one chunk and is summed by the wavefront that stores it.  The chunks of
// a longer run are summed by merge_chunks_kernel, launched in FRONT of the merge launch (only when n - u >= 64: a run of L rows has
// L - 1 repeats): one wavefront per window of 64 sorted places [64 w, 64 w + 64), which finds the runs that cross its window by a
// 64-way search of starts (one probe per lane and round, at most 8 rounds) and sums every chunk
// that BEGINS in its window -- at most two: a long run has at most one chunk start in any 64 places and at most one long run begins in
// a window -- into workspace row 2 w + (the chunk is its run's first).  The merge launch's wavefront then adds the run's ceil(L / 64)
// partial rows in chunk order, eight rows' loads in flight.  So a run of 20,000 rows is read by 313 wavefronts, and its owner reads
// 313 partial rows; no atomics, plain stores, and the launch boundary is the only synchronisation.  Every loop ends on an argument
// (n, u) or a constant.
//
// Timed beside this form on an MI355X (tools/merge_positions_time.py with ALT_LIB; profiles/merge_positions.log): the run's further rows
// added four at a time with each row's perm entry loaded when it is needed -- 126.0 against 101.6 us at 163,840 rows of 9x9, 29.6
// against 24.1 us at 1,000 rows of 5x5 -- and a bisection of starts (up to 32 dependent loads) in place of the 64-way search --
// with the caches flushed in front of every call 115.5 against 110.7 us at 163,840 rows, 22.1 against 19.8 us at 4,000, 36.0 against
// 34.5 us at 5x5; without the flush the two were equal.  Neither is the one kept.
#include "aqg_common.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"

#ifdef __FAST_MATH__
#error "replay_merge.hip: the mean must be the correctly rounded f32 division (no fast-math)"
#endif
// sums and the quotient exactly as written (replay.merge_reference is the same in numpy)
#pragma clang fp contract(off)

namespace aqg {

namespace {

constexpr int MRG_WAVES = 4;
constexpr int MRG_GROUP = 4;                        // rows a wavefront loads before it uses any
constexpr int MRG_ROWS = MRG_WAVES * MRG_GROUP;     // rows of one workgroup: output rows (merge), input rows (keys, heads)
constexpr int MRG_CHUNK = 64;                       // rows of one chunk of the summation order
constexpr int MRG_ADD = 8;                          // rows in flight when a run's further rows (or a long run's chunk sums) are added

// ---- the hash

__host__ __device__ constexpr uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the multiplier of byte place k: odd; 0 for the three bytes that are no part of the key
__device__ __forceinline__ uint64_t place_multiplier(int k) {
    return (k == 68 || k == 69 || k == 71) ? 0ull : (splitmix64((uint64_t)k) | 1ull);
}
__device__ __forceinline__ bool is_key_byte(int k) { return k != 68 && k != 69 && k != 71; }

__global__ __launch_bounds__(MRG_WAVES * WAVE) void position_keys_kernel(const uint8_t* __restrict__ states72,
                                                                        const int64_t* __restrict__ index, int n,
                                                                        int64_t* __restrict__ keys) {
    const int first = blockIdx.x * MRG_ROWS;                    // < n: the grid is ceil(n / MRG_ROWS)
    const int rows = min(MRG_ROWS, n - first);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t m0 = place_multiplier(lane), m1 = lane < STATE72 - WAVE ? place_multiplier(WAVE + lane) : 0ull;
    uint8_t b[MRG_GROUP][2];
#pragma unroll
    for (int g = 0; g < MRG_GROUP; ++g) {
        const int q = wave * MRG_GROUP + g;
        if (q >= rows) continue;
        const size_t r = index ? (size_t)index[first + q] : (size_t)(first + q);
        b[g][0] = states72[r * STATE72 + lane];
        b[g][1] = lane < STATE72 - WAVE ? states72[r * STATE72 + WAVE + lane] : (uint8_t)0;
    }
#pragma unroll
    for (int g = 0; g < MRG_GROUP; ++g) {
        const int q = wave * MRG_GROUP + g;
        if (q >= rows) continue;                                // wave-uniform: the reduction runs on whole wavefronts
        const uint64_t h = wave_xor_sum(((uint64_t)b[g][0] + 1) * m0 + ((uint64_t)b[g][1] + 1) * m1);
        if (lane == 0) keys[first + q] = (int64_t)splitmix64(h);
    }
}

__global__ __launch_bounds__(MRG_WAVES * WAVE) void run_heads_kernel(const uint8_t* __restrict__ states72,
                                                                    const int64_t* __restrict__ perm, int n,
                                                                    uint8_t* __restrict__ heads) {
    const int first = blockIdx.x * MRG_ROWS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool key0 = is_key_byte(lane), key1 = lane < STATE72 - WAVE && is_key_byte(WAVE + lane);
    bool differ[MRG_GROUP];
#pragma unroll
    for (int g = 0; g < MRG_GROUP; ++g) {
        const int i = first + wave * MRG_GROUP + g;
        differ[g] = true;
        if (i >= n || i == 0) continue;
        const uint8_t* __restrict__ a = states72 + (size_t)perm[i] * STATE72;
        const uint8_t* __restrict__ c = states72 + (size_t)perm[i - 1] * STATE72;
        differ[g] = (key0 && a[lane] != c[lane]) || (key1 && a[WAVE + lane] != c[WAVE + lane]);
    }
#pragma unroll
    for (int g = 0; g < MRG_GROUP; ++g) {
        const int i = first + wave * MRG_GROUP + g;
        if (i >= n) continue;
        const bool any = __any(differ[g]) != 0;
        if (lane == 0) heads[i] = (uint8_t)(any ? 1 : 0);
    }
}

// ---- the merge

// A row of A + 1 summands: A policy values at `p` and the value at `v` (a source row: pi + r A and z + r; a partial row: its A + 1
// floats).  Lane `lane` holds columns lane, 64 + lane, ...; column A (the value) falls into the last pass on every board.
template <int A, int PASSES>
__device__ __forceinline__ void load_row(float (&x)[PASSES], const float* __restrict__ p, const float* __restrict__ v, int lane) {
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        const int j = k * WAVE + lane;
        x[k] = j < A ? p[j] : j == A ? *v : 0.f;
    }
}

// acc += row(from), then row(from + 1), ... row(to - 1), in that order, INFLIGHT rows' loads issued before the first is added
template <int A, int PASSES, int INFLIGHT, class RowAt>
__device__ __forceinline__ void add_rows(float (&acc)[PASSES], int from, int to, int lane, RowAt row_at) {
    for (int k0 = from; k0 < to; k0 += INFLIGHT) {
        float x[INFLIGHT][PASSES];
#pragma unroll
        for (int g = 0; g < INFLIGHT; ++g) {
            if (k0 + g >= to) continue;
            const float* p;
            const float* v;
            row_at(k0 + g, p, v);
            load_row<A, PASSES>(x[g], p, v, lane);
        }
#pragma unroll
        for (int g = 0; g < INFLIGHT; ++g) {
            if (k0 + g >= to) continue;
#pragma unroll
            for (int k = 0; k < PASSES; ++k) acc[k] += x[g][k];
        }
    }
}

__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// acc += source rows perm[from], ..., perm[to - 1] in that order, to - from <= 64 (one chunk): the lanes read the chunk's perm entries
// in ONE coalesced load, so a row's address costs a shuffle and not a dependent load
template <int A, int PASSES>
__device__ __forceinline__ void add_source_rows(float (&acc)[PASSES], const float* __restrict__ pi, const float* __restrict__ z,
                                                const int64_t* __restrict__ perm, int from, int to, int lane) {
    const int64_t mine = from + lane < to ? perm[from + lane] : 0;
    add_rows<A, PASSES, MRG_ADD>(acc, 0, to - from, lane, [&](int i, const float*& p, const float*& v) {
        const size_t r = (size_t)shfl_i64(mine, i);
        p = pi + r * A;
        v = z + r;
    });
}

// workspace row of chunk c of the run that begins at sorted place s
__device__ __forceinline__ size_t partial_row(int s, int c) {
    return 2 * (((size_t)s + (size_t)c * MRG_CHUNK) / MRG_CHUNK) + (c == 0 ? 1 : 0);
}

template <int N>
__global__ __launch_bounds__(MRG_WAVES * WAVE) void merge_chunks_kernel(const float* __restrict__ pi, const float* __restrict__ z,
                                                                       const int64_t* __restrict__ perm,
                                                                       const int64_t* __restrict__ starts, int n, int u,
                                                                       float* __restrict__ partials) {
    constexpr int A = Geo<N>::A;
    constexpr int PASSES = (A + 1 + WAVE - 1) / WAVE;
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * MRG_WAVES + (threadIdx.x >> 6);
    if (w * MRG_CHUNK >= n) return;                             // wave-uniform
    const int W = (int)(w * MRG_CHUNK), Wend = min(W + MRG_CHUNK, n);
    // the run that holds place W: the last o with starts[o] <= W (starts[0] = 0)
    // -- a 64-way search, one probe per lane and round (3 rounds at 200,000 runs, where a bisection is 18 dependent loads): the
    // answer is in [lo, hi); the lanes probe increasing places of (lo, hi), all of them once 64 lanes cover it
    int lo = 0, hi = u;
    for (int it = 0; it < 8 && hi - lo > 1; ++it) {
        const int inside = hi - lo - 1;                         // places lo + 1 .. hi - 1
        const int probes = min(inside, WAVE);
        auto place = [&](int l) { return lo + 1 + (inside <= WAVE ? l : (int)((long long)inside * l / WAVE)); };
        const int below = __popcll(__ballot(lane < probes && (int)starts[place(lane)] <= W));     // starts increases: a prefix of the lanes
        const int new_hi = below < probes ? place(below) : hi;
        if (below > 0) lo = place(below - 1);
        hi = new_hi;
    }
    // lane l looks at run lo + l: the runs that begin inside the window are at most 63 more
    const int o = lo + lane;
    const int s = o < u ? (int)starts[o] : n, e = o + 1 < u ? (int)starts[o + 1] : n;
    const int c = s >= W ? 0 : (W - s + MRG_CHUNK - 1) / MRG_CHUNK;      // the first chunk that begins at or after W
    const int b = s + c * MRG_CHUNK;
    unsigned long long todo = __ballot(o < u && e - s > MRG_CHUNK && b < Wend && b < e);
    for (int it = 0; it < 2 && todo != 0; ++it) {
        const int l = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int rs = __shfl(s, l), re = __shfl(e, l), rc = __shfl(c, l);
        const int from = rs + rc * MRG_CHUNK, to = min(from + MRG_CHUNK, re);
        float acc[PASSES];
        {
            const size_t r = (size_t)perm[from];
            load_row<A, PASSES>(acc, pi + r * A, z + r, lane);
        }
        add_source_rows<A, PASSES>(acc, pi, z, perm, from + 1, to, lane);
        float* __restrict__ out = partials + partial_row(rs, rc) * (A + 1);
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
            const int j = k * WAVE + lane;
            if (j <= A) out[j] = acc[k];
        }
    }
}

template <int N>
__global__ __launch_bounds__(MRG_WAVES * WAVE) void merge_runs_kernel(
        const uint8_t* __restrict__ states72, const float* __restrict__ pi, const float* __restrict__ z,
        const int64_t* __restrict__ perm, const int64_t* __restrict__ starts, int n, int u, uint8_t* __restrict__ out72,
        float* __restrict__ out_pi, float* __restrict__ out_z, int32_t* __restrict__ count, const float* __restrict__ partials) {
    constexpr int A = Geo<N>::A;
    constexpr int PASSES = (A + 1 + WAVE - 1) / WAVE;          // 1, 1, 2, 4 at 3x3 .. 9x9: the value's column fits the last pass
    __shared__ int run_start[MRG_ROWS], run_len[MRG_ROWS];
    __shared__ int64_t run_row[MRG_ROWS];
    const int first = blockIdx.x * MRG_ROWS;                    // < u: the grid is ceil(u / MRG_ROWS)
    const int rows = min(MRG_ROWS, u - first);
    const int t = threadIdx.x;
    if (t < rows) {
        const int o = first + t;
        const int s = (int)starts[o], e = o + 1 < u ? (int)starts[o + 1] : n;
        const int64_t r = perm[s];
        run_start[t] = s;
        run_len[t] = e - s;
        run_row[t] = r;
        count[o] = e - s;
        if (e - s == 1) out_z[o] = z[r];
    }
    __syncthreads();
    const int wave = t >> 6, lane = t & 63;
    const int q0 = wave * MRG_GROUP;
    float pv[MRG_GROUP][PASSES];
    uint8_t sv[MRG_GROUP][2];
#pragma unroll
    for (int g = 0; g < MRG_GROUP; ++g) {
        const int q = q0 + g;
        if (q >= rows) continue;
        const size_t r = (size_t)run_row[q];
        const bool longer = run_len[q] > 1;
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
            const int j = k * WAVE + lane;
            pv[g][k] = j < A ? pi[r * A + j] : (j == A && longer) ? z[r] : 0.f;
        }
        sv[g][0] = states72[r * STATE72 + lane];
        if (lane < STATE72 - WAVE) sv[g][1] = states72[r * STATE72 + WAVE + lane];
    }
#pragma unroll
    for (int g = 0; g < MRG_GROUP; ++g) {
        const int q = q0 + g;
        if (q >= rows) continue;
        const size_t o = (size_t)(first + q);
        const int s = run_start[q], len = run_len[q];
        if (len > 1) {                                          // wave-uniform
            if (len <= MRG_CHUNK) {
                add_source_rows<A, PASSES>(pv[g], pi, z, perm, s + 1, s + len, lane);
            } else {
                auto partial = [&](int c, const float*& p, const float*& v) {
                    p = partials + partial_row(s, c) * (A + 1);
                    v = p + A;
                };
                const float* p;
                const float* v;
                partial(0, p, v);
                load_row<A, PASSES>(pv[g], p, v, lane);
                add_rows<A, PASSES, MRG_ADD>(pv[g], 1, (len + MRG_CHUNK - 1) / MRG_CHUNK, lane, partial);
            }
            const float by = (float)len;
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                pv[g][k] = pv[g][k] / by;
                if (k * WAVE + lane == A) out_z[o] = pv[g][k];
            }
        }
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
            const int j = k * WAVE + lane;
            if (j < A) out_pi[o * A + j] = pv[g][k];
        }
        out72[o * STATE72 + lane] = sv[g][0];
        if (lane < STATE72 - WAVE) out72[o * STATE72 + WAVE + lane] = sv[g][1];
    }
}

}  // namespace

int launch_replay_position_keys(const uint8_t* states72, const int64_t* index, int n, int64_t* keys, hipStream_t st) {
    if (n < 0) return fail("aqg_replay_position_keys: negative row count");
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at
    if (!states72 || !keys) return fail("aqg_replay_position_keys: states72 and keys must be given");
    // of a gathered source only one row is certain (its row count is no argument), as in aqg_augment_gather
    if (overlap(keys, (size_t)n * sizeof(int64_t), states72, (index ? (size_t)1 : (size_t)n) * STATE72) ||
        overlap(keys, (size_t)n * sizeof(int64_t), index, (size_t)n * sizeof(int64_t)))
        return fail("aqg_replay_position_keys: keys overlaps a source");
    hipLaunchKernelGGL(position_keys_kernel, dim3((unsigned)(((size_t)n + MRG_ROWS - 1) / MRG_ROWS)), dim3(MRG_WAVES * WAVE), 0, st,
                       states72, index, n, keys);
    return check_launch("position_keys_kernel");
}

int launch_replay_run_heads(const uint8_t* states72, const int64_t* perm, int n, uint8_t* heads, hipStream_t st) {
    if (n < 0) return fail("aqg_replay_run_heads: negative row count");
    if (n == 0) return 0;
    if (!states72 || !perm || !heads) return fail("aqg_replay_run_heads: states72, perm and heads must be given");
    if (overlap(heads, (size_t)n, states72, STATE72) || overlap(heads, (size_t)n, perm, (size_t)n * sizeof(int64_t)))
        return fail("aqg_replay_run_heads: heads overlaps a source");
    hipLaunchKernelGGL(run_heads_kernel, dim3((unsigned)(((size_t)n + MRG_ROWS - 1) / MRG_ROWS)), dim3(MRG_WAVES * WAVE), 0, st,
                       states72, perm, n, heads);
    return check_launch("run_heads_kernel");
}

size_t replay_merge_workspace_floats(int N, int n, int u) {
    if (!board_size_supported(N) || n < 0 || u < 0 || u > n || n - u < MRG_CHUNK) return 0;    // no run longer than one chunk
    const size_t A = (size_t)action_count(N);
    return 2 * (((size_t)n + MRG_CHUNK - 1) / MRG_CHUNK) * (A + 1);
}

int launch_replay_merge_runs(int N, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* perm,
                             const int64_t* starts, int n, int u, uint8_t* out72, float* out_pi, float* out_z, int32_t* count,
                             float* workspace, size_t workspace_floats, hipStream_t st) {
    if (!board_size_supported(N)) return fail("aqg_replay_merge_runs: unsupported board_size (odd 3..9)");
    const int A = action_count(N);
    if (policy_size != A) return fail("aqg_replay_merge_runs: policy_size is not the board's action count N^2 + 2 (N - 1)^2");
    if (n < 0 || u < 0) return fail("aqg_replay_merge_runs: negative row count");
    if (u > n) return fail("aqg_replay_merge_runs: more runs than rows (u > n)");
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at (an empty array's may be NULL)
    if (u == 0) return fail("aqg_replay_merge_runs: rows without a run (u == 0 with n > 0)");
    if (!states72 || !pi || !z || !perm || !starts || !out72 || !out_pi || !out_z || !count)
        return fail("aqg_replay_merge_runs: the three sources, perm, starts and the four outputs must be given");
    const size_t need = replay_merge_workspace_floats(N, n, u);
    if (need > 0 && (!workspace || workspace_floats < need))
        return fail("aqg_replay_merge_runs: workspace too small (aqg_replay_merge_workspace_floats)");
    // the outputs have u rows, the workspace `need` floats; of a gathered source one row is certain, perm has n entries, starts u
    const void* outs[5] = {out72, out_pi, out_z, count, need ? workspace : nullptr};
    const size_t out_bytes[5] = {(size_t)u * STATE72, (size_t)u * A * sizeof(float), (size_t)u * sizeof(float),
                                 (size_t)u * sizeof(int32_t), need * sizeof(float)};
    const void* srcs[5] = {states72, pi, z, perm, starts};
    const size_t src_bytes[5] = {STATE72, (size_t)A * sizeof(float), sizeof(float), (size_t)n * sizeof(int64_t),
                                 (size_t)u * sizeof(int64_t)};
    for (int o = 0; o < 5; ++o)
        for (int i = 0; i < 5; ++i)
            if (overlap(outs[o], out_bytes[o], srcs[i], src_bytes[i])) return fail("aqg_replay_merge_runs: an output overlaps a source");
    for (int o = 0; o < 5; ++o)
        for (int i = o + 1; i < 5; ++i)
            if (overlap(outs[o], out_bytes[o], outs[i], out_bytes[i])) return fail("aqg_replay_merge_runs: two outputs overlap");
    const dim3 block(MRG_WAVES * WAVE);
    return for_board_size(N, [&](auto nn) {
        if (need > 0) {
            const size_t windows = ((size_t)n + MRG_CHUNK - 1) / MRG_CHUNK;
            hipLaunchKernelGGL(merge_chunks_kernel<decltype(nn)::value>, dim3((unsigned)((windows + MRG_WAVES - 1) / MRG_WAVES)), block, 0,
                               st, pi, z, perm, starts, n, u, workspace);
            if (int r = check_launch("merge_chunks_kernel")) return r;
        }
        hipLaunchKernelGGL(merge_runs_kernel<decltype(nn)::value>, dim3((unsigned)(((size_t)u + MRG_ROWS - 1) / MRG_ROWS)), block, 0, st,
                           states72, pi, z, perm, starts, n, u, out72, out_pi, out_z, count, workspace);
        return check_launch("merge_runs_kernel");
    });
}

}  // namespace aqg
