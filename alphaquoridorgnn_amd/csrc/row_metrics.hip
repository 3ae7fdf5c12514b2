// row_metrics.hip -- held-out validation: what a network scores on rows no update trains on (include/aqgnn.h, "row metrics").  Three
// entries: the metrics of every row of a chunk, their deterministic reduction per ply bucket, and the split of rows by position.
//
// aqg_replay_row_metrics: for one chunk of n rows whose network outputs the caller has just computed (net_policy [n, A], net_value
// [n], row i of the chunk), against the ring's targets of row index[offset + i] (index NULL: row offset + i): vals[offset + i] = {ce,
// ent, lp, se} in float64 and tag[offset + i] = bucket | hit << 8 | sign counted << 9 | sign agrees << 10.  The geometry is
// replay_surprise_rows_kernel's: a workgroup owns RM_ROWS = 16 consecutive rows of the chunk, every one of its RM_WAVES = 4 wavefronts
// takes RM_GROUP = 4 rows whole, the four ring rows first, then all the rows' loads of both arrays, of the two values and of the two
// ply bytes in flight before the first use.  No LDS, no atomics, no workgroup barrier, no scratch; every loop is bounded by a constant
// and every row by n.
//
// Every sum is float64, evaluated exactly as written (no contraction), in the FIXED order replay.row_metrics_reference repeats: lane l
// adds its own entries a = l, l + 64, ... in ascending order to +0.0 (an entry that adds nothing adds +0.0, which changes no bit: an
// accumulator that starts at +0.0 is never -0.0), then the xor-shuffle wave reduction 32, 16, ..., 1.  Five sums a row: S_ce = sum
// t ln max(p, 2^-126) and S_ent = sum t ln t over t > 0, S_t = sum t, S_e = sum exp(p), S_tp = sum t p over all A entries;
// ce = 0 - S_ce, ent = 0 - S_ent, lp = S_t ln(S_e) - S_tp.  The first maximum of p is a wave_xor_max of the value and then the least
// index among the entries that hold it.  The row predicates are pure and made wave-uniform by ballot; a rejected row, and a row whose
// index entry is outside the ring (it is then not read), stores zeros and the tag `buckets`.
//
// aqg_row_metrics_reduce: two launches in the manner of grad_norm.hip, no atomics.  One: workgroup (c, b) of 256 lanes takes the RMR_CHUNK
// = 4,096 rows of chunk c; lane l adds the rows l, l + 256, ... in ascending order whose tag names bucket b (4 float64 sums from +0.0, 4
// integer counts), each goes through wave_xor_sum, the four wave results are added in wave order ((w0 + w1) + w2) + w3 through LDS, and
// partial[c][b] = 4 doubles and 4 int64 is stored.  Two: one wavefront per bucket adds the chunk partials lane, lane + 64, ... ascending
// to +0.0, then wave_xor_sum.  Every loop ends at an argument (m, or the chunk count derived from it on the host).
//
// aqg_replay_holdout_mask: mask[i] = counter_uniform(stream_key(seed, AQG_HOLDOUT_STREAM), (uint64)keys[i]) < share, one lane per row.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "counter_rng.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"
#include <cfloat>
#include <climits>
#include <cmath>

#ifdef __FAST_MATH__
#error "row_metrics.hip: the float64 sums, their logarithms and exponentials must be the IEEE ones (no fast-math)"
#endif
// t * ln p, acc + term, S_t * ln S_e - S_tp, (v - z) * (v - z): every operation rounded on its own (replay.row_metrics_reference is the
// same in numpy)
#pragma clang fp contract(off)

namespace aqg {

constexpr int RM_WAVES = 4;
constexpr int RM_GROUP = 4;     // rows a wavefront loads before it uses any
constexpr int RM_ROWS = RM_WAVES * RM_GROUP;        // rows of one workgroup
constexpr int RM_MAX_ROWS = 1 << 24;       // m at most
constexpr int RM_MAX_BUCKETS = 64;
constexpr float RM_TINY = 0x1.0p-126f;     // the least p a logarithm is taken of
constexpr int RMR_LANES = 256;
constexpr int RMR_CHUNK = 4096;            // rows of one workgroup column of the reduction's first launch
constexpr int RMR_WORDS = 8;               // 8-byte words of one partial: 4 float64 sums, 4 int64 counts
constexpr int HM_LANES = 256;

template <int N>
__global__ __launch_bounds__(RM_WAVES * WAVE) void replay_row_metrics_kernel(
        const float* __restrict__ net_policy, const float* __restrict__ net_value, const uint8_t* __restrict__ states72,
        const float* __restrict__ ring_pi, const float* __restrict__ ring_z, const int64_t* __restrict__ index, int rows, int offset, int n,
        int bucket_plies, int buckets, double* __restrict__ vals, int32_t* __restrict__ tag) {
    constexpr int A = Geo<N>::A;
    constexpr int PASSES = (A + WAVE - 1) / WAVE;              // 1, 1, 2, 4 at 3x3 .. 9x9
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = blockIdx.x * RM_ROWS + wave * RM_GROUP;          // this wavefront's first row of the chunk
    int64_t r[RM_GROUP];
    float t[RM_GROUP][PASSES], p[RM_GROUP][PASSES], v[RM_GROUP], z[RM_GROUP];
    int ply[RM_GROUP];
    // ---- the ring rows of the group, then every load, none waiting for another
#pragma unroll
    for (int g = 0; g < RM_GROUP; ++g) {
        const int i = first + g;
        r[g] = i >= n ? (int64_t)-1 : index ? index[(size_t)offset + i] : (int64_t)offset + i;      // wave-uniform
    }
#pragma unroll
    for (int g = 0; g < RM_GROUP; ++g) {
        const bool live = r[g] >= 0 && r[g] < (int64_t)rows;           // first + g < n, and a row the ring has
#pragma unroll
        for (int s = 0; s < PASSES; ++s) {
            const int a = s * WAVE + lane;
            const bool in = live && a < A;
            t[g][s] = in ? ring_pi[(size_t)r[g] * A + a] : 0.f;        // past the row: neither negative, nor positive, nor non-finite
            p[g][s] = in ? net_policy[(size_t)(first + g) * A + a] : 0.f;
        }
        v[g] = live ? net_value[first + g] : 0.f;                      // the same address in every lane
        z[g] = live ? ring_z[r[g]] : 0.f;
        ply[g] = live ? (int)states72[(size_t)r[g] * 72 + 68] | (int)states72[(size_t)r[g] * 72 + 69] << 8 : 0;
    }
#pragma unroll
    for (int g = 0; g < RM_GROUP; ++g) {
        if (first + g >= n) continue;                                   // wave-uniform: the reductions below run on whole wavefronts
        bool bad = false, some = false;
        double a_ce = 0.0, a_ent = 0.0, a_t = 0.0, a_e = 0.0, a_tp = 0.0;
        float pmax = -INFINITY, tmax = -INFINITY;
#pragma unroll
        for (int s = 0; s < PASSES; ++s) {
            const float tt = t[g][s], pp = p[g][s];
            const bool in = s * WAVE + lane < A;
            bad = bad || !(tt >= 0.f && tt <= FLT_MAX) || !(fabsf(pp) <= FLT_MAX);       // negative, infinite or NaN
            some = some || tt > 0.f;
            if (tt > 0.f) {
                const float pc = pp > RM_TINY ? pp : RM_TINY;
                const double td = (double)tt;
                const double c = td * log((double)pc);
                const double e = td * log(td);
                a_ce = a_ce + c;
                a_ent = a_ent + e;
            }
            if (in) {
                const double td = (double)tt, pd = (double)pp;
                const double tp = td * pd;
                a_t = a_t + td;
                a_e = a_e + exp(pd);
                a_tp = a_tp + tp;
                pmax = fmaxf(pmax, pp);
                tmax = fmaxf(tmax, tt);
            }
        }
        const double s_ce = wave_xor_sum(a_ce), s_ent = wave_xor_sum(a_ent), s_t = wave_xor_sum(a_t), s_e = wave_xor_sum(a_e),
                     s_tp = wave_xor_sum(a_tp);
        pmax = wave_xor_max(pmax);
        tmax = wave_xor_max(tmax);
        int least = INT_MAX;                                            // the first maximum of p: the least index that holds it
#pragma unroll
        for (int s = PASSES - 1; s >= 0; --s)
            if (s * WAVE + lane < A && p[g][s] == pmax) least = s * WAVE + lane;
        least = -wave_xor_max(-least);
        float t_at = -INFINITY;                                         // the target at that index
#pragma unroll
        for (int s = 0; s < PASSES; ++s)
            if (s * WAVE + lane == least) t_at = t[g][s];
        t_at = wave_xor_max(t_at);
        const float vv = v[g], zz = z[g];
        const bool finite = fabsf(vv) <= FLT_MAX && fabsf(zz) <= FLT_MAX;
        const bool ok = r[g] >= 0 && r[g] < (int64_t)rows && __ballot(bad) == 0 && __ballot(some) != 0 && finite;
        if (lane == 0) {
            double* out = vals + ((size_t)offset + first + g) * 4;
            int32_t word = buckets;
            if (ok) {
                const double d = (double)vv - (double)zz;
                const double lse = log(s_e);
                const double lp = s_t * lse;
                out[0] = 0.0 - s_ce;
                out[1] = 0.0 - s_ent;
                out[2] = lp - s_tp;
                out[3] = d * d;
                const int b = ply[g] / bucket_plies;
                const double prod = (double)vv * (double)zz;
                word = (b < buckets - 1 ? b : buckets - 1) | (t_at == tmax ? 1 << 8 : 0) | (zz != 0.f ? 1 << 9 : 0) |
                       (zz != 0.f && prod > 0.0 ? 1 << 10 : 0);
            } else {
                out[0] = 0.0;
                out[1] = 0.0;
                out[2] = 0.0;
                out[3] = 0.0;
            }
            tag[(size_t)offset + first + g] = word;
        }
    }
}

// grid (chunks, buckets + 1): partial[(c * (buckets + 1) + b) * 8 ..] = {4 float64 sums, 4 int64 counts (as 8-byte words)}
__global__ __launch_bounds__(RMR_LANES) void row_metrics_partial_kernel(const double* __restrict__ vals, const int32_t* __restrict__ tag,
                                                                          int m, double* __restrict__ partial) {
    __shared__ double red_sum[RMR_LANES / WAVE][4];
    __shared__ long long red_cnt[RMR_LANES / WAVE][4];
    const int lane = threadIdx.x, b = blockIdx.y;
    const long long base = (long long)blockIdx.x * RMR_CHUNK;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int k = 0; k < RMR_CHUNK / RMR_LANES; ++k) {
        const long long row = base + (long long)k * RMR_LANES + lane;
        if (row >= m) break;
        const int32_t w = tag[row];
        if ((w & 255) != b) continue;
        const double* x = vals + (size_t)row * 4;
        s0 = s0 + x[0];
        s1 = s1 + x[1];
        s2 = s2 + x[2];
        s3 = s3 + x[3];
        c0 += 1;
        c1 += (w >> 8) & 1;
        c2 += (w >> 9) & 1;
        c3 += (w >> 10) & 1;
    }
    s0 = wave_xor_sum(s0), s1 = wave_xor_sum(s1), s2 = wave_xor_sum(s2), s3 = wave_xor_sum(s3);
    c0 = wave_xor_sum(c0), c1 = wave_xor_sum(c1), c2 = wave_xor_sum(c2), c3 = wave_xor_sum(c3);
    if ((lane & 63) == 0) {
        const int w = lane >> 6;
        red_sum[w][0] = s0, red_sum[w][1] = s1, red_sum[w][2] = s2, red_sum[w][3] = s3;
        red_cnt[w][0] = c0, red_cnt[w][1] = c1, red_cnt[w][2] = c2, red_cnt[w][3] = c3;
    }
    __syncthreads();
    if (lane < 4) {
        double* out = partial + ((size_t)blockIdx.x * gridDim.y + b) * RMR_WORDS;
        out[lane] = ((red_sum[0][lane] + red_sum[1][lane]) + red_sum[2][lane]) + red_sum[3][lane];
        reinterpret_cast<long long*>(out)[4 + lane] = ((red_cnt[0][lane] + red_cnt[1][lane]) + red_cnt[2][lane]) + red_cnt[3][lane];
    }
}

// grid buckets + 1, one wavefront each
__global__ __launch_bounds__(WAVE) void row_metrics_total_kernel(const double* __restrict__ partial, int chunks, double* __restrict__ sums,
                                                                  long long* __restrict__ counts) {
    const int lane = threadIdx.x, b = blockIdx.x, nb = gridDim.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    long long c[4] = {0, 0, 0, 0};
    for (int k = lane; k < chunks; k += WAVE) {
        const double* x = partial + ((size_t)k * nb + b) * RMR_WORDS;
        const long long* y = reinterpret_cast<const long long*>(x) + 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = s[j] + x[j];
            c[j] += y[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j] = wave_xor_sum(s[j]);
        c[j] = wave_xor_sum(c[j]);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sums[(size_t)b * 4 + j] = s[j];
            counts[(size_t)b * 4 + j] = c[j];
        }
    }
}

__global__ __launch_bounds__(HM_LANES) void replay_holdout_mask_kernel(const int64_t* __restrict__ keys, int n, uint64_t key, double share,
                                                                       uint8_t* __restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * HM_LANES + threadIdx.x;
    if (i >= (size_t)n) return;
    mask[i] = counter_uniform(key, (uint64_t)keys[i]) < share ? 1 : 0;
}

int launch_replay_row_metrics(int N, int policy_size, const float* net_policy, const float* net_value, const uint8_t* states72,
                              const float* ring_pi, const float* ring_z, const int64_t* index, int rows, int m, int offset, int n,
                              int bucket_plies, int buckets, double* vals, int32_t* tag, hipStream_t st) {
    const char* what = "aqg_replay_row_metrics";
    if (!board_size_supported(N)) return fail(what, "unsupported board_size (odd 3..9)");
    const int A = action_count(N);
    if (policy_size != A) return fail(what, "policy_size is not the board's action count N^2 + 2 (N - 1)^2");
    if (m < 0 || m > RM_MAX_ROWS) return fail(what, "m out of range (0 .. 2^24 rows)");
    if (rows < 0) return fail(what, "negative row count of the ring");
    if (!index && m > rows) return fail(what, "m out of range (without an index, m <= rows)");
    if (offset < 0 || n < 0 || n > m - offset) return fail(what, "the chunk is not inside the m rows (0 <= offset, 0 <= n, offset + n <= m)");
    if (buckets < 1 || buckets > RM_MAX_BUCKETS) return fail(what, "buckets must be in 1 .. 64");
    if (bucket_plies < 1) return fail(what, "bucket_plies must be >= 1");
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at
    if (!net_policy || !net_value || !states72 || !ring_pi || !ring_z || !vals || !tag)
        return fail(what, "net_policy, net_value, states72, ring_pi, ring_z, vals and tag must be given");
    const size_t ring = index ? 1 : (size_t)rows;      // of a gathered ring one row is assumed, as aqg_augment_gather does
    const void* outs[2] = {vals, tag};
    const size_t out_bytes[2] = {(size_t)m * 4 * sizeof(double), (size_t)m * sizeof(int32_t)};
    const void* srcs[6] = {net_policy, net_value, states72, ring_pi, ring_z, index};
    const size_t src_bytes[6] = {(size_t)n * A * sizeof(float), (size_t)n * sizeof(float), ring * 72, ring * A * sizeof(float),
                                 ring * sizeof(float), (size_t)m * sizeof(int64_t)};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 6; ++i)
            if (overlap(outs[o], out_bytes[o], srcs[i], src_bytes[i])) return fail(what, "an output overlaps a source");
    if (overlap(vals, out_bytes[0], tag, out_bytes[1])) return fail(what, "vals overlaps tag");
    const dim3 grid((unsigned)(((size_t)n + RM_ROWS - 1) / RM_ROWS)), block(RM_WAVES * WAVE);
    return for_board_size(N, [&](auto nn) {
        hipLaunchKernelGGL((replay_row_metrics_kernel<decltype(nn)::value>), grid, block, 0, st, net_policy, net_value, states72, ring_pi,
                           ring_z, index, rows, offset, n, bucket_plies, buckets, vals, tag);
        return check_launch("replay_row_metrics_kernel");
    });
}

// doubles of workspace for m rows in `buckets` buckets; 0 = nothing to reduce (m == 0) or an argument out of range
size_t row_metrics_workspace_doubles(int m, int buckets) {
    if (m < 1 || m > RM_MAX_ROWS || buckets < 1 || buckets > RM_MAX_BUCKETS) return 0;
    return (size_t)((m + RMR_CHUNK - 1) / RMR_CHUNK) * (buckets + 1) * RMR_WORDS;
}

int launch_row_metrics_reduce(const double* vals, const int32_t* tag, int m, int buckets, double* partial, double* sums,
                              long long* counts, hipStream_t st) {
    const char* what = "aqg_row_metrics_reduce";
    if (m < 0 || m > RM_MAX_ROWS) return fail(what, "m out of range (0 .. 2^24 rows)");
    if (buckets < 1 || buckets > RM_MAX_BUCKETS) return fail(what, "buckets must be in 1 .. 64");
    if (!sums || !counts) return fail(what, "sums and counts must be given");
    if (m > 0 && (!vals || !tag || !partial)) return fail(what, "vals, tag and partial must be given");
    const size_t table = (size_t)(buckets + 1) * 4 * 8, work = row_metrics_workspace_doubles(m, buckets) * sizeof(double);
    const void* outs[3] = {sums, counts, m > 0 ? partial : nullptr};
    const size_t out_bytes[3] = {table, table, work};
    for (int o = 0; o < 3; ++o) {
        if (m > 0 && (overlap(outs[o], out_bytes[o], vals, (size_t)m * 4 * sizeof(double)) ||
                      overlap(outs[o], out_bytes[o], tag, (size_t)m * sizeof(int32_t))))
            return fail(what, "an output overlaps a source");
        for (int u = o + 1; u < 3; ++u)
            if (overlap(outs[o], out_bytes[o], outs[u], out_bytes[u])) return fail(what, "two outputs overlap");
    }
    const int chunks = (m + RMR_CHUNK - 1) / RMR_CHUNK;
    if (chunks > 0) {
        hipLaunchKernelGGL(row_metrics_partial_kernel, dim3((unsigned)chunks, (unsigned)(buckets + 1)), dim3(RMR_LANES), 0, st, vals, tag, m,
                           partial);
        if (int rc = check_launch("row_metrics_partial_kernel")) return rc;
    }
    hipLaunchKernelGGL(row_metrics_total_kernel, dim3((unsigned)(buckets + 1)), dim3(WAVE), 0, st, partial, chunks, sums, counts);
    return check_launch("row_metrics_total_kernel");
}

int launch_replay_holdout_mask(const int64_t* keys, int n, uint64_t seed, double share, uint8_t* mask, hipStream_t st) {
    const char* what = "aqg_replay_holdout_mask";
    if (n < 0) return fail(what, "negative row count");
    if (!(share > 0.0 && share < 1.0)) return fail(what, "share must be in (0, 1)");          // NaN fails both
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at
    if (!keys || !mask) return fail(what, "keys and mask must be given");
    if (overlap(mask, (size_t)n, keys, (size_t)n * sizeof(int64_t))) return fail(what, "mask overlaps keys");
    hipLaunchKernelGGL(replay_holdout_mask_kernel, dim3((unsigned)(((size_t)n + HM_LANES - 1) / HM_LANES)), dim3(HM_LANES), 0, st, keys, n,
                       stream_key(seed, AQG_HOLDOUT_STREAM), share, mask);
    return check_launch("replay_holdout_mask_kernel");
}

}  // namespace aqg
