// replay_refresh.hip -- replay window: the targets of chosen ring slots overwritten by fresh search results, in ONE launch
// (include/aqgnn.h, "reanalyse").  Source row i is a searched root as aqg_engine_root_visits leaves it -- visit counts and action
// ids in legal_actions() order, and their number -- and goes to ring slot slots[i]: the dense policy row pi[a_j] = f32(v_j) / f32(tot),
// zero elsewhere, and (BLEND) the value target keep * ring_z[slot] + blend * search_value[i].  The record bytes of the ring are not an
// argument: they cannot be touched.
//
// The geometry is replay.hip's: a workgroup owns RFR_ROWS = 16 consecutive SOURCE rows, every one of its RFR_WAVES = 4 wavefronts
// takes RFR_GROUP = 4 rows whole, all four rows' loads (3 lane rounds of counts and of action bytes, the count, the slot) in flight
// before the first store.  The loads do not wait for the count: [n, MAX_LEGAL] is read whole and masked by it afterwards.  A row's
// total is the wave reduction of the lanes' integer partial sums over j < count (exact: visit totals stay below 2^24, the caller's
// part -- selfplay_options.check_tree_reuse caps the simulations); pi is the correctly rounded f32 division, which has the bits of
// f32(f64(v_j) / f64(tot)) for every tot < 2^24 -- so this unit must never be built with a fast-math flag.
//
// Legal order -> dense row: through LDS, one [PI_PASSES * 64] f32 row per (wavefront, row of its group), 16 KB at 9x9.  The wavefront
// zeroes its rows, scatters the quotients at the action ids (an id >= A is dropped; ids of one row are distinct, so no two lanes
// write one word), and reads the rows back lane-contiguous: each output row is then stored ONCE, 64 consecutive floats per store, no
// global address is written twice and nothing is atomic.  A row belongs to one wavefront, so the three phases are ordered by
// wavefront-scope fences and wave barriers that every lane reaches (they stand outside the per-row branches); the kernel has no
// workgroup barrier.  A skipped row (count <= 0 or > MAX_LEGAL, total <= 0, slot outside the ring) writes nothing; the decision is
// uniform over its wavefront.  No input byte is used as an address unguarded: the slot is compared with the capacity, the action
// id with A.  Every loop is bounded by a constant.
#include "aqg_common.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"
#include <cfloat>

#ifdef __FAST_MATH__
#error "replay_refresh.hip: pi = v / tot must be the correctly rounded f32 division (no fast-math)"
#endif
// the blend must be evaluated exactly as written: x = keep * z, y = blend * v, x + y (replay.refresh_reference is the same in numpy)
#pragma clang fp contract(off)

namespace aqg {

constexpr int RFR_WAVES = 4;
constexpr int RFR_GROUP = 4;    // rows a wavefront loads before it stores any
constexpr int RFR_ROWS = RFR_WAVES * RFR_GROUP;     // source rows of one workgroup
constexpr int RFR_SRC_PASSES = (MAX_LEGAL + WAVE - 1) / WAVE;      // 3 lane rounds cover a legal list

// POLICY (aqg_replay_refresh_policy; aqgnn.h, "completed-Q policy targets"): the source words are f32 policy entries, not counts -- they
// arrive through the same loads as their bits and are copied VERBATIM to their action ids: no total, no division.  A row is written
// iff every entry j < count is finite and >= 0 and one is > 0 -- pure predicates, wave-uniform by ballot, so no order is involved.
template <int N, bool BLEND, bool POLICY>
__global__ __launch_bounds__(RFR_WAVES * WAVE) void replay_refresh_kernel(
        const int32_t* __restrict__ visits, const uint8_t* __restrict__ actions, const int32_t* __restrict__ count,
        const float* __restrict__ search_value, float blend, const int64_t* __restrict__ slots, int n, int capacity,
        float* __restrict__ ring_pi, float* __restrict__ ring_z) {
    constexpr int A = Geo<N>::A;
    constexpr int PI_PASSES = (A + WAVE - 1) / WAVE;           // 1, 1, 2, 4 at 3x3 .. 9x9
    static_assert(A <= 256, "an action id is a byte");
    __shared__ float stage[RFR_WAVES][RFR_GROUP][PI_PASSES * WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t first = (size_t)blockIdx.x * RFR_ROWS + (size_t)wave * RFR_GROUP;     // this wavefront's first source row
    int32_t v[RFR_GROUP][RFR_SRC_PASSES];
    uint32_t a[RFR_GROUP][RFR_SRC_PASSES];
    int c[RFR_GROUP];
    int64_t s[RFR_GROUP];
    float q[RFR_GROUP];
    // ---- every load of the group's rows, none waiting for another
#pragma unroll
    for (int g = 0; g < RFR_GROUP; ++g) {
        const size_t r = first + g;
        const bool live = r < (size_t)n;                        // wave-uniform
        c[g] = live ? count[r] : 0;
        s[g] = live ? slots[r] : (int64_t)-1;
        if (BLEND) q[g] = live ? search_value[r] : 0.f;
#pragma unroll
        for (int p = 0; p < RFR_SRC_PASSES; ++p) {
            const int j = p * WAVE + lane;
            const bool in = live && j < MAX_LEGAL;
            v[g][p] = in ? visits[r * MAX_LEGAL + j] : 0;
            a[g][p] = in ? (uint32_t)actions[r * MAX_LEGAL + j] : 0xFFu;
        }
    }
    // ---- which rows are written, and their totals (wave-uniform)
    bool ok[RFR_GROUP];
    float tot[RFR_GROUP];
#pragma unroll
    for (int g = 0; g < RFR_GROUP; ++g) {
        if constexpr (POLICY) {
            bool bad = false, some = false;
#pragma unroll
            for (int p = 0; p < RFR_SRC_PASSES; ++p) {
                if (p * WAVE + lane >= c[g]) v[g][p] = 0;       // past the count: +0.0f
                const float f = __int_as_float(v[g][p]);
                bad = bad || !(f >= 0.f && f <= FLT_MAX);       // negative, infinite or NaN
                some = some || f > 0.f;
            }
            ok[g] = c[g] > 0 && c[g] <= MAX_LEGAL && __ballot(bad) == 0 && __ballot(some) != 0 && s[g] >= 0 && s[g] < (int64_t)capacity;
            tot[g] = 1.f;                                       // not used
        } else {
            int part = 0;
#pragma unroll
            for (int p = 0; p < RFR_SRC_PASSES; ++p) {
                if (p * WAVE + lane >= c[g]) v[g][p] = 0;       // past the count (and every entry of a row with count <= 0)
                part += v[g][p];
            }
            const int t = wave_xor_sum(part);
            ok[g] = c[g] > 0 && c[g] <= MAX_LEGAL && t > 0 && s[g] >= 0 && s[g] < (int64_t)capacity;
            tot[g] = (float)t;                                  // exact: < 2^24
        }
    }
    // ---- the dense rows in LDS: zeros, then the quotients at their action ids
#pragma unroll
    for (int g = 0; g < RFR_GROUP; ++g)
#pragma unroll
        for (int p = 0; p < PI_PASSES; ++p) stage[wave][g][p * WAVE + lane] = 0.f;
    wave_lds_sync();
#pragma unroll
    for (int g = 0; g < RFR_GROUP; ++g) {
        if (!ok[g]) continue;
#pragma unroll
        for (int p = 0; p < RFR_SRC_PASSES; ++p) {
            const int j = p * WAVE + lane;
            if (j < c[g] && a[g][p] < (uint32_t)A) stage[wave][g][a[g][p]] = POLICY ? __int_as_float(v[g][p]) : (float)v[g][p] / tot[g];
        }
    }
    wave_lds_sync();
    // ---- each row stored once, lane-contiguous; the value target by the row's first lane
#pragma unroll
    for (int g = 0; g < RFR_GROUP; ++g) {
        if (!ok[g]) continue;
        const size_t i = (size_t)s[g];                          // 0 <= i < capacity
#pragma unroll
        for (int p = 0; p < PI_PASSES; ++p) {
            const int j = p * WAVE + lane;
            if (j < A) ring_pi[i * A + j] = stage[wave][g][j];
        }
        if (BLEND && lane == 0) {
            const float keep = 1.0f - blend;
            const float x = keep * ring_z[i], y = blend * q[g];
            ring_z[i] = x + y;
        }
    }
}

// both forms of the launch behind one set of checks: `rows` is visits (i32) or, POLICY, the f32 policy rows read through the same loads
template <bool POLICY>
static int refresh_launch(int N, int policy_size, const int32_t* rows, const uint8_t* actions, const int32_t* count,
                          const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                          float* ring_z, hipStream_t st) {
    const char* what = POLICY ? "aqg_replay_refresh_policy" : "aqg_replay_refresh";
    if (!board_size_supported(N)) return fail(what, "unsupported board_size (odd 3..9)");
    const int A = action_count(N);
    if (policy_size != A) return fail(what, "policy_size is not the board's action count N^2 + 2 (N - 1)^2");
    if (n < 0) return fail(what, "negative row count");
    if (capacity < 1) return fail(what, "capacity must be >= 1");
    if (!(blend >= 0.f && blend <= 1.f)) return fail(what, "blend must be in [0, 1]");      // NaN fails both
    if (blend != 0.f && !search_value) return fail(what, "a blend needs search_value");
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at
    const bool blended = search_value && blend != 0.f;
    if (!rows || !actions || !count || !slots || !ring_pi)
        return fail(what, POLICY ? "policy, actions, count, slots and ring_pi must be given" : "visits, actions, count, slots and ring_pi must be given");
    if (blended && !ring_z) return fail(what, "a blend needs ring_z");
    const void* rings[2] = {ring_pi, blended ? ring_z : nullptr};
    const size_t ring_bytes[2] = {(size_t)A * sizeof(float), sizeof(float)};
    const void* srcs[5] = {rows, actions, count, slots, blended ? search_value : nullptr};
    const size_t src_bytes[5] = {(size_t)MAX_LEGAL * sizeof(int32_t), (size_t)MAX_LEGAL, sizeof(int32_t), sizeof(int64_t), sizeof(float)};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 5; ++i)
            if (overlap(rings[o], (size_t)capacity * ring_bytes[o], srcs[i], (size_t)n * src_bytes[i]))
                return fail(what, "a ring overlaps a source");
    if (overlap(rings[0], (size_t)capacity * ring_bytes[0], rings[1], (size_t)capacity * ring_bytes[1]))
        return fail(what, "ring_pi overlaps ring_z");
    const dim3 grid((unsigned)(((size_t)n + RFR_ROWS - 1) / RFR_ROWS)), block(RFR_WAVES * WAVE);
    return for_board_size(N, [&](auto nn) {
        if (blended)
            hipLaunchKernelGGL((replay_refresh_kernel<decltype(nn)::value, true, POLICY>), grid, block, 0, st, rows, actions, count,
                               search_value, blend, slots, n, capacity, ring_pi, ring_z);
        else
            hipLaunchKernelGGL((replay_refresh_kernel<decltype(nn)::value, false, POLICY>), grid, block, 0, st, rows, actions, count, nullptr,
                               0.f, slots, n, capacity, ring_pi, nullptr);
        return check_launch("replay_refresh_kernel");
    });
}

int launch_replay_refresh(int N, int policy_size, const int32_t* visits, const uint8_t* actions, const int32_t* count,
                          const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                          float* ring_z, hipStream_t st) {
    return refresh_launch<false>(N, policy_size, visits, actions, count, search_value, blend, slots, n, capacity, ring_pi, ring_z, st);
}

static_assert(sizeof(float) == sizeof(int32_t), "a policy row is read through the loads of a visit row");
int launch_replay_refresh_policy(int N, int policy_size, const float* policy, const uint8_t* actions, const int32_t* count,
                                 const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                                 float* ring_z, hipStream_t st) {
    return refresh_launch<true>(N, policy_size, reinterpret_cast<const int32_t*>(policy), actions, count, search_value, blend, slots, n,
                                capacity, ring_pi, ring_z, st);
}

}  // namespace aqg
