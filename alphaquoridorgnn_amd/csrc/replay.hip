// replay.hip -- replay window: one generation of training rows appended to a ring that stays on the device, in ONE launch
// (include/aqgnn.h, "replay window").  Source row i goes to ring slot (head + i) % capacity; a generation straight from the engine
// (counts form: u16 visit counts, i8 z) is converted on the way to the f32 targets the trainers read, a finished one (rows form) is
// copied.
//
// A bandwidth-bound converting copy, ~2A + 73 bytes in and 4A + 76 bytes out per row (491 + 912 at 9x9).  The geometry is
// augment.hip's: a workgroup owns RPL_ROWS = 16 consecutive SOURCE rows, its first lanes copy z one lane per row, then every one of the
// RPL_WAVES = 4 wavefronts takes RPL_GROUP = 4 rows whole, all four rows' loads in flight before the first store.  A row's total is
// the wave reduction of the lanes' integer partial sums (at most 209 * 65,535 < 2^24); pi_j = f32(v_j) / f32(tot) is the correctly
// rounded f32 division, which has the bits of f32(f64(v_j) / f64(tot)) for every tot < 2^24 -- so this unit must never be built with
// a fast-math flag.  The 72 record bytes are copied verbatim: no byte is interpreted or used as an address.  No atomics, no scratch;
// every loop ends on n.
//
// Blended value target (aqg_replay_append_blend; template switch BLEND of the one kernel, counts form only): the lanes that write
// ring_z also load the row's search value v and write keep * f32(z) + blend * v, keep = 1 - blend -- two f32 products and one f32
// sum, each rounded, which is why this unit is compiled without fma contraction.  BLEND = false is the plain kernel, instruction
// for instruction.
//
// Policy form (aqg_replay_append_policy; aqgnn.h, "recording completed-Q targets during self-play"): the engine's f32 policy rows with
// its i8 outcomes -- pi of the rows form, z of the counts form, selected by which pointers are given: the row is copied verbatim as
// the rows form copies it, and the lanes that write ring_z convert z_i8 (whichever of z_i8 / z_f32 is given is the one read).  BLEND
// applies as in the counts form.  No further instantiation.
//
// Loads of the counts: per-row 16-bit loads, one count per lane and pass.  The other candidate -- the workgroup's 16 rows read as ONE
// 32A-byte span with 16-byte loads and staged through LDS -- was timed beside this one on an MI355X (tools/replay_window_time.py with
// ALT_LIB; profiles/replay_window.log, where it is the "ALT_LIB" line): 62.6 against 67.4 us at 163,840 rows of 9x9 (-7 %), inside
// the spread at 4,000 rows and at 1,000 rows of 5x5.  It is NOT the one kept: its 16-bit tail and its path for an array that is not
// 16-byte aligned have not been through the bit-for-bit tests on the GPU, and this form has, at every edge.
#include "aqg_common.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"

#ifdef __FAST_MATH__
#error "replay.hip: pi = v / tot must be the correctly rounded f32 division (no fast-math)"
#endif
// the blend must be evaluated exactly as written: x = keep * z, y = blend * v, x + y (replay.blend_targets is the same in numpy)
#pragma clang fp contract(off)

namespace aqg {

constexpr int RPL_WAVES = 4;
constexpr int RPL_GROUP = 4;    // rows a wavefront loads before it stores any (rows per wavefront group)
constexpr int RPL_ROWS = RPL_WAVES * RPL_GROUP;     // source rows of one workgroup

template <int N, bool BLEND>
__global__ __launch_bounds__(RPL_WAVES * WAVE) void replay_append_kernel(
        const uint8_t* __restrict__ states72, const uint16_t* __restrict__ visits, const int8_t* __restrict__ z_i8,
        const float* __restrict__ pi, const float* __restrict__ z_f32, int n, int capacity, int head,
        uint8_t* __restrict__ ring72, float* __restrict__ ring_pi, float* __restrict__ ring_z,
        const float* __restrict__ search_value, float blend) {
    constexpr int A = Geo<N>::A;
    constexpr int PI_PASSES = (A + WAVE - 1) / WAVE;           // 1, 1, 2, 4 at 3x3 .. 9x9
    const int first = blockIdx.x * RPL_ROWS;                    // < n: the grid is ceil(n / RPL_ROWS)
    const int rows = min(RPL_ROWS, n - first);
    const int t = threadIdx.x;
    // head < capacity and first + q < n <= capacity: one conditional subtraction is the modulo
    auto slot_of = [&](int q) -> size_t {
        const size_t s = (size_t)head + (size_t)(first + q);
        return s >= (size_t)capacity ? s - (size_t)capacity : s;
    };
    if (t < rows) {
        float zt = z_i8 ? (float)z_i8[first + t] : z_f32[first + t];
        if (BLEND) {
            const float keep = 1.0f - blend;
            const float x = keep * zt, y = blend * search_value[first + t];
            zt = x + y;
        }
        ring_z[slot_of(t)] = zt;
    }
    const int wave = t >> 6, lane = t & 63;
    for (int q0 = wave * RPL_GROUP; q0 < rows; q0 += RPL_WAVES * RPL_GROUP) {
        uint32_t pv[RPL_GROUP][PI_PASSES];      // a count, or the bits of a finished f32
        uint8_t sv[RPL_GROUP][2];
#pragma unroll
        for (int g = 0; g < RPL_GROUP; ++g) {
            const int q = q0 + g;
            if (q >= rows) continue;
            const size_t r = (size_t)(first + q);
#pragma unroll
            for (int p = 0; p < PI_PASSES; ++p) {
                const int j = p * WAVE + lane;
                pv[g][p] = j >= A ? 0u : visits ? (uint32_t)visits[r * A + j] : __float_as_uint(pi[r * A + j]);
            }
            sv[g][0] = states72[r * STATE72 + lane];
            if (lane < STATE72 - WAVE) sv[g][1] = states72[r * STATE72 + WAVE + lane];
        }
#pragma unroll
        for (int g = 0; g < RPL_GROUP; ++g) {
            const int q = q0 + g;
            if (q >= rows) continue;                            // wave-uniform: the reduction below runs on whole wavefronts
            const size_t i = slot_of(q);
            float tot = 0.f;
            if (visits) {
                int part = 0;
#pragma unroll
                for (int p = 0; p < PI_PASSES; ++p) part += (int)pv[g][p];
                tot = (float)wave_xor_sum(part);                // exact: < 2^24
            }
#pragma unroll
            for (int p = 0; p < PI_PASSES; ++p) {
                const int j = p * WAVE + lane;
                if (j >= A) continue;
                const float x = !visits ? __uint_as_float(pv[g][p]) : tot > 0.f ? (float)pv[g][p] / tot : 0.f;
                ring_pi[i * A + j] = x;
            }
            ring72[i * STATE72 + lane] = sv[g][0];
            if (lane < STATE72 - WAVE) ring72[i * STATE72 + WAVE + lane] = sv[g][1];
        }
    }
}

int launch_replay_append(int N, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8, const float* pi,
                         const float* z_f32, int n, int capacity, int head, uint8_t* ring72, float* ring_pi, float* ring_z,
                         hipStream_t st, const float* search_value, float blend, bool policy_form) {
    if (!board_size_supported(N)) return fail("aqg_replay_append: unsupported board_size (odd 3..9)");
    const int A = action_count(N);
    if (policy_size != A) return fail("aqg_replay_append: policy_size is not the board's action count N^2 + 2 (N - 1)^2");
    if (n < 0) return fail("aqg_replay_append: negative row count");
    if (capacity < 1) return fail("aqg_replay_append: capacity must be >= 1");
    if (head < 0 || head >= capacity) return fail("aqg_replay_append: head must be a slot of the ring, 0 <= head < capacity");
    if (n > capacity) return fail("aqg_replay_append: more rows than the ring holds (n > capacity)");
    if (n == 0) return 0;                   // nothing to write: the pointers are not looked at (an empty array's may be NULL)
    const bool counts = visits && z_i8 && !pi && !z_f32, finished = pi && z_f32 && !visits && !z_i8;
    if (policy_form) {                      // aqg_replay_append_policy: f32 rows with i8 outcomes, and nothing else
        if (!pi || !z_i8 || visits || z_f32) return fail("aqg_replay_append_policy: pi and z_i8 must be given");
    } else if (!counts && !finished)
        return fail("aqg_replay_append: give the counts form (visits, z_i8) or the rows form (pi, z_f32), whole, and not both");
    if (!states72 || !ring72 || !ring_pi || !ring_z) return fail("aqg_replay_append: states72 and the three rings must be given");
    const size_t ring_bytes[3] = {STATE72, (size_t)A * sizeof(float), sizeof(float)};
    const void* rings[3] = {ring72, ring_pi, ring_z};
    const void* srcs[3] = {states72, counts ? (const void*)visits : (const void*)pi, z_i8 ? (const void*)z_i8 : (const void*)z_f32};
    const size_t src_bytes[3] = {STATE72, counts ? (size_t)A * sizeof(uint16_t) : (size_t)A * sizeof(float),
                                 z_i8 ? sizeof(int8_t) : sizeof(float)};
    for (int o = 0; o < 3; ++o)
        for (int i = 0; i < 3; ++i)
            if (overlap(rings[o], (size_t)capacity * ring_bytes[o], srcs[i], (size_t)n * src_bytes[i]))
                return fail("aqg_replay_append: a ring overlaps a source");
    for (int o = 0; o < 3; ++o)
        if (overlap(rings[o], (size_t)capacity * ring_bytes[o], search_value, (size_t)n * sizeof(float)))
            return fail("aqg_replay_append_blend: a ring overlaps search_value");
    const dim3 grid((unsigned)(((size_t)n + RPL_ROWS - 1) / RPL_ROWS)), block(RPL_WAVES * WAVE);
    return for_board_size(N, [&](auto nn) {
        if (search_value)
            hipLaunchKernelGGL((replay_append_kernel<decltype(nn)::value, true>), grid, block, 0, st, states72, visits, z_i8, pi, z_f32, n,
                               capacity, head, ring72, ring_pi, ring_z, search_value, blend);
        else
            hipLaunchKernelGGL((replay_append_kernel<decltype(nn)::value, false>), grid, block, 0, st, states72, visits, z_i8, pi, z_f32, n,
                               capacity, head, ring72, ring_pi, ring_z, nullptr, 0.f);
        return check_launch("replay_append_kernel");
    });
}

// the counts form with a blended value target: what it refuses of its own, then aqg_replay_append's checks and launch
int launch_replay_append_blend(int N, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8,
                               const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                               float* ring_z, hipStream_t st) {
    if (!(blend >= 0.f && blend <= 1.f)) return fail("aqg_replay_append_blend: blend must be in [0, 1]");      // NaN fails both
    if (!search_value && n != 0) return fail("aqg_replay_append_blend: search_value must be given");      // n == 0: no pointer is looked at
    return launch_replay_append(N, policy_size, states72, visits, z_i8, nullptr, nullptr, n, capacity, head, ring72, ring_pi, ring_z, st,
                                search_value, blend);
}

// the policy form: what it refuses of its own, then aqg_replay_append's checks and launch
int launch_replay_append_policy(int N, int policy_size, const uint8_t* states72, const float* pi, const int8_t* z_i8,
                                const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                                float* ring_z, hipStream_t st) {
    if (!(blend >= 0.f && blend <= 1.f)) return fail("aqg_replay_append_policy: blend must be in [0, 1]");      // NaN fails both
    if (!search_value && blend != 0.f && n != 0) return fail("aqg_replay_append_policy: a blend needs search_value");      // n == 0: no pointer is looked at
    return launch_replay_append(N, policy_size, states72, nullptr, z_i8, pi, nullptr, n, capacity, head, ring72, ring_pi, ring_z, st,
                                search_value, blend, true);
}

}  // namespace aqg
