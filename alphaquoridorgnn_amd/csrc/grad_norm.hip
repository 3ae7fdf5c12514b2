// grad_norm.hip -- the L2 norm of a flat f32 buffer, deterministic and without a host read: what global-norm gradient clipping
// (train_adam.hpp, struct aqg_optim in include/aqgnn.h) needs between "gradients complete" and "Adam reads them".
//
//   stage 1   grad_sumsq_kernel: workgroup b squares and adds chunk b of GN_CHUNK = 8,192 floats and stores ONE partial with a plain
//             store.  The chunks are cut on the 16-byte grid the base sits in: with `mis` = the floats between that grid and the base
//             (0..3), chunk b holds the grid's floats [b C, (b + 1) C) and element j of the buffer is float mis + j of the grid.  Lane t
//             takes the 16-byte words t, t + 256, ... of its chunk: eight loads issued before the first is used (32 KB in flight per
//             workgroup).  A word that lies wholly inside the buffer is one 16-byte load; the first and last words of the buffer are
//             read float by float, each load guarded by the range, so nothing outside [base, base + n) is read and any 4-byte-aligned
//             base and any n >= 1 work.  There is no loop over memory at all: 8 unrolled words per lane, P = ceil((mis + n) / C)
//             workgroups.
//   combine   partials_total (train_adam.hpp) in the prologue of EVERY workgroup of the finish kernel that applies the clip -- the
//             launch-boundary reduce: no third launch, no atomics, no grid-wide wait.  The stand-alone aqg_grad_norm and a mode-0 step
//             (norm wanted, nothing to update) run it as grad_norm_combine_kernel, one workgroup.
//
// Summation order: fixed by (n, C) and mis alone (a torch tensor's storage is 16-byte aligned: mis = 0 for every trainer).  Depth: a
// term passes through at most 8 additions in its lane's vector component, 2 across the components, 6 across the wave, 2 across
// the four waves = 18 in stage 1, and at most 64 + 6 + 2 = 72 in the combine: 90 <= 128.  No float atomics anywhere.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "train_adam.hpp"
#include <cmath>

namespace aqg {

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_WORDS = 8;                                   // 16-byte words per lane
constexpr int GN_CHUNK = GN_THREADS * GN_WORDS * 4;           // floats per workgroup
typedef float gn_f32x4 __attribute__((ext_vector_type(4)));

// aligned = base - mis (16-byte aligned; never dereferenced outside [base, base + n)); nv = mis + n
__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_kernel(const float* aligned, int mis, long long nv, float* partials) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    const long long w0 = (long long)blockIdx.x * (GN_CHUNK / 4) + t;      // this lane's first word
    gn_f32x4 x[GN_WORDS];
#pragma unroll
    for (int k = 0; k < GN_WORDS; ++k) {
        const long long f = (w0 + (long long)k * GN_THREADS) * 4;         // first float of the word, on the grid
        if (f >= mis && f + 4 <= nv) {
            x[k] = *reinterpret_cast<const gn_f32x4*>(aligned + f);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) x[k][c] = (f + c >= mis && f + c < nv) ? aligned[f + c] : 0.f;
        }
    }
    gn_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < GN_WORDS; ++k) acc += x[k] * x[k];
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(GN_SLOTS) void grad_norm_combine_kernel(const float* partials, int P, float* out) {
    __shared__ float red[4];
    const float total = partials_total(partials, P, red);
    if (threadIdx.x == 0) *out = sqrtf(total);
}

// The fused 6/128/3 step's clip (gcn_train.hip final_optim, train_adam.hpp): every workgroup adds up the partials, derives the
// coefficient and, unless it is exactly 1, scales its 1,024 stored gradient elements in place; workgroup 0 stores the norm.
__global__ __launch_bounds__(GN_SLOTS) void grad_clip_scale_kernel(float* g, long long n, OptimStep o) {
    __shared__ float red[4];
    const float coef = optim_prologue(o, red);
    if (coef == 1.f) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = (long long)blockIdx.x * (4 * GN_SLOTS) + k * GN_SLOTS + threadIdx.x;
        if (i < n) g[i] = coef * g[i];
    }
}

inline int mis_of(const float* x) { return (int)(((uintptr_t)x >> 2) & 3); }
inline long long partials_of(const float* x, size_t n) { return ((long long)n + mis_of(x) + GN_CHUNK - 1) / GN_CHUNK; }

int launch_sumsq(const float* x, size_t n, float* partials, hipStream_t st) {
    const int mis = mis_of(x);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)partials_of(x, n)), dim3(GN_THREADS), 0, st, x - mis, mis, (long long)n + mis,
                       partials);
    return check_launch("grad_sumsq_kernel");
}

}  // namespace

// floats of workspace for a buffer of n floats at any 4-byte-aligned base; 0 = n is 0 or beyond what two combining levels take
size_t optim_workspace_floats(size_t n) {
    if (n < 1 || n > (size_t)GN_MAX_PARTIALS * GN_CHUNK - 3) return 0;
    return (n + 3 + GN_CHUNK - 1) / GN_CHUNK;
}

int launch_grad_norm(const float* x, size_t n, float* out, float* workspace, size_t workspace_floats, hipStream_t st) {
    const char* what = "aqg_grad_norm";
    if (!x || !out || !workspace) return fail(what, "null argument");
    if (((uintptr_t)x & 3) != 0) return fail(what, "x must be 4-byte aligned");
    const size_t need = optim_workspace_floats(n);
    if (need == 0) return fail(what, "n must be 1 .. 134,217,725");
    if (workspace_floats < need) return fail(what, "workspace too small (aqg_optim_workspace_floats)");
    if (int r = launch_sumsq(x, n, workspace, st)) return r;
    hipLaunchKernelGGL(grad_norm_combine_kernel, dim3(1), dim3(GN_SLOTS), 0, st, workspace, (int)partials_of(x, n), out);
    return check_launch("grad_norm_combine_kernel");
}

int check_optim(const aqg_optim* o, int tensors, const size_t* numel, float* const* grads, const char* what, OptimPlan* plan,
                bool* on) {
    *on = false;
    if (!o) return 0;
    bool decay = false;
    if (o->weight_decay) {
        if (o->num_tensors != tensors) return fail(what, "aqg_optim.num_tensors is not the trainer's tensor count");
        for (int i = 0; i < tensors; ++i) {
            if (!std::isfinite(o->weight_decay[i]) || o->weight_decay[i] < 0.f) return fail(what, "weight decay must be finite and >= 0");
            decay = decay || o->weight_decay[i] != 0.f;
        }
    }
    if (!std::isfinite(o->max_grad_norm) || o->max_grad_norm < 0.f) return fail(what, "max_grad_norm must be finite and >= 0");
    const bool norm = o->max_grad_norm > 0.f || o->grad_norm;
    if (!decay && !norm) return 0;
    size_t n = 0;
    for (int i = 0; i < tensors; ++i) n += numel[i];
    if (norm) {
        for (int i = 0; i + 1 < tensors; ++i)
            if (grads[i + 1] != grads[i] + numel[i])
                return fail(what, "the gradient norm needs the gradient tensors consecutive in one flat buffer");
        const size_t need = optim_workspace_floats(n);
        if (need == 0 || !o->workspace || o->workspace_floats < need)
            return fail(what, "aqg_optim.workspace too small (aqg_optim_workspace_floats)");
    }
    *plan = OptimPlan{decay ? o->weight_decay : nullptr, o->decoupled ? 1 : 0, o->max_grad_norm, o->grad_norm, o->workspace, grads[0], n};
    *on = true;
    return 0;
}

int optim_before_finish(const OptimPlan& plan, int step_index, OptimLaunch* ol, hipStream_t st) {
    *ol = OptimLaunch{OptimStep{nullptr, 0, plan.max_norm, plan.decoupled, nullptr}, plan.wd};
    if (!plan.norm()) return 0;
    if (int r = launch_sumsq(plan.flat, plan.n, plan.partials, st)) return r;
    ol->s.partials = plan.partials;
    ol->s.P = (int)partials_of(plan.flat, plan.n);
    ol->s.norm_out = plan.norm_out ? plan.norm_out + step_index : nullptr;
    return 0;
}

int launch_clip_scale(const OptimPlan& plan, const OptimLaunch& ol, hipStream_t st) {
    hipLaunchKernelGGL(grad_clip_scale_kernel, dim3((unsigned)((plan.n + 4 * GN_SLOTS - 1) / (4 * GN_SLOTS))), dim3(GN_SLOTS), 0, st,
                       const_cast<float*>(plan.flat), (long long)plan.n, ol.s);
    return check_launch("grad_clip_scale_kernel");
}

int optim_norm_only(const OptimPlan& plan, hipStream_t st) {
    if (!plan.norm_out) return 0;
    return launch_grad_norm(plan.flat, plan.n, plan.norm_out, plan.partials, optim_workspace_floats(plan.n), st);
}

}  // namespace aqg
