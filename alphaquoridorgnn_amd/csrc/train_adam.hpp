// train_adam.hpp -- torch.optim.Adam.step() (no amsgrad) as the three trainers' finish kernels apply it: the fused
// 6/128/3 step (gcn_train_final.hip), the any-shape GNN (gcn_train_general.hip) and the CNN (cnn_train.hip).  Each kernel keeps its
// own way from a thread to (tensor, element); the step's scalars, the element update and the batch means of the loss terms are here.
//
// The optimiser controls (struct aqg_optim, include/aqgnn.h; all off by default) sit in front of that update, in torch's order:
//   1. clip    torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2): norm = the L2 norm of EVERY gradient element (the
//              per-workgroup partial sums of squares of grad_norm.hip, added up by optim_prologue in the prologue of each
//              workgroup of the finish kernel -- the launch-boundary reduce: no combine launch, no host read),
//              coef = min(1, max_norm / (norm + 1e-6)) in f32 and g <- coef g.  Nothing clipped: coef is exactly 1.0f and the
//              product exact.  A non-finite norm gets no special treatment (torch's error_if_nonfinite=False): a NaN norm gives a
//              NaN coefficient (the minimum is taken as torch.clamp takes it) and with it NaN moments and parameters.
//   2. decay   one coefficient per tensor (0 = none).  Coupled, torch.optim.Adam(weight_decay=wd): g <- g + wd p before the
//              moments.  Decoupled, torch.optim.AdamW: p <- p (1 - lr wd), then the unchanged Adam update on that p.
//   3. adam_moments / adam_param, unchanged.
// Steps 1 and 2 are optim_apply(), written once; a finish kernel calls it only in its second instantiation (OptimArgs<T> beside its
// arguments), so the plain kernels stay the code they were.
// The fused 6/128/3 step clips differently (gcn_train.hip final_optim): hipcc contracts the update's multiply-adds differently in
// train_final_kernel's two instantiations (and differently per unrolled element inside one), so a clip that changes nothing could
// not be bit-identical to the plain step through the second instantiation.  Its clip therefore scales the stored gradients in place
// (grad_clip_scale_kernel, grad_norm.hip: skipped when the coefficient is exactly 1) in front of the PLAIN update-only launch, and
// leaves the clipped gradient in grads, as clip_grad_norm_ leaves it in .grad; the other two trainers leave grads as computed.
//
// AdamStep, LossMeans and OptimStep sit inside each kernel's by-value argument block.  A kernel whose block also holds the pointer to a
// device table (cnn_adam_kernel) hands a LOCAL COPY to the functions below: a reference into the block itself makes hipcc 7.2 read the
// table's pointers as generic ones (flat_ loads and stores instead of global_ ones).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace aqg {

struct AdamStep { float lr, beta1, beta2, eps, bc1, bc2_sqrt; };

// bias corrections of step `step` (1-based) in f64, as torch computes them on the host
inline AdamStep adam_step(float lr, float beta1, float beta2, float eps, int step) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    return AdamStep{lr, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2)};
}

// One element, in two halves with the caller's stores of the moments in between (the order the kernels have always had):
//   const AdamMoments n = adam_moments(a, grad, old_m, old_v);  m[e] = n.m; v[e] = n.v;  p[e] = adam_param(a, old_p, n);
struct AdamMoments { float m, v; };
__device__ __forceinline__ AdamMoments adam_moments(const AdamStep& a, float gr, float om, float ov) {
    const float mi = a.beta1 * om + (1.f - a.beta1) * gr;          // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = a.beta2 * ov + (1.f - a.beta2) * gr * gr;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    return AdamMoments{mi, vi};
}
__device__ __forceinline__ float adam_param(const AdamStep& a, float op, const AdamMoments& n) {
    const float denom = sqrtf(n.v) / a.bc2_sqrt + a.eps;
    return op - (a.lr / a.bc1) * (n.m / denom);
}

// ---- optimiser controls
// Stage 1 of the norm (grad_norm.hip) leaves P <= GN_MAX_PARTIALS sums of squares.  partials_total adds them in an order fixed by P
// alone: slot t < 256 adds partials t, t + 256, ... in index order (at most 64 additions), the 64 slots of a wave are added by a
// butterfly (6), the four wave sums pairwise (2).  With stage 1's 18 additions per term that is at most 90 additions on any term's
// way to the total (the bound asked of the norm is 128: relative error <= 129 u / (1 - 129 u), u = 2^-24, of a sum of squares).
// Called by every thread of a workgroup of >= 256 threads (whole waves); `red` = 4 floats of LDS; every thread gets the same total.
constexpr int GN_SLOTS = 256;
constexpr int GN_MAX_PARTIALS = 64 * GN_SLOTS;
__device__ __forceinline__ float partials_total(const float* part, int P, float* red) {
    const int t = threadIdx.x;
    if (t < GN_SLOTS) {                                      // waves 0..3, whole
        float s = 0.f;
        for (int k = t; k < P; k += GN_SLOTS) s += part[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((t & 63) == 0) red[t >> 6] = s;
    }
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// min(1, max_norm / (norm + 1e-6)) as torch.clamp(max=1) takes the minimum (a NaN stays a NaN); max_norm 0 = clipping off
__device__ __host__ __forceinline__ float clip_coef(float norm, float max_norm) {
    if (!(max_norm > 0.f)) return 1.f;
    const float c = max_norm / (norm + 1e-6f);
    return c > 1.f ? 1.f : c;
}

// the scalars of a step's controls; the per-tensor decay coefficients follow in OptimArgs<T> (T = the kernel's tensor capacity)
struct OptimStep {
    const float* partials; int P;     // stage 1's sums of squares; P = 0: no norm this launch (coef = 1)
    float max_norm;                   // 0 = no clipping (the norm may still be wanted)
    int decoupled;
    float* norm_out;                  // optional: workgroup 0 stores the norm
};
template <int T> struct OptimArgs { OptimStep s; float wd[T]; };

// Host side.  OptimPlan: a step entry point's checked aqg_optim (grad_norm.hip check_optim) with the flat gradient buffer it found.
// OptimLaunch: what one finish launch gets of it (optim_before_finish: stage 1 enqueued, or P = 0 when no norm is wanted).
struct OptimPlan {
    const float* wd; int decoupled; float max_norm;      // wd: HOST array, one coefficient per tensor, or null
    float* norm_out;                                     // device, element 0 of the call's grad_norm, or null
    float* partials; const float* flat; size_t n;        // stage 1's output and input
    bool norm() const { return max_norm > 0.f || norm_out; }
};
struct OptimLaunch { OptimStep s; const float* wd; };
inline void fill_optim(const OptimLaunch& l, int tensors, OptimStep* s, float* wd) {
    *s = l.s;
    for (int i = 0; i < tensors; ++i) wd[i] = l.wd ? l.wd[i] : 0.f;
}

// the prologue of every workgroup of a finish kernel's <true> form: the clip coefficient of this step (1 when no norm was taken)
__device__ __forceinline__ float optim_prologue(const OptimStep& o, float* red) {
    if (o.P <= 0) return 1.f;                                // uniform over the launch
    const float norm = sqrtf(partials_total(o.partials, o.P, red));
    if (o.norm_out && blockIdx.x == 0 && threadIdx.x == 0) *o.norm_out = norm;
    return clip_coef(norm, o.max_norm);
}

// (g, p) -> the (g', p') that adam_moments / adam_param then take
struct GradParam { float g, p; };
__device__ __forceinline__ GradParam optim_apply(float coef, float wd, int decoupled, float lr, float g, float p) {
#pragma clang fp contract(off)       // every product and sum rounded, as train_network.adam_reference states them
    g = coef * g;
    if (wd != 0.f) {
        if (decoupled) p = p * (1.f - lr * wd);
        else g = g + wd * p;
    }
    return GradParam{g, p};
}

// The workgroup behind the last element's, in the any-shape and CNN finish kernels: the two batch means of the per-position loss
// terms loss[2 b + e], summed in position order -> loss_mean[e], added to loss_sums[e]; either of the two may be null.
struct LossMeans { const float* loss; float* loss_mean; float* loss_sums; };
__device__ __forceinline__ void loss_means(const LossMeans& l, int B) {
    if (threadIdx.x < 2) {
        const int e = threadIdx.x;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += l.loss[2 * b + e];
        const float mean = s / (float)B;
        if (l.loss_mean) l.loss_mean[e] = mean;
        if (l.loss_sums) l.loss_sums[e] += mean;
    }
}

}  // namespace aqg
