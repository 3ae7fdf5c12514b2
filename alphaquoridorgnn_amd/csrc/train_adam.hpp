// train_adam.hpp -- torch.optim.Adam.step() (no weight decay, no amsgrad) as the three trainers' finish kernels apply it: the fused
// 6/128/3 step (gcn_train_final.hip), the any-shape GNN (gcn_train_general.hip) and the CNN (cnn_train.hip).  Each kernel keeps its
// own way from a thread to (tensor, element); the step's scalars, the element update and the batch means of the loss terms are here.
//
// AdamStep and LossMeans sit inside each kernel's by-value argument block.  A kernel whose block also holds the pointer to a device
// table (cnn_adam_kernel) hands a LOCAL COPY to the functions below: a reference into the block itself makes hipcc 7.2 read the
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
