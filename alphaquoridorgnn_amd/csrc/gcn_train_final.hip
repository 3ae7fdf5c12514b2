// gcn_train_final.hip -- train_final_kernel: the second launch of the fused training step.  Sums the per-board partials of the board
// launch in a fixed order, writes every gradient and applies Adam (train_adam.hpp) to that element.
#define AQG_TRAIN_TU final
#include "gcn_train_common.hpp"
#include "train_adam.hpp"
#include <type_traits>

namespace aqg {

// ---------------------------------------------------------------------------------------------
// gradient of every parameter element + its Adam update.   One thread per element of the 14 tensors.
// parameter order = state_dict order (KEYS in INTEGRATION.md):
//  0 gcn0.w [H,F]  1 gcn0.b  2 gcn1.w [H,H]  3 gcn1.b  4 gcn2.w  5 gcn2.b
//  6 pol0.w [H/2,H]  7 pol0.b  8 pol2.w [A,H/2]  9 pol2.b  10 val0.w [H/2,H]  11 val0.b  12 val2.w [1,H/2]  13 val2.b
// torch.optim.Adam.step() by train_adam.hpp.
// ---------------------------------------------------------------------------------------------
struct FinalJobs {
    float* p[14]; float* g[14]; float* m[14]; float* v[14];
    unsigned int end[14];                        // running element count after tensor i
    const float* part_dW[3]; const float* part_db[3];
    const float *dlg, *dvp, *hp, *hv, *dhp, *dhv, *gp, *loss;
    float* loss_sums;                            // optional: += the two batch-mean losses (elements end[13], end[13] + 1)
    int B, A, compute, update;
    AdamStep adam;
};
// (the old state is fetched by adam_fetch() BEFORE the gradient's own loads: one memory round trip per workgroup instead of two)
struct AdamOld { float m, v, p; };
__device__ __forceinline__ AdamOld adam_fetch(const FinalJobs& jb, int i, unsigned int e) { return AdamOld{jb.m[i][e], jb.v[i][e], jb.p[i][e]}; }
__device__ __forceinline__ void adam_update(const FinalJobs& jb, int i, unsigned int e, float gr, const AdamOld& o) {
    const AdamMoments n = adam_moments(jb.adam, gr, o.m, o.v);
    jb.m[i][e] = n.m; jb.v[i][e] = n.v;
    jb.p[i][e] = adam_param(jb.adam, o.p, n);
}
// the same with the optimiser controls in front (train_adam.hpp): the argument block of the kernel's second instantiation
struct FinalOptimJobs : FinalJobs { OptimArgs<14> op; };
template <class Jobs>
__device__ __forceinline__ void adam_update(const Jobs& jb, float coef, int i, unsigned int e, float gr, const AdamOld& o) {
    if constexpr (std::is_same_v<Jobs, FinalOptimJobs>) {
        const GradParam gp = optim_apply(coef, jb.op.wd[i], jb.op.s.decoupled, jb.adam.lr, gr, o.p);
        adam_update(jb, i, e, gp.g, AdamOld{o.m, o.v, gp.p});
    } else {
        adam_update(jb, i, e, gr, o);
    }
}
// A team = 32 lanes x FINAL_GROUPS board groups: a thread sums its group's boards in order, the group sums are added pairwise in
// group order -- a fixed summation order with FINAL_GROUPS x the loads in flight of one thread per element.  The first
// FINAL_BIG_BLOCKS teams ("rows") take the two [128,128] trunk weights four elements per lane (16-byte loads of the 16 MB of
// per-board partials); the rest take every other tensor one element per lane (end[] counts those tensors only).  A workgroup =
// FINAL_TEAMS teams = 1,024 threads.
constexpr int FINAL_BIG_BLOCKS = 2 * TH * TH / 128;
constexpr int FINAL_GROUPS = 4;     // board groups per element: a thread sums B / groups boards (4 / 8 / 16 groups: 0.0467 / 0.0473 / 0.0527 ms per step)
constexpr int FINAL_TEAM_THREADS = 32 * FINAL_GROUPS;
constexpr int FINAL_TEAMS = 1024 / FINAL_TEAM_THREADS;
// Two instantiations: <FinalJobs>, the step as it has always been (the same instructions and registers as before the template), and
// <FinalOptimJobs>: every workgroup first adds up the norm's partials and derives the clip coefficient, and every update goes through
// optim_apply.
template <class Jobs>
__global__ __launch_bounds__(FINAL_TEAM_THREADS * FINAL_TEAMS) void train_final_kernel(Jobs jb) {
    __shared__ f32x4 red4s[FINAL_TEAMS][FINAL_GROUPS][33];
    float coef = 1.f;
    if constexpr (std::is_same_v<Jobs, FinalOptimJobs>) {
        __shared__ float norm_red[4];
        coef = optim_prologue(jb.op.s, norm_red);
    }
    TS_DECL
    const int team = threadIdx.x / FINAL_TEAM_THREADS, tt = threadIdx.x % FINAL_TEAM_THREADS;
    const unsigned int row = blockIdx.x * FINAL_TEAMS + team;
    f32x4 (*red4)[33] = red4s[team];
    const int le = tt & 31, grp = tt >> 5;
    const int B = jb.B, A = jb.A;
    const int per = (B + FINAL_GROUPS - 1) / FINAL_GROUPS, b0 = grp * per, b1 = min(B, b0 + per);
    if (row < FINAL_BIG_BLOCKS) {
        const unsigned int q4 = row * 32 + le;                    // float4 index over gcn1.w then gcn2.w
        const int i = q4 < TH * TH / 4 ? 2 : 4;
        const unsigned int e = (q4 & (TH * TH / 4 - 1)) * 4;
        f32x4 gr4;
        AdamOld old[4];
        if (jb.update && grp == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) old[k] = adam_fetch(jb, i, e + k);
        }
        if (jb.compute) {
            const float* src = jb.part_dW[i >> 1] + e;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 16
            for (int b = b0; b < b1; ++b) s += ld4(src + (size_t)b * TH * TH);
            red4[grp][le] = s;
            __syncthreads();
            TS(0, 1)
            if (grp != 0) return;
            gr4 = (red4[0][le] + red4[1][le]) + (red4[2][le] + red4[3][le]);
            st4(jb.g[i] + e, gr4);
        } else {
            if (grp != 0) return;
            gr4 = ld4(jb.g[i] + e);
        }
        if (jb.update) {
#pragma unroll
            for (int k = 0; k < 4; ++k) adam_update(jb, coef, i, e + k, gr4[k], old[k]);
        }
        return;
    }
    float (*red)[33] = reinterpret_cast<float (*)[33]>(&red4[0][0]);
    const unsigned int e0 = (row - FINAL_BIG_BLOCKS) * 32 + le;
    const unsigned int total = jb.end[13] + (jb.loss_sums ? 2u : 0u);
    const bool live = e0 < total;
    int i = 0;
    if (live) while (i < 14 && e0 >= jb.end[i]) ++i;
    const unsigned int e = e0 - (i ? jb.end[i - 1] : 0u);
    TS(0, 0)
    AdamOld old{0.f, 0.f, 0.f};
    if (jb.update && grp == 0 && live && i < 14) old = adam_fetch(jb, i, e);
    if (jb.compute) {
        float s = 0.f;
        if (!live) {
        } else if (i < 6) {
            if (i & 1) {
                const float* src = jb.part_db[i >> 1] + e;
#pragma unroll 16
                for (int b = b0; b < b1; ++b) s += src[(size_t)b * TH];
            } else {
                const float* src = jb.part_dW[0] + e;                                                                      // gcn0.w
#pragma unroll 16
                for (int b = b0; b < b1; ++b) s += src[(size_t)b * TH * TF];
            }
        } else if (i == 6 || i == 10) {
            const int j = e / TH, k = e % TH;
            const float* d = (i == 6 ? jb.dhp : jb.dhv) + j;
            const float* x = jb.gp + k;
#pragma unroll 16
            for (int b = b0; b < b1; ++b) s = fmaf(d[(size_t)b * HH], x[(size_t)b * TH], s);
        } else if (i == 7 || i == 11) {
            const float* d = (i == 7 ? jb.dhp : jb.dhv) + e;
#pragma unroll 16
            for (int b = b0; b < b1; ++b) s += d[(size_t)b * HH];
        } else if (i == 8) {
            const int a = e / HH, j = e % HH;
#pragma unroll 16
            for (int b = b0; b < b1; ++b) s = fmaf(jb.dlg[(size_t)b * A + a], jb.hp[(size_t)b * HH + j], s);
        } else if (i == 9) {
#pragma unroll 16
            for (int b = b0; b < b1; ++b) s += jb.dlg[(size_t)b * A + e];
        } else if (i == 12) {
#pragma unroll 16
            for (int b = b0; b < b1; ++b) s = fmaf(jb.dvp[b], jb.hv[(size_t)b * HH + e], s);
        } else if (i == 13) {
            for (int b = b0; b < b1; ++b) s += jb.dvp[b];
        } else {
            for (int b = b0; b < b1; ++b) s += jb.loss[2 * b + e];
        }
        red[grp][le] = s;
    }
    __syncthreads();
    if (grp != 0 || !live) return;
    float gr;
    if (jb.compute) {
        gr = (red[0][le] + red[1][le]) + (red[2][le] + red[3][le]);
        if (i == 14) { jb.loss_sums[e] += gr / (float)B; return; }
        jb.g[i][e] = gr;
    } else {
        if (i == 14) return;
        gr = jb.g[i][e];
    }
    if (jb.update) adam_update(jb, coef, i, e, gr, old);
}

AQG_TRAIN_STAMP_READER(train_stamps_final)

void train_tensor_sizes(const aqg_train& t, size_t* numel) {
    const int A = t.policy_size;
    const size_t sizes[14] = {(size_t)TH * TF, TH, (size_t)TH * TH, TH, (size_t)TH * TH, TH, (size_t)HH * TH, (size_t)HH, (size_t)A * HH, (size_t)A,
                              (size_t)HH * TH, (size_t)HH, (size_t)HH, 1};
    for (int i = 0; i < 14; ++i) numel[i] = sizes[i];
}

int launch_train_final(const aqg_train& t, int B, bool compute, bool update, int step, float* loss_sums, hipStream_t st,
                       const OptimLaunch* ol) {
    const int A = t.policy_size;
    size_t sizes[14];
    train_tensor_sizes(t, sizes);
    FinalJobs jb{};
    unsigned int run = 0;
    for (int i = 0; i < 14; ++i) {
        jb.p[i] = t.params[i]; jb.g[i] = t.grads[i]; jb.m[i] = t.adam_m[i]; jb.v[i] = t.adam_v[i];
        if (i != 2 && i != 4) run += (unsigned int)sizes[i];      // the two big trunk weights have their own workgroups
        jb.end[i] = run;
    }
    const float* pdW3 = t.part;
    const float* pdW2 = pdW3 + (size_t)B * TH * TH;
    const float* pdW1 = pdW2 + (size_t)B * TH * TH;
    const float* pdb = pdW1 + (size_t)B * TH * TF;
    jb.part_dW[0] = pdW1; jb.part_dW[1] = pdW2; jb.part_dW[2] = pdW3;
    jb.part_db[0] = pdb; jb.part_db[1] = pdb + (size_t)B * TH; jb.part_db[2] = pdb + (size_t)2 * B * TH;
    jb.dlg = t.lg; jb.dvp = t.vp; jb.hp = t.hp; jb.hv = t.hv; jb.dhp = t.dhp; jb.dhv = t.dhv; jb.gp = t.g; jb.loss = t.loss;
    jb.loss_sums = compute ? loss_sums : nullptr;
    jb.B = B; jb.A = A; jb.compute = compute; jb.update = update;
    jb.adam = adam_step(t.lr, t.beta1, t.beta2, t.eps, step);
    const unsigned int rows = FINAL_BIG_BLOCKS + (run + 2 + 31) / 32;
    const dim3 grid((rows + FINAL_TEAMS - 1) / FINAL_TEAMS), blk(FINAL_TEAM_THREADS * FINAL_TEAMS);
    if (ol) {
        FinalOptimJobs jo{};
        static_cast<FinalJobs&>(jo) = jb;
        fill_optim(*ol, 14, &jo.op.s, jo.op.wd);
        hipLaunchKernelGGL(train_final_kernel<FinalOptimJobs>, grid, blk, 0, st, jo);
        return check_launch("train_final_kernel<FinalOptimJobs>");
    }
    hipLaunchKernelGGL(train_final_kernel<FinalJobs>, grid, blk, 0, st, jb);
    return check_launch("train_final_kernel");
}

}  // namespace aqg
