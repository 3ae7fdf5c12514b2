// gcn_train.hip -- one optimisation step of the reference's training loop on the GNN, for gfx950.
//
// train_network.py:68-95 (forward, CrossEntropyLoss on the ALREADY-softmaxed policy + MSELoss on the
// tanh value, backward, Adam) applied to GraphPolicyValueNetwork (pv_network_gnn.py:23-64, GCNConv = PyG defaults).
//
//   forward   Z = H W^T, P = A_hat Z + b, H' = relu(P)   x3;  g = mean_nodes H3;  heads;  pol = softmax, val = tanh
//   loss      Lp = mean_b -sum_a t_a log_softmax(pol)_a   (the reference's double softmax, kept on purpose)
//             Lv = mean_b (val - z)^2
//             (the _loss entry points: the cross-entropy on the logits and a value weight, include/aqgnn.h "loss form")
//   backward  dP = dH' (.) [H' > 0];  db = colsum dP;  dZ = A_hat dP (A_hat symmetric);  dW = dZ^T H;  dH = dZ W
//   update    torch.optim.Adam (lr, betas, eps; bias-corrected; no amsgrad); weight decay and global-norm clipping are options of
//             the _optim entry points (train_adam.hpp, final_optim below), off in every other call
//
// The batch is 128 positions (train_network.py:15) = 10,368 graph nodes and 2.2 GFLOP per step.  Two launches per step:
//
//   board   (position)            forward, heads + losses and backward of one position in one 8-wave workgroup; writes the
//                                 per-board partial gradients.  Two forms (aqg_set_option("train_fused")), both within 2e-5
//                                 max|g| of fp64 autograd:
//     2, split (default on 9x9): train_board_split_kernel -- every contraction on the 16-bit matrix pipe in fp16 hi/lo split
//       precision (split_mfma.hpp; three fp16 products per f32 product, f32 accumulation: fp32-equivalent), the neighbourhood
//       aggregation included (banded A_hat blocks as MFMA operands).  A position whose values leave fp16 range is redone by the
//       f32 body in the same launch (3 = every position sent through that fallback: tests).
//     1, f32: train_board_kernel -- the same structure on the f32-input matrix pipe (v_mfma_f32_16x16x4_f32: exact f32
//       products), aggregation as a VALU gather over LDS; the default on 3x3 / 5x5 / 7x7.
//   final   (parameter element)   sums the per-board partials in a fixed order, forms the head weight gradients as
//                                 batch dot products, writes the gradient and applies Adam to that element
//
// A board's 81 node rows never leave its workgroup (the aggregation needs all of them).  No atomics on any result (only on the
// fallback counter): results are run-to-run identical.
//
// The files (build.sh lists the units; launchers.hpp declares what crosses them):
//   gcn_train_common.hpp   sizes, the small f32x4 helpers, record_of, the marks of the two diagnostic builds
//   gcn_train_heads.hpp    heads_board: the heads, both losses and the head gradients of one position
//   gcn_train_exact.hpp    the exact-f32 board body (a header: the split kernel's fallback inlines it too)
//   gcn_train_exact.hip    train_board_kernel<N> and its launcher
//   gcn_train_split.hip    train_board_split_kernel, heads_board_call, the fallback counter, its launcher
//   gcn_train_final.hip    train_final_kernel and its launcher
//   train_adam.hpp         the Adam element update and its step scalars, shared with gcn_train_general.hip and cnn_train.hip;
//                          the optimiser controls (weight decay, global-norm clipping) in front of it
//   gcn_train.hip          this map; the option, the choice between the two board launchers, train_step, train_steps
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "train_adam.hpp"

namespace aqg {

// aqg_set_option("train_fused"): 2 (default) = contractions in fp16 split precision on the 9x9 board (other boards: as 1);
// 1 = f32-input MFMA;  3 = as 2 with every board sent through the f32 fallback (tests).  capi.hip refuses other values.
int g_train_fused = 2;

static int forward_backward(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first,
                            int B, hipStream_t st, const aqg_loss* lf) {
    if (t.board_size == 9 && g_train_fused >= 2)
        return launch_train_board_split(t, states72, pi, z, order, first, B, g_train_fused == 3 ? 1 : 0, st, lf);
    return launch_train_board_exact(t, states72, pi, z, order, first, B, st, lf);
}

static int validate(const aqg_train& t) {
    const int N = t.board_size, A = t.policy_size;
    if (!board_size_supported(N)) return fail("board_size must be 3, 5, 7 or 9");
    if (A != N * N + 2 * (N - 1) * (N - 1) || A > 256) return fail("policy_size does not match the board");
    return 0;
}

// The final launch(es) of a step with the optimiser controls.  train_final_kernel forms a gradient element and updates it in the same
// thread, so a step that needs the norm of ALL elements first runs it with `compute` alone, then stage 1 of the norm, then the clip
// of the stored gradients in place (train_adam.hpp says why not inside the update), then the update alone (the mode-2 form): the
// plain kernel, or with decay its second instantiation.  Decay without a norm stays the one launch.
static int final_optim(const aqg_train& t, int B, bool compute, int step, int step_index, float* loss_sums, const OptimPlan& plan,
                       hipStream_t st) {
    OptimLaunch ol;
    if (!plan.norm()) {
        if (int r = optim_before_finish(plan, step_index, &ol, st)) return r;
        return launch_train_final(t, B, compute, true, step, loss_sums, st, &ol);
    }
    if (compute)
        if (int r = launch_train_final(t, B, true, false, step, loss_sums, st)) return r;
    if (int r = optim_before_finish(plan, step_index, &ol, st)) return r;
    if (int r = launch_clip_scale(plan, ol, st)) return r;
    ol.s.partials = nullptr; ol.s.P = 0; ol.s.norm_out = nullptr;        // clipped already
    return launch_train_final(t, B, false, true, step, nullptr, st, plan.wd ? &ol : nullptr);
}

// mode 0 = gradients only, 1 = gradients + Adam, 2 = Adam only (data-parallel: local gradients, all-reduce, update)
static int train_step_launches(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
                               const OptimPlan* plan, const aqg_loss* lf) {
    const int B = t.batch;
    if (mode != 2 && B > 0) {
        if (int r = forward_backward(t, states72, pi, z, nullptr, 0, B, st, lf)) return r;
        if (plan && mode == 1) return final_optim(t, B, true, t.step, 0, nullptr, *plan, st);
        if (int r = launch_train_final(t, B, true, mode == 1, t.step, nullptr, st)) return r;
        return plan ? optim_norm_only(*plan, st) : 0;
    }
    if (mode >= 1) return plan ? final_optim(t, B, false, t.step, 0, nullptr, *plan, st) : launch_train_final(t, B, false, true, t.step, nullptr, st);
    return plan ? optim_norm_only(*plan, st) : 0;
}
// avg (may be null; include/aqgnn.h "weight averaging"): the averaging launch behind the last launch of an updating step
// lf (may be null; include/aqgnn.h "loss form"): the board launch's second (cross-entropy) or third (value weight alone) instantiation
int train_step(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
               const OptimPlan* plan, const aqg_weight_average* avg, const aqg_loss* lf) {
    if (int r = validate(t)) return r;
    if (int r = train_step_launches(t, states72, pi, z, mode, st, plan, lf)) return r;
    return mode >= 1 ? average_after_update(avg, t.step, st) : 0;
}

// A run of consecutive single-process steps over a shuffled data set, no host work in between: step i takes the positions
// order[i * batch .. (i + 1) * batch) (the last batch may be short, train_network.py's DataLoader keeps it) of the
// resident arrays, t.step counts up from its entry value, and each step's loss terms are added to loss_sums[2]
// (policy, value: the per-step batch means, what train_network.py:89-90 accumulates per epoch).
int train_steps(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, long long positions,
                float* loss_sums, hipStream_t st, const OptimPlan* plan, const aqg_weight_average* avg, const aqg_loss* lf) {
    if (int r = validate(t)) return r;
    if (t.batch < 1) return fail("aqg_gcn_train_steps: batch must be >= 1");
    int step = t.step;
    for (long long first = 0; first < positions; first += t.batch, ++step) {
        const int B = (int)(positions - first < t.batch ? positions - first : t.batch);
        if (int r = forward_backward(t, states72, pi, z, order, (int)first, B, st, lf)) return r;
        if (plan) { if (int r = final_optim(t, B, true, step, step - t.step, loss_sums, *plan, st)) return r; }
        else if (int r = launch_train_final(t, B, true, true, step, loss_sums, st)) return r;
        if (int r = average_after_update(avg, step, st)) return r;
    }
    return 0;
}

// the diagnostic builds' entry points: every unit keeps its own copy of the stamp array / dump pointer (gcn_train_common.hpp)
#ifdef AQG_TRAIN_DEBUG
extern "C" int aqg_debug_train_buf(float* buf) { return train_debug_buf_exact(buf) | train_debug_buf_split(buf); }
#endif
#ifdef AQG_STAMP
// out[4][16]: the element-wise sum of the units' counters (they only ever accumulate); reset clears every unit's
extern "C" int aqg_debug_train_stamps(unsigned long long* out_host, int reset) {
    memset(out_host, 0, sizeof(unsigned long long) * 64);
    return train_stamps_final(out_host, reset) | train_stamps_exact(out_host, reset) | train_stamps_split(out_host, reset);
}
#endif

}  // namespace aqg
