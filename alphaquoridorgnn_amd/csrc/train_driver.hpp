// train_driver.hpp -- the host side of a step and of an epoch of the two workspace trainers, the any-shape GNN (gcn_train_general.hip)
// and the residual CNN (cnn_train.hip), written once.  A kind K supplies what really differs: Workspace and layout(t, B, ws) (the floats
// needed at batch B; ws non-null: carved out of t.workspace), validate(t, what) (the checks it makes here, not in capi.hip), its launches
// forward_backward and launch_finish, the strings of this file's refusals, and empty_batch_mode1_updates.
// The fused 6/128/3 step (gcn_train.hip) forms gradients and updates in one kernel and clips in place: it is not a kind.
#pragma once
#include "launchers.hpp"
#include "train_adam.hpp"

namespace aqg {

// one batch: forward and backward, stage 1 of the norm when the controls (plan, may be null) want one, the finish launch and, behind
// an update of a step the average (avg, may be null: include/aqgnn.h "weight averaging") takes, the averaging launch; lf (may be
// null: include/aqgnn.h "loss form") is handed to the kind's forward_backward
template <class K, class Net>
int train_driver_batch(const Net& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first, int B,
                       bool update, int step, float* loss_sums, const OptimPlan* plan, hipStream_t st,
                       const aqg_weight_average* avg = nullptr, const aqg_loss* lf = nullptr) {
    typename K::Workspace ws;
    K::layout(t, B, &ws);
    float* loss = t.loss ? t.loss : ws.loss;
    if (int r = K::forward_backward(t, states72, pi, z, order, first, B, ws, t.policy ? t.policy : ws.policy,
                                    t.value ? t.value : ws.value, loss, st, lf))
        return r;
    OptimLaunch ol;
    if (plan) if (int r = optim_before_finish(*plan, step - t.step, &ol, st)) return r;
    if (int r = K::launch_finish(t, B, update, step, loss, t.loss_mean ? t.loss_mean : ws.loss_mean, loss_sums, st, plan ? &ol : nullptr))
        return r;
    return update ? average_after_update(avg, step, st) : 0;
}

// mode 0 = gradients only, 1 = gradients + Adam, 2 = Adam only (data-parallel: local gradients, all-reduce, update)
template <class K, class Net>
int train_driver_step(const Net& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
                      const OptimPlan* plan, const aqg_weight_average* avg = nullptr, const aqg_loss* lf = nullptr) {
    const OptimPlan* update_plan = mode >= 1 ? plan : nullptr;
    if (int r = K::validate(t, K::step_name)) return r;
    if (mode != 2 && t.batch > 0) {
        if (!t.workspace || t.workspace_floats < K::layout(t, t.batch, nullptr)) return fail(K::step_name, K::workspace_refusal);
        if (int r = train_driver_batch<K>(t, states72, pi, z, nullptr, 0, t.batch, mode == 1, t.step, nullptr, update_plan, st, avg, lf))
            return r;
    } else if (mode == 2 || (mode == 1 && K::empty_batch_mode1_updates)) {
        OptimLaunch ol;
        if (update_plan) if (int r = optim_before_finish(*plan, 0, &ol, st)) return r;
        if (int r = K::launch_finish(t, t.batch, true, t.step, nullptr, nullptr, nullptr, st, update_plan ? &ol : nullptr)) return r;
        return average_after_update(avg, t.step, st);
    }
    return plan && mode == 0 ? optim_norm_only(*plan, st) : 0;
}

// an epoch, every step mode 1: step i trains on positions [i batch, (i + 1) batch) of `order` (null: of the arrays), the short last one kept
template <class K, class Net>
int train_driver_steps(const Net& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, long long positions,
                       float* loss_sums, hipStream_t st, const OptimPlan* plan, const aqg_weight_average* avg = nullptr,
                       const aqg_loss* lf = nullptr) {
    if (int r = K::validate(t, K::steps_name)) return r;
    if (t.batch < 1) return fail(K::steps_name, "batch must be >= 1");
    if (!t.workspace || t.workspace_floats < K::layout(t, t.batch, nullptr))       // serves the short last batch too
        return fail(K::steps_name, K::workspace_refusal);
    for (long long first = 0; first < positions; first += t.batch) {
        const int B = (int)(positions - first < t.batch ? positions - first : t.batch), step = t.step + (int)(first / t.batch);
        if (int r = train_driver_batch<K>(t, states72, pi, z, order, (int)first, B, true, step, loss_sums, plan, st, avg, lf)) return r;
    }
    return 0;
}

}  // namespace aqg
