// launchers.hpp -- the host functions and option globals one .hip file defines and another calls, declared once.  Included by
// the defining file as well, so a definition that drifts from its declaration does not compile.  Declarations only.
#pragma once
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"

namespace aqg {

// ---- legal_mask.hip
int launch_legal_actions(int N, const void* states, int fmt, int B, uint8_t* mask, uint8_t* order, int32_t* count,
                         const uint8_t* active, hipStream_t st);
int launch_state_next(int N, const uint8_t* in, const int32_t* actions, int B, uint8_t* out, hipStream_t st);
int launch_state_status(int N, const uint8_t* in, int B, int draw, uint8_t* flags, hipStream_t st);

// ---- state_check.hip
int launch_states72_check(int N, const uint8_t* in, int B, int num_walls, int draw, uint8_t* flags, hipStream_t st);
int host_check_state(int N, const uint8_t* rec72, int num_walls, int draw);

// ---- gcn_forward.hip
extern int g_trunk_variant, g_profile_trunk;
void profile_mark(hipStream_t st, long long units);
int profile_collect(double* total_ms, long long* launches, long long* boards, int reset);
int launch_poison_lds(hipStream_t st);
int launch_gcn_forward_boards(int N, const void* states, int fmt, int B, const float* packed, float* pooled,
                              float* logits, float* policy, float* value_pre, float* value, const uint8_t* active,
                              int flags, int32_t* saturated, hipStream_t st, const int32_t* list = nullptr,
                              const int32_t* list_count = nullptr);

// ---- gcn_pack.hip
size_t packed_floats();
int pack_weights_host(int N, const float* const* t, float* out);

// ---- gcn_trunk_split.hip  (the trunk launchers only enqueue: launch_gcn_forward_boards checks the launch behind its profiling event)
extern int g_trunk_grid, g_trunk_phase_delay, g_trunk_delay_min_boards, g_trunk_prio, g_heads_prio;
int set_trace_gcn(void* buf, unsigned int cap);
void launch_gcn_trunk_split(int track, const void* states, int fmt, int B, const float* packed, float* pooled, const uint8_t* active,
                            int32_t* saturated, const int32_t* list, const int32_t* list_count, hipStream_t st);
void trunk_split_launch_shape(int B, bool list, int& grid, int& opts);
int launch_gcn_heads_split(float* pooled, int B, int A, const float* packed, float* logits, float* policy, float* value_pre,
                           float* value, const uint8_t* active, int32_t* saturated, hipStream_t st);

// ---- gcn_trunk_exact.hip
void launch_gcn_trunk_exact(int variant, const void* states, int fmt, int B, const float* packed, float* pooled,
                            const uint8_t* active, hipStream_t st);
int launch_gcn_heads_exact(const float* pooled, int B, int A, const float* packed, float* logits, float* policy, float* value_pre,
                           float* value, const uint8_t* active, hipStream_t st);

// ---- gcn_boards_plain.hip
size_t boards_any_workspace_floats(int N, int B);
int launch_gcn_forward_boards_any(int N, const void* states, int fmt, int B, const float* packed, float* workspace,
                                  size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre,
                                  float* value, const uint8_t* active, int flags, int32_t* saturated, hipStream_t st,
                                  const int32_t* list = nullptr, const int32_t* list_count = nullptr);

// ---- board_featuriser.hip
int launch_gcn_boards_graph(int N, const void* states, int fmt, int B, float* x0, int32_t* ell_idx, float* ell_w, hipStream_t st);
int launch_gcn_boards_features(int N, const void* states, int fmt, int B, float* x0, hipStream_t st);

// ---- gcn_general.hip
int launch_gen_linear(int M, int K, int N, const float* X, const float* W, const float* bias, const float* mask, int flags,
                      float* Y, hipStream_t st);
size_t gen_linear_grad_workspace_floats(int M, int N, int K);
size_t gen_linear_grad_workspace_floats_bound(long long max_rows, int N, int K);
int launch_gen_linear_grad(int M, int K, int N, const float* dY, const float* X, const float* dYb, float* workspace,
                           size_t workspace_floats, float* dW, float* db, hipStream_t st);
int launch_gen_aggregate(int n, int N, const float* Y, const int32_t* ptr, const int32_t* src, const float* w, const float* bias,
                         int relu, float* out, hipStream_t st);
int launch_gen_mean_pool(int N, const float* H, const int32_t* gptr, int G, float* pooled, hipStream_t st);
int launch_gen_mean_pool_backward(int n, int N, const float* dpooled, const int32_t* gptr, int G, const float* mask, float* dH,
                                  hipStream_t st);
int launch_gen_heads(int G, int A, const float* logits, const float* vpre, float* policy, float* value, hipStream_t st,
                     const uint8_t* active = nullptr);
int launch_gen_heads_backward(int G, int A, const float* policy, const float* dpolicy, const float* value, const float* dvalue,
                              float* dlogits, float* dvpre, hipStream_t st);

// ---- gcn_boards_general.hip
int launch_board_gcn_layer(int N, int B, int K, int Nout, const float* X, const float* W, const float* bias, const int32_t* ell_idx,
                           const float* ell_w, const uint8_t* active, float* H, float* pooled, hipStream_t st);
size_t boards_general_workspace_floats(int N, int hidden, int A, int B);
int check_general_net(const aqg_gcn_general_net* net, const char** why);
int launch_gcn_forward_boards_general(int N, const void* states, int fmt, int B, const aqg_gcn_general_net* net,
                                      const uint8_t* active, float* workspace, size_t workspace_floats, float* pooled, float* logits,
                                      float* policy, float* value_pre, float* value, hipStream_t st);

// ---- cnn_forward.hip
int check_cnn_net(const aqg_cnn_net* net, int N, const char** why);
size_t cnn_packed_floats(int F, int L, int A);
int launch_cnn_pack(int F, int L, int A, const float* const* params, const float* eps, float* packed, hipStream_t st);
size_t cnn_workspace_floats(int N, int F, int A, int B);
int launch_cnn_forward_boards(int N, const void* states, int fmt, int B, const aqg_cnn_net* net, const uint8_t* active, float* workspace,
                              size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                              hipStream_t st);
int launch_cnn_forward_planes(int N, const float* planes, int B, const aqg_cnn_net* net, const uint8_t* active, float* workspace,
                              size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                              hipStream_t st);

// ---- mcts.hip  (the engine's entry points; host code only)
extern int g_use_graph;
// the options of one move, all zero = the plain move: the self-play targets (aqgnn.h, "self-play targets"), tree reuse, resignation
// and the recorded completed-Q policy target
struct MoveOptions {
    int temperature_plies;
    float* hist_value;
    const aqg_tree_reuse* reuse;
    const aqg_resign* resign;
    const aqg_policy_record* policy = nullptr;
    const aqg_start_table* start = nullptr;      // the refill behind the move starts its games from the table (aqgnn.h, "start positions")
    const aqg_gumbel* gumbel = nullptr;          // the root is searched by sequential halving over Gumbel top-m actions (aqgnn.h, "Gumbel root search")
};
// what a selecting step launch of a Gumbel search is handed beside the engine struct (aqgnn.h, "Gumbel root search"): the schedule
// table T[0 .. considered][0 .. stride), the per-slot words m_g, the f32 constants of the score and `sim`, the simulation the launch
// selects for (1 .. sims - 1: the root's children are then scored against T[m_g][sim - 1])
struct GumbelStep {
    const int32_t* schedule;
    int32_t* m;
    float c_visit, c_scale;
    int32_t considered, stride, sim;
};
int engine_reset(const aqg_engine& e, hipStream_t st, const aqg_start_table* start = nullptr);
int validate_start_table(const aqg_engine& e, const aqg_start_table* start, const char* what);
int engine_clear_eval_cache(const aqg_engine& e, hipStream_t st);
int engine_begin_move(const aqg_engine& e, hipStream_t st);
int engine_step(const aqg_engine& e, int do_expand, int do_select, hipStream_t st);
int engine_finish_move(const aqg_engine& e, const double* uniforms, const MoveOptions& opts, hipStream_t st);
int engine_set_roots(const aqg_engine& e, const uint8_t* roots72, hipStream_t st);
int engine_move(const aqg_engine& e, const double* uniforms, const MoveOptions& opts, hipStream_t st);
int engine_search(const aqg_engine& e, const uint8_t* roots72, hipStream_t st);
int engine_root_visits(const aqg_engine& e, int32_t* visits, uint8_t* actions, int32_t* count, hipStream_t st);
int engine_refill(const aqg_engine& e, hipStream_t st, const aqg_start_table* start = nullptr);
int engine_root_noise(const aqg_engine& e, hipStream_t st);
int engine_root_priors(const aqg_engine& e, float* priors, int32_t* count, hipStream_t st);
int engine_root_values(const aqg_engine& e, float* value, hipStream_t st);
int engine_root_improved_policy(const aqg_engine& e, double c_visit, double c_scale, float* policy, uint8_t* actions, int32_t* count,
                                float* vmix, hipStream_t st);
int engine_record_improved_policy(const aqg_engine& e, const aqg_policy_record& pr, hipStream_t st);
int engine_keep_subtrees(const aqg_engine& e, const aqg_tree_reuse& ru, const int32_t* child_index, hipStream_t st);
int engine_reset_reuse(const aqg_engine& e, const aqg_tree_reuse& ru, hipStream_t st);
int engine_reset_resign(const aqg_engine& e, const aqg_resign& rs, hipStream_t st);
int engine_search_gumbel(const aqg_engine& e, const uint8_t* roots72, const aqg_gumbel& gb, hipStream_t st);
int engine_gumbel_root(const aqg_engine& e, const aqg_gumbel& gb, hipStream_t st);
int engine_root_gumbel(const aqg_engine& e, const aqg_gumbel& gb, float* gl, int32_t* m, int32_t* winner, hipStream_t st);

// ---- mcts_step.hip  (launchers of the engine's kernels only enqueue: the entry point checks the launch)
extern int g_step_waves, g_step_prio, g_step_fast_depth, g_step_heads;
int set_trace_mcts(void* buf, unsigned int cap);
int launch_engine_step(const aqg_engine& e, int do_expand, int do_select, hipStream_t st, int list_sim, bool heads, bool defer_legal = false,
                       bool policy_beside = false, const GumbelStep* gumbel = nullptr);

// ---- mcts_eval.hip
extern int g_legal_beside_trunk, g_policy_beside_step;
int set_trace_eval(void* buf, unsigned int cap);
bool engine_step_defers_legal(const aqg_engine& e, bool step_heads);
bool engine_policy_beside_step(const aqg_engine& e, bool defer_legal);
int launch_engine_eval(const aqg_engine& e, hipStream_t st, bool policy_jobs = false);

// ---- mcts_move.hip
void launch_engine_reset(const aqg_engine& e, hipStream_t st, const aqg_start_table* start = nullptr);
void launch_engine_set_roots(const aqg_engine& e, const uint8_t* roots72, hipStream_t st);
void launch_engine_begin_move(const aqg_engine& e, hipStream_t st, const uint8_t* kept = nullptr);
void launch_engine_kept_root_noise(const aqg_engine& e, const uint8_t* kept, hipStream_t st);
int launch_engine_fake_eval(const aqg_engine& e, hipStream_t st);
int launch_engine_root_noise(const aqg_engine& e, hipStream_t st);
int launch_engine_finish_move(const aqg_engine& e, const double* uniforms, const MoveOptions& opts, hipStream_t st);
void launch_engine_refill(const aqg_engine& e, hipStream_t st, const aqg_start_table* start = nullptr);
int launch_engine_root_visits(const aqg_engine& e, int32_t* visits, uint8_t* actions, int32_t* count, hipStream_t st);
void launch_engine_root_priors(const aqg_engine& e, float* priors, int32_t* count, hipStream_t st);
void launch_engine_root_values(const aqg_engine& e, float* value, hipStream_t st);
int engine_root_states72(const aqg_engine& e, uint8_t* out72, hipStream_t st);
int engine_apply_actions(const aqg_engine& e, const int32_t* actions, hipStream_t st, const aqg_start_table* start = nullptr);

// ---- mcts_improve.hip
void launch_engine_root_improved_policy(const aqg_engine& e, double c_visit, double c_scale, float* policy, uint8_t* actions,
                                        int32_t* count, float* vmix, hipStream_t st);

// ---- mcts_record.hip
int launch_engine_record_improved_policy(const aqg_engine& e, const aqg_policy_record& pr, hipStream_t st);

// ---- mcts_gumbel.hip
void launch_engine_gumbel_root(const aqg_engine& e, const aqg_gumbel& gb, hipStream_t st);
int launch_engine_finish_move_gumbel(const aqg_engine& e, const MoveOptions& opts, hipStream_t st);
void launch_engine_root_gumbel(const aqg_engine& e, const aqg_gumbel& gb, float* gl, int32_t* m, int32_t* winner, hipStream_t st);

// ---- mcts_reuse.hip
void launch_engine_keep_subtrees(const aqg_engine& e, const aqg_tree_reuse& ru, const int32_t* child_index, hipStream_t st);

// ---- agents.hip
int launch_agent_random(int N, const uint8_t* states72, int B, const double* uniforms, int stride, uint64_t seed, int32_t* actions,
                        hipStream_t st);
int launch_playouts(int N, const uint8_t* states72, int B, int plies_for_draw, const double* uniforms, int stride, uint64_t seed,
                    int32_t* value, int32_t* plies, int32_t* draws, uint8_t* final72, hipStream_t st);
size_t agent_mcts_workspace_bytes(int B, int evaluations);
int launch_agent_mcts(int N, const uint8_t* states72, int B, int evaluations, int plies_for_draw, const double* explore,
                      const double* uniforms, int stride, uint64_t seed, void* workspace, size_t workspace_bytes, int32_t* action,
                      int32_t* visits, uint8_t* actions, int32_t* count, int32_t* draws, hipStream_t st);
int launch_agent_shortest_paths(int N, const uint8_t* states72, int B, int32_t* out, hipStream_t st);
size_t agent_alpha_beta_workspace_bytes(int N, int B, int max_depth);
int launch_agent_alpha_beta(int N, const uint8_t* states72, int B, const uint8_t* active, int plies_for_draw, int max_dist,
                            int max_depth, void* workspace, size_t workspace_bytes, int32_t* action, int64_t* nodes, hipStream_t st);

// ---- grad_norm.hip  (the optimiser controls: train_adam.hpp defines OptimPlan and OptimLaunch)
struct OptimPlan;
struct OptimLaunch;
size_t optim_workspace_floats(size_t n);
int launch_grad_norm(const float* x, size_t n, float* out, float* workspace, size_t workspace_floats, hipStream_t st);
// the checks of a step entry point: 0 with *on = whether any control is on and *plan filled, or a refusal.  numel[tensors].
int check_optim(const aqg_optim* o, int tensors, const size_t* numel, float* const* grads, const char* what, OptimPlan* plan,
                bool* on);
int optim_before_finish(const OptimPlan& plan, int step_index, OptimLaunch* ol, hipStream_t st);   // stage 1 (when a norm is wanted)
int launch_clip_scale(const OptimPlan& plan, const OptimLaunch& ol, hipStream_t st);               // the fused step: g <- coef g in place
int optim_norm_only(const OptimPlan& plan, hipStream_t st);                                        // mode 0: stage 1 + combine

// ---- weight_average.hip  (include/aqgnn.h "weight averaging")
int check_weight_average(const aqg_weight_average* a, const char* what);           // every refusal, on the host; nothing launched
int launch_weight_average(const aqg_weight_average& a, hipStream_t st);             // of a checked struct
// behind the Adam launch of 1-based step `step`: the averaging launch when an average is kept and the step is a multiple of `every`
inline int average_after_update(const aqg_weight_average* avg, int step, hipStream_t st) {
    return avg && step % avg->every == 0 ? launch_weight_average(*avg, st) : 0;
}

// ---- gcn_train.hip  (plan: null = the step as it has always been; avg: null = no average is kept; lf: null = the reference's loss)
extern int g_train_fused;
int train_step(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
               const OptimPlan* plan = nullptr, const aqg_weight_average* avg = nullptr, const aqg_loss* lf = nullptr);
int train_steps(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, long long positions,
                float* loss_sums, hipStream_t st, const OptimPlan* plan = nullptr, const aqg_weight_average* avg = nullptr,
                const aqg_loss* lf = nullptr);
void train_tensor_sizes(const aqg_train& t, size_t* numel);

// ---- gcn_train_exact.hip, gcn_train_split.hip, gcn_train_final.hip: the two launches of a fused training step
int launch_train_board_exact(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first,
                             int B, hipStream_t st, const aqg_loss* lf = nullptr);
int launch_train_board_split(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first,
                             int B, int force_fallback, hipStream_t st, const aqg_loss* lf = nullptr);
long long train_fallbacks(int reset);
int launch_train_final(const aqg_train& t, int B, bool compute, bool update, int step, float* loss_sums, hipStream_t st,
                       const OptimLaunch* ol = nullptr);
#ifdef AQG_STAMP            // diagnostic builds only (gcn_train_common.hpp): each unit's own stamp counters / dump pointer
int train_stamps_exact(unsigned long long* out, int reset);
int train_stamps_split(unsigned long long* out, int reset);
int train_stamps_final(unsigned long long* out, int reset);
#endif
#ifdef AQG_TRAIN_DEBUG
int train_debug_buf_exact(float* buf);
int train_debug_buf_split(float* buf);
#endif

// ---- gcn_train_general.hip
int launch_train_general_prep(int V, int B, const uint8_t* states72, const int64_t* order, int first, int32_t* gptr, uint8_t* gathered,
                              hipStream_t st);
int launch_train_general_loss(int B, int A, const float* policy, const float* value, const float* pi, const float* z,
                              const int64_t* order, int first, float* loss, float* dpol, float* dval, hipStream_t st);
int launch_policy_value_loss(int B, int A, const float* logits, const float* value, const float* pi, const float* z, const int64_t* order,
                             int first, float value_weight, float* loss, float* dlogits, float* dvpre, hipStream_t st);
int launch_train_losses(int B, int A, const float* logits, const float* policy, const float* value, const float* pi, const float* z,
                        const int64_t* order, int first, const aqg_loss* lf, float* loss, float* dpol, float* dval, float* dlogits,
                        float* dvpre, hipStream_t st);
size_t train_general_workspace_floats(int N, int hidden, int num_layers, int policy_size, int max_batch);
int train_step_general(const aqg_train_general& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
                       const OptimPlan* plan = nullptr, const aqg_weight_average* avg = nullptr, const aqg_loss* lf = nullptr);
int train_steps_general(const aqg_train_general& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                        long long positions, float* loss_sums, hipStream_t st, const OptimPlan* plan = nullptr, const aqg_weight_average* avg = nullptr,
                        const aqg_loss* lf = nullptr);
void train_general_tensor_sizes(const aqg_train_general& t, size_t* numel);

// ---- cnn_train.hip
size_t cnn_train_workspace_floats(int N, int F, int L, int A, int max_batch);
int check_cnn_train(const aqg_cnn_train& t, bool adam, const char* what);
int cnn_train_step(const aqg_cnn_train& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
                   const OptimPlan* plan = nullptr, const aqg_weight_average* avg = nullptr, const aqg_loss* lf = nullptr);
int cnn_train_steps(const aqg_cnn_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                    long long positions, float* loss_sums, hipStream_t st, const OptimPlan* plan = nullptr, const aqg_weight_average* avg = nullptr,
                    const aqg_loss* lf = nullptr);
void cnn_train_tensor_sizes(const aqg_cnn_train& t, size_t* numel);

// ---- augment.hip
int launch_augment_gather(int N, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                          const uint8_t* flips, int use_seed, uint64_t seed, uint64_t epoch, int n, uint8_t* out72, float* out_pi,
                          float* out_z, hipStream_t st);

// ---- replay.hip
int launch_replay_append(int N, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8, const float* pi,
                         const float* z_f32, int n, int capacity, int head, uint8_t* ring72, float* ring_pi, float* ring_z,
                         hipStream_t st, const float* search_value = nullptr, float blend = 0.f, bool policy_form = false);
int launch_replay_append_policy(int N, int policy_size, const uint8_t* states72, const float* pi, const int8_t* z_i8,
                                const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                                float* ring_z, hipStream_t st);
int launch_replay_append_blend(int N, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8,
                               const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                               float* ring_z, hipStream_t st);

// ---- replay_refresh.hip
int launch_replay_refresh(int N, int policy_size, const int32_t* visits, const uint8_t* actions, const int32_t* count,
                          const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                          float* ring_z, hipStream_t st);
int launch_replay_refresh_policy(int N, int policy_size, const float* policy, const uint8_t* actions, const int32_t* count,
                                 const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                                 float* ring_z, hipStream_t st);

// ---- replay_merge.hip
int launch_replay_position_keys(const uint8_t* states72, const int64_t* index, int n, int64_t* keys, hipStream_t st);
int launch_replay_run_heads(const uint8_t* states72, const int64_t* perm, int n, uint8_t* heads, hipStream_t st);
size_t replay_merge_workspace_floats(int N, int n, int u);
int launch_replay_merge_runs(int N, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* perm,
                             const int64_t* starts, int n, int u, uint8_t* out72, float* out_pi, float* out_z, int32_t* count,
                             float* workspace, size_t workspace_floats, hipStream_t st);

// ---- replay_surprise.hip
int launch_replay_surprise_rows(int N, int policy_size, const float* net_policy, const float* ring_pi, const int64_t* index, int rows,
                                int m, int offset, int n, float* k, int32_t* q, hipStream_t st);
int launch_replay_surprise_counts(const int32_t* q, const int64_t* index, const int64_t* total, int m, long long expected_rows,
                                  double uniform_share, int max_copies, uint64_t seed, uint64_t update, int32_t* count, hipStream_t st);

// ---- row_metrics.hip
int launch_replay_row_metrics(int N, int policy_size, const float* net_policy, const float* net_value, const uint8_t* states72,
                              const float* ring_pi, const float* ring_z, const int64_t* index, int rows, int m, int offset, int n,
                              int bucket_plies, int buckets, double* vals, int32_t* tag, hipStream_t st);
size_t row_metrics_workspace_doubles(int m, int buckets);
int launch_row_metrics_reduce(const double* vals, const int32_t* tag, int m, int buckets, double* partial, double* sums,
                              long long* counts, hipStream_t st);
int launch_replay_holdout_mask(const int64_t* keys, int n, uint64_t seed, double share, uint8_t* mask, hipStream_t st);

// ---- value_targets.hip
int launch_lambda_values(int quota, int hp, const int32_t* game_plies, const int8_t* game_result, const uint8_t* game_done,
                         const float* hist_value, float lambda, float* out, hipStream_t st);

}  // namespace aqg
