// capi.hip -- extern "C" entry points of libaqgnn_hip.so (declared in include/aqgnn.h).
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "train_adam.hpp"

namespace aqg {
thread_local char g_err[512] = "";
}  // namespace aqg

using namespace aqg;

// ---- training.  Per kind (the fused 6/128/3 GNN, the any-shape GNN, the residual CNN): check_net = the checks of its struct,
// plan_optim = the checks of a call's optimiser controls against its tensors.  check_step / check_steps are an entry point's argument
// checks under `what`, the name of the entry point that was called; a plain call and its _optim form make the same ones.
template <class Net>
static int check_tensors(const Net& t, int tensors, bool adam, const char* what) {
    for (int i = 0; i < tensors; ++i)
        if (!t.params[i] || !t.grads[i] || (adam && (!t.adam_m[i] || !t.adam_v[i]))) return fail(what, "null parameter tensor");
    return adam && t.step < 1 ? fail(what, "step must be >= 1") : 0;
}
static int check_net(const aqg_train& t, bool adam, const char* what) { return check_tensors(t, 14, adam, what); }
static int check_net(const aqg_train_general& t, bool adam, const char* what) {
    if (t.num_layers < 1 || t.num_layers > AQG_GENERAL_MAX_LAYERS) return fail(what, "num_layers must be 1..32");
    return check_tensors(t, 2 * t.num_layers + 8, adam, what);
}
static int check_net(const aqg_cnn_train& t, bool adam, const char* what) { return check_cnn_train(t, adam, what); }

static int plan_optim(const aqg_train& t, const aqg_optim* optim, const char* what, OptimPlan* plan, bool* on) {
    size_t numel[14];
    train_tensor_sizes(t, numel);
    return check_optim(optim, 14, numel, t.grads, what, plan, on);
}
static int plan_optim(const aqg_train_general& t, const aqg_optim* optim, const char* what, OptimPlan* plan, bool* on) {
    // sizes are taken of a shape inside the kernels' limits only, refused in the words of the plain call (check_general_net)
    if (t.hidden < 2 || t.hidden > 1024) return fail(what, "hidden must be 2..1024");
    if (t.policy_size < 1 || t.policy_size > 4096) return fail(what, "policy_size must be 1..4096");
    size_t numel[2 * AQG_GENERAL_MAX_LAYERS + 8];
    train_general_tensor_sizes(t, numel);
    return check_optim(optim, 2 * t.num_layers + 8, numel, t.grads, what, plan, on);
}
static int plan_optim(const aqg_cnn_train& t, const aqg_optim* optim, const char* what, OptimPlan* plan, bool* on) {
    size_t numel[AQG_CNN_TRAIN_TENSORS];
    cnn_train_tensor_sizes(t, numel);
    return check_optim(optim, 3 * (2 * t.num_blocks + 1) + 4, numel, t.grads, what, plan, on);
}

static int check_step(const aqg_train* t, const uint8_t* states72, const float* pi, const float* z, int mode, const char* what) {
    if (!t || mode < 0 || mode > 2) return fail(what, "bad argument");
    if (mode != 2 && (!states72 || !pi || !z)) return fail(what, "null argument");
    return check_net(*t, mode >= 1, what);
}
template <class Net>      // the two workspace trainers: the batch is the struct's, and an empty one needs no arrays
static int check_step(const Net* t, const uint8_t* states72, const float* pi, const float* z, int mode, const char* what) {
    if (!t || mode < 0 || mode > 2) return fail(what, "bad argument");
    if (t->batch < 0) return fail(what, "negative batch");
    if (mode != 2 && t->batch > 0 && (!states72 || !pi || !z)) return fail(what, "null argument");
    return check_net(*t, mode >= 1, what);
}
template <class Net>
static int check_steps(const Net* t, const uint8_t* states72, const float* pi, const float* z, long long positions, const char* what) {
    if (!t || !states72 || !pi || !z || positions < 0 || positions > 0x7fffffffLL) return fail(what, "bad argument");
    return check_net(*t, true, what);
}

// the loss form of a _loss call (include/aqgnn.h "loss form")
static int check_loss_form(const aqg_loss* lf, const char* what) {
    if (!lf) return 0;
    if (lf->policy_form != 0 && lf->policy_form != 1) return fail(what, "policy_form must be 0 (reference) or 1 (cross-entropy)");
    if (!(lf->value_weight >= 0.f) || !std::isfinite(lf->value_weight)) return fail(what, "value_weight must be finite and >= 0");
    return 0;
}
static bool loss_form_is_default(const aqg_loss* lf) { return !lf || (lf->policy_form == 0 && lf->value_weight == 1.f); }
template <class Net>
static int check_loss_call(const Net* t, const aqg_optim* optim, const aqg_weight_average* avg, const char* what, OptimPlan* plan,
                           bool* on) {
    if (int r = plan_optim(*t, optim, what, plan, on)) return r;
    return avg ? check_weight_average(avg, what) : 0;
}

extern "C" {

int aqg_abi_version(void) { return AQG_ABI_VERSION; }
const char* aqg_last_error(void) { return g_err; }

int aqg_set_option(const char* name, int value) {
    if (name && !strcmp(name, "trunk_variant")) { if (!(value == 0 || value == 1 || value == 3 || value == 6)) return fail("trunk_variant must be 0, 1, 3 or 6"); g_trunk_variant = value; return 0; }
    if (name && !strcmp(name, "heads_prio")) { g_heads_prio = value < 0 ? 0 : (value > 3 ? 3 : value); return 0; }
    if (name && !strcmp(name, "trunk_prio")) { g_trunk_prio = value < 0 ? -1 : (value & 15); return 0; }
    if (name && !strcmp(name, "trunk_grid")) { g_trunk_grid = value; return 0; }
    if (name && !strcmp(name, "trunk_phase_delay")) { if (value < 0 || value > 4096) return fail("trunk_phase_delay out of range"); g_trunk_phase_delay = value; return 0; }
    if (name && !strcmp(name, "trunk_delay_min_boards")) { g_trunk_delay_min_boards = value; return 0; }
    if (name && !strcmp(name, "step_prio")) { g_step_prio = value & 3; return 0; }
    if (name && !strcmp(name, "step_waves")) { g_step_waves = value; return 0; }
    if (name && !strcmp(name, "step_heads")) { g_step_heads = value ? 1 : 0; return 0; }
    if (name && !strcmp(name, "legal_beside_trunk")) { g_legal_beside_trunk = value ? 1 : 0; return 0; }
    if (name && !strcmp(name, "policy_beside_step")) { g_policy_beside_step = value ? 1 : 0; return 0; }
    if (name && !strcmp(name, "step_fast_depth")) { if (value < 0 || value > 61) return fail("step_fast_depth must be 0..61"); g_step_fast_depth = value; return 0; }
    if (name && !strcmp(name, "train_fused")) { if (value < 1 || value > 3) return fail("train_fused must be 1, 2 or 3"); g_train_fused = value; return 0; }
    if (name && !strcmp(name, "use_graph")) { g_use_graph = value ? 1 : 0; return 0; }
    if (name && !strcmp(name, "profile_trunk")) { g_profile_trunk = (value == 1 || value == 2) ? value : 0; return 0; }   // 1 = trunk launches, 2 = step launches
    return fail("unknown option", name ? name : "(null)");
}

int aqg_debug_poison_lds(void* stream) { return launch_poison_lds((hipStream_t)stream); }

int aqg_debug_trace(void* buffer, unsigned int capacity) {
    if (set_trace_gcn(buffer, capacity) || set_trace_mcts(buffer, capacity) || set_trace_eval(buffer, capacity)) return fail("aqg_debug_trace: hipMemcpyToSymbol");
    return 0;
}

int aqg_profile_collect(double* total_ms_host, long long* launches_host, long long* boards_host, int reset) {
    return profile_collect(total_ms_host, launches_host, boards_host, reset);
}

int aqg_legal_actions(int board_size, const uint8_t* states72, int B, uint8_t* mask, uint8_t* order, int32_t* count,
                      void* stream) {
    if (B < 0 || (B > 0 && !states72)) return fail("aqg_legal_actions: bad arguments");
    return launch_legal_actions(board_size, states72, 0, B, mask, order, count, nullptr, (hipStream_t)stream);
}

int aqg_state_next(int board_size, const uint8_t* states72, const int32_t* actions, int B, uint8_t* out72, void* stream) {
    if (B < 0 || (B > 0 && (!states72 || !actions || !out72))) return fail("aqg_state_next: bad arguments");
    return launch_state_next(board_size, states72, actions, B, out72, (hipStream_t)stream);
}

int aqg_state_status(int board_size, const uint8_t* states72, int B, int plies_for_draw, uint8_t* flags, void* stream) {
    if (B < 0 || (B > 0 && (!states72 || !flags))) return fail("aqg_state_status: bad arguments");
    return launch_state_status(board_size, states72, B, plies_for_draw, flags, (hipStream_t)stream);
}

size_t aqg_gcn_packed_floats(int board_size) { (void)board_size; return packed_floats(); }

int aqg_gcn_pack_weights_host(int board_size, const float* const* tensors_host, float* packed_host) {
    if (!tensors_host || !packed_host) return fail("aqg_gcn_pack_weights_host: null argument");
    for (int i = 0; i < 14; ++i) if (!tensors_host[i]) return fail("aqg_gcn_pack_weights_host: null tensor");
    return pack_weights_host(board_size, tensors_host, packed_host);
}

int aqg_gcn_forward_boards(int board_size, const void* states, int state_fmt, int B, const float* packed, float* pooled,
                           float* logits, float* policy, float* value_pre, float* value, int flags, void* stream) {
    if (B < 0 || (B > 0 && (!states || !packed))) return fail("aqg_gcn_forward_boards: bad arguments");
    if (state_fmt != 0 && state_fmt != 1) return fail("aqg_gcn_forward_boards: state_fmt must be 0 or 1");
    return launch_gcn_forward_boards(board_size, states, state_fmt, B, packed, pooled, logits, policy, value_pre, value, nullptr,
                                     flags, nullptr, (hipStream_t)stream);
}

int aqg_gcn_forward_boards_guarded(int board_size, const void* states, int state_fmt, int B, const float* packed, float* pooled,
                                   float* logits, float* policy, float* value_pre, float* value, int flags, int32_t* saturated,
                                   void* stream) {
    if (B < 0 || (B > 0 && (!states || !packed))) return fail("aqg_gcn_forward_boards_guarded: bad arguments");
    if (state_fmt != 0 && state_fmt != 1) return fail("aqg_gcn_forward_boards_guarded: state_fmt must be 0 or 1");
    return launch_gcn_forward_boards(board_size, states, state_fmt, B, packed, pooled, logits, policy, value_pre, value, nullptr,
                                     flags, saturated, (hipStream_t)stream);
}

size_t aqg_gcn_boards_any_workspace_floats(int board_size, int B) { return B > 0 ? boards_any_workspace_floats(board_size, B) : 0; }

int aqg_gcn_forward_boards_any(int board_size, const void* states, int state_fmt, int B, const float* packed, float* workspace,
                               size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                               int flags, void* stream) {
    if (B < 0 || (B > 0 && (!states || !packed))) return fail("aqg_gcn_forward_boards_any: bad arguments");
    if (state_fmt != 0 && state_fmt != 1) return fail("aqg_gcn_forward_boards_any: state_fmt must be 0 or 1");
    return launch_gcn_forward_boards_any(board_size, states, state_fmt, B, packed, workspace, workspace_floats, pooled, logits, policy,
                                         value_pre, value, nullptr, flags, nullptr, (hipStream_t)stream);
}

int aqg_graph_linear(int M, int K, int N, const float* X, const float* W, const float* bias, const float* mask, int flags,
                     float* Y, void* stream) {
    if (M < 0 || K < 0 || N < 0) return fail("aqg_graph_linear: negative size");
    if (flags & ~(AQG_LIN_RELU | AQG_LIN_W_KN | AQG_LIN_ACCUMULATE)) return fail("aqg_graph_linear: unknown flag");
    if (M == 0 || N == 0) return 0;
    if (!Y || (K > 0 && (!X || !W))) return fail("aqg_graph_linear: null argument");
    return launch_gen_linear(M, K, N, X, W, bias, mask, flags, Y, (hipStream_t)stream);
}

size_t aqg_graph_linear_grad_workspace_floats(int M, int N, int K) { return gen_linear_grad_workspace_floats(M, N, K); }

int aqg_graph_linear_grad(int M, int K, int N, const float* dY, const float* X, const float* dYb, float* workspace,
                          size_t workspace_floats, float* dW, float* db, void* stream) {
    if (M < 0 || K < 0 || N < 0) return fail("aqg_graph_linear_grad: negative size");
    if (K == 0) return fail("aqg_graph_linear_grad: K must be >= 1");
    if (N == 0) return 0;
    if (!dW || (M > 0 && (!dY || !X || !workspace))) return fail("aqg_graph_linear_grad: null argument");
    return launch_gen_linear_grad(M, K, N, dY, X, dYb, workspace, workspace_floats, dW, db, (hipStream_t)stream);
}

int aqg_graph_aggregate(int num_nodes, int N, const float* Y, const int32_t* csr_ptr, const int32_t* csr_src, const float* csr_w,
                        const float* bias, int relu, float* out, void* stream) {
    if (num_nodes < 0 || N < 0) return fail("aqg_graph_aggregate: negative size");
    if (num_nodes == 0 || N == 0) return 0;
    if (!Y || !csr_ptr || !csr_src || !csr_w || !out) return fail("aqg_graph_aggregate: null argument");
    return launch_gen_aggregate(num_nodes, N, Y, csr_ptr, csr_src, csr_w, bias, relu, out, (hipStream_t)stream);
}

int aqg_graph_mean_pool(int num_nodes, int N, const float* H, const int32_t* graph_ptr, int num_graphs, float* pooled,
                        void* stream) {
    if (num_nodes < 0 || N < 0 || num_graphs < 0) return fail("aqg_graph_mean_pool: negative size");
    if (num_graphs == 0 || N == 0) return 0;
    if ((num_nodes > 0 && !H) || !graph_ptr || !pooled) return fail("aqg_graph_mean_pool: null argument");
    return launch_gen_mean_pool(N, H, graph_ptr, num_graphs, pooled, (hipStream_t)stream);
}

int aqg_graph_mean_pool_backward(int num_nodes, int N, const float* dpooled, const int32_t* graph_ptr, int num_graphs,
                                 const float* mask, float* dH, void* stream) {
    if (num_nodes < 0 || N < 0 || num_graphs < 0) return fail("aqg_graph_mean_pool_backward: negative size");
    if (num_nodes == 0 || N == 0) return 0;
    if (num_graphs == 0) return fail("aqg_graph_mean_pool_backward: nodes without graphs");
    if (!dpooled || !graph_ptr || !dH) return fail("aqg_graph_mean_pool_backward: null argument");
    return launch_gen_mean_pool_backward(num_nodes, N, dpooled, graph_ptr, num_graphs, mask, dH, (hipStream_t)stream);
}

int aqg_graph_heads(int num_graphs, int A, const float* logits, const float* value_pre, float* policy, float* value,
                    void* stream) {
    if (num_graphs < 0 || A <= 0) return fail("aqg_graph_heads: bad size");
    if (num_graphs == 0) return 0;
    if (!logits || !policy || (!value_pre != !value)) return fail("aqg_graph_heads: null argument");
    return launch_gen_heads(num_graphs, A, logits, value_pre, policy, value, (hipStream_t)stream);
}

int aqg_graph_heads_backward(int num_graphs, int A, const float* policy, const float* dpolicy, const float* value,
                             const float* dvalue, float* dlogits, float* dvalue_pre, void* stream) {
    if (num_graphs < 0 || A <= 0) return fail("aqg_graph_heads_backward: bad size");
    if (num_graphs == 0) return 0;
    if ((dpolicy && !policy) || (dvalue && !value)) return fail("aqg_graph_heads_backward: null argument");
    return launch_gen_heads_backward(num_graphs, A, policy, dpolicy, value, dvalue, dlogits, dvalue_pre, (hipStream_t)stream);
}

int aqg_gcn_boards_graph(int board_size, const uint8_t* states72, int B, float* x, int32_t* ell_idx, float* ell_w, void* stream) {
    if (B < 0) return fail("aqg_gcn_boards_graph: negative size");
    if (B > 0 && (!states72 || !x || !ell_idx || !ell_w)) return fail("aqg_gcn_boards_graph: null argument");
    return launch_gcn_boards_graph(board_size, states72, 0, B, x, ell_idx, ell_w, (hipStream_t)stream);
}

size_t aqg_gcn_boards_general_workspace_floats(int board_size, int hidden, int policy_size, int B) {
    return boards_general_workspace_floats(board_size, hidden, policy_size, B);
}

int aqg_gcn_forward_boards_general(int board_size, const void* states, int state_fmt, int B, const aqg_gcn_general_net* net,
                                   const uint8_t* active, float* workspace, size_t workspace_floats, float* pooled, float* logits,
                                   float* policy, float* value_pre, float* value, void* stream) {
    return launch_gcn_forward_boards_general(board_size, states, state_fmt, B, net, active, workspace, workspace_floats, pooled,
                                             logits, policy, value_pre, value, (hipStream_t)stream);
}

size_t aqg_cnn_packed_floats(int num_filters, int num_blocks, int policy_size) {
    return cnn_packed_floats(num_filters, num_blocks, policy_size);
}
int aqg_cnn_pack(int num_filters, int num_blocks, int policy_size, const float* const* params_host, const float* eps_host, float* packed,
                 void* stream) {
    return launch_cnn_pack(num_filters, num_blocks, policy_size, params_host, eps_host, packed, (hipStream_t)stream);
}
size_t aqg_cnn_workspace_floats(int board_size, int num_filters, int policy_size, int B) {
    return cnn_workspace_floats(board_size, num_filters, policy_size, B);
}
int aqg_cnn_forward_boards(int board_size, const void* states, int state_fmt, int B, const aqg_cnn_net* net, const uint8_t* active,
                           float* workspace, size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre,
                           float* value, void* stream) {
    return launch_cnn_forward_boards(board_size, states, state_fmt, B, net, active, workspace, workspace_floats, pooled, logits, policy,
                                     value_pre, value, (hipStream_t)stream);
}
int aqg_cnn_forward_planes(int board_size, const float* planes, int B, const aqg_cnn_net* net, const uint8_t* active, float* workspace,
                           size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                           void* stream) {
    return launch_cnn_forward_planes(board_size, planes, B, net, active, workspace, workspace_floats, pooled, logits, policy, value_pre,
                                     value, (hipStream_t)stream);
}

int aqg_engine_reset(const aqg_engine* e, void* stream) {
    if (!e) return fail("aqg_engine_reset: null engine");
    return engine_reset(*e, (hipStream_t)stream);
}
int aqg_engine_clear_eval_cache(const aqg_engine* e, void* stream) {
    if (!e) return fail("aqg_engine_clear_eval_cache: null engine");
    return engine_clear_eval_cache(*e, (hipStream_t)stream);
}
int aqg_engine_move(const aqg_engine* e, const double* uniforms, void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_move: null argument");
    return engine_move(*e, uniforms, MoveOptions{}, (hipStream_t)stream);
}
int aqg_engine_move_targets(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value, void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_move_targets: null argument");
    return engine_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, nullptr, nullptr}, (hipStream_t)stream);
}
int aqg_engine_begin_move(const aqg_engine* e, void* stream) {
    if (!e) return fail("aqg_engine_begin_move: null engine");
    return engine_begin_move(*e, (hipStream_t)stream);
}
int aqg_engine_step(const aqg_engine* e, int do_expand, int do_select, void* stream) {
    if (!e) return fail("aqg_engine_step: null engine");
    return engine_step(*e, do_expand ? 1 : 0, do_select ? 1 : 0, (hipStream_t)stream);
}
int aqg_engine_finish_move(const aqg_engine* e, const double* uniforms, void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_finish_move: null argument");
    return engine_finish_move(*e, uniforms, MoveOptions{}, (hipStream_t)stream);
}
int aqg_engine_finish_move_targets(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                   void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_finish_move_targets: null argument");
    return engine_finish_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, nullptr, nullptr}, (hipStream_t)stream);
}
int aqg_engine_move_reuse(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                          const aqg_tree_reuse* reuse, void* stream) {
    if (!e || !uniforms || !reuse) return fail("aqg_engine_move_reuse: null argument");
    return engine_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, nullptr}, (hipStream_t)stream);
}
int aqg_engine_finish_move_reuse(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                 const aqg_tree_reuse* reuse, void* stream) {
    if (!e || !uniforms || !reuse) return fail("aqg_engine_finish_move_reuse: null argument");
    return engine_finish_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, nullptr}, (hipStream_t)stream);
}
int aqg_engine_keep_subtrees(const aqg_engine* e, const aqg_tree_reuse* reuse, const int32_t* child_index, void* stream) {
    if (!e || !reuse || !child_index) return fail("aqg_engine_keep_subtrees: null argument");
    return engine_keep_subtrees(*e, *reuse, child_index, (hipStream_t)stream);
}
int aqg_engine_reset_reuse(const aqg_engine* e, const aqg_tree_reuse* reuse, void* stream) {
    if (!e || !reuse) return fail("aqg_engine_reset_reuse: null argument");
    return engine_reset_reuse(*e, *reuse, (hipStream_t)stream);
}
int aqg_engine_move_resign(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                           const aqg_tree_reuse* reuse, const aqg_resign* resign, void* stream) {
    if (!e || !uniforms || !resign) return fail("aqg_engine_move_resign: null argument");
    return engine_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, resign}, (hipStream_t)stream);
}
int aqg_engine_finish_move_resign(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                  const aqg_tree_reuse* reuse, const aqg_resign* resign, void* stream) {
    if (!e || !uniforms || !resign) return fail("aqg_engine_finish_move_resign: null argument");
    return engine_finish_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, resign}, (hipStream_t)stream);
}
int aqg_engine_move_policy(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                           const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy, void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_move_policy: null argument");
    return engine_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, resign, policy}, (hipStream_t)stream);
}
int aqg_engine_finish_move_policy(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                  const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy, void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_finish_move_policy: null argument");
    return engine_finish_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, resign, policy}, (hipStream_t)stream);
}
int aqg_engine_record_improved_policy(const aqg_engine* e, const aqg_policy_record* policy, void* stream) {
    if (!e || !policy) return fail("aqg_engine_record_improved_policy: null argument");
    return engine_record_improved_policy(*e, *policy, (hipStream_t)stream);
}
int aqg_engine_reset_resign(const aqg_engine* e, const aqg_resign* resign, void* stream) {
    if (!e || !resign) return fail("aqg_engine_reset_resign: null argument");
    return engine_reset_resign(*e, *resign, (hipStream_t)stream);
}
int aqg_engine_set_roots(const aqg_engine* e, const uint8_t* root_states72, void* stream) {
    if (!e || !root_states72) return fail("aqg_engine_set_roots: null argument");
    return engine_set_roots(*e, root_states72, (hipStream_t)stream);
}
int aqg_engine_search(const aqg_engine* e, const uint8_t* root_states72, void* stream) {
    if (!e || !root_states72) return fail("aqg_engine_search: null argument");
    return engine_search(*e, root_states72, (hipStream_t)stream);
}
int aqg_engine_root_visits(const aqg_engine* e, int32_t* visits, uint8_t* actions, int32_t* count, void* stream) {
    if (!e || !visits || !actions || !count) return fail("aqg_engine_root_visits: null argument");
    return engine_root_visits(*e, visits, actions, count, (hipStream_t)stream);
}

int aqg_engine_root_noise(const aqg_engine* e, void* stream) {
    if (!e) return fail("aqg_engine_root_noise: null engine");
    return engine_root_noise(*e, (hipStream_t)stream);
}
int aqg_engine_root_priors(const aqg_engine* e, float* priors, int32_t* count, void* stream) {
    if (!e || !priors || !count) return fail("aqg_engine_root_priors: null argument");
    return engine_root_priors(*e, priors, count, (hipStream_t)stream);
}
int aqg_engine_root_values(const aqg_engine* e, float* value, void* stream) {
    if (!e || !value) return fail("aqg_engine_root_values: null argument");
    return engine_root_values(*e, value, (hipStream_t)stream);
}
int aqg_engine_root_improved_policy(const aqg_engine* e, double c_visit, double c_scale, float* policy, uint8_t* actions, int32_t* count,
                                    float* vmix, void* stream) {
    if (!e || !policy || !actions || !count || !vmix) return fail("aqg_engine_root_improved_policy: null argument");
    return engine_root_improved_policy(*e, c_visit, c_scale, policy, actions, count, vmix, (hipStream_t)stream);
}

int aqg_engine_root_states72(const aqg_engine* e, uint8_t* out72, void* stream) {
    if (!e || !out72) return fail("aqg_engine_root_states72: null argument");
    return engine_root_states72(*e, out72, (hipStream_t)stream);
}
int aqg_engine_apply_actions(const aqg_engine* e, const int32_t* actions, void* stream) {
    if (!e || !actions) return fail("aqg_engine_apply_actions: null argument");
    return engine_apply_actions(*e, actions, (hipStream_t)stream);
}

// start positions (include/aqgnn.h, "start positions"): start NULL = the call without the table
int aqg_states72_check(int board_size, const uint8_t* states72, int B, int num_walls, int plies_for_draw, uint8_t* flags, void* stream) {
    if (B < 0 || (B > 0 && (!states72 || !flags))) return fail("aqg_states72_check: bad arguments");
    if (num_walls < 0 || num_walls > 127) return fail("aqg_states72_check: num_walls must be 0..127");
    if (plies_for_draw < 0 || plies_for_draw > 65535) return fail("aqg_states72_check: plies_for_draw must be 0..65535");
    return launch_states72_check(board_size, states72, B, num_walls, plies_for_draw, flags, (hipStream_t)stream);
}
int aqg_host_check_state(int board_size, const uint8_t* rec72_host, int num_walls, int plies_for_draw) {
    if (!rec72_host || num_walls < 0 || num_walls > 127 || plies_for_draw < 0 || plies_for_draw > 65535) return -1;
    return host_check_state(board_size, rec72_host, num_walls, plies_for_draw);
}
int aqg_engine_reset_start(const aqg_engine* e, const aqg_start_table* start, void* stream) {
    if (!e) return fail("aqg_engine_reset_start: null engine");
    return engine_reset(*e, (hipStream_t)stream, start);
}
int aqg_engine_move_start(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                          const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                          const aqg_start_table* start, void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_move_start: null argument");
    return engine_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, resign, policy, start}, (hipStream_t)stream);
}
int aqg_engine_finish_move_start(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                 const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                                 const aqg_start_table* start, void* stream) {
    if (!e || !uniforms) return fail("aqg_engine_finish_move_start: null argument");
    return engine_finish_move(*e, uniforms, MoveOptions{temperature_plies, hist_value, reuse, resign, policy, start}, (hipStream_t)stream);
}
int aqg_engine_apply_actions_start(const aqg_engine* e, const int32_t* actions, const aqg_start_table* start, void* stream) {
    if (!e || !actions) return fail("aqg_engine_apply_actions_start: null argument");
    if (int r = validate_start_table(*e, start, "aqg_engine_apply_actions_start")) return r;
    return engine_apply_actions(*e, actions, (hipStream_t)stream, start);
}

// Gumbel root search (include/aqgnn.h, "Gumbel root search"): no uniform is read, so `uniforms` may be NULL
int aqg_engine_move_gumbel(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                           const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                           const aqg_start_table* start, const aqg_gumbel* gumbel, void* stream) {
    if (!e || !gumbel) return fail("aqg_engine_move_gumbel: null argument");
    MoveOptions o{temperature_plies, hist_value, reuse, resign, policy, start};
    o.gumbel = gumbel;
    return engine_move(*e, uniforms, o, (hipStream_t)stream);
}
int aqg_engine_finish_move_gumbel(const aqg_engine* e, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                  const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                                  const aqg_start_table* start, const aqg_gumbel* gumbel, void* stream) {
    if (!e || !gumbel) return fail("aqg_engine_finish_move_gumbel: null argument");
    MoveOptions o{temperature_plies, hist_value, reuse, resign, policy, start};
    o.gumbel = gumbel;
    return engine_finish_move(*e, uniforms, o, (hipStream_t)stream);
}
int aqg_engine_search_gumbel(const aqg_engine* e, const uint8_t* root_states72, const aqg_gumbel* gumbel, void* stream) {
    if (!e || !root_states72 || !gumbel) return fail("aqg_engine_search_gumbel: null argument");
    return engine_search_gumbel(*e, root_states72, *gumbel, (hipStream_t)stream);
}
int aqg_engine_gumbel_root(const aqg_engine* e, const aqg_gumbel* gumbel, void* stream) {
    if (!e || !gumbel) return fail("aqg_engine_gumbel_root: null argument");
    return engine_gumbel_root(*e, *gumbel, (hipStream_t)stream);
}
int aqg_engine_root_gumbel(const aqg_engine* e, const aqg_gumbel* gumbel, float* gl, int32_t* m, int32_t* winner, void* stream) {
    if (!e || !gumbel || !gl || !m || !winner) return fail("aqg_engine_root_gumbel: null argument");
    return engine_root_gumbel(*e, *gumbel, gl, m, winner, (hipStream_t)stream);
}

static int check_draw_source(const char* what, const double* uniforms, int uniforms_stride) {
    if (uniforms && uniforms_stride < 0) return fail(what, "negative uniforms_stride");
    return 0;
}
int aqg_agent_random(int board_size, const uint8_t* states72, int B, const double* uniforms, int uniforms_stride, uint64_t seed,
                     int32_t* actions, void* stream) {
    const char* what = "aqg_agent_random";
    if (B < 0 || (B > 0 && (!states72 || !actions))) return fail(what, "bad arguments");
    if (int r = check_draw_source(what, uniforms, uniforms_stride)) return r;
    return launch_agent_random(board_size, states72, B, uniforms, uniforms_stride, seed, actions, (hipStream_t)stream);
}
int aqg_playouts(int board_size, const uint8_t* states72, int B, int plies_for_draw, const double* uniforms, int uniforms_stride,
                 uint64_t seed, int32_t* value, int32_t* plies, int32_t* draws, uint8_t* final72, void* stream) {
    const char* what = "aqg_playouts";
    if (B < 0 || (B > 0 && (!states72 || !value))) return fail(what, "bad arguments");
    if (plies_for_draw < 0 || plies_for_draw > 65535) return fail(what, "plies_for_draw must be 0..65535");
    if (int r = check_draw_source(what, uniforms, uniforms_stride)) return r;
    return launch_playouts(board_size, states72, B, plies_for_draw, uniforms, uniforms_stride, seed, value, plies, draws, final72,
                           (hipStream_t)stream);
}
size_t aqg_agent_mcts_workspace_bytes(int board_size, int B, int evaluations) {
    (void)board_size;
    return agent_mcts_workspace_bytes(B, evaluations);
}
int aqg_agent_mcts(int board_size, const uint8_t* states72, int B, int evaluations, int plies_for_draw, const double* explore,
                   const double* uniforms, int uniforms_stride, uint64_t seed, void* workspace, size_t workspace_bytes,
                   int32_t* action, int32_t* visits, uint8_t* actions, int32_t* count, int32_t* draws, void* stream) {
    const char* what = "aqg_agent_mcts";
    if (B < 0 || (B > 0 && (!states72 || !action || !explore || !workspace))) return fail(what, "bad arguments");
    if (evaluations < 0 || evaluations > AQG_AGENT_MCTS_MAX_EVALUATIONS) return fail(what, "evaluations must be 0..AQG_AGENT_MCTS_MAX_EVALUATIONS (2048)");
    if (plies_for_draw < 0 || plies_for_draw > 65535) return fail(what, "plies_for_draw must be 0..65535");
    if (int r = check_draw_source(what, uniforms, uniforms_stride)) return r;
    return launch_agent_mcts(board_size, states72, B, evaluations, plies_for_draw, explore, uniforms, uniforms_stride, seed, workspace,
                             workspace_bytes, action, visits, actions, count, draws, (hipStream_t)stream);
}

int aqg_agent_shortest_paths(int board_size, const uint8_t* states72, int B, int32_t* out, void* stream) {
    if (B < 0 || (B > 0 && (!states72 || !out))) return fail("aqg_agent_shortest_paths", "bad arguments");
    return launch_agent_shortest_paths(board_size, states72, B, out, (hipStream_t)stream);
}
size_t aqg_agent_alpha_beta_workspace_bytes(int board_size, int B, int max_depth) {
    return agent_alpha_beta_workspace_bytes(board_size, B, max_depth);
}
int aqg_agent_alpha_beta(int board_size, const uint8_t* states72, int B, const uint8_t* active, int plies_for_draw,
                         int max_dist_from_goal, int max_depth, void* workspace, size_t workspace_bytes, int32_t* action,
                         int64_t* nodes, void* stream) {
    const char* what = "aqg_agent_alpha_beta";
    if (B < 0 || (B > 0 && (!states72 || !action || !workspace))) return fail(what, "bad arguments");
    if (max_depth < 0 || max_depth > AQG_AGENT_AB_MAX_DEPTH) return fail(what, "max_depth must be 0..AQG_AGENT_AB_MAX_DEPTH (4)");
    if (plies_for_draw < 0 || plies_for_draw > 65535) return fail(what, "plies_for_draw must be 0..65535");
    if (max_dist_from_goal <= 0 || max_dist_from_goal > 65535) return fail(what, "max_dist_from_goal must be 1..65535");
    return launch_agent_alpha_beta(board_size, states72, B, active, plies_for_draw, max_dist_from_goal, max_depth, workspace,
                                   workspace_bytes, action, nodes, (hipStream_t)stream);
}

// The _optim entry points (include/aqgnn.h "optimiser controls"): the plain call's own checks first (it refuses what it always
// refused, under the name that was called), then the controls'; with optim NULL, the plain call itself.
int aqg_gcn_train_step(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                       void* stream) {
    if (int r = check_step(t, states72, pi_target, z_target, mode, "aqg_gcn_train_step")) return r;
    return train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream);
}
int aqg_gcn_train_step_optim(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                             const aqg_optim* optim, void* stream) {
    if (!optim) return aqg_gcn_train_step(t, states72, pi_target, z_target, mode, stream);
    const char* what = "aqg_gcn_train_step_optim";
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    return train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr);
}
long long aqg_gcn_train_fallbacks(int reset) { return train_fallbacks(reset); }
int aqg_gcn_train_steps(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, const int64_t* order,
                        long long positions, float* loss_sums, void* stream) {
    if (int r = check_steps(t, states72, pi_target, z_target, positions, "aqg_gcn_train_steps")) return r;
    return train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream);
}
int aqg_gcn_train_steps_optim(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                              const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim, void* stream) {
    if (!optim) return aqg_gcn_train_steps(t, states72, pi_target, z_target, order, positions, loss_sums, stream);
    const char* what = "aqg_gcn_train_steps_optim";
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    return train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr);
}

size_t aqg_gcn_train_general_workspace_floats(int board_size, int hidden, int num_layers, int policy_size, int max_batch) {
    return train_general_workspace_floats(board_size, hidden, num_layers, policy_size, max_batch);
}
int aqg_gcn_train_step_general(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                               int mode, void* stream) {
    if (int r = check_step(t, states72, pi_target, z_target, mode, "aqg_gcn_train_step_general")) return r;
    return train_step_general(*t, states72, pi_target, z_target, mode, (hipStream_t)stream);
}
int aqg_gcn_train_step_general_optim(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                                     int mode, const aqg_optim* optim, void* stream) {
    if (!optim) return aqg_gcn_train_step_general(t, states72, pi_target, z_target, mode, stream);
    const char* what = "aqg_gcn_train_step_general_optim";
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    return train_step_general(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr);
}
int aqg_gcn_train_steps_general(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                                const int64_t* order, long long positions, float* loss_sums, void* stream) {
    if (int r = check_steps(t, states72, pi_target, z_target, positions, "aqg_gcn_train_steps_general")) return r;
    return train_steps_general(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream);
}
int aqg_gcn_train_steps_general_optim(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                                      const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                                      void* stream) {
    if (!optim) return aqg_gcn_train_steps_general(t, states72, pi_target, z_target, order, positions, loss_sums, stream);
    const char* what = "aqg_gcn_train_steps_general_optim";
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    return train_steps_general(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr);
}

size_t aqg_cnn_train_workspace_floats(int board_size, int num_filters, int num_blocks, int policy_size, int max_batch) {
    return cnn_train_workspace_floats(board_size, num_filters, num_blocks, policy_size, max_batch);
}
int aqg_cnn_train_step(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                       void* stream) {
    if (int r = check_step(t, states72, pi_target, z_target, mode, "aqg_cnn_train_step")) return r;
    return cnn_train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream);
}
int aqg_cnn_train_step_optim(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                             const aqg_optim* optim, void* stream) {
    if (!optim) return aqg_cnn_train_step(t, states72, pi_target, z_target, mode, stream);
    const char* what = "aqg_cnn_train_step_optim";
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    return cnn_train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr);
}
int aqg_cnn_train_steps(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                        const int64_t* order, long long positions, float* loss_sums, void* stream) {
    if (int r = check_steps(t, states72, pi_target, z_target, positions, "aqg_cnn_train_steps")) return r;
    return cnn_train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream);
}
int aqg_cnn_train_steps_optim(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                              const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim, void* stream) {
    if (!optim) return aqg_cnn_train_steps(t, states72, pi_target, z_target, order, positions, loss_sums, stream);
    const char* what = "aqg_cnn_train_steps_optim";
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    return cnn_train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr);
}

size_t aqg_optim_workspace_floats(size_t n) { return optim_workspace_floats(n); }
int aqg_grad_norm(const float* x, size_t n, float* out, float* workspace, size_t workspace_floats, void* stream) {
    return launch_grad_norm(x, n, out, workspace, workspace_floats, (hipStream_t)stream);
}

// The _avg entry points (include/aqgnn.h "weight averaging"): avg NULL is the _optim call itself; otherwise the call's own checks,
// the controls' (optim may be NULL) and the average's, all in front of the first launch.
int aqg_weight_average_update(const aqg_weight_average* avg, void* stream) {
    if (int r = check_weight_average(avg, "aqg_weight_average_update")) return r;
    return launch_weight_average(*avg, (hipStream_t)stream);
}
int aqg_gcn_train_step_avg(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                           const aqg_optim* optim, const aqg_weight_average* avg, void* stream) {
    if (!avg) return aqg_gcn_train_step_optim(t, states72, pi_target, z_target, mode, optim, stream);
    const char* what = "aqg_gcn_train_step_avg";
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    if (int r = check_weight_average(avg, what)) return r;
    return train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr, avg);
}
int aqg_gcn_train_steps_avg(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                            const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                            const aqg_weight_average* avg, void* stream) {
    if (!avg) return aqg_gcn_train_steps_optim(t, states72, pi_target, z_target, order, positions, loss_sums, optim, stream);
    const char* what = "aqg_gcn_train_steps_avg";
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    if (int r = check_weight_average(avg, what)) return r;
    return train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr, avg);
}
int aqg_gcn_train_step_general_avg(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                                   int mode, const aqg_optim* optim, const aqg_weight_average* avg, void* stream) {
    if (!avg) return aqg_gcn_train_step_general_optim(t, states72, pi_target, z_target, mode, optim, stream);
    const char* what = "aqg_gcn_train_step_general_avg";
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    if (int r = check_weight_average(avg, what)) return r;
    return train_step_general(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr, avg);
}
int aqg_gcn_train_steps_general_avg(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                                    const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                                    const aqg_weight_average* avg, void* stream) {
    if (!avg) return aqg_gcn_train_steps_general_optim(t, states72, pi_target, z_target, order, positions, loss_sums, optim, stream);
    const char* what = "aqg_gcn_train_steps_general_avg";
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    if (int r = check_weight_average(avg, what)) return r;
    return train_steps_general(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr,
                               avg);
}
int aqg_cnn_train_step_avg(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                           const aqg_optim* optim, const aqg_weight_average* avg, void* stream) {
    if (!avg) return aqg_cnn_train_step_optim(t, states72, pi_target, z_target, mode, optim, stream);
    const char* what = "aqg_cnn_train_step_avg";
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    if (int r = check_weight_average(avg, what)) return r;
    return cnn_train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr, avg);
}
int aqg_cnn_train_steps_avg(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                            const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                            const aqg_weight_average* avg, void* stream) {
    if (!avg) return aqg_cnn_train_steps_optim(t, states72, pi_target, z_target, order, positions, loss_sums, optim, stream);
    const char* what = "aqg_cnn_train_steps_avg";
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = plan_optim(*t, optim, what, &plan, &on)) return r;
    if (int r = check_weight_average(avg, what)) return r;
    return cnn_train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr, avg);
}

// The _loss entry points (include/aqgnn.h "loss form"): the form's own refusals first; a NULL or default form is the _avg call
// itself; otherwise the call's checks, the controls' and the average's (either may be NULL), all in front of the first launch.
int aqg_policy_value_loss(int B, int A, const float* logits, const float* value, const float* pi, const float* z, const int64_t* order,
                          int first, const aqg_loss* lf, float* loss, float* dlogits, float* dvpre, void* stream) {
    const char* what = "aqg_policy_value_loss";
    if (B < 0 || A < 1 || A > 4096 || first < 0) return fail(what, "bad argument");
    if (!lf || !logits || !value || !pi || !z || !loss || !dlogits || !dvpre) return fail(what, "null argument");
    if (int r = check_loss_form(lf, what)) return r;
    if (lf->policy_form != 1) return fail(what, "policy_form must be 1 (cross-entropy)");
    return launch_policy_value_loss(B, A, logits, value, pi, z, order, first, lf->value_weight, loss, dlogits, dvpre, (hipStream_t)stream);
}
int aqg_gcn_train_step_loss(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                            const aqg_optim* optim, const aqg_weight_average* avg, const aqg_loss* lf, void* stream) {
    const char* what = "aqg_gcn_train_step_loss";
    if (int r = check_loss_form(lf, what)) return r;
    if (loss_form_is_default(lf)) return aqg_gcn_train_step_avg(t, states72, pi_target, z_target, mode, optim, avg, stream);
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = check_loss_call(t, optim, avg, what, &plan, &on)) return r;
    return train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr, avg, lf);
}
int aqg_gcn_train_steps_loss(const aqg_train* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                             const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                             const aqg_weight_average* avg, const aqg_loss* lf, void* stream) {
    const char* what = "aqg_gcn_train_steps_loss";
    if (int r = check_loss_form(lf, what)) return r;
    if (loss_form_is_default(lf))
        return aqg_gcn_train_steps_avg(t, states72, pi_target, z_target, order, positions, loss_sums, optim, avg, stream);
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = check_loss_call(t, optim, avg, what, &plan, &on)) return r;
    return train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr, avg, lf);
}
int aqg_gcn_train_step_general_loss(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                                    int mode, const aqg_optim* optim, const aqg_weight_average* avg, const aqg_loss* lf, void* stream) {
    const char* what = "aqg_gcn_train_step_general_loss";
    if (int r = check_loss_form(lf, what)) return r;
    if (loss_form_is_default(lf)) return aqg_gcn_train_step_general_avg(t, states72, pi_target, z_target, mode, optim, avg, stream);
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = check_loss_call(t, optim, avg, what, &plan, &on)) return r;
    return train_step_general(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr, avg, lf);
}
int aqg_gcn_train_steps_general_loss(const aqg_train_general* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                                     const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                                     const aqg_weight_average* avg, const aqg_loss* lf, void* stream) {
    const char* what = "aqg_gcn_train_steps_general_loss";
    if (int r = check_loss_form(lf, what)) return r;
    if (loss_form_is_default(lf))
        return aqg_gcn_train_steps_general_avg(t, states72, pi_target, z_target, order, positions, loss_sums, optim, avg, stream);
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = check_loss_call(t, optim, avg, what, &plan, &on)) return r;
    return train_steps_general(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr,
                               avg, lf);
}
int aqg_cnn_train_step_loss(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                            const aqg_optim* optim, const aqg_weight_average* avg, const aqg_loss* lf, void* stream) {
    const char* what = "aqg_cnn_train_step_loss";
    if (int r = check_loss_form(lf, what)) return r;
    if (loss_form_is_default(lf)) return aqg_cnn_train_step_avg(t, states72, pi_target, z_target, mode, optim, avg, stream);
    OptimPlan plan;
    bool on;
    if (int r = check_step(t, states72, pi_target, z_target, mode, what)) return r;
    if (int r = check_loss_call(t, optim, avg, what, &plan, &on)) return r;
    return cnn_train_step(*t, states72, pi_target, z_target, mode, (hipStream_t)stream, on ? &plan : nullptr, avg, lf);
}
int aqg_cnn_train_steps_loss(const aqg_cnn_train* t, const uint8_t* states72, const float* pi_target, const float* z_target,
                             const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                             const aqg_weight_average* avg, const aqg_loss* lf, void* stream) {
    const char* what = "aqg_cnn_train_steps_loss";
    if (int r = check_loss_form(lf, what)) return r;
    if (loss_form_is_default(lf))
        return aqg_cnn_train_steps_avg(t, states72, pi_target, z_target, order, positions, loss_sums, optim, avg, stream);
    OptimPlan plan;
    bool on;
    if (int r = check_steps(t, states72, pi_target, z_target, positions, what)) return r;
    if (int r = check_loss_call(t, optim, avg, what, &plan, &on)) return r;
    return cnn_train_steps(*t, states72, pi_target, z_target, order, positions, loss_sums, (hipStream_t)stream, on ? &plan : nullptr, avg,
                           lf);
}

int aqg_augment_gather(int board_size, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                       const uint8_t* flips, int use_seed, uint64_t seed, uint64_t epoch, int n, uint8_t* out72, float* out_pi,
                       float* out_z, void* stream) {
    return launch_augment_gather(board_size, policy_size, states72, pi, z, order, flips, use_seed, seed, epoch, n, out72, out_pi, out_z,
                                 (hipStream_t)stream);
}

int aqg_replay_append(int board_size, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8,
                      const float* pi, const float* z_f32, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                      float* ring_z, void* stream) {
    return launch_replay_append(board_size, policy_size, states72, visits, z_i8, pi, z_f32, n, capacity, head, ring72, ring_pi, ring_z,
                                (hipStream_t)stream);
}
int aqg_replay_append_blend(int board_size, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8,
                            const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                            float* ring_z, void* stream) {
    return launch_replay_append_blend(board_size, policy_size, states72, visits, z_i8, search_value, blend, n, capacity, head, ring72,
                                      ring_pi, ring_z, (hipStream_t)stream);
}
int aqg_replay_append_policy(int board_size, int policy_size, const uint8_t* states72, const float* pi, const int8_t* z_i8,
                             const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                             float* ring_z, void* stream) {
    return launch_replay_append_policy(board_size, policy_size, states72, pi, z_i8, search_value, blend, n, capacity, head, ring72,
                                       ring_pi, ring_z, (hipStream_t)stream);
}
int aqg_replay_refresh(int board_size, int policy_size, const int32_t* visits, const uint8_t* actions, const int32_t* count,
                       const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                       float* ring_z, void* stream) {
    return launch_replay_refresh(board_size, policy_size, visits, actions, count, search_value, blend, slots, n, capacity, ring_pi,
                                 ring_z, (hipStream_t)stream);
}
int aqg_replay_refresh_policy(int board_size, int policy_size, const float* policy, const uint8_t* actions, const int32_t* count,
                              const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                              float* ring_z, void* stream) {
    return launch_replay_refresh_policy(board_size, policy_size, policy, actions, count, search_value, blend, slots, n, capacity, ring_pi,
                                        ring_z, (hipStream_t)stream);
}

int aqg_replay_position_keys(const uint8_t* states72, const int64_t* index, int n, int64_t* keys, void* stream) {
    return launch_replay_position_keys(states72, index, n, keys, (hipStream_t)stream);
}
int aqg_replay_run_heads(const uint8_t* states72, const int64_t* perm, int n, uint8_t* heads, void* stream) {
    return launch_replay_run_heads(states72, perm, n, heads, (hipStream_t)stream);
}
size_t aqg_replay_merge_workspace_floats(int board_size, int n, int u) { return replay_merge_workspace_floats(board_size, n, u); }
int aqg_replay_merge_runs(int board_size, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* perm,
                          const int64_t* starts, int n, int u, uint8_t* out72, float* out_pi, float* out_z, int32_t* count,
                          float* workspace, size_t workspace_floats, void* stream) {
    return launch_replay_merge_runs(board_size, policy_size, states72, pi, z, perm, starts, n, u, out72, out_pi, out_z, count, workspace,
                                    workspace_floats, (hipStream_t)stream);
}

int aqg_replay_surprise_rows(int board_size, int policy_size, const float* net_policy, const float* ring_pi, const int64_t* index,
                             int rows, int m, int offset, int n, float* k, int32_t* q, void* stream) {
    return launch_replay_surprise_rows(board_size, policy_size, net_policy, ring_pi, index, rows, m, offset, n, k, q, (hipStream_t)stream);
}
int aqg_replay_surprise_counts(const int32_t* q, const int64_t* index, const int64_t* total, int m, long long expected_rows,
                               double uniform_share, int max_copies, uint64_t seed, uint64_t update, int32_t* count, void* stream) {
    return launch_replay_surprise_counts(q, index, total, m, expected_rows, uniform_share, max_copies, seed, update, count,
                                         (hipStream_t)stream);
}

int aqg_replay_row_metrics(int board_size, int policy_size, const float* net_policy, const float* net_value, const uint8_t* states72,
                           const float* ring_pi, const float* ring_z, const int64_t* index, int rows, int m, int offset, int n,
                           int bucket_plies, int buckets, double* vals, int32_t* tag, void* stream) {
    return launch_replay_row_metrics(board_size, policy_size, net_policy, net_value, states72, ring_pi, ring_z, index, rows, m, offset, n,
                                     bucket_plies, buckets, vals, tag, (hipStream_t)stream);
}
size_t aqg_row_metrics_workspace_doubles(int m, int buckets) { return row_metrics_workspace_doubles(m, buckets); }
int aqg_row_metrics_reduce(const double* vals, const int32_t* tag, int m, int buckets, double* partial, double* sums, int64_t* counts,
                           void* stream) {
    return launch_row_metrics_reduce(vals, tag, m, buckets, partial, sums, reinterpret_cast<long long*>(counts), (hipStream_t)stream);
}
int aqg_replay_holdout_mask(const int64_t* keys, int n, uint64_t seed, double share, uint8_t* mask, void* stream) {
    return launch_replay_holdout_mask(keys, n, seed, share, mask, (hipStream_t)stream);
}

int aqg_lambda_values(int quota, int hp, const int32_t* game_plies, const int8_t* game_result, const uint8_t* game_done,
                      const float* hist_value, float lambda, float* out, void* stream) {
    return launch_lambda_values(quota, hp, game_plies, game_result, game_done, hist_value, lambda, out, (hipStream_t)stream);
}

}  // extern "C"
