"""ctypes binding of libaqgnn_hip.so (C ABI in include/aqgnn.h).

The HIP library IS the product path.  There is no CPU fallback: if the shared object is missing or a call
fails, this module raises -- loudly -- instead of computing anything on the host.
"""
import ctypes
import os

import torch

from .constants import MAX_LEGAL  # noqa: F401   (the numpy statements import it from there, without ctypes)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AQG_LIB_PATH", os.path.join(_HERE, "libaqgnn_hip.so"))  # override: diagnostic builds only
GNN_EXACT_F32 = 1        # AQG_GNN_EXACT_F32 (include/aqgnn.h)
GNN_RANGE_PROVEN = 2     # AQG_GNN_RANGE_PROVEN
GNN_PROVEN_MAX_WALLS = 16
ABI_VERSION = 15
AGENT_AB_MAX_DEPTH = 4     # AQG_AGENT_AB_MAX_DEPTH
TRAIN_PART_FLOATS = 2 * 128 * 128 + 128 * 6 + 3 * 128    # AQG_TRAIN_PART_FLOATS, per position of the batch
LIN_RELU, LIN_W_KN, LIN_ACCUMULATE = 1, 2, 4             # AQG_LIN_* flags of aqg_graph_linear

_c = ctypes
_vp, _i32, _f32 = _c.c_void_p, _c.c_int32, _c.c_float


class EngineStruct(_c.Structure):
    """Mirror of `struct aqg_engine` (include/aqgnn.h) up to eval_cache_log2 -- the ABI 10-13 layout; ABI 14 appends general_net
    (EngineStructGeneral, which the entry points take)."""
    _fields_ = (
        [(n, _i32) for n in ("board_size", "num_walls", "plies_for_draw", "num_games", "quota", "sims", "node_cap",
                             "max_plies", "prior_mode", "fake_bias", "gnn_flags")]
        + [("c_puct", _f32), ("temperature", _f32)]
        + [(n, _vp) for n in ("node_rec",
                              "node_count", "root_state", "path", "path_len",
                              "leaf_flag", "leaf_state",
                              "game_active", "slot_game", "game_plies", "game_result", "game_done", "game_slot", "game_first_move",
                              "legal_order", "legal_count", "pooled", "policy", "value",
                              "hist_state72", "hist_visits", "hist_action",
                              "counters", "stat_leaf_evals", "stat_terminal_sims", "packed_weights", "gnn_workspace",
                              "eval_cache_keys", "eval_cache_rows", "eval_cache_slot", "eval_mask", "stat_cache_hits", "eval_list", "eval_count")]
        + [("eval_cache_log2", _i32)]
    )


GENERAL_MAX_LAYERS = 32   # AQG_GENERAL_MAX_LAYERS


class GeneralNetStruct(_c.Structure):
    """Mirror of `struct aqg_gcn_general_net` (include/aqgnn.h, ABI 14): a network of any shape by reference to its parameters."""
    _fields_ = ([(n, _i32) for n in ("num_features", "hidden", "num_layers", "policy_size")]
                + [("params", _vp * (2 * GENERAL_MAX_LAYERS + 8))])


CNN_MAX_FILTERS, CNN_MAX_BLOCKS = 512, 40   # AQG_CNN_MAX_FILTERS, AQG_CNN_MAX_BLOCKS


class CnnNetStruct(_c.Structure):
    """Mirror of `struct aqg_cnn_net` (include/aqgnn.h): the residual CNN's shape and its packed buffer (aqg_cnn_pack)."""
    _fields_ = [(n, _i32) for n in ("board_size", "num_filters", "num_blocks", "policy_size")] + [("packed", _vp)]


class EngineStructGeneral(EngineStruct):
    """The whole `struct aqg_engine` of ABI 14: EngineStruct's fields (unchanged offsets) followed by `general_net`, the
    descriptor of prior_mode 3, and `cnn_net`, the descriptor of prior_mode 4.  The engine entry points take this one."""
    _fields_ = [("general_net", GeneralNetStruct), ("cnn_net", CnnNetStruct),
                # root exploration noise (appended: every earlier offset is unchanged; all zero = off)
                ("root_noise_eps", _f32), ("root_noise_alpha", _f32), ("root_noise_seed", _c.c_uint64), ("root_noise", _vp)]


class TreeReuseStruct(_c.Structure):
    """Mirror of `struct aqg_tree_reuse` (include/aqgnn.h, "tree reuse"): the option beside the engine struct."""
    _fields_ = [("keep_visits", _i32), ("kept", _vp), ("child_index", _vp), ("stat_moves_kept", _vp), ("stat_visits_kept", _vp)]


class ResignStruct(_c.Structure):
    """Mirror of `struct aqg_resign` (include/aqgnn.h, "resignation"): the option beside the engine struct."""
    _fields_ = [("threshold", _c.c_float), ("min_ply", _i32), ("disable_fraction", _c.c_double), ("seed", _c.c_uint64),
                ("resign_min", _vp), ("game_resigned", _vp)]


class PolicyRecordStruct(_c.Structure):
    """Mirror of `struct aqg_policy_record` (include/aqgnn.h, "recording completed-Q targets during self-play"): the option beside
    the engine struct."""
    _fields_ = [("c_visit", _c.c_double), ("c_scale", _c.c_double), ("hist_policy", _vp)]


class StartTableStruct(_c.Structure):
    """Mirror of `struct aqg_start_table` (include/aqgnn.h, "start positions"): the option beside the engine struct."""
    _fields_ = [("states72", _vp), ("index", _vp), ("count", _i32)]


class GumbelStruct(_c.Structure):
    """Mirror of `struct aqg_gumbel` (include/aqgnn.h, "Gumbel root search"): the option beside the engine struct."""
    _fields_ = [("table", _vp), ("seed", _c.c_uint64), ("scale", _c.c_double), ("considered", _i32), ("c_visit", _f32), ("c_scale", _f32),
                ("schedule", _vp), ("m", _vp)]


# the checker's flag bits (AQG_CHECK_*)
CHECK_BOARD, CHECK_WALLS, CHECK_WALL_COUNT, CHECK_SAME_SQUARE, CHECK_OVER, CHECK_ODD_PLY, CHECK_NO_PATH = 1, 2, 4, 8, 16, 32, 64


class TrainStruct(_c.Structure):
    """Mirror of `struct aqg_train` (include/aqgnn.h)."""
    _fields_ = (
        [(n, _i32) for n in ("board_size", "batch", "policy_size", "step")]
        + [(n, _f32) for n in ("lr", "beta1", "beta2", "eps")]
        + [(n, _vp * 14) for n in ("params", "grads", "adam_m", "adam_v")]
        + [(n, _vp) for n in ("h1", "h2", "g", "hp", "hv", "dhp", "dhv",
                              "lg", "pol", "vp", "val", "loss", "part")]
    )


class TrainGeneralStruct(_c.Structure):
    """Mirror of `struct aqg_train_general` (include/aqgnn.h): the training step of a network of any shape."""
    _fields_ = (
        [(n, _i32) for n in ("board_size", "num_features", "hidden", "num_layers", "policy_size", "batch", "step")]
        + [(n, _f32) for n in ("lr", "beta1", "beta2", "eps")]
        + [(n, _vp * (2 * GENERAL_MAX_LAYERS + 8)) for n in ("params", "grads", "adam_m", "adam_v")]
        + [(n, _vp) for n in ("policy", "value", "loss", "loss_mean", "workspace")]
        + [("workspace_floats", _c.c_size_t)]
    )


CNN_TRAIN_CONVS = 2 * 40 + 1            # AQG_CNN_TRAIN_CONVS: convs of the largest CNN (AQG_CNN_MAX_BLOCKS = 40)
CNN_TRAIN_TENSORS = 3 * CNN_TRAIN_CONVS + 4


class CnnTrainStruct(_c.Structure):
    """Mirror of `struct aqg_cnn_train` (include/aqgnn.h): the residual CNN's training step."""
    _fields_ = (
        [(n, _i32) for n in ("board_size", "num_filters", "num_blocks", "policy_size", "batch", "step")]
        + [(n, _f32) for n in ("lr", "beta1", "beta2", "eps")]
        + [(n, _f32 * CNN_TRAIN_CONVS) for n in ("bn_eps", "bn_momentum")]
        + [(n, _vp * CNN_TRAIN_TENSORS) for n in ("params", "grads")]
        + [(n, _vp * CNN_TRAIN_CONVS) for n in ("running_mean", "running_var")]
        + [(n, _vp) for n in ("adam_table", "policy", "value", "loss", "loss_mean", "workspace")]
        + [("workspace_floats", _c.c_size_t)]
    )


class OptimStruct(_c.Structure):
    """Mirror of `struct aqg_optim` (include/aqgnn.h, "optimiser controls"): the option beside a trainer struct.  weight_decay is a
    HOST array of num_tensors floats."""
    _fields_ = [("decoupled", _i32), ("num_tensors", _i32), ("weight_decay", _c.POINTER(_f32)), ("max_grad_norm", _f32),
                ("grad_norm", _vp), ("workspace", _vp), ("workspace_floats", _c.c_size_t)]


class WeightAverageStruct(_c.Structure):
    """Mirror of `struct aqg_weight_average` (include/aqgnn.h, "weight averaging"): the option beside a trainer struct.  table is the
    device copy of the 4 T + 1 words, host_table the host copy the library's checks read."""
    _fields_ = [("table", _vp), ("host_table", _c.POINTER(_c.c_int64)), ("num_tensors", _i32), ("every", _i32),
                ("total_chunks", _c.c_int64), ("decay", _f32)]


class LossStruct(_c.Structure):
    """Mirror of `struct aqg_loss` (include/aqgnn.h, "loss form"): the option beside a trainer struct.  policy_form 0 = the
    reference's loss, 1 = the cross-entropy on the logits; value_weight scales the value term's gradient."""
    _fields_ = [("policy_form", _i32), ("value_weight", _f32)]


WEIGHT_AVERAGE_CHUNK = 4096          # AQG_WEIGHT_AVERAGE_CHUNK
WEIGHT_AVERAGE_MAX_TENSORS = 1024    # AQG_WEIGHT_AVERAGE_MAX_TENSORS

SIGNATURES = {
    "aqg_abi_version": (_c.c_int, []),
    "aqg_last_error": (_c.c_char_p, []),
    "aqg_set_option": (_c.c_int, [_c.c_char_p, _c.c_int]),
    "aqg_debug_poison_lds": (_c.c_int, [_vp]),
    "aqg_debug_trace": (_c.c_int, [_vp, _c.c_uint]),
    "aqg_profile_collect": (_c.c_int, [_c.POINTER(_c.c_double), _c.POINTER(_c.c_longlong), _c.POINTER(_c.c_longlong), _c.c_int]),
    "aqg_legal_actions": (_c.c_int, [_c.c_int, _vp, _c.c_int, _vp, _vp, _vp, _vp]),
    "aqg_state_next": (_c.c_int, [_c.c_int, _vp, _vp, _c.c_int, _vp, _vp]),
    "aqg_state_status": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _vp, _vp]),
    "aqg_gcn_packed_floats": (_c.c_size_t, [_c.c_int]),
    "aqg_gcn_pack_weights_host": (_c.c_int, [_c.c_int, _c.POINTER(_vp), _vp]),
    "aqg_gcn_forward_boards": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _c.c_int, _vp]),
    "aqg_gcn_forward_boards_guarded": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _c.c_int, _vp, _vp]),
    "aqg_gcn_boards_any_workspace_floats": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "aqg_gcn_forward_boards_any": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _vp, _vp, _c.c_size_t, _vp, _vp, _vp, _vp, _vp, _c.c_int, _vp]),
    "aqg_graph_linear": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _c.c_int, _vp, _vp]),
    "aqg_graph_linear_grad_workspace_floats": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "aqg_graph_linear_grad": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _c.c_size_t, _vp, _vp, _vp]),
    "aqg_graph_aggregate": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _c.c_int, _vp, _vp]),
    "aqg_graph_mean_pool": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _c.c_int, _vp, _vp]),
    "aqg_graph_mean_pool_backward": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _c.c_int, _vp, _vp, _vp]),
    "aqg_graph_heads": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp]),
    "aqg_graph_heads_backward": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "aqg_gcn_boards_graph": (_c.c_int, [_c.c_int, _vp, _c.c_int, _vp, _vp, _vp, _vp]),
    "aqg_gcn_boards_general_workspace_floats": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "aqg_gcn_forward_boards_general": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _c.POINTER(GeneralNetStruct), _vp, _vp,
                                                  _c.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp]),
    "aqg_cnn_packed_floats": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "aqg_cnn_pack": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_vp), _c.POINTER(_f32), _vp, _vp]),
    "aqg_cnn_workspace_floats": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "aqg_cnn_forward_boards": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _c.POINTER(CnnNetStruct), _vp, _vp, _c.c_size_t, _vp, _vp,
                                          _vp, _vp, _vp, _vp]),
    "aqg_cnn_forward_planes": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.POINTER(CnnNetStruct), _vp, _vp, _c.c_size_t, _vp, _vp, _vp,
                                          _vp, _vp, _vp]),
    "aqg_engine_reset": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp]),
    "aqg_engine_clear_eval_cache": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp]),
    "aqg_engine_move": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp]),
    "aqg_engine_move_targets": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _vp]),
    "aqg_engine_search": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp]),
    "aqg_engine_begin_move": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp]),
    "aqg_engine_step": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.c_int, _c.c_int, _vp]),
    "aqg_engine_finish_move": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp]),
    "aqg_engine_finish_move_targets": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _vp]),
    "aqg_engine_move_reuse": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct), _vp]),
    "aqg_engine_finish_move_reuse": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct), _vp]),
    "aqg_engine_keep_subtrees": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.POINTER(TreeReuseStruct), _vp, _vp]),
    "aqg_engine_reset_reuse": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.POINTER(TreeReuseStruct), _vp]),
    "aqg_engine_move_resign": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                          _c.POINTER(ResignStruct), _vp]),
    "aqg_engine_finish_move_resign": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                                 _c.POINTER(ResignStruct), _vp]),
    "aqg_engine_reset_resign": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.POINTER(ResignStruct), _vp]),
    "aqg_engine_move_policy": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                          _c.POINTER(ResignStruct), _c.POINTER(PolicyRecordStruct), _vp]),
    "aqg_engine_finish_move_policy": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                                 _c.POINTER(ResignStruct), _c.POINTER(PolicyRecordStruct), _vp]),
    "aqg_engine_record_improved_policy": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.POINTER(PolicyRecordStruct), _vp]),
    "aqg_engine_set_roots": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp]),
    "aqg_engine_root_visits": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp, _vp, _vp]),
    "aqg_engine_root_noise": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp]),
    "aqg_engine_root_priors": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp, _vp]),
    "aqg_engine_root_values": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp]),
    "aqg_engine_root_improved_policy": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.c_double, _c.c_double, _vp, _vp, _vp, _vp, _vp]),
    "aqg_engine_root_states72": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp]),
    "aqg_engine_apply_actions": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _vp]),
    "aqg_states72_check": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _vp]),
    "aqg_host_check_state": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int]),
    "aqg_engine_reset_start": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.POINTER(StartTableStruct), _vp]),
    "aqg_engine_move_start": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                         _c.POINTER(ResignStruct), _c.POINTER(PolicyRecordStruct), _c.POINTER(StartTableStruct), _vp]),
    "aqg_engine_finish_move_start": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                                _c.POINTER(ResignStruct), _c.POINTER(PolicyRecordStruct), _c.POINTER(StartTableStruct), _vp]),
    "aqg_engine_apply_actions_start": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _c.POINTER(StartTableStruct), _vp]),
    "aqg_engine_move_gumbel": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                          _c.POINTER(ResignStruct), _c.POINTER(PolicyRecordStruct), _c.POINTER(StartTableStruct),
                                          _c.POINTER(GumbelStruct), _vp]),
    "aqg_engine_finish_move_gumbel": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _i32, _vp, _c.POINTER(TreeReuseStruct),
                                                 _c.POINTER(ResignStruct), _c.POINTER(PolicyRecordStruct), _c.POINTER(StartTableStruct),
                                                 _c.POINTER(GumbelStruct), _vp]),
    "aqg_engine_search_gumbel": (_c.c_int, [_c.POINTER(EngineStructGeneral), _vp, _c.POINTER(GumbelStruct), _vp]),
    "aqg_engine_gumbel_root": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.POINTER(GumbelStruct), _vp]),
    "aqg_engine_root_gumbel": (_c.c_int, [_c.POINTER(EngineStructGeneral), _c.POINTER(GumbelStruct), _vp, _vp, _vp, _vp]),
    "aqg_agent_random": (_c.c_int, [_c.c_int, _vp, _c.c_int, _vp, _c.c_int, _c.c_uint64, _vp, _vp]),
    "aqg_playouts": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _vp, _c.c_int, _c.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "aqg_agent_mcts_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "aqg_agent_mcts": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _c.c_int, _c.c_uint64, _vp, _c.c_size_t,
                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    "aqg_agent_shortest_paths": (_c.c_int, [_c.c_int, _vp, _c.c_int, _vp, _vp]),
    "aqg_agent_alpha_beta_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "aqg_agent_alpha_beta": (_c.c_int, [_c.c_int, _vp, _c.c_int, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_size_t, _vp, _vp, _vp]),
    "aqg_gcn_train_step": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _c.c_int, _vp]),
    "aqg_gcn_train_steps": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _vp]),
    "aqg_gcn_train_fallbacks": (_c.c_longlong, [_c.c_int]),
    "aqg_gcn_train_general_workspace_floats": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "aqg_gcn_train_step_general": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _c.c_int, _vp]),
    "aqg_gcn_train_steps_general": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _vp]),
    "aqg_cnn_train_workspace_floats": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "aqg_cnn_train_step": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _c.c_int, _vp]),
    "aqg_cnn_train_steps": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _vp]),
    "aqg_optim_workspace_floats": (_c.c_size_t, [_c.c_size_t]),
    "aqg_grad_norm": (_c.c_int, [_vp, _c.c_size_t, _vp, _vp, _c.c_size_t, _vp]),
    "aqg_gcn_train_step_optim": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct), _vp]),
    "aqg_gcn_train_steps_optim": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _c.POINTER(OptimStruct),
                                             _vp]),
    "aqg_gcn_train_step_general_optim": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct),
                                                    _vp]),
    "aqg_gcn_train_steps_general_optim": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp,
                                                     _c.POINTER(OptimStruct), _vp]),
    "aqg_cnn_train_step_optim": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct), _vp]),
    "aqg_cnn_train_steps_optim": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _c.POINTER(OptimStruct),
                                             _vp]),
    "aqg_weight_average_update": (_c.c_int, [_c.POINTER(WeightAverageStruct), _vp]),
    "aqg_gcn_train_step_avg": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct),
                                          _c.POINTER(WeightAverageStruct), _vp]),
    "aqg_gcn_train_steps_avg": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _c.POINTER(OptimStruct),
                                           _c.POINTER(WeightAverageStruct), _vp]),
    "aqg_gcn_train_step_general_avg": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct),
                                                  _c.POINTER(WeightAverageStruct), _vp]),
    "aqg_gcn_train_steps_general_avg": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp,
                                                   _c.POINTER(OptimStruct), _c.POINTER(WeightAverageStruct), _vp]),
    "aqg_cnn_train_step_avg": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct),
                                          _c.POINTER(WeightAverageStruct), _vp]),
    "aqg_cnn_train_steps_avg": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _c.POINTER(OptimStruct),
                                           _c.POINTER(WeightAverageStruct), _vp]),
    "aqg_policy_value_loss": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _c.c_int, _c.POINTER(LossStruct), _vp, _vp, _vp, _vp]),
    "aqg_gcn_train_step_loss": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct),
                                           _c.POINTER(WeightAverageStruct), _c.POINTER(LossStruct), _vp]),
    "aqg_gcn_train_steps_loss": (_c.c_int, [_c.POINTER(TrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _c.POINTER(OptimStruct),
                                            _c.POINTER(WeightAverageStruct), _c.POINTER(LossStruct), _vp]),
    "aqg_gcn_train_step_general_loss": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct),
                                                   _c.POINTER(WeightAverageStruct), _c.POINTER(LossStruct), _vp]),
    "aqg_gcn_train_steps_general_loss": (_c.c_int, [_c.POINTER(TrainGeneralStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp,
                                                    _c.POINTER(OptimStruct), _c.POINTER(WeightAverageStruct), _c.POINTER(LossStruct),
                                                    _vp]),
    "aqg_cnn_train_step_loss": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _c.c_int, _c.POINTER(OptimStruct),
                                           _c.POINTER(WeightAverageStruct), _c.POINTER(LossStruct), _vp]),
    "aqg_cnn_train_steps_loss": (_c.c_int, [_c.POINTER(CnnTrainStruct), _vp, _vp, _vp, _vp, _c.c_longlong, _vp, _c.POINTER(OptimStruct),
                                            _c.POINTER(WeightAverageStruct), _c.POINTER(LossStruct), _vp]),
    "aqg_augment_gather": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _c.c_int, _c.c_uint64, _c.c_uint64, _c.c_int, _vp, _vp, _vp,
                                      _vp]),
    "aqg_replay_append": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    "aqg_replay_append_blend": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _f32, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    "aqg_replay_append_policy": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _f32, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    "aqg_replay_refresh": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _f32, _vp, _c.c_int, _c.c_int, _vp, _vp, _vp]),
    "aqg_replay_refresh_policy": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _f32, _vp, _c.c_int, _c.c_int, _vp, _vp, _vp]),
    "aqg_replay_position_keys": (_c.c_int, [_vp, _vp, _c.c_int, _vp, _vp]),
    "aqg_replay_run_heads": (_c.c_int, [_vp, _vp, _c.c_int, _vp, _vp]),
    "aqg_replay_merge_workspace_floats": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "aqg_replay_merge_runs": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _c.c_size_t,
                                         _vp]),
    "aqg_replay_surprise_rows": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp]),
    "aqg_replay_surprise_counts": (_c.c_int, [_vp, _vp, _vp, _c.c_int, _c.c_longlong, _c.c_double, _c.c_int, _c.c_uint64, _c.c_uint64, _vp,
                                              _vp]),
    "aqg_replay_row_metrics": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                          _c.c_int, _vp, _vp, _vp]),
    "aqg_row_metrics_workspace_doubles": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "aqg_row_metrics_reduce": (_c.c_int, [_vp, _vp, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    "aqg_replay_holdout_mask": (_c.c_int, [_vp, _c.c_int, _c.c_uint64, _c.c_double, _vp, _vp]),
    "aqg_lambda_values": (_c.c_int, [_c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _f32, _vp, _vp]),
    "aqg_host_legal_actions": (_c.c_int, [_c.c_int, _vp, _vp]),
    "aqg_host_next": (_c.c_int, [_c.c_int, _vp, _c.c_int, _vp]),
    "aqg_host_shortest_path": (_c.c_int, [_c.c_int, _vp]),
    "aqg_host_heuristic_eval": (_c.c_double, [_c.c_int, _vp, _c.c_int]),
    "aqg_host_alpha_beta_action": (_c.c_int, [_c.c_int, _vp, _c.c_int, _c.c_int, _c.c_int]),
}

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load():
    """Load libaqgnn_hip.so; raises HipLibraryError if it is missing (build with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or alphaquoridorgnn_amd/csrc/build.sh")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.aqg_abi_version() != ABI_VERSION:
        raise HipLibraryError(f"ABI mismatch: library {lib.aqg_abi_version()} vs binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().aqg_last_error().decode(errors="replace")
        raise HipLibraryError(f"{what} failed: {msg}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "HIP entry points take contiguous device tensors"
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(device=None):
    if not torch.cuda.is_available():
        raise HipLibraryError("no MI355X visible (torch.cuda.is_available() is False): the hot path runs on the GPU only")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def set_option(name, value):
    check(load().aqg_set_option(name.encode(), int(value)), f"aqg_set_option({name})")


def profile_collect(reset=False):
    """(total_ms, launches, boards) of the profiled trunk launches so far (see aqg_profile_collect)."""
    ms, n, b = _c.c_double(0), _c.c_longlong(0), _c.c_longlong(0)
    check(load().aqg_profile_collect(_c.byref(ms), _c.byref(n), _c.byref(b), 1 if reset else 0), "aqg_profile_collect")
    return ms.value, n.value, b.value


def poison_lds(device=None):
    """Fill every CU's LDS with NaN patterns (tests: makes LDS read-before-write deterministic)."""
    check(load().aqg_debug_poison_lds(stream_ptr(device)), "aqg_debug_poison_lds")
