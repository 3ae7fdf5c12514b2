"""CPU tests (no GPU) of the engine's any-shape evaluator (prior_mode 3, ABI 14): the C ABI and its ctypes mirror, the argument
checks the library makes on the host before it launches anything, and the Python refusals."""
import ctypes
import os
import subprocess

import pytest
import torch

from tests import _util as U

REPO = U.REPO


def test_abi_version_15():
    from alphaquoridorgnn_amd import _lib
    assert _lib.ABI_VERSION == 15
    assert _lib.load().aqg_abi_version() == 15


def test_general_net_layout_matches_header(tmp_path):
    """Sizes and offsets of aqg_gcn_general_net and of the engine's general_net field, from a C++ compile of the header."""
    from alphaquoridorgnn_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\n'
                   "int main() { std::printf(\"%zu %zu %zu %zu %zu %zu %d\\n\", sizeof(aqg_gcn_general_net),"
                   " offsetof(aqg_gcn_general_net, hidden), offsetof(aqg_gcn_general_net, policy_size),"
                   " offsetof(aqg_gcn_general_net, params), sizeof(aqg_engine), offsetof(aqg_engine, general_net),"
                   " AQG_GENERAL_MAX_LAYERS); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    G, E = _lib.GeneralNetStruct, _lib.EngineStructGeneral
    assert got == [ctypes.sizeof(G), G.hidden.offset, G.policy_size.offset, G.params.offset, ctypes.sizeof(E), E.general_net.offset,
                   _lib.GENERAL_MAX_LAYERS]
    assert ctypes.sizeof(G) == 16 + (2 * 32 + 8) * 8
    assert E.general_net.offset == ctypes.sizeof(_lib.EngineStruct)        # appended: every ABI 13 offset is unchanged


def test_general_net_refuses_other_feature_counts():
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    with pytest.raises(ValueError, match="6 feature planes"):
        GraphPolicyValueNetwork(8, 64, 2, 209).general_net("cpu")


def test_engine_general_refuses_other_feature_counts():
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    with pytest.raises(ValueError, match="6 feature planes"):
        BatchedSelfPlay(GraphPolicyValueNetwork(8, 64, 2, 209), num_games=2, sims=4, evaluator="general")


def test_general_net_descriptor_points_at_parameters():
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    net = GraphPolicyValueNetwork(6, 64, 2, 17, board_size=3)
    d = net.general_net("cpu")
    assert (d.num_features, d.hidden, d.num_layers, d.policy_size) == (6, 64, 2, 17)
    params = [p for _, p in net._ordered_params()]
    assert len(params) == 2 * 2 + 8
    assert [d.params[i] for i in range(len(params))] == [p.data_ptr() for p in params]
    assert all(d.params[i] is None for i in range(len(params), 2 * 32 + 8))
    with pytest.raises(ValueError, match="float32"):
        net.double().general_net("cpu")
    key = net.float().general_weights_key()
    with torch.no_grad():
        net.gcn_layers[0].bias.add_(1.0)
    assert net.general_weights_key() != key


def _engine_struct(prior_mode, net=None, workspace=True, N=5):
    """An engine struct that passes every check but prior_mode 3's (dummy non-NULL pointers: the checks run before any launch)."""
    from alphaquoridorgnn_amd import _lib
    e = _lib.EngineStructGeneral()
    e.board_size, e.num_games, e.quota, e.sims, e.node_cap, e.prior_mode = N, 4, 4, 8, 1 + 8 * 136, prior_mode
    for name in ("slot_game", "game_done", "game_slot", "game_first_move"):
        setattr(e, name, 0x1000)
    e.gnn_workspace = 0x1000 if workspace else None
    if net is not None:
        e.general_net = net
    return e


def _full_net(A, L=2, hidden=64):
    from alphaquoridorgnn_amd import _lib
    d = _lib.GeneralNetStruct()
    d.num_features, d.hidden, d.num_layers, d.policy_size = 6, hidden, L, A
    for i in range(2 * L + 8):
        d.params[i] = 0x1000 + 64 * i
    return d


def test_engine_refuses_mode_3_without_descriptor_or_workspace():
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()

    def err(e):
        rc = lib.aqg_engine_begin_move(ctypes.byref(e), None)
        return rc, lib.aqg_last_error().decode()

    rc, msg = err(_engine_struct(3))
    assert rc != 0 and "general_net" in msg
    partial = _full_net(57)
    partial.params[5] = None
    rc, msg = err(_engine_struct(3, partial))
    assert rc != 0 and "general_net" in msg and "NULL" in msg
    rc, msg = err(_engine_struct(3, _full_net(57), workspace=False))
    assert rc != 0 and "gnn_workspace" in msg
    rc, msg = err(_engine_struct(3, _full_net(209)))                 # a 9x9 policy head on a 5x5 board (57 actions)
    assert rc != 0 and "policy_size" in msg
    bad = _full_net(57)
    bad.num_features = 8
    rc, msg = err(_engine_struct(3, bad))
    assert rc != 0 and "num_features" in msg
    rc, msg = err(_engine_struct(4, _full_net(57)))
    assert rc != 0 and "prior_mode" in msg


def test_forward_boards_general_argument_checks():
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    net = _full_net(41)
    ws = int(lib.aqg_gcn_boards_general_workspace_floats(5, 64, 41, 3))
    assert ws >= 3 * 25 * (6 + 5 + 5 + 2 * 64) + 3 * (64 + 64 + 41 + 1)
    assert lib.aqg_gcn_boards_general_workspace_floats(5, 64, 41, 0) == 0
    p = ctypes.c_void_p(0x1000)
    call = lambda N, fmt, B, d, w: lib.aqg_gcn_forward_boards_general(N, p, fmt, B, ctypes.byref(d), None, p, w, None, None, p,  # noqa: E731
                                                                        None, None, None)
    assert call(5, 0, 0, net, 0) == 0                                # no boards: nothing to do
    for N, fmt, B, d, w, what in ((4, 0, 3, net, ws, "board_size"), (5, 2, 3, net, ws, "state_fmt"),
                                  (5, 0, 3, net, ws - 1, "workspace"), (5, 0, -1, net, ws, "negative")):
        assert call(N, fmt, B, d, w) != 0
        assert what in lib.aqg_last_error().decode()
    for field, value in (("num_features", 5), ("hidden", 1), ("hidden", 1025), ("num_layers", 0), ("num_layers", 33),
                         ("policy_size", 0)):
        bad = _full_net(41)
        setattr(bad, field, value)
        assert call(5, 0, 3, bad, ws) != 0, (field, value)
