"""CPU tests (no GPU) of the reference's residual CNN (alphaquoridorgnn_amd/pv_network_cnn.py): its module surface and state_dict
against the reference's, the featuriser and the stock forward against fixtures the reference wrote, the C ABI of aqg_cnn_* and the
engine's prior_mode 4, and the host's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _util as U

REPO = U.REPO


def _triples(recs, N):
    nw = (N - 1) ** 2
    return [((int(r[0]), int(r[1])), (int(r[2]), int(r[3])), [int(w) for w in r[4:4 + nw]]) for r in recs]


def _golden_net(name):
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    g = U.golden(name)
    F, L, N = (int(v) for v in g["shape"])
    net = CNNNetwork(F, L, board_size=N)
    net.load_state_dict({k[len("param."):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("param.")})
    return net.eval(), g, N


def test_state_dict_matches_the_reference():
    from alphaquoridorgnn_amd import pv_network_cnn as cnn
    net = cnn.CNNNetwork()
    sd = net.state_dict()
    assert len(sd) == 202
    assert list(sd) == cnn.state_dict_keys(16)
    assert sum(p.numel() for p in net.parameters()) == 4_761_042
    assert sd["conv.conv.weight"].shape == (128, 6, 3, 3)
    assert sd["policy_head.1.weight"].shape == (209, 128) and sd["value_head.1.weight"].shape == (1, 128)
    assert (cnn.NUM_FILTERS, cnn.NUM_RESIDUAL_BLOCKS, cnn.INPUT_SHAPE, cnn.POLICY_OUTPUT_SIZE) == (128, 16, (6, 9, 9), 209)
    assert net.name == "CNN"
    # the golden fixture holds the reference's own state_dict keys (16 filters x 2 blocks)
    g = U.golden("cnn_9x9.npz")
    assert sorted(k[len("param."):] for k in g.files if k.startswith("param.")) == sorted(cnn.state_dict_keys(2))


def test_load_network_round_trips_a_cnn_state_dict(tmp_path):
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import load_network
    torch.manual_seed(0)
    net = CNNNetwork(24, 3, board_size=5)
    path = tmp_path / "best.pth"
    torch.save(net.state_dict(), path)
    got = load_network(str(path), device="cpu")
    assert isinstance(got, CNNNetwork) and not got.training
    assert (got.num_filters, got.num_residual_blocks, got.board_size, got.policy_output_size) == (24, 3, 5, 57)
    for (k, a), (k2, b) in zip(net.state_dict().items(), got.state_dict().items()):
        assert k == k2 and torch.equal(a, b)


@pytest.mark.parametrize("N", [3, 5, 9])
def test_preprocess_input_equals_reference_planes(N):
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    g = U.golden(f"feat_{N}x{N}.npz")
    planes = CNNNetwork(8, 0, board_size=N).preprocess_input(_triples(g["states"], N))
    assert planes.dtype == np.float32 and planes.shape == g["planes"].shape
    assert np.array_equal(planes.view(np.uint32), g["planes"].view(np.uint32))


@pytest.mark.parametrize("name", ["cnn_9x9.npz", "cnn_5x5.npz"])
def test_stock_forward_reproduces_the_reference(name):
    net, g, N = _golden_net(name)
    x = torch.from_numpy(net.preprocess_input(_triples(g["states"], N)))
    with torch.no_grad():
        policy, value = net(x)                       # a CPU tensor: the stock modules
    np.testing.assert_allclose(policy.numpy(), g["policy"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(value.numpy()[:, 0], g["value"], atol=1e-6, rtol=0)


def test_cnn_net_layout_matches_header(tmp_path):
    from alphaquoridorgnn_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\n'
                   "int main() { std::printf(\"%zu %zu %zu %zu %zu %zu %zu %d %d\\n\", sizeof(aqg_cnn_net),"
                   " offsetof(aqg_cnn_net, num_filters), offsetof(aqg_cnn_net, packed), sizeof(aqg_engine),"
                   " offsetof(aqg_engine, general_net), offsetof(aqg_engine, cnn_net), sizeof(aqg_gcn_general_net),"
                   " AQG_CNN_MAX_FILTERS, AQG_CNN_MAX_BLOCKS); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    C, E = _lib.CnnNetStruct, _lib.EngineStructGeneral
    assert got == [ctypes.sizeof(C), C.num_filters.offset, C.packed.offset, ctypes.sizeof(E), E.general_net.offset, E.cnn_net.offset,
                   ctypes.sizeof(_lib.GeneralNetStruct), _lib.CNN_MAX_FILTERS, _lib.CNN_MAX_BLOCKS]
    assert ctypes.sizeof(C) == 24
    assert E.general_net.offset == ctypes.sizeof(_lib.EngineStruct)                         # unchanged
    assert E.cnn_net.offset == E.general_net.offset + ctypes.sizeof(_lib.GeneralNetStruct)   # appended


@pytest.mark.parametrize("kw", [dict(num_filters=0), dict(num_filters=513), dict(num_residual_blocks=-1),
                                dict(num_residual_blocks=41), dict(board_size=4), dict(board_size=11), dict(num_filters=2.5)])
def test_shapes_outside_the_limits_are_refused(kw):
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    with pytest.raises(ValueError):
        CNNNetwork(**kw)


def test_shapes_at_the_limits_are_accepted():
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    CNNNetwork(1, 0, board_size=3)
    lib = _lib.load()
    assert lib.aqg_cnn_packed_floats(512, 40, 4096) > 0 and lib.aqg_cnn_packed_floats(1, 0, 1) > 0
    for bad in [(0, 2, 209), (513, 2, 209), (64, -1, 209), (64, 41, 209), (64, 2, 0), (64, 2, 4097)]:
        assert lib.aqg_cnn_packed_floats(*bad) == 0, bad
    assert lib.aqg_cnn_workspace_floats(9, 128, 209, 0) == 0 and lib.aqg_cnn_workspace_floats(4, 128, 209, 8) == 0


def _net_struct(N=5, F=32, L=2, A=57, packed=0x1000):
    from alphaquoridorgnn_amd import _lib
    d = _lib.CnnNetStruct()
    d.board_size, d.num_filters, d.num_blocks, d.policy_size, d.packed = N, F, L, A, packed
    return d


def _engine_struct(net=None, workspace=True, N=5):
    """An engine struct that passes every check but prior_mode 4's (dummy non-NULL pointers: the checks run before any launch)."""
    from alphaquoridorgnn_amd import _lib
    e = _lib.EngineStructGeneral()
    e.board_size, e.num_games, e.quota, e.sims, e.node_cap, e.prior_mode = N, 4, 4, 8, 1 + 8 * 136, 4
    for name in ("slot_game", "game_done", "game_slot", "game_first_move"):
        setattr(e, name, 0x1000)
    e.gnn_workspace = 0x1000 if workspace else None
    if net is not None:
        e.cnn_net = net
    return e


def test_engine_refuses_mode_4_without_descriptor_workspace_or_matching_policy():
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()

    def err(e):
        rc = lib.aqg_engine_begin_move(ctypes.byref(e), None)
        return rc, lib.aqg_last_error().decode()

    rc, msg = err(_engine_struct())
    assert rc != 0 and "cnn_net" in msg
    rc, msg = err(_engine_struct(_net_struct(packed=0)))
    assert rc != 0 and "cnn_net" in msg and "packed" in msg
    rc, msg = err(_engine_struct(_net_struct(), workspace=False))
    assert rc != 0 and "gnn_workspace" in msg
    rc, msg = err(_engine_struct(_net_struct(A=209)))                 # a 9x9 policy head on a 5x5 board (57 actions)
    assert rc != 0 and "policy_size" in msg
    rc, msg = err(_engine_struct(_net_struct(F=600)))
    assert rc != 0 and "num_filters" in msg
    rc, msg = err(_engine_struct(_net_struct(N=9, A=209)))           # the descriptor's board is not the engine's
    assert rc != 0 and "board_size" in msg
    e = _engine_struct(_net_struct())
    e.prior_mode = 5
    rc, msg = err(e)
    assert rc != 0 and "prior_mode" in msg


def test_forward_boards_argument_checks():
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    net = _net_struct()

    def call(N=5, fmt=0, B=4, d=net, ws=0x1000, nws=1 << 40, policy=0x1000):
        return lib.aqg_cnn_forward_boards(N, 0x1000, fmt, B, ctypes.byref(d), None, ws, nws, None, None, policy, None, None, None)

    assert call(N=4) != 0 and "board_size" in lib.aqg_last_error().decode()
    assert call(fmt=2) != 0 and "state_fmt" in lib.aqg_last_error().decode()
    assert call(nws=10) != 0 and "workspace" in lib.aqg_last_error().decode()
    assert call(policy=None) != 0 and "policy" in lib.aqg_last_error().decode()
    assert call(d=_net_struct(L=41)) != 0 and "num_blocks" in lib.aqg_last_error().decode()
    assert call(B=0) == 0                                               # nothing to do: no launch
    assert lib.aqg_cnn_pack(32, 2, 57, None, None, None, None) != 0


def test_train_network_refuses_a_cnn(tmp_path, monkeypatch):
    from alphaquoridorgnn_amd import train_network
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    torch.save(CNNNetwork(8, 1, board_size=5).state_dict(), tmp_path / "best.pth")
    monkeypatch.setattr(train_network, "PV_NETWORK_PATH", str(tmp_path) + "/")
    with pytest.raises(NotImplementedError, match="CNN.*not built yet"):
        train_network.train_network()
    with pytest.raises(NotImplementedError, match="not built yet"):
        train_network.trainer_for(CNNNetwork(8, 1, board_size=5))


def test_evaluator_of():
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork

    class _StockLike(torch.nn.Module):
        def predict(self, state, device):
            return None

    assert pv_mcts.evaluator_of(CNNNetwork(8, 1, board_size=5)) == "cnn"
    assert pv_mcts.evaluator_of(_StockLike()) == "external"
    assert pv_mcts.evaluator_of(GraphPolicyValueNetwork(6, 64, 2, 209)) == "external"
    assert pv_mcts.evaluator_of(GNNNetwork()) == "gnn"


def test_dropin_exposes_the_reference_surface():
    from alphaquoridorgnn_amd.dropin import pv_network_cnn as d
    for name in ("NUM_FILTERS", "NUM_RESIDUAL_BLOCKS", "INPUT_SHAPE", "POLICY_OUTPUT_SIZE", "ConvBN", "ResidualBlock", "CNNNetwork",
                 "create_network"):
        assert hasattr(d, name), name
