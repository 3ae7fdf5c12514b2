"""GraphPolicyValueNetwork of any shape, host side (no GPU): construction within SHAPE_LIMITS with PyG's parameter names,
the refusals of the fused paths for a non-default shape, and _prepare_graph's num_features keyword."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = [(6, 64, 2), (6, 65, 1), (8, 96, 4), (6, 256, 3), (3, 32, 6), (6, 1024, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_any_shape_constructs_with_pyg_names(shape):
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, state_dict_keys
    F_, H, L = shape
    A = 37
    torch.manual_seed(0)
    net = GraphPolicyValueNetwork(F_, H, L, A)
    assert not net.fused
    sd = net.state_dict()
    assert set(sd) == set(state_dict_keys(L)) and len(sd) == 2 * L + 8
    hh = H // 2
    want = {"policy_head.0.weight": (hh, H), "policy_head.0.bias": (hh,), "policy_head.2.weight": (A, hh),
            "policy_head.2.bias": (A,), "value_head.0.weight": (hh, H), "value_head.0.bias": (hh,),
            "value_head.2.weight": (1, hh), "value_head.2.bias": (1,)}
    for i in range(L):
        want[f"gcn_layers.{i}.lin.weight"] = (H, F_ if i == 0 else H)
        want[f"gcn_layers.{i}.bias"] = (H,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    for i, layer in enumerate(net.gcn_layers):            # PyG's initialisation: Glorot-uniform lin, zero bias
        a = (6.0 / (layer.in_channels + layer.out_channels)) ** 0.5
        assert float(layer.lin.weight.detach().abs().max()) <= a and not layer.bias.detach().any()
    fresh = GraphPolicyValueNetwork(F_, H, L, A)
    fresh.load_state_dict(sd)
    assert all(torch.equal(fresh.state_dict()[k], v) for k, v in sd.items())


@pytest.mark.parametrize("arg,bad", [("num_features", 0), ("num_features", 1025), ("num_features", -3),
                                     ("hidden_dim", 1), ("hidden_dim", 0), ("hidden_dim", 1025),
                                     ("num_gcn_layers", 0), ("num_gcn_layers", 33),
                                     ("policy_output_size", 0), ("policy_output_size", 4097),
                                     ("hidden_dim", 64.0), ("num_gcn_layers", True)])
def test_out_of_range_shape_raises(arg, bad):
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, SHAPE_LIMITS
    kw = dict(num_features=6, hidden_dim=64, num_gcn_layers=2, policy_output_size=37)
    kw[arg] = bad
    lo, hi = SHAPE_LIMITS[arg]
    with pytest.raises(ValueError, match=rf"{arg} must be an integer in \[{lo}, {hi}\]"):
        GraphPolicyValueNetwork(**kw)


def test_shape_limits_are_inclusive():
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    net = GraphPolicyValueNetwork(1, 2, 1, 1)
    assert net.policy_head[0].out_features == 1 and net.value_head[2].in_features == 1
    net = GraphPolicyValueNetwork(1024, 3, 32, 4096)
    assert len(net.gcn_layers) == 32 and net.policy_head[2].out_features == 4096


def test_default_shape_keeps_state_dict_keys():
    from alphaquoridorgnn_amd.pv_network_gnn import (GraphPolicyValueNetwork, GNNNetwork, STATE_DICT_KEYS, state_dict_keys)
    assert state_dict_keys(3) == STATE_DICT_KEYS
    for net in (GraphPolicyValueNetwork(), GraphPolicyValueNetwork(6, 128, 3, 17, board_size=3), GNNNetwork()):
        assert net.fused
        assert set(net.state_dict()) == set(STATE_DICT_KEYS)
        assert [k for k, _ in net._ordered_params()] == STATE_DICT_KEYS


def test_non_default_shape_refuses_fused_paths():
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import GNNTrainer
    net = GraphPolicyValueNetwork(6, 64, 2, 209)
    assert pv_mcts.evaluator_of(net) == "external"
    assert pv_mcts.evaluator_of(GraphPolicyValueNetwork()) == "gnn"
    with pytest.raises(ValueError, match="autograd"):
        net.packed_weights(torch.device("cpu"))
    with pytest.raises(ValueError, match="evaluator='external'"):
        net.gnn_flags(torch.device("cpu"))
    with pytest.raises(ValueError, match="GNNTrainer"):
        GNNTrainer(net)


def test_prepare_graph_num_features():
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    prep = GraphPolicyValueNetwork._prepare_graph
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    batch = torch.zeros(3, dtype=torch.int64)
    ptr, src, w, gptr, G = prep(torch.randn(3, 8), ei, batch, num_features=8)
    assert G == 1 and ptr.tolist() == [0, 2, 4, 6] and gptr.tolist() == [0, 3]
    ref = prep(torch.randn(3, 6), ei, batch)
    assert all(torch.equal(a, b) for a, b in zip((ptr, src, w, gptr), ref[:4]))
    with pytest.raises(ValueError, match=r"\[num_nodes, 8\]"):
        prep(torch.randn(3, 6), ei, batch, num_features=8)
    with pytest.raises(ValueError, match=r"\[num_nodes, 6\]"):
        prep(torch.randn(3, 8), ei, batch)
    assert len(prep(torch.randn(3, 8), ei, batch, transpose=True, num_features=8)) == 8
