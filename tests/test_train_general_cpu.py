"""The any-shape training step without a GPU: the aqg_train_general layout against a C++ compile of the header, the host-side
argument checks of its entry points, GeneralTrainer's refusals, load_network and the shape options of create_network and
train_cycle."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = [(6, 64, 2), (6, 65, 1), (6, 256, 3), (6, 96, 4), (6, 1024, 1), (6, 128, 3)]


def _lib_or_skip():
    from alphaquoridorgnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: build first")
    return _lib, _lib.load()


def test_train_general_layout_matches_header(tmp_path):
    from alphaquoridorgnn_amd import _lib
    src = tmp_path / "layout.cpp"
    fields = ["num_features", "hidden", "num_layers", "policy_size", "batch", "step", "lr", "eps", "params", "grads", "adam_m",
              "adam_v", "policy", "value", "loss", "loss_mean", "workspace", "workspace_floats"]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\nint main() { std::printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(aqg_train_general)'
                   + "".join(f", offsetof(aqg_train_general, {f})" for f in fields) + "); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = _lib.TrainGeneralStruct
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]


def _struct(_lib, hidden=64, layers=2, A=41, N=5, batch=4, step=1, fill=True):
    t = _lib.TrainGeneralStruct()
    t.board_size, t.num_features, t.hidden, t.num_layers, t.policy_size, t.batch, t.step = N, 6, hidden, layers, A, batch, step
    t.lr, t.beta1, t.beta2, t.eps = 1e-3, 0.9, 0.999, 1e-8
    if fill:                                   # never dereferenced: every check below fails on the host before any launch
        for name in ("params", "grads", "adam_m", "adam_v"):
            arr = getattr(t, name)
            for i in range(min(2 * layers + 8, len(arr))):
                arr[i] = 4096
    t.workspace, t.workspace_floats = 4096, 1
    return t


def _err(lib):
    return lib.aqg_last_error().decode()


def test_entry_points_check_arguments_on_the_host():
    _lib, lib = _lib_or_skip()
    dummy = ctypes.c_void_p(4096)
    ok = _struct(_lib)
    assert lib.aqg_gcn_train_step_general(None, dummy, dummy, dummy, 1, None) < 0
    assert lib.aqg_gcn_train_step_general(ctypes.byref(ok), dummy, dummy, dummy, 3, None) < 0 and "bad argument" in _err(lib)
    assert lib.aqg_gcn_train_step_general(ctypes.byref(ok), None, dummy, dummy, 1, None) < 0 and "null argument" in _err(lib)
    cases = [(dict(N=4), "board_size"), (dict(hidden=1), "hidden"), (dict(hidden=2048), "hidden"), (dict(layers=0), "num_layers"),
             (dict(layers=33), "num_layers"), (dict(A=0), "policy_size"), (dict(A=5000), "policy_size"), (dict(step=0), "step"),
             (dict(fill=False), "null parameter")]
    for kw, msg in cases:
        t = _struct(_lib, **kw)
        assert lib.aqg_gcn_train_step_general(ctypes.byref(t), dummy, dummy, dummy, 1, None) < 0, kw
        assert msg in _err(lib), (kw, _err(lib))
    t = _struct(_lib)
    t.num_features = 8
    assert lib.aqg_gcn_train_step_general(ctypes.byref(t), dummy, dummy, dummy, 1, None) < 0 and "num_features" in _err(lib)
    t = _struct(_lib, batch=-1)
    assert lib.aqg_gcn_train_step_general(ctypes.byref(t), dummy, dummy, dummy, 0, None) < 0
    t = _struct(_lib)                                                                   # workspace of 1 float
    assert lib.aqg_gcn_train_step_general(ctypes.byref(t), dummy, dummy, dummy, 1, None) < 0 and "workspace too small" in _err(lib)
    assert lib.aqg_gcn_train_steps_general(ctypes.byref(t), dummy, dummy, dummy, None, 10, None, None) < 0
    assert "workspace too small" in _err(lib)
    t = _struct(_lib, batch=0)
    assert lib.aqg_gcn_train_steps_general(ctypes.byref(t), dummy, dummy, dummy, None, 10, None, None) < 0 and "batch" in _err(lib)
    assert lib.aqg_gcn_train_steps_general(ctypes.byref(ok), dummy, dummy, dummy, None, -1, None, None) < 0
    assert lib.aqg_gcn_train_steps_general(ctypes.byref(ok), None, dummy, dummy, None, 10, None, None) < 0


def test_workspace_floats():
    _lib, lib = _lib_or_skip()
    f = lib.aqg_gcn_train_general_workspace_floats
    assert f(4, 64, 2, 41, 8) == 0 and f(5, 1, 2, 41, 8) == 0 and f(5, 64, 0, 41, 8) == 0 and f(5, 64, 2, 41, 0) == 0
    sizes = [f(9, 64, 2, 209, b) for b in (1, 37, 128)]
    assert 0 < sizes[0] <= sizes[1] <= sizes[2]
    assert f(9, 256, 3, 209, 128) > f(9, 64, 2, 209, 128)


def test_general_trainer_refusals():
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import GeneralTrainer, GNNTrainer
    with pytest.raises(ValueError, match="6 feature planes"):
        GeneralTrainer(GraphPolicyValueNetwork(8, 64, 2, 209))
    with pytest.raises(ValueError, match="float32"):
        GeneralTrainer(GraphPolicyValueNetwork(6, 64, 2, 209).double())
    with pytest.raises(ValueError, match="exists for the default"):
        GNNTrainer(GraphPolicyValueNetwork(6, 64, 2, 209))                 # the fused trainer keeps refusing other shapes


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_load_network_round_trip(tmp_path, shape):
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork, POLICY_OUTPUT_SIZE, load_network
    torch.manual_seed(sum(shape))
    net = GraphPolicyValueNetwork(*shape, POLICY_OUTPUT_SIZE)
    path = str(tmp_path / "net.pth")
    torch.save(net.state_dict(), path)
    got = load_network(path, "cpu")
    assert isinstance(got, GNNNetwork) == (shape == (6, 128, 3))
    assert (got.num_features, got.hidden_dim, got.num_gcn_layers, got.policy_output_size) == shape + (POLICY_OUTPUT_SIZE,)
    sd = got.state_dict()
    assert list(sd) == list(net.state_dict()) and all(torch.equal(sd[k], v) for k, v in net.state_dict().items())


def test_create_network_shape(tmp_path, monkeypatch):
    from alphaquoridorgnn_amd import pv_network_gnn as pg
    monkeypatch.setattr(pg, "PV_NETWORK_PATH", str(tmp_path / "a") + "/")
    pg.create_network(hidden_dim=96, num_gcn_layers=4)
    m = pg.load_network(str(tmp_path / "a" / "best.pth"), "cpu")
    assert (m.hidden_dim, m.num_gcn_layers) == (96, 4)
    pg.create_network(hidden_dim=32, num_gcn_layers=1)                   # best.pth exists: nothing is written
    assert pg.load_network(str(tmp_path / "a" / "best.pth"), "cpu").hidden_dim == 96
    monkeypatch.setattr(pg, "PV_NETWORK_PATH", str(tmp_path / "b") + "/")
    pg.create_network()
    assert isinstance(pg.load_network(str(tmp_path / "b" / "best.pth"), "cpu"), pg.GNNNetwork)


def test_train_cycle_shape_options(tmp_path, monkeypatch):
    """--hidden-dim / --num-gcn-layers shape the best.pth that the cycle creates (the stages themselves are stubbed here)."""
    from alphaquoridorgnn_amd import pv_network_gnn as pg, train_cycle as tc
    monkeypatch.setattr(pg, "PV_NETWORK_PATH", str(tmp_path) + "/")
    monkeypatch.setattr(tc, "_STAGES", ())
    tc.main(["--cycles", "1", "--hidden-dim", "80", "--num-gcn-layers", "5"])
    m = pg.load_network(str(tmp_path / "best.pth"), "cpu")
    assert (m.num_features, m.hidden_dim, m.num_gcn_layers) == (6, 80, 5)
