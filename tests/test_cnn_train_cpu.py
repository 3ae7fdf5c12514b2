"""The residual CNN's training step without a GPU: the aqg_cnn_train layout against a C++ compile of the header, the host-side
argument checks of its entry points, the workspace size, CNNTrainer's refusals, train_cycle's network options and the wording of
the GNN entry points' refusal."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _lib_or_fail():
    from alphaquoridorgnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: build first")
    return _lib, _lib.load()


def test_cnn_train_layout_matches_header(tmp_path):
    from alphaquoridorgnn_amd import _lib
    src = tmp_path / "layout.cpp"
    fields = ["board_size", "num_filters", "num_blocks", "policy_size", "batch", "step", "lr", "beta1", "beta2", "eps", "bn_eps",
              "bn_momentum", "params", "grads", "running_mean", "running_var", "adam_table", "policy", "value", "loss", "loss_mean",
              "workspace", "workspace_floats"]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\nint main() { std::printf("%zu %d %d'
                   + " %zu" * len(fields) + '\\n", sizeof(aqg_cnn_train), AQG_CNN_TRAIN_CONVS, AQG_CNN_TRAIN_TENSORS'
                   + "".join(f", offsetof(aqg_cnn_train, {f})" for f in fields) + "); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = _lib.CnnTrainStruct
    assert got == [ctypes.sizeof(T), _lib.CNN_TRAIN_CONVS, _lib.CNN_TRAIN_TENSORS] + [getattr(T, f).offset for f in fields]
    assert _lib.CNN_TRAIN_TENSORS == 247


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _struct(_lib, F=16, L=2, N=5, batch=4, step=1, fill=True):
    t = _lib.CnnTrainStruct()
    t.board_size, t.num_filters, t.num_blocks, t.policy_size, t.batch, t.step = N, F, L, _A(N), batch, step
    t.lr, t.beta1, t.beta2, t.eps = 1e-3, 0.9, 0.999, 1e-8
    C = 2 * min(max(L, 0), 40) + 1
    for i in range(C):
        t.bn_eps[i], t.bn_momentum[i] = 1e-5, 0.1
    if fill:                                   # never dereferenced: every check below fails on the host before any launch
        for i in range(3 * C + 4):
            t.params[i] = t.grads[i] = 4096
        for i in range(C):
            t.running_mean[i] = t.running_var[i] = 4096
        t.adam_table = 4096
    t.workspace, t.workspace_floats = 4096, 1
    return t


def _err(lib):
    return lib.aqg_last_error().decode()


def test_entry_points_check_arguments_on_the_host():
    _lib, lib = _lib_or_fail()
    d = ctypes.c_void_p(4096)
    step, steps = lib.aqg_cnn_train_step, lib.aqg_cnn_train_steps

    def rc_step(t, mode=1, s=d):
        return step(ctypes.byref(t), s, d, d, mode, None)

    assert step(None, d, d, d, 1, None) != 0 and "bad argument" in _err(lib)
    assert rc_step(_struct(_lib), mode=3) != 0 and "bad argument" in _err(lib)
    assert rc_step(_struct(_lib), s=None) != 0 and "null argument" in _err(lib)
    assert rc_step(_struct(_lib, N=4)) != 0 and "board_size" in _err(lib)
    assert rc_step(_struct(_lib, F=0)) != 0 and "num_filters" in _err(lib)
    assert rc_step(_struct(_lib, F=513)) != 0 and "num_filters" in _err(lib)
    assert rc_step(_struct(_lib, L=41)) != 0 and "num_blocks" in _err(lib)
    assert rc_step(_struct(_lib, L=-1)) != 0 and "num_blocks" in _err(lib)
    t = _struct(_lib)
    t.policy_size = 40
    assert rc_step(t) != 0 and "policy_size" in _err(lib)
    assert rc_step(_struct(_lib, fill=False)) != 0 and "null parameter" in _err(lib)
    t = _struct(_lib)
    t.running_var[3] = None
    assert rc_step(t) != 0 and "running statistics" in _err(lib)
    t = _struct(_lib)
    t.bn_momentum[0] = 1.5
    assert rc_step(t) != 0 and "bn_momentum" in _err(lib)
    t = _struct(_lib)
    t.bn_eps[2] = 0.0
    assert rc_step(t) != 0 and "bn_eps" in _err(lib)
    t = _struct(_lib)
    t.adam_table = None
    assert rc_step(t) != 0 and "adam_table" in _err(lib)
    assert rc_step(_struct(_lib, step=0)) != 0 and "step" in _err(lib)
    assert rc_step(_struct(_lib)) != 0 and "workspace too small" in _err(lib)
    t = _struct(_lib, batch=-1)
    assert rc_step(t, mode=0) != 0 and "negative batch" in _err(lib)
    assert rc_step(_struct(_lib, batch=0), mode=0) == 0                       # batch 0: nothing to do, nothing launched
    assert rc_step(_struct(_lib, batch=0), mode=0, s=None) == 0
    t = _struct(_lib)
    assert steps(ctypes.byref(t), d, d, d, None, -1, None, None) != 0 and "bad argument" in _err(lib)
    assert steps(ctypes.byref(t), None, d, d, None, 4, None, None) != 0 and "bad argument" in _err(lib)
    assert steps(ctypes.byref(_struct(_lib, batch=0)), d, d, d, None, 4, None, None) != 0 and "batch" in _err(lib)
    assert steps(ctypes.byref(t), d, d, d, None, 4, None, None) != 0 and "workspace too small" in _err(lib)
    assert steps(ctypes.byref(_struct(_lib, fill=False)), d, d, d, None, 4, None, None) != 0 and "null parameter" in _err(lib)


def test_workspace_size_limits_and_monotone_in_the_batch():
    _lib, lib = _lib_or_fail()
    ws = lib.aqg_cnn_train_workspace_floats
    assert ws(9, 128, 16, _A(9), 0) == 0
    assert ws(4, 16, 1, _A(4), 8) == 0
    assert ws(5, 0, 1, _A(5), 8) == 0 and ws(5, 513, 1, _A(5), 8) == 0
    assert ws(5, 16, 41, _A(5), 8) == 0 and ws(5, 16, -1, _A(5), 8) == 0
    assert ws(5, 16, 1, _A(7), 8) == 0
    for N, F, L in ((3, 1, 0), (5, 7, 1), (7, 65, 3), (9, 128, 16), (5, 512, 1), (3, 16, 40)):
        sizes = [int(ws(N, F, L, _A(N), b)) for b in (1, 2, 3, 31, 32, 33, 127, 128, 129, 256)]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes), (N, F, L, sizes)


def test_cnn_trainer_refusals():
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    with pytest.raises(ValueError, match="GPU"):
        CNNTrainer(CNNNetwork(8, 1, 5))
    with pytest.raises(ValueError, match="float32"):
        CNNTrainer(CNNNetwork(8, 1, 5).double())
    m = CNNNetwork(8, 1, 5)
    m.residual_blocks[0].conv_bn2.bn.momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        CNNTrainer(m)
    m = CNNNetwork(8, 1, 5)
    m.conv.bn.track_running_stats = False
    with pytest.raises(ValueError, match="track_running_stats"):
        CNNTrainer(m)
    with pytest.raises(ValueError, match="CNNNetwork"):
        CNNTrainer(torch.nn.Linear(2, 2))


def test_train_cycle_network_options(tmp_path, monkeypatch):
    """--network cnn / --num-filters / --num-residual-blocks shape the best.pth that the cycle creates (the stages are stubbed)."""
    from alphaquoridorgnn_amd import constants, pv_network_cnn as pc, pv_network_gnn as pg, train_cycle as tc
    monkeypatch.setattr(constants, "PV_NETWORK_PATH", str(tmp_path / "c") + "/")
    monkeypatch.setattr(tc, "_STAGES", ())
    tc.main(["--cycles", "1", "--network", "cnn", "--num-filters", "24", "--num-residual-blocks", "3"])
    sd = torch.load(str(tmp_path / "c" / "best.pth"), map_location="cpu", weights_only=True)
    assert pc.shape_of_state_dict(sd) == (24, 3, constants.BOARD_SIZE)
    tc.main(["--cycles", "1", "--network", "cnn", "--num-filters", "8"])        # best.pth exists: nothing is written
    sd = torch.load(str(tmp_path / "c" / "best.pth"), map_location="cpu", weights_only=True)
    assert pc.shape_of_state_dict(sd)[0] == 24
    monkeypatch.setattr(pg, "PV_NETWORK_PATH", str(tmp_path / "g") + "/")
    tc.main(["--cycles", "1"])                                                  # default: the GNN, as before
    assert isinstance(pg.load_network(str(tmp_path / "g" / "best.pth"), "cpu"), pg.GNNNetwork)
    with pytest.raises(SystemExit):
        tc.main(["--cycles", "1", "--network", "rnn"])


def test_parameter_update_dispatches_on_best_pth(tmp_path, monkeypatch):
    from alphaquoridorgnn_amd import constants, pv_network_cnn as pc, pv_network_gnn as pg, train_cycle as tc, train_network as tn
    monkeypatch.setattr(constants, "PV_NETWORK_PATH", str(tmp_path) + "/")
    calls = []
    monkeypatch.setattr(tn, "train_network", lambda: calls.append("gnn"))
    monkeypatch.setattr(tn, "train_cnn_network", lambda: calls.append("cnn"))
    tc.parameter_update()                                                       # no best.pth: the GNN's stage (which reports it)
    torch.save(pc.CNNNetwork(8, 1, 5).state_dict(), str(tmp_path / "best.pth"))
    tc.parameter_update()
    torch.save(pg.GNNNetwork().state_dict(), str(tmp_path / "best.pth"))
    tc.parameter_update()
    assert calls == ["gnn", "cnn", "gnn"]
    assert dict(tc._STAGES)["parameter update"] is tc.train_network             # run through parameter_update() by the cycle
    calls.clear()
    monkeypatch.setattr(pg, "PV_NETWORK_PATH", str(tmp_path) + "/")
    monkeypatch.setattr(tc, "self_play", lambda: None)
    monkeypatch.setattr(tc, "_STAGES", (("self-play", tc.self_play), ("parameter update", tc.train_network)))
    tc.train_cycle(num_cycles=1)
    assert calls == ["gnn"]


def test_gnn_entry_points_refusal_points_at_the_cnn_trainer():
    from alphaquoridorgnn_amd import train_network as tn
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    import re
    assert re.search("CNN.*not built yet", tn.CNN_TRAINING_NOT_BUILT)
    assert "CNNTrainer" in tn.CNN_TRAINING_NOT_BUILT and "train_cnn_network" in tn.CNN_TRAINING_NOT_BUILT
    with pytest.raises(NotImplementedError, match="CNN.*not built yet"):
        tn.trainer_for(CNNNetwork(8, 1, 5))
