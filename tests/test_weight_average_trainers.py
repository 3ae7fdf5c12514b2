"""Weight averaging inside the three trainers' HIP steps, under data parallelism and in the training loop (include/aqgnn.h "weight
averaging", train_network.WeightAverage): the feature trains nothing differently, and the average is weight_average_reference applied
to a twin trainer's parameter snapshots at the multiples of `every`."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_cnn import _make_net as _make_cnn, _states   # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["gnn-3x3", "gnn-9x9", "general-3x3", "cnn-3x3"]
ROWS, B = 20, 8                            # three steps per epoch call, the last one of four rows


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _make(kind, dev, **controls):
    """A trainer on a freshly seeded network of `kind`: two calls give bit-identical parameters."""
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer
    N = int(kind[-1])
    torch.manual_seed(11)
    if kind.startswith("cnn"):
        return CNNTrainer(_make_cnn(4, 1, N, seed=11).to(dev), max_batch=B, **controls)
    fused = kind.startswith("gnn")
    net = GraphPolicyValueNetwork(6, 128 if fused else 16, 3 if fused else 2, _A(N), board_size=N)
    return (GNNTrainer if fused else GeneralTrainer)(net.to(dev), max_batch=B, **controls)


_DATA = {}


def _data(N, dev):
    """ROWS positions with random probability and value targets and the two epochs' orders, made once per board size."""
    if N not in _DATA:
        rng = np.random.RandomState(N)
        A = _A(N)
        pi = rng.rand(ROWS, A) * (rng.rand(ROWS, A) < 0.3)
        pi[:, 0] += 1e-3
        pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
        z = rng.choice([-1.0, 0.0, 1.0], ROWS).astype(np.float32)
        orders = [torch.from_numpy(rng.permutation(ROWS)).to(dev) for _ in range(2)]
        _DATA[N] = tuple(torch.from_numpy(x).to(dev) for x in (_states(N, ROWS), pi, z)) + (orders,)
    return _DATA[N]


def _state(tr):
    return [x.detach().clone() for x in tr.params + tr.buffers + tr.adam_m + tr.adam_v]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _snapshot(tr):
    return [x.detach().cpu().numpy().copy() for x in tr.params + tr.buffers]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _twin_reference(kind, dev, every, decays, controls):
    """The twin without an average, stepped one batch at a time: (its final state, the reference applied to its snapshots at the
    multiples of `every`, the number of updates).  decays[c] is the decay in force during epoch call c."""
    from alphaquoridorgnn_amd.train_network import weight_average_reference
    tr = _make(kind, dev, **controls)
    S, P, Z, orders = _data(tr.N, dev)
    want, step, updates = _snapshot(tr), 0, 0
    for order, decay in zip(orders, decays):
        for i in range(0, ROWS, B):
            idx = order[i:i + B]
            tr.step(S[idx], P[idx], Z[idx], lr=2e-3)
            step += 1
            if step % every == 0:
                want = [weight_average_reference(w, p, decay) for w, p in zip(want, _snapshot(tr))]
                updates += 1
    assert tr.step_count == step == 6
    return _state(tr), want, updates


def _run(kind, dev, every, decays, controls):
    from alphaquoridorgnn_amd.train_network import WeightAverage
    S, P, Z, orders = _data(int(kind[-1]), dev)
    plain = _make(kind, dev, **controls)
    plain_sums = [plain.run_epoch(S, P, Z, order, lr=2e-3).clone() for order in orders]
    tr = _make(kind, dev, **controls)
    avg = WeightAverage(tr, decay=decays[0], every=every)
    assert tr.average is avg and avg.updates == 0
    assert len(avg.tensors()) == len(tr.params) + len(tr.buffers)
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(avg.tensors(), tr.params + tr.buffers))
    sums = []
    for order, decay in zip(orders, decays):
        avg.decay = decay                                # a plain attribute, read at every call
        sums.append(tr.run_epoch(S, P, Z, order, lr=2e-3).clone())
    # the feature trains nothing differently: parameters (and running statistics), moments and loss sums, bit for bit
    assert _same(_state(tr), _state(plain)), kind
    assert _same(sums, plain_sums), kind
    twin_state, want, updates = _twin_reference(kind, dev, every, decays, controls)
    assert _same(_state(tr), twin_state), kind
    assert avg.updates == updates == 6 // every
    for k, (e, w) in enumerate(zip(avg.tensors(), want)):
        assert np.array_equal(_bits(e.cpu().numpy()), _bits(w)), (kind, every, k)
    assert any(not torch.equal(e, p) for e, p in zip(avg.tensors(), tr.params))      # (an average, not a copy of the last iterate)
    return tr, avg


@pytest.mark.parametrize("every", (1, 2, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_average_inside_the_steps(dev, kind, every):
    """Two run_epoch calls of three steps each (n = 20 at batch 8): with K = 2 the update of step 4, with K = 3 that of step 6 falls
    on a step of the second call.  The decay changes between the calls and takes effect."""
    tr, avg = _run(kind, dev, every, (0.9, 0.5), {})
    if kind.startswith("cnn"):                           # the running statistics are shadowed, num_batches_tracked is the model's
        sd, model = avg.state_dict(), tr.model.state_dict()
        assert list(sd.keys()) == list(model.keys())
        tracked = [k for k in sd if k.endswith("num_batches_tracked")]
        assert tracked and all(int(sd[k]) == 6 and sd[k].dtype == torch.int64 for k in tracked)
        stats = [k for k in sd if k.endswith("running_mean") or k.endswith("running_var")]
        assert len(stats) == len(tr.buffers) and all(k in avg.keys for k in stats)
        assert any(not torch.equal(sd[k], model[k]) for k in stats)


@pytest.mark.parametrize("kind", KINDS)
def test_average_beside_the_optimiser_controls(dev, kind):
    """Weight decay and clipping on: the _avg entry points get the controls' struct beside the average's."""
    tr, _ = _run(kind, dev, 2, (0.9, 0.9), dict(weight_decay=1e-2, max_grad_norm=0.5))
    assert tr.grad_norms.numel() == 3 and bool(torch.isfinite(tr.grad_norms).all())


@pytest.mark.parametrize("kind", KINDS)
def test_single_steps_state_dict_and_copy_to(dev, kind):
    """step(update=False) makes no update; step(update=True) makes the one of its step number; state_dict() loads into a module of the
    same shape and copy_to writes the same values, advancing version counters."""
    from alphaquoridorgnn_amd.train_network import WeightAverage, weight_average_reference
    tr = _make(kind, dev)
    S, P, Z, _ = _data(tr.N, dev)
    avg = WeightAverage(tr, decay=0.5, every=2)
    start = _snapshot(tr)
    tr.step(S[:B], P[:B], Z[:B], update=False)
    tr.step(S[:B], P[:B], Z[:B])                         # step 1: not a multiple of 2
    assert avg.updates == 0 and all(np.array_equal(e.cpu().numpy(), w) for e, w in zip(avg.tensors(), start))
    tr.step(S[B:2 * B], P[B:2 * B], Z[B:2 * B])          # step 2
    want = [weight_average_reference(w, p, 0.5) for w, p in zip(start, _snapshot(tr))]
    tr.step(S[:B], P[:B], Z[:B], update=False)           # (a CNN's forward moves its running statistics: snapshot taken before)
    assert avg.updates == 1
    for e, w in zip(avg.tensors(), want):
        assert np.array_equal(_bits(e.cpu().numpy()), _bits(w)), kind
    avg.update()                                         # the stand-alone launch
    want = [weight_average_reference(w, p, 0.5) for w, p in zip(want, _snapshot(tr))]
    assert avg.updates == 2 and all(np.array_equal(_bits(e.cpu().numpy()), _bits(w)) for e, w in zip(avg.tensors(), want))
    sd = avg.state_dict()
    a, b = _make(kind, dev).model, _make(kind, dev).model
    a.load_state_dict(sd)
    versions = [x._version for x in b.state_dict().values()]
    avg.copy_to(b)
    for (k, x), y, v in zip(a.state_dict().items(), b.state_dict().values(), versions):
        if k in avg.keys:
            assert torch.equal(x, y) and y._version > v, (kind, k)
        else:                                            # num_batches_tracked: loaded from the state, left alone by copy_to
            assert torch.equal(x, tr.model.state_dict()[k]) and y._version == v, (kind, k)
    for k, w in zip(avg.keys, want):
        assert np.array_equal(_bits(sd[k].cpu().numpy()), _bits(w)), (kind, k)


def test_for_module_on_the_gpu(dev):
    """WeightAverage.for_module on a GPU module: the HIP launch is the backend, update() by the user, no trainer involved."""
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import WeightAverage, weight_average_reference
    torch.manual_seed(2)
    net = GraphPolicyValueNetwork(6, 16, 2, 17, board_size=3).to(dev)
    avg = WeightAverage.for_module(net, 0.999)
    assert not avg.host and avg.trainer is None
    want = [p.detach().cpu().numpy().copy() for p in net.parameters()]
    for k in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        avg.update()
        want = [weight_average_reference(w, p.detach().cpu().numpy(), 0.999) for w, p in zip(want, net.parameters())]
    assert avg.updates == 3
    for e, w in zip(avg.tensors(), want):
        assert np.array_equal(_bits(e.cpu().numpy()), _bits(w))
    assert list(avg.state_dict().keys()) == list(net.state_dict().keys())


def test_entry_point_refuses_a_bad_average_before_any_launch(dev):
    """aqg_gcn_train_step_avg with an average the library refuses: -1 under the entry point's name, parameters, moments and average
    untouched -- and a Python-side bad decay is refused before the call."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_network import WeightAverage
    tr = _make("gnn-3x3", dev)
    S, P, Z, _ = _data(3, dev)
    avg = WeightAverage(tr, decay=0.9)
    tr.step(S[:B], P[:B], Z[:B])
    before, shadows = _state(tr), [e.clone() for e in avg.tensors()]
    tr.t.step = 2
    for field, value in (("decay", 1.0), ("every", 0), ("num_tensors", 0), ("total_chunks", avg.total_chunks + 1)):
        a = avg._struct()
        setattr(a, field, value)
        rc = tr.lib.aqg_gcn_train_step_avg(ctypes.byref(tr.t), _lib.ptr(S[:B]), _lib.ptr(P[:B]), _lib.ptr(Z[:B]), 1, None, ctypes.byref(a),
                                           _lib.stream_ptr(dev))
        assert rc == -1 and b"aqg_gcn_train_step_avg" in tr.lib.aqg_last_error(), field
        torch.cuda.synchronize()
        assert _same(_state(tr), before) and _same(avg.tensors(), shadows), field
    avg.decay = 1.0
    with pytest.raises(ValueError):
        tr.step(S[:B], P[:B], Z[:B])
    torch.cuda.synchronize()
    assert _same(avg.tensors(), shadows)


# ------------------------------------------------------------------ data parallel
_DP_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np, torch, torch.distributed as dist
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
from alphaquoridorgnn_amd.train_network import GNNTrainer, WeightAverage, weight_average_reference
rank = int(os.environ["RANK"])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + os.environ["AQG_PORT"], rank=rank, world_size=2)
d = np.load(os.environ["AQG_DATA"])
torch.manual_seed(5)
m = GraphPolicyValueNetwork(policy_output_size=17, board_size=3).to("cuda")
tr = GNNTrainer(m, max_batch=8)
avg = WeightAverage(tr, decay=0.9, every=2)
want = [p.detach().cpu().numpy().copy() for p in tr.params]
for i in range(4):
    sl = slice(rank, None, 2) if i != 2 else (slice(0, None) if rank == 0 else slice(0, 0))   # step 3: rank 1 holds nothing
    tr.step(torch.from_numpy(d["s"][8 * i:8 * i + 8][sl]), torch.from_numpy(d["p"][8 * i:8 * i + 8][sl]),
            torch.from_numpy(d["z"][8 * i:8 * i + 8][sl]))
    if (i + 1) % 2 == 0:
        want = [weight_average_reference(w, p.detach().cpu().numpy(), 0.9) for w, p in zip(want, tr.params)]
out = {f"avg{k}": e.cpu().numpy() for k, e in enumerate(avg.tensors())}
out.update({f"want{k}": w for k, w in enumerate(want)})
np.savez(os.environ["AQG_OUT"] + f".{rank}.npz", updates=avg.updates, **out)
dist.destroy_process_group()
'''


def test_data_parallel_ranks_keep_identical_averages(dev, tmp_path):
    """Two ranks on one GPU over gloo, four steps, the third with an empty shard on rank 1 (the mode-2 update of an empty batch):
    both ranks' averages are identical and equal the reference applied to rank 0's own post-step parameters."""
    rng = np.random.RandomState(4)
    pi = rng.rand(32, 17).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    np.savez(tmp_path / "data.npz", s=_states(3, 32), p=pi, z=rng.choice([-1.0, 0.0, 1.0], 32).astype(np.float32))
    (tmp_path / "worker.py").write_text(_DP_WORKER)
    env = dict(os.environ, AQG_REPO=REPO, AQG_PORT=str(29900 + os.getpid() % 300), AQG_DATA=str(tmp_path / "data.npz"),
               AQG_OUT=str(tmp_path / "out"))
    procs = [subprocess.Popen([sys.executable, str(tmp_path / "worker.py")], env=dict(env, RANK=str(r))) for r in range(2)]
    assert all(p.wait(timeout=300) == 0 for p in procs)
    outs = [np.load(str(tmp_path / "out") + f".{r}.npz") for r in range(2)]
    assert int(outs[0]["updates"]) == int(outs[1]["updates"]) == 2
    for k in range(14):
        assert np.array_equal(_bits(outs[0][f"avg{k}"]), _bits(outs[1][f"avg{k}"])), k
        assert np.array_equal(_bits(outs[0][f"avg{k}"]), _bits(outs[0][f"want{k}"])), k


# ------------------------------------------------------------------ the loop
def _loop_fixture(kind, dev, tmp_path, monkeypatch):
    from alphaquoridorgnn_amd import train_network as tn
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.replay import ReplayWindow
    N = int(kind[-1])
    path = str(tmp_path) + "/"
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(tn, "PV_NETWORK_PATH", path)
    monkeypatch.setattr(tn, "NUM_EPOCH", 2)
    monkeypatch.setattr(tn, "BATCH_SIZE", B)
    for k in ("TRAIN_EMA_DECAY", "TRAIN_EMA_EVERY"):
        monkeypatch.setattr(tn, k, getattr(tn, k))
    torch.manual_seed(3)
    net = _make_cnn(4, 1, N, seed=3) if kind.startswith("cnn") else GraphPolicyValueNetwork(6, 16, 2, _A(N), board_size=N)
    torch.save(net.state_dict(), path + "best.pth")
    S, P, Z, _ = _data(N, dev)
    window = ReplayWindow(N, max_generations=1, device=dev)
    window.append_rows(S, P, Z)
    monkeypatch.setattr(tn, "TRAIN_WINDOW", window)
    return tn, path, window


def _loop_run(tn, kind, path):
    torch.manual_seed(21)                                # the epochs' shuffles
    (tn.train_cnn_network if kind.startswith("cnn") else tn.train_network)()
    with open(path + "latest.pth", "rb") as f:
        data = f.read()
    return data, torch.load(path + "latest.pth", map_location="cpu", weights_only=True)


@pytest.mark.parametrize("kind", ["general-9x9", "cnn-3x3"])
def test_loop_saves_the_average(dev, tmp_path, monkeypatch, capsys, kind):
    """NUM_EPOCH = 2 on a 20-row window at batch 8: TRAIN_EMA_DECAY = 0.9 writes the reference applied to a hand-run twin loop under
    the same seed; 0.0 writes the option-off file's tensors; unset writes, byte for byte, what the twin's last iterate saves to."""
    from alphaquoridorgnn_amd.pv_network_cnn import load_network as load_cnn
    from alphaquoridorgnn_amd.pv_network_gnn import load_network
    tn, path, window = _loop_fixture(kind, dev, tmp_path, monkeypatch)
    cnn = kind.startswith("cnn")
    off_bytes, off = _loop_run(tn, kind, path)
    assert "weight average" not in capsys.readouterr().out
    # the hand-run twin: the loop's own epochs, one step at a time
    torch.manual_seed(21)
    model = (load_cnn if cnn else load_network)(path + "best.pth", dev)
    tr = tn.CNNTrainer(model, max_batch=B) if cnn else tn.trainer_for(model, max_batch=B)
    S, P, Z = window.tensors()
    index = window.index()
    want, step = _snapshot(tr), 0
    keys = {x.data_ptr(): k for k, x in model.state_dict().items()}
    keys = [keys[x.data_ptr()] for x in tr.params + tr.buffers]
    for epoch in range(2):
        order = index[torch.randperm(ROWS, device=dev)]
        for i in range(0, ROWS, B):
            idx = order[i:i + B]
            tr.step(S[idx], P[idx], Z[idx], lr=tn.LEARNING_RATE * tn.lr_lambda(epoch))
            step += 1
            if step % 2 == 0:
                want = [tn.weight_average_reference(w, p, 0.9) for w, p in zip(want, _snapshot(tr))]
    twin = {k: v.cpu() for k, v in model.state_dict().items()}
    assert list(off.keys()) == list(twin.keys()) and all(torch.equal(off[k], twin[k]) for k in twin)
    os.makedirs(path + "twin")
    torch.save(model.state_dict(), path + "twin/latest.pth")
    with open(path + "twin/latest.pth", "rb") as f:
        assert off_bytes == f.read()                     # unset: the last iterate's file
    tn.TRAIN_EMA_DECAY, tn.TRAIN_EMA_EVERY = 0.9, 2
    _, on = _loop_run(tn, kind, path)
    line = [x for x in capsys.readouterr().out.splitlines() if x.startswith("weight average:")]
    assert len(line) == 1 and "decay 0.9, every 2, 3 updates, |avg - raw| / |raw| = " in line[0]
    assert list(on.keys()) == list(off.keys())
    expected = dict(twin)
    expected.update({k: torch.from_numpy(w) for k, w in zip(keys, want)})
    for k in on:
        assert on[k].dtype == expected[k].dtype and torch.equal(on[k], expected[k]), (kind, k)
    assert any(not torch.equal(on[k], off[k]) for k in keys)
    tn.TRAIN_EMA_DECAY, tn.TRAIN_EMA_EVERY = 0.0, 1
    _, zero = _loop_run(tn, kind, path)
    assert list(zero.keys()) == list(off.keys()) and all(torch.equal(zero[k], off[k]) for k in off), kind
