"""The residual CNN's training step on HIP (csrc/cnn_train.hip, aqg_cnn_train_*, train_network.CNNTrainer): one step against the
same module in fp64 torch in train mode, against the reference's recorded step, Adam against torch.optim.Adam, the epoch call and
determinism, trained weights reaching the engine, and the whole learning loop on the CNN."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _util as U   # noqa: E402
from tests.test_cnn import BAR, _make_net, _states   # noqa: E402
from tests.test_cnn_cpu import _triples   # noqa: E402
from tests.test_gnn_graph_autograd import _sync_count   # noqa: E402
from tests.test_gpu_parity import _root_children   # noqa: E402

pytestmark = pytest.mark.gpu

# ||g - g64|| / ||g64|| per tensor, against the same bar for stock fp32: a tensor passes at max(GRAD_REL, 4 x the largest error of the
# stock fp32 CPU step of the same module on the same batch).  The stock step itself is not that accurate on a deep network: at 128
# filters x 16 blocks on 9x9 it is off by ~2e-3 at the stem (the BatchNorm backward's cancellations, compounded over 33 layers), and
# so is this step (~1.6e-3); at 16 x 2 both are below 1e-6.  Largest error seen on an MI355X: see the test output ("worst").
GRAD_REL = 1e-4


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _targets(B, A, seed):
    rng = np.random.RandomState(seed)
    pi = rng.rand(B, A) * (rng.rand(B, A) < 0.2)
    pi[:, 0] += 1e-3
    pi = pi / pi.sum(1, keepdims=True)
    z = rng.choice([-1.0, 0.0, 1.0], B)
    return pi.astype(np.float32), z.astype(np.float32)


def _ref_step(net, recs, pi, z, N, dtype=torch.float64):
    """train_network.py:84-91 on a copy of the module in `dtype`, train mode, on the CPU: (outputs, losses, grads in parameter
    order, the module after its forward -- running statistics updated)."""
    m = copy.deepcopy(net).cpu().to(dtype).train()
    x = torch.from_numpy(m.preprocess_input(_triples(recs, N))).to(dtype)
    policy, value = m._forward_stock(x)
    pl = torch.nn.CrossEntropyLoss()(policy, torch.from_numpy(pi).to(dtype))
    vl = torch.nn.MSELoss()(value.view(-1), torch.from_numpy(z).to(dtype))
    (pl + vl).backward()
    grads = [p.grad.double().numpy() for p in m.parameters()]
    return (policy.detach().double().numpy(), value.detach().double().numpy()[:, 0]), (pl.item(), vl.item()), grads, m


def _rel(g, r):
    g = g.astype(np.float64)
    n = np.linalg.norm(r)
    return np.linalg.norm(g - r) / n if n > 0 else np.linalg.norm(g)


def _check_step(net, tr, recs, dev, what, seed=0):
    """One mode-0 step of `tr` on `recs` against _ref_step in fp64 (outputs, losses, gradients, running statistics)."""
    N, B = net.board_size, recs.shape[0]
    pi, z = _targets(B, _A(N), seed)
    outs, losses, g_ref, m64 = _ref_step(net, recs, pi, z, N)
    stock = max(_rel(g, r) for g, r in zip(_ref_step(net, recs, pi, z, N, torch.float32)[2], g_ref))
    nbt = [int(bn.num_batches_tracked) for bn in tr.bns]
    pl, vl = tr.step(torch.from_numpy(recs).to(dev), torch.from_numpy(pi), torch.from_numpy(z), update=False)
    assert abs(float(pl) - losses[0]) <= 1e-5 * abs(losses[0]), what
    assert abs(float(vl) - losses[1]) <= 1e-5 * abs(losses[1]) + 1e-7, what
    pol, val = tr.outputs(B)
    np.testing.assert_allclose(pol.cpu().numpy(), outs[0], **BAR, err_msg=what)
    np.testing.assert_allclose(val.cpu().numpy(), outs[1], **BAR, err_msg=what)
    bar = max(GRAD_REL, 4 * stock)
    worst = 0.0
    for (k, _), g, r in zip(net.named_parameters(), tr.grads, g_ref):
        e = _rel(g.cpu().numpy(), r)
        worst = max(worst, e)
        assert e <= bar, (what, k, e, stock)
    print(f"{what}: worst {worst:.3g} (stock fp32 {stock:.3g})")
    for bn, bn64, n0 in zip(tr.bns, [cb.bn for cb in m64._convs()], nbt):
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), bn64.running_mean.numpy(), **BAR, err_msg=what)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), bn64.running_var.numpy(), **BAR, err_msg=what)
        assert int(bn.num_batches_tracked) == n0 + 1 == int(bn64.num_batches_tracked), what


def test_step_default_shape_9x9_batch_128_and_a_short_batch(dev):
    """128 filters x 16 blocks on 9x9: a step of the reference's batch (128) and then a short last batch (37) on the same trainer."""
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    net = _make_net(128, 16, 9, seed=3).to(dev)
    tr = CNNTrainer(net, max_batch=128)
    recs = _states(9, 128)
    _check_step(net, tr, recs, dev, "128x16 B128", seed=1)
    _check_step(net, tr, recs[::3][:37].copy(), dev, "128x16 B37", seed=2)
    assert not net.training                        # the mode is left as it was


def test_step_batch_of_one(dev):
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    net = _make_net(16, 2, 5, seed=5).to(dev).train()
    tr = CNNTrainer(net, max_batch=4)
    _check_step(net, tr, _states(5, 8)[3:4].copy(), dev, "B1", seed=3)
    assert net.training


SHAPES = [(F, L) for F in (1, 7, 64, 65, 130) for L in (0, 1, 3)]


@pytest.mark.parametrize("F,L", SHAPES, ids=[f"{F}x{L}" for F, L in SHAPES])
def test_step_other_shapes_and_boards(dev, F, L):
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    N = (3, 5, 7)[(F + L) % 3]
    net = _make_net(F, L, N, seed=F * 10 + L).to(dev)
    tr = CNNTrainer(net, max_batch=24)
    _check_step(net, tr, _states(N, 24), dev, f"{F}x{L} {N}x{N}", seed=F + L)


@pytest.mark.parametrize("F,L,N", [(512, 1, 3), (16, 40, 5)], ids=["512-filters", "40-blocks"])
def test_step_at_the_shape_limits(dev, F, L, N):
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    net = _make_net(F, L, N, seed=F + L).to(dev)
    tr = CNNTrainer(net, max_batch=8)
    _check_step(net, tr, _states(N, 8), dev, f"{F}x{L}", seed=7)


def test_step_reproduces_the_reference_fixture(dev):
    """cnn_train_5x5.npz (tools/gen_golden_cnn_train.py): the reference module's own fp32 step -- losses, every .grad, the running
    statistics after the forward and the parameters after torch.optim.Adam."""
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    g = U.golden("cnn_train_5x5.npz")
    F, L, N = (int(v) for v in g["shape"])
    net = CNNNetwork(F, L, board_size=N)
    net.load_state_dict({k[len("param."):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("param.")})
    net = net.to(dev)
    tr = CNNTrainer(net, max_batch=64)
    pl, vl = tr.step(torch.from_numpy(g["states"]).to(dev), torch.from_numpy(g["pi"]), torch.from_numpy(g["z"]), lr=1e-3)
    np.testing.assert_allclose([float(pl), float(vl)], g["losses"], rtol=1e-5, atol=1e-6)
    B = g["states"].shape[0]
    pol, val = tr.outputs(B)
    np.testing.assert_allclose(pol.cpu().numpy(), g["policy"], **BAR)
    np.testing.assert_allclose(val.cpu().numpy(), g["value"], **BAR)
    for (k, _), gr in zip(net.named_parameters(), tr.grads):
        assert _rel(gr.cpu().numpy(), g["grad." + k].astype(np.float64)) <= GRAD_REL, k
    sd = net.state_dict()
    for k in g.files:
        if k.startswith("stats."):
            key = k[len("stats."):]
            if key.endswith("num_batches_tracked"):
                assert int(sd[key]) == int(g[k]), key
            else:
                np.testing.assert_allclose(sd[key].cpu().numpy(), g[k], **BAR, err_msg=key)
    for k, p in net.named_parameters():
        d = np.abs(p.detach().cpu().numpy() - g["after." + k])
        assert d.max() <= 0.25 * 1e-3, k                         # Adam moves each element by at most ~lr
        gr = np.abs(g["grad." + k])
        well = gr >= 1e-3 * gr.max()
        if well.any():
            assert d[well].max() <= 1e-5, (k, d[well].max())


def test_adam_steps_vs_torch(dev):
    """Three steps with the LambdaLR factors 1.0 / 0.5 / 0.25 against torch.optim.Adam fed the same gradients, at the bar of
    test_train_general.test_adam_steps_vs_torch."""
    from alphaquoridorgnn_amd.train_network import CNNTrainer, LEARNING_RATE, lr_lambda
    N = 7
    net = _make_net(32, 2, N, seed=21).to(dev)
    shadow = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    opt = torch.optim.Adam(shadow, lr=LEARNING_RATE)
    tr = CNNTrainer(net, max_batch=32)
    recs = _states(N, 96)
    for i, epoch in enumerate((0, 50, 80)):
        pi, z = _targets(32, _A(N), 40 + i)
        lr = LEARNING_RATE * lr_lambda(epoch)
        tr.step(torch.from_numpy(recs[32 * i:32 * (i + 1)].copy()).to(dev), torch.from_numpy(pi), torch.from_numpy(z), lr=lr)
        for gp in opt.param_groups:
            gp["lr"] = lr
        for s, gr in zip(shadow, tr.grads):
            s.grad = gr.detach().clone()
        opt.step()
        for (k, p), s, gr in zip(net.named_parameters(), shadow, tr.grads):
            d = (p.detach() - s.detach()).abs()
            assert float(d.max()) <= 0.25 * LEARNING_RATE, (i, k)
            well = gr.abs() >= 1e-3 * gr.abs().max()
            if bool(well.any()):
                assert float(d[well].max()) <= 1e-5, (i, k, float(d[well].max()))


def _snapshot(net):
    return [t.detach().clone() for t in net.state_dict().values()]


def test_run_epoch_equals_single_steps_and_is_deterministic(dev):
    """run_epoch (one library call, both order forms) takes bit-identically the steps step() takes on the same batches (the short
    last batch included); two runs give bit-identical parameters and running statistics; a step makes no host read."""
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    N, n, batch = 5, 75, 32
    recs = _states(N, n)
    pi, z = _targets(n, _A(N), 9)
    S, P, Z = torch.from_numpy(recs).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev)
    order = torch.from_numpy(np.random.RandomState(3).permutation(n))
    finals = []
    for pre_shuffle in (True, False, True):
        ma, mb = _make_net(24, 2, N, seed=2).to(dev), _make_net(24, 2, N, seed=2).to(dev)
        ta, tb = CNNTrainer(ma, max_batch=batch), CNNTrainer(mb, max_batch=batch)
        sums = ta.run_epoch(S, P, Z, order, lr=7e-4, pre_shuffle=pre_shuffle)
        ref = torch.zeros(2, device=dev)
        od = order.to(dev)
        for i in range(0, n, batch):
            idx = od[i:i + batch]
            pl, vl = tb.step(S[idx], P[idx], Z[idx], lr=7e-4)
            ref += torch.stack([pl, vl])
        for x, y in zip(_snapshot(ma), _snapshot(mb)):
            assert torch.equal(x, y), pre_shuffle
        np.testing.assert_allclose(sums.cpu().numpy(), ref.cpu().numpy(), rtol=1e-6)
        assert int(ma.conv.bn.num_batches_tracked) == 3 and ta.step_count == tb.step_count == 3
        finals.append(_snapshot(ma))
    for x, y in zip(finals[0], finals[2]):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    s, p, zz = S[:batch], P[:batch], Z[:batch]
    tb.step(s, p, zz)
    torch.cuda.synchronize()
    assert _sync_count(lambda: torch.zeros(1, device=dev).item()) == 1       # the counter sees a read
    assert _sync_count(lambda: tb.step(s, p, zz)) == 0


def test_empty_batch_rule_of_each_workspace_trainer(dev):
    """What a mode-1 step does with batch == 0 (include/aqgnn.h; the one trait in which the two kinds of csrc/train_driver.hpp differ),
    bit for bit on 3x3 boards.  The any-shape GNN (6, 8, 1): it applies Adam from whatever grads holds, as mode 2 does.  The CNN
    (2 filters, no block): it is a no-op -- parameters, moments and running statistics stay as they were."""
    from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer
    from tests.test_gnn_any_shape import _make_net as _make_gnn
    N, B = 3, 2
    pi, z = _targets(B, _A(N), 4)
    S, P, Z = torch.from_numpy(_states(N, B)).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev)

    def general(second_mode, second_batch):
        net = _make_gnn((6, 8, 1), _A(N), seed=17, N=N)
        tr = GeneralTrainer(net, max_batch=B)
        before = [p.detach().clone() for p in tr.params]
        tr.t.batch, tr.t.step, tr.t.lr = B, 1, 1e-3
        tr._call(S, P, Z, 0)
        tr.t.batch = second_batch
        tr._call(S, P, Z, second_mode)
        return tr, before

    a, before = general(2, B)
    b, _ = general(1, 0)
    assert any(not torch.equal(x, y) for x, y in zip(a.params, before))           # the update happened
    for x, y in zip(a.params + a.adam_m + a.adam_v, b.params + b.adam_m + b.adam_v):
        assert torch.equal(x, y)

    net = _make_net(2, 0, N, seed=6).to(dev)
    tr = CNNTrainer(net, max_batch=B)
    tr.t.batch, tr.t.step, tr.t.lr = B, 1, 1e-3
    tr._call(S, P, Z, 0)
    kept = tr.params + tr.adam_m + tr.adam_v + tr.buffers
    was = [x.detach().clone() for x in kept]
    tr.t.batch = 0
    tr._call(S, P, Z, 1)
    torch.cuda.synchronize()
    for x, y in zip(kept, was):
        assert torch.equal(x, y)
    assert float(tr.flat_grads.abs().max()) > 0                                    # there were gradients to apply


@pytest.mark.parametrize("cache", [0, 64])
def test_trained_weights_reach_the_engine(dev, cache):
    """After a step (and after an epoch call) and refresh_weights(), a 'cnn' engine's root priors are those of the eval-mode forward
    of the updated module -- with the evaluation cache off, and on."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    from oracle import quoridor as oq
    N = 5
    net = _make_net(32, 2, N, seed=61).to(dev)
    recs = _states(N, 32)
    pi, z = _targets(32, _A(N), 62)
    roots = recs[[not oq.State(r).is_done() for r in recs]][:8]
    eng = BatchedSelfPlay(net, num_games=roots.shape[0], sims=4, board_size=N, evaluator="cnn", record_history=False,
                          eval_cache_slots=cache)
    S, P, Z = torch.from_numpy(recs).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev)
    tr = CNNTrainer(net, max_batch=32)
    for update in ("step", "epoch"):
        eng.search(roots)
        eng.search(roots)
        before = [c[0].copy() for c in _root_children(eng)]
        key = net.weights_key()
        if update == "step":
            tr.step(S, P, Z, lr=1e-2)
        else:
            tr.run_epoch(S, P, Z, torch.arange(32), lr=1e-2, batch=16)
        assert net.weights_key() != key, update
        eng.refresh_weights()
        eng.search(roots)
        with torch.no_grad():
            pol = net.eval().forward_states(torch.from_numpy(roots).to(dev))[0].cpu().numpy()
        changed = False
        for gi, (pri, _, act) in enumerate(_root_children(eng)):
            want = pol[gi][act.astype(np.int64)]
            want = want / want.sum()
            np.testing.assert_allclose(pri, want, rtol=2e-6, atol=1e-9, err_msg=update)
            changed |= not np.array_equal(pri, before[gi])
        assert changed, update


_LOOP = r'''
import os, shutil, sys
sys.path.insert(0, os.environ["AQG_REPO"])
from alphaquoridorgnn_amd import constants, train_cycle as tc


def keep_best_then_update():            # the evaluation may promote latest.pth over best.pth: keep the one training started from
    shutil.copy(constants.PV_NETWORK_PATH + "best.pth", "start.pth")
    return tc.parameter_update()


tc._STAGES = tuple((t, keep_best_then_update if s is tc.train_network else s) for t, s in tc._STAGES)
tc.main(["--network", "cnn", "--num-filters", "16", "--num-residual-blocks", "2", "--cycles", "1", "--games", "4", "--sims", "8",
         "--epochs", "2", "--eval-games", "2"])
'''

_CHECK = r'''
import os, sys, pickle
sys.path.insert(0, os.environ["AQG_REPO"])
from pathlib import Path
import torch
from alphaquoridorgnn_amd import constants
from alphaquoridorgnn_amd.pv_network_cnn import load_network, CNNNetwork
m = load_network(constants.PV_NETWORK_PATH + "latest.pth", "cpu")
print("LATEST", type(m).__name__, m.num_filters, m.num_residual_blocks, m.board_size)
best = torch.load("start.pth", map_location="cpu", weights_only=True)
latest = torch.load(constants.PV_NETWORK_PATH + "latest.pth", map_location="cpu", weights_only=True)
print("DIFFERS", sorted(best) == sorted(latest) and all(not torch.equal(best[k], latest[k]) for k in latest if k.endswith("conv.weight")))
with sorted(Path("data").glob("*.history"))[-1].open("rb") as f:
    n = len(pickle.load(f))
steps = 2 * ((n + 127) // 128)
print("TRACKED", all(int(v) == steps for k, v in latest.items() if k.endswith("num_batches_tracked")), steps)
'''


def test_learning_loop_on_the_cnn(dev, tmp_path):
    """train_cycle --network cnn --num-filters 16 --num-residual-blocks 2 on 5x5 in a scratch directory: latest.pth is a trained
    16 x 2 CNNNetwork, every conv weight differs from the best.pth training started from, and num_batches_tracked is the number
    of steps taken."""
    (tmp_path / "loop.py").write_text(_LOOP)
    (tmp_path / "check.py").write_text(_CHECK)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Epoch 2/2" in r.stdout, r.stdout[-2000:]
    r = subprocess.run([sys.executable, str(tmp_path / "check.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "LATEST CNNNetwork 16 2 5" in r.stdout, r.stdout
    assert "DIFFERS True" in r.stdout, r.stdout
    assert "TRACKED True" in r.stdout, r.stdout
