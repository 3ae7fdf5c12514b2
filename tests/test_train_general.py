"""The training step of GraphPolicyValueNetwork at any shape (aqg_gcn_train_step_general, train_network.GeneralTrainer) against
an fp64 autograd statement of the L-layer network and the reference's losses, against the autograd route through
forward(x, edge_index, batch), and against torch.optim.Adam; the epoch call, determinism and host reads; trained weights in the
engine; evaluation matches between networks of different shapes; and the whole learning loop at a non-default shape."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_gnn_any_shape import _make_net                        # noqa: E402
from tests.test_gnn_graph_autograd import _sync_count                  # noqa: E402
from tests.test_gpu_parity import _board_graphs, _root_children, _walk_states   # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(6, 64, 2), (6, 65, 1), (6, 65, 2), (6, 256, 3), (6, 96, 4), (6, 1024, 1)]
SID = lambda s: "x".join(map(str, s))                     # noqa: E731
KINK_MARGIN = 5e-7          # as test_gpu_parity._train_batch: nearer than this to a ReLU kink the branch is decided by rounding
KINK_DROP_BOUND = 0.35


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _net(shape, A, seed, N=9):
    """test_gnn_any_shape's network with its GCN biases moved off the grid through zero (linspace(-0.3, 0.5, 65) holds a bias of
    ~1e-9: every empty tile of a board would then sit at a ReLU kink, and the kink filter would discard most positions)."""
    net = _make_net(shape, A, seed, N)
    with torch.no_grad():
        for layer in net.gcn_layers:
            layer.bias.add_(0.00317)
    return net


def _params64(net):
    return {k: v.detach().double().cpu() for k, v in net.state_dict().items()}


def _dense(recs):
    """node features [B, V, 6] and D^-1/2 (A + I) D^-1/2 [B, V, V] of the board graphs, fp64 (oracle/gnn.py, oracle/train.py)."""
    from oracle import gnn as og, train as ot
    x = torch.tensor(np.stack([og.node_features(r) for r in recs]), dtype=torch.float64)
    adj = torch.tensor(np.stack([ot.dense_adjacency(r) for r in recs]), dtype=torch.float64)
    return x, adj


def _ref_forward(p, L, recs):
    """fp64 statement of the reference's forward (pv_network_gnn.py:53-64) at L layers on board records.  Returns
    (policy, value [B,1], per-position ReLU kink margin)."""
    x, adj = _dense(recs)
    B = x.shape[0]
    h, margin = x, np.full(B, np.inf)

    def note(pre, axes):
        a = pre.detach().abs().numpy()
        np.minimum(margin, np.where(a == 0.0, np.inf, a).min(axis=axes), out=margin)

    for l in range(L):
        pre = adj @ (h @ p[f"gcn_layers.{l}.lin.weight"].T) + p[f"gcn_layers.{l}.bias"]
        note(pre, (1, 2))
        h = torch.relu(pre)
    g = h.mean(dim=1)
    pre_p = g @ p["policy_head.0.weight"].T + p["policy_head.0.bias"]
    pre_v = g @ p["value_head.0.weight"].T + p["value_head.0.bias"]
    note(pre_p, 1)
    note(pre_v, 1)
    policy = torch.softmax(torch.relu(pre_p) @ p["policy_head.2.weight"].T + p["policy_head.2.bias"], dim=1)
    value = torch.tanh(torch.relu(pre_v) @ p["value_head.2.weight"].T + p["value_head.2.bias"])
    return policy, value, margin


def _ref_step(net, recs, pi, z):
    """One step of train_network.py:84-91 in fp64: CrossEntropyLoss on the softmaxed policy + MSELoss on the tanh value, autograd.
    Returns (grads in state_dict order, policy_loss, value_loss)."""
    p = {k: v.clone().requires_grad_(True) for k, v in _params64(net).items()}
    policy, value, _ = _ref_forward(p, net.num_gcn_layers, recs)
    pl = torch.nn.CrossEntropyLoss()(policy, torch.tensor(np.asarray(pi), dtype=torch.float64))
    vl = torch.nn.MSELoss()(value.view(-1), torch.tensor(np.asarray(z), dtype=torch.float64))
    (pl + vl).backward()
    keys = [k for k, _ in net._ordered_params()]
    return [p[k].grad.numpy() for k in keys], float(pl.detach()), float(vl.detach())


def _batch(net, N, B, seed):
    """B positions away from the ReLU kinks of `net` (see KINK_MARGIN) with random probability and value targets."""
    rng = np.random.RandomState(seed)
    pool = _walk_states(N, 4 * B, seed + 100)
    cand = pool[rng.choice(pool.shape[0], min(3 * B, pool.shape[0]), replace=False)]
    with torch.no_grad():
        margin = _ref_forward(_params64(net), net.num_gcn_layers, cand)[2]
    keep = cand[margin >= KINK_MARGIN]
    assert cand.shape[0] - keep.shape[0] <= KINK_DROP_BOUND * cand.shape[0], (cand.shape[0], keep.shape[0])
    recs = keep[rng.choice(keep.shape[0], B, replace=keep.shape[0] < B)]
    A = _A(N)
    pi = rng.rand(B, A) * (rng.rand(B, A) < 0.2)
    pi[:, 0] += 1e-3
    pi = pi / pi.sum(1, keepdims=True)
    z = rng.choice([-1.0, 0.0, 1.0], B)
    return np.ascontiguousarray(recs), pi.astype(np.float32), z.astype(np.float32)


def _check_step(net, tr, recs, pi, z, dev, what):
    from alphaquoridorgnn_amd import _lib
    B = recs.shape[0]
    S = torch.from_numpy(recs).to(dev)
    _lib.poison_lds(dev)
    pl, vl = tr.step(S, torch.from_numpy(pi), torch.from_numpy(z), update=False)
    g_ref, pl_ref, vl_ref = _ref_step(net, recs, pi.astype(np.float64), z.astype(np.float64))
    assert abs(float(pl) - pl_ref) <= 1e-5 * abs(pl_ref), what
    assert abs(float(vl) - vl_ref) <= 1e-5 * abs(vl_ref) + 1e-7, what
    for (k, _), gt, r in zip(net._ordered_params(), tr.grads, g_ref):
        tol = 2e-5 * np.abs(r).max() + 1e-7
        assert np.abs(gt.cpu().numpy().astype(np.float64) - r).max() <= tol, (what, k)
    pol, val = tr.outputs(B)
    fpol, fval = net.forward_states(S)
    assert torch.equal(pol, fpol) and torch.equal(val, fval[:, 0]), what          # bit-identical to the network's own forward


CASES = [(s, 9) for s in SHAPES] + [(s, 5) for s in SHAPES] + [((6, 64, 2), 3), ((6, 64, 2), 7)]


@pytest.mark.parametrize("shape,N", CASES, ids=[f"{SID(s)}-{n}x{n}" for s, n in CASES])
def test_step_vs_fp64_autograd(dev, shape, N):
    """Losses, all 2 L + 8 gradients, policy and value of one step (batch 48, LDS poisoned) against fp64 autograd: the bars of
    test_train_step_gradients_vs_autograd; policy and value bit-identical to forward_states."""
    from alphaquoridorgnn_amd.train_network import GeneralTrainer
    net = _net(shape, _A(N), seed=7 * sum(shape) + N, N=N)
    tr = GeneralTrainer(net, max_batch=64)
    recs, pi, z = _batch(net, N, 48, seed=N + shape[1])
    _check_step(net, tr, recs, pi, z, dev, f"{SID(shape)} {N}x{N}")


def test_default_shape_step_vs_fp64_and_fused_trainer(dev):
    """GeneralTrainer at the default 6/128/3 shape: against fp64 autograd at the usual bars, against GNNTrainer's gradients (the
    fused step, fp16-split products on 9x9: both within 2e-5 max|g| of fp64, so within 4e-5 of each other), and its policy / value
    bit-identical to the any-shape forward (forward_states of this shape takes the fused kernels: compared at a tolerance)."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_network import GeneralTrainer, GNNTrainer
    N = 9
    net = _net((6, 128, 3), _A(N), seed=131)
    assert net.fused
    recs, pi, z = _batch(net, N, 48, seed=132)
    S = torch.from_numpy(recs).to(dev)
    tr, tf = GeneralTrainer(net, max_batch=48), GNNTrainer(net, max_batch=48)
    _lib.poison_lds(dev)
    pl, vl = tr.step(S, torch.from_numpy(pi), torch.from_numpy(z), update=False)
    tf.step(S, torch.from_numpy(pi), torch.from_numpy(z), update=False)
    g_ref, pl_ref, vl_ref = _ref_step(net, recs, pi.astype(np.float64), z.astype(np.float64))
    assert abs(float(pl) - pl_ref) <= 1e-5 * abs(pl_ref)
    assert abs(float(vl) - vl_ref) <= 1e-5 * abs(vl_ref) + 1e-7
    for (k, _), g, gf, r in zip(net._ordered_params(), tr.grads, tf.grads, g_ref):
        g, gf = g.double().cpu().numpy(), gf.double().cpu().numpy()
        assert np.abs(g - r).max() <= 2e-5 * np.abs(r).max() + 1e-7, k
        assert np.abs(g - gf).max() <= 4e-5 * np.abs(gf).max() + 2e-7, k
    pol, val = tr.outputs(48)
    gpol, gval = net._forward_states_general(S, False, 0)
    assert torch.equal(pol, gpol) and torch.equal(val, gval[:, 0])
    fpol, fval = net.forward_states(S)
    np.testing.assert_allclose(pol.cpu().numpy(), fpol.cpu().numpy(), atol=1e-6, rtol=1e-4)
    np.testing.assert_allclose(val.cpu().numpy(), fval[:, 0].cpu().numpy(), atol=1e-5, rtol=1e-4)


def test_step_at_reference_batch_size(dev):
    """train_network.py:15 BATCH_SIZE = 128 and the short last batch DataLoader keeps (37), same bars."""
    from alphaquoridorgnn_amd.train_network import GeneralTrainer, BATCH_SIZE
    net = _net((6, 64, 2), _A(9), seed=11)
    tr = GeneralTrainer(net, max_batch=BATCH_SIZE)
    for B, seed in ((128, 30), (37, 31)):
        recs, pi, z = _batch(net, 9, B, seed)
        _check_step(net, tr, recs, pi, z, dev, f"batch {B}")


@pytest.mark.parametrize("shape", [(6, 64, 2), (6, 96, 4)], ids=SID)
def test_step_matches_autograd_route(dev, shape):
    """The gradients equal autograd through forward(x, edge_index, batch) on the same board graphs (the route GeneralTrainer
    replaces) within a tight f32 bar."""
    from alphaquoridorgnn_amd.train_network import GeneralTrainer
    N = 9
    net = _net(shape, _A(N), seed=5 + shape[2])
    recs, pi, z = _batch(net, N, 40, seed=3)
    tr = GeneralTrainer(net, max_batch=40)
    tr.step(torch.from_numpy(recs).to(dev), torch.from_numpy(pi), torch.from_numpy(z), update=False)
    xn, en, bn = _board_graphs(recs)
    net.train().zero_grad()                       # train mode: forward(x, edge_index, batch) records for autograd
    policy, value = net(torch.from_numpy(xn).float().to(dev), torch.from_numpy(en).to(dev), torch.from_numpy(bn).to(dev))
    loss = (torch.nn.CrossEntropyLoss()(policy, torch.from_numpy(pi).to(dev))
            + torch.nn.MSELoss()(value.squeeze(), torch.from_numpy(z).to(dev)))
    loss.backward()
    for (k, p), g in zip(net._ordered_params(), tr.grads):
        r = p.grad.double().cpu().numpy()
        assert np.abs(g.double().cpu().numpy() - r).max() <= 5e-6 * np.abs(r).max() + 1e-8, k
    net.eval().zero_grad()


def test_adam_steps_vs_torch(dev):
    """Three steps with the LambdaLR factors 1.0 / 0.5 / 0.25: the parameters after each step against torch.optim.Adam fed the
    same gradients, at the bar of test_train_adam_steps_vs_torch."""
    from alphaquoridorgnn_amd.train_network import GeneralTrainer, LEARNING_RATE, lr_lambda
    net = _net((6, 96, 3), _A(9), seed=21)
    shadow = [p.detach().clone() for _, p in net._ordered_params()]
    shadow = [torch.nn.Parameter(p) for p in shadow]
    opt = torch.optim.Adam(shadow, lr=LEARNING_RATE)
    tr = GeneralTrainer(net, max_batch=32)
    for i, epoch in enumerate((0, 50, 80)):
        recs, pi, z = _batch(net, 9, 32, seed=40 + i)
        lr = LEARNING_RATE * lr_lambda(epoch)
        tr.step(torch.from_numpy(recs).to(dev), torch.from_numpy(pi), torch.from_numpy(z), lr=lr)
        for g in opt.param_groups:
            g["lr"] = lr
        for s, gr in zip(shadow, tr.grads):
            s.grad = gr.detach().clone()
        opt.step()
        for (k, p), s, gr in zip(net._ordered_params(), shadow, tr.grads):
            d = (p.detach() - s.detach()).abs()
            assert float(d.max()) <= 0.25 * LEARNING_RATE, (i, k)
            well = gr.abs() >= 1e-3 * gr.abs().max()
            if bool(well.any()):
                assert float(d[well].max()) <= 1e-5, (i, k, float(d[well].max()))


def test_run_epoch_equals_single_steps_and_is_deterministic(dev):
    """run_epoch (one library call, both order forms) takes bit-identically the steps step() takes on the same batches; two runs
    give bit-identical parameters; a step makes no host read."""
    from alphaquoridorgnn_amd.train_network import GeneralTrainer
    N, n, batch = 9, 150, 64
    recs, pi, z = _batch(_net((6, 64, 2), _A(N), seed=1), N, n, seed=9)
    S, P, Z = torch.from_numpy(recs).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev)
    order = torch.from_numpy(np.random.RandomState(3).permutation(n))
    finals = []
    for pre_shuffle in (True, False, True):
        ma, mb = _net((6, 64, 2), _A(N), seed=2), _net((6, 64, 2), _A(N), seed=2)
        ta, tb = GeneralTrainer(ma, max_batch=batch), GeneralTrainer(mb, max_batch=batch)
        sums = ta.run_epoch(S, P, Z, order, lr=7e-4, pre_shuffle=pre_shuffle)
        ref = torch.zeros(2, device=dev)
        for i in range(0, n, batch):
            idx = order[i:i + batch].to(dev)
            pl, vl = tb.step(S[idx], P[idx], Z[idx], lr=7e-4)
            ref += torch.stack([pl, vl])
        assert ta.step_count == tb.step_count == (n + batch - 1) // batch
        for (k, a), (_, b) in zip(ma._ordered_params(), mb._ordered_params()):
            assert torch.equal(a, b), (pre_shuffle, k)
        np.testing.assert_allclose(sums.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5)
        finals.append([p.detach().clone() for _, p in ma._ordered_params()])
    assert all(torch.equal(a, b) for a, b in zip(finals[0], finals[2]))      # two runs: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(finals[0], finals[1]))
    torch.cuda.synchronize()
    idx = order[:batch].to(dev)
    s, p, zz = S[idx].contiguous(), P[idx].contiguous(), Z[idx].contiguous()
    tb.step(s, p, zz)
    torch.cuda.synchronize()
    assert _sync_count(lambda: torch.zeros(1, device=dev).item()) == 1       # the counter sees a read
    assert _sync_count(lambda: tb.step(s, p, zz)) == 0


@pytest.mark.parametrize("cache", [0, 64])
def test_trained_weights_reach_the_engine(dev, cache):
    """After a step (and after an epoch call) and refresh_weights(), a 'general' engine's root priors are forward_states of the
    updated network -- with the evaluation cache off, and on (the trainer's in-place update must change general_weights_key, or
    the refreshed engine keeps serving the cached outputs of the old weights)."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.train_network import GeneralTrainer
    from oracle import quoridor as oq
    N = 9
    net = _net((6, 64, 2), _A(N), seed=61)
    recs, pi, z = _batch(net, N, 32, seed=62)
    roots = recs[[not oq.State(r).is_done() for r in recs]][:8]
    eng = BatchedSelfPlay(net, num_games=roots.shape[0], sims=4, board_size=N, evaluator="general", record_history=False,
                          eval_cache_slots=cache)
    S, P, Z = torch.from_numpy(recs).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev)
    tr = GeneralTrainer(net, max_batch=32)
    for update in ("step", "epoch"):
        eng.search(roots)
        eng.search(roots)                          # with the cache on, the second search is served from the table
        before = [c[0].copy() for c in _root_children(eng)]
        key = net.general_weights_key()
        if update == "step":
            tr.step(S, P, Z, lr=1e-2)
        else:
            tr.run_epoch(S, P, Z, torch.arange(32), lr=1e-2, batch=16)
        assert net.general_weights_key() != key, update
        eng.refresh_weights()
        eng.search(roots)
        pol = net.forward_states(torch.from_numpy(roots).to(dev))[0].cpu().numpy()
        changed = False
        for g, (pri, _, act) in enumerate(_root_children(eng)):
            want = pol[g][act.astype(np.int64)]
            want = want / want.sum()
            np.testing.assert_allclose(pri, want, rtol=2e-6, atol=1e-9, err_msg=update)
            changed |= not np.array_equal(pri, before[g])
        assert changed, update


def _sample(visits, u):
    """The engine's move rule at temperature 1 (csrc/mcts_move.hip engine_finish_move_kernel: np.random.choice over n / sum n)."""
    x = visits.astype(np.float64)
    tot = x.sum()
    last = 0.0
    for v in x:
        last += v / tot
    acc, idx = 0.0, 0
    for i, v in enumerate(x):
        acc += v / tot
        if acc / last <= u:
            idx = i + 1
    return min(idx, len(x) - 1)


def test_match_between_shapes_equals_host_replay(dev):
    """BatchedMatch(evaluator='general') of a 6/64/2 against a 6/128/4 network: every game equals a host replay that searches each
    ply with the mover's network (a stand-alone 'general' engine's search()) and samples with the engine's rule on the same
    uniform."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    from oracle import quoridor as oq
    N, G, sims = 5, 4, 6
    nets = (_net((6, 64, 2), _A(N), seed=71, N=N), _net((6, 128, 4), _A(N), seed=72, N=N))
    m = BatchedMatch(nets, G, sims=sims, board_size=N, evaluator="general")
    rng = np.random.RandomState(5)
    uni = [rng.random_sample(size=(e.max_plies, e.G)) for e in m.engines]
    points = m.play(uniforms=[torch.from_numpy(u) for u in uni])
    solo = [BatchedSelfPlay(n, num_games=1, sims=sims, board_size=N, evaluator="general", record_history=False, eval_cache_slots=0)
            for n in nets]
    for i in range(G):
        first, col = i % 2, i // 2
        eng = m.engines[first]
        st = oq.State(N=N)
        actions = []
        while not st.is_done() and len(actions) < eng.max_plies:
            mover = first if len(actions) % 2 == 0 else 1 - first
            visits, acts, cnt = solo[mover].search(st.rec[None].copy())
            c = int(cnt[0])
            a = int(acts[0, :c][_sample(visits[0, :c].cpu().numpy(), uni[first][len(actions), col])])
            actions.append(a)
            st = st.next(a)
        plies = int(eng.t["game_plies"][col])
        assert plies == len(actions), i
        assert eng.t["hist_action"][col, :plies].cpu().numpy().astype(np.int64).tolist() == actions, i
        fp = 0.5 if not st.is_lose() else (0.0 if st.is_first_player() else 1.0)
        assert points[i] == (fp if first == 0 else 1.0 - fp), i


def test_match_against_itself_equals_self_play(dev):
    """A network against itself in a 'general' match plays the games 'general' self-play plays under the same uniforms."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    N, G, sims = 5, 6, 8
    net = _net((6, 80, 3), _A(N), seed=81, N=N)
    m = BatchedMatch((net, net), G, sims=sims, board_size=N, evaluator="general")
    rng = np.random.RandomState(6)
    uni = [torch.from_numpy(rng.random_sample(size=(e.max_plies, e.G))) for e in m.engines]
    m.play(uniforms=uni)
    for first, eng in enumerate(m.engines):
        sp = BatchedSelfPlay(net, num_games=eng.G, sims=sims, board_size=N, evaluator="general", temperature=1.0, eval_cache_slots=0)
        ply = 0
        while sp.counters()["active"] and ply < sp.max_plies:
            sp.move(uni[first][ply])
            ply += 1
        assert torch.equal(sp.t["game_plies"], eng.t["game_plies"]), first
        assert torch.equal(sp.t["hist_action"], eng.t["hist_action"]), first


_LOOP = r'''
import os, sys, shutil
sys.path.insert(0, os.environ["AQG_REPO"])
import torch
from alphaquoridorgnn_amd import train_cycle as tc, constants
from alphaquoridorgnn_amd.pv_network_gnn import load_network
from alphaquoridorgnn_amd.train_network import train_network


def update_stage():                 # keep the network the update starts from: evaluation may copy latest.pth over best.pth
    shutil.copy(constants.PV_NETWORK_PATH + "best.pth", "start.pth")
    return train_network()


tc._STAGES = tuple((title, update_stage if f is train_network else f) for title, f in tc._STAGES)
tc.main(["--cycles", "1", "--games", "6", "--sims", "6", "--epochs", "2", "--eval-games", "4", "--hidden-dim", "64",
         "--num-gcn-layers", "2"])
start = torch.load("start.pth", map_location="cpu", weights_only=True)
latest = torch.load(constants.PV_NETWORK_PATH + "latest.pth", map_location="cpu", weights_only=True)
m = load_network(constants.PV_NETWORK_PATH + "latest.pth")
print("LATEST", m.hidden_dim, m.num_gcn_layers, type(m).__name__)
print("DIFFERS", sorted(start) == sorted(latest) and all(not torch.equal(start[k], latest[k]) for k in latest if k.endswith("weight")))
'''


def test_learning_loop_at_another_shape(dev, tmp_path):
    """train_cycle --hidden-dim 64 --num-gcn-layers 2 on 5x5 in a scratch directory: self-play, training and evaluation all run a
    6/64/2 network, and latest.pth is a trained 6/64/2 network (every weight differs from the best.pth it was trained from)."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "LATEST 64 2 GraphPolicyValueNetwork" in r.stdout, r.stdout[-2000:]
    assert "DIFFERS True" in r.stdout, r.stdout[-2000:]
    assert len(list((tmp_path / "data").glob("*.history"))) == 1


def test_self_play_writes_history_for_another_shape(dev, tmp_path, monkeypatch):
    """self_play(model) with a 6/64/2 network plays on the engine's 'general' evaluator and writes a .history."""
    from alphaquoridorgnn_amd import pv_mcts, self_play as sp
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pv_mcts, "PV_EVALUATE_COUNT", 6)
    net = _net((6, 64, 2), sp.POLICY_OUTPUT_SIZE, seed=91, N=sp.BOARD_SIZE)
    path = sp.self_play(net, games=4, seed=3)
    assert path is not None and os.path.exists(path) and path.endswith(".history")
