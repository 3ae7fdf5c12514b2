"""The reference's residual CNN on HIP (csrc/cnn_forward.hip, aqg_cnn_*) and in the engine (evaluator='cnn', prior_mode 4): the
forward against the same module in fp64 torch and against the reference's recorded outputs, bit-identity across batches and masks,
the predict contract, priors and visit counts against oracle.mcts, whole generations, the evaluation cache, weight refreshes, host
reads, self-play, matches and evaluate_network."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _util as U   # noqa: E402
from tests.test_cnn_cpu import _golden_net, _triples   # noqa: E402
from tests.test_gnn_graph_autograd import _sync_count   # noqa: E402
from tests.test_gpu_parity import _root_children, _small_board_states   # noqa: E402

pytestmark = pytest.mark.gpu

BAR = dict(atol=1e-5, rtol=1e-4)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _make_net(F, L, N, seed):
    """A CNNNetwork with random weights and non-trivial BatchNorm statistics, gamma and beta, in eval mode on the CPU."""
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    torch.manual_seed(seed)
    net = CNNNetwork(F, L, board_size=N)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 2.0)
    return net.eval()


def _states(N, B):
    pool = U.golden("feat_9x9.npz")["states"] if N == 9 else _small_board_states(N)
    idx = np.arange(B) * max(1, pool.shape[0] // max(B, 1)) % pool.shape[0]
    return np.ascontiguousarray(pool[idx])


def _fp64(net, recs, N):
    """(policy, value, pooled) of the same module in float64 torch on the CPU."""
    import copy
    m = copy.deepcopy(net).cpu().double().eval()
    x = torch.from_numpy(m.preprocess_input(_triples(recs, N))).double()
    with torch.no_grad():
        h = torch.relu(m.conv(x))
        h = m.residual_blocks(h)
        pooled = m.global_avg_pool(h).flatten(1)
        policy, value = m._forward_stock(x)
    return policy.numpy(), value.numpy()[:, 0], pooled.numpy()


def _hip(net, dev, recs):
    with torch.no_grad():
        policy, value, pooled = net.forward_states(torch.from_numpy(recs).to(dev), want_pooled=True)
    return policy.cpu().numpy(), value.cpu().numpy()[:, 0], pooled.cpu().numpy()


def _check(got, want):
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, **BAR)


def test_forward_9x9_default_shape_vs_fp64(dev):
    net = _make_net(128, 16, 9, seed=1).to(dev)
    recs = U.golden("feat_9x9.npz")["states"]                      # 200 states
    _check(_hip(net, dev, recs), _fp64(net, recs, 9))


@pytest.mark.parametrize("N,F,L", [(3, 48, 0), (5, 48, 2), (7, 64, 3), (5, 256, 1), (9, 7, 1), (3, 200, 2)])
def test_forward_other_boards_and_shapes_vs_fp64(dev, N, F, L):
    net = _make_net(F, L, N, seed=N * 100 + F + L).to(dev)
    recs = _states(N, 150)
    _check(_hip(net, dev, recs), _fp64(net, recs, N))


@pytest.mark.parametrize("name", ["cnn_9x9.npz", "cnn_5x5.npz"])
def test_forward_reproduces_the_reference_fixture(dev, name):
    net, g, N = _golden_net(name)
    net = net.to(dev)
    policy, value, _ = _hip(net, dev, g["states"])
    np.testing.assert_allclose(policy, g["policy"], **BAR)
    np.testing.assert_allclose(value, g["value"], **BAR)
    planes = torch.from_numpy(net.preprocess_input(_triples(g["states"], N))).to(dev)
    with torch.no_grad():
        p2, v2 = net(planes)                                         # forward(x): the HIP path (GPU, eval, no autograd)
    np.testing.assert_allclose(p2.cpu().numpy(), g["policy"], **BAR)
    np.testing.assert_allclose(v2.cpu().numpy()[:, 0], g["value"], **BAR)


def test_bit_identity_batch_mask_and_planes(dev):
    from alphaquoridorgnn_amd import _lib
    N = 9
    net = _make_net(64, 2, N, seed=7).to(dev)
    recs = _states(N, 4096)
    d72 = torch.from_numpy(recs).to(dev)
    with torch.no_grad():
        big = net.forward_states(d72, want_logits=True, want_pooled=True)
        for i in (0, 1234, 4095):
            one = net.forward_states(d72[i:i + 1], want_logits=True, want_pooled=True)
            for a, b in zip(one, big):
                assert torch.equal(a[0], b[i]), i
        # forward(preprocess_input(s)) == forward_states(s), bit for bit
        planes = torch.from_numpy(net.preprocess_input(_triples(recs[:300], N))).to(dev)
        p, v = net(planes)
        assert torch.equal(p, big[0][:300]) and torch.equal(v, big[1][:300])
    # the active mask: skipped rows keep their contents, the others equal the unmasked call
    B = 300
    lib = _lib.load()
    active = torch.from_numpy((np.random.RandomState(3).rand(B) < 0.4).astype(np.uint8)).to(dev)
    active[5] = 2
    policy = torch.full((B, _A(N)), -7.0, device=dev)
    value = torch.full((B,), -7.0, device=dev)
    nws = int(lib.aqg_cnn_workspace_floats(N, 64, _A(N), B))
    ws = torch.empty((nws,), device=dev)
    d = net.cnn_net(dev)
    _lib.check(lib.aqg_cnn_forward_boards(N, _lib.ptr(d72[:B].contiguous()), 0, B, ctypes.byref(d), _lib.ptr(active), _lib.ptr(ws), nws,
                                          None, None, _lib.ptr(policy), None, _lib.ptr(value), _lib.stream_ptr(dev)), "forward")
    on = active == 1
    assert torch.equal(policy[on], big[0][:B][on]) and torch.equal(value[on], big[1][:B, 0][on])
    assert bool((policy[~on] == -7.0).all()) and bool((value[~on] == -7.0).all())


def test_engine_records_and_packed_weights_cache(dev):
    from tests.test_engine_general import _pack24
    N = 5
    net = _make_net(32, 1, N, seed=3).to(dev)
    recs = _states(N, 64)
    with torch.no_grad():
        a = net.forward_states(torch.from_numpy(recs).to(dev))
        b = net.forward_states(torch.from_numpy(_pack24(recs, N)).to(dev))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    p1 = net.packed_weights(dev)
    assert net.packed_weights(dev) is p1
    with torch.no_grad():
        net.residual_blocks[0].conv_bn1.bn.running_mean.add_(0.1)
    assert net.packed_weights(dev) is not p1


def test_predict_contract(dev):
    from alphaquoridorgnn_amd.game_logic import State
    net = _make_net(32, 2, 9, seed=5).to(dev)
    s = State()
    for a in (1, 2, 100):
        s = s.next(s.legal_actions()[a % len(s.legal_actions())])
    pol, val = net.predict(s, dev)
    assert isinstance(pol, np.ndarray) and pol.dtype == np.float32 and len(pol) == len(s.legal_actions())
    assert abs(float(pol.sum()) - 1) < 1e-5 and isinstance(val, float) and -1 <= val <= 1
    full, v = net.forward_states(torch.from_numpy(s.record()).to(dev).unsqueeze(0))
    want = full[0].cpu().numpy()[list(s.legal_actions())]
    np.testing.assert_allclose(pol, want / want.sum(), rtol=1e-6, atol=1e-7)


class _Fp64Cnn:
    """predict() (pv_network_cnn.py:117-137) of a CNNNetwork in fp64 on the CPU, over oracle.quoridor states."""

    def __init__(self, net, N):
        self.net, self.N = net, N

    def predict(self, state, device=None):
        pol, val, _ = _fp64(self.net, state.rec[None], self.N)
        legal = state.legal_actions()
        pol = pol[0][legal].astype(np.float32)
        s = pol.sum()
        return (pol / (s if s else 1)).astype(np.float32), float(np.float32(val[0]))


@pytest.mark.parametrize("N", [9, 5])
def test_engine_cnn_priors_and_visits_vs_oracle(dev, N):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from oracle import mcts as om, quoridor as oq
    net = _make_net(32, 2, N, seed=N).to(dev)
    oracle = _Fp64Cnn(net, N)
    if N == 9:
        g = U.golden("walk_9x9.npz")
        recs = np.stack([g["states"][i] for i in [0, 5, 40, 333, 1200, 2600, 5000, 9000]])
    else:
        pool = _small_board_states(N)
        recs = pool[np.linspace(0, pool.shape[0] - 1, 8).astype(int)]
    recs = recs[[not oq.State(r).is_done() for r in recs]]
    sims = 10
    eng = BatchedSelfPlay(net, num_games=recs.shape[0], sims=sims, board_size=N, evaluator="cnn", record_history=False)
    eng.search(recs)
    torch.cuda.synchronize()
    for rec, (pri, vis, act) in zip(recs, _root_children(eng)):
        st = oq.State(rec)
        legal = st.legal_actions()
        assert [int(a) for a in act] == [int(a) for a in legal]
        want, _ = oracle.predict(st)
        np.testing.assert_allclose(pri, want, atol=1e-6, rtol=1e-5)
        root = om.search(oracle, st, sims)
        assert [int(v) for v in vis] == [c.n for c in root.children]


def _rows(eng):
    return [x.cpu() for x in eng.history_tensors()]


def test_engine_cnn_play_generation_and_sets(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay, MultiSetSelfPlay
    N = 5
    net = _make_net(32, 2, N, seed=25).to(dev)
    runs = []
    for _ in range(2):
        eng = BatchedSelfPlay(net, num_games=48, sims=12, board_size=N, evaluator="cnn", seed=5)
        c = eng.play_generation()
        assert c["finished"] == 48 and c["active"] == 0
        runs.append(_rows(eng))
    s, v, z = runs[0]
    assert s.shape[0] > 0 and bool((s[:, 70] == N).all()) and set(z.tolist()) <= {-1, 0, 1}
    assert all(torch.equal(a, b) for a, b in zip(*runs))                   # deterministic
    ms = MultiSetSelfPlay(net, num_games=48, sims=12, num_sets=2, seed=5, board_size=N, evaluator="cnn")
    assert ms.play_generation()["finished"] == 48
    for k, eng_k in enumerate(ms.sets):
        alone = BatchedSelfPlay(net, num_games=eng_k.G, sims=12, board_size=N, evaluator="cnn", seed=5 * 64 + k)
        alone.play_generation()
        with torch.cuda.stream(ms.streams[k]):
            rows_k = _rows(eng_k)
        assert all(torch.equal(a, b) for a, b in zip(rows_k, _rows(alone))), k


def test_engine_cnn_eval_cache_bit_identical(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    N = 5
    net = _make_net(40, 1, N, seed=31).to(dev)
    off = BatchedSelfPlay(net, num_games=40, sims=24, board_size=N, evaluator="cnn", seed=9, eval_cache_slots=0)
    off.play_generation()
    on = BatchedSelfPlay(net, num_games=40, sims=24, board_size=N, evaluator="cnn", seed=9, eval_cache_slots=256)
    c = on.play_generation()
    assert c["cache_hits"] > 0
    assert all(torch.equal(a, b) for a, b in zip(_rows(off), _rows(on)))


def test_engine_cnn_refresh_after_in_place_update(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    N = 5
    net = _make_net(32, 2, N, seed=41).to(dev)
    recs = _states(N, 16)
    kw = dict(num_games=16, sims=24, board_size=N, evaluator="cnn", eval_cache_slots=128, record_history=False)
    eng = BatchedSelfPlay(net, **kw)
    before = eng.search(recs)[0].clone()
    state = eng.t["eval_cache_keys"].view(-1, 32)[:, 20:24].contiguous().view(torch.int32)
    assert int((state != 0).sum()) > 0
    eng.refresh_weights()                                           # nothing changed: the table stays
    state = eng.t["eval_cache_keys"].view(-1, 32)[:, 20:24].contiguous().view(torch.int32)
    assert int((state != 0).sum()) > 0
    with torch.no_grad():                                           # an optimiser step's kind of change: in place
        for p in net.parameters():
            p.mul_(1.5).add_(0.01)
    eng.refresh_weights()
    state = eng.t["eval_cache_keys"].view(-1, 32)[:, 20:24].contiguous().view(torch.int32)
    assert int((state != 0).sum()) == 0                             # the table was emptied
    got = eng.search(recs)
    want = BatchedSelfPlay(net, **kw).search(recs)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(got[0], before)


def test_engine_cnn_move_makes_no_host_read(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    net = _make_net(32, 1, 9, seed=51).to(dev)
    eng = BatchedSelfPlay(net, num_games=32, sims=8, evaluator="cnn", seed=1)
    eng.move()
    torch.cuda.synchronize()
    assert _sync_count(lambda: torch.zeros(1, device=dev).item()) == 1       # the counter sees a read
    assert _sync_count(lambda: (eng.move(), eng.move())) == 0


def test_self_play_pv_mcts_and_match(dev):
    from alphaquoridorgnn_amd import pv_mcts, self_play
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    from alphaquoridorgnn_amd.game_logic import State
    net = _make_net(16, 1, 9, seed=61).to(dev)
    sims = pv_mcts.PV_EVALUATE_COUNT
    pv_mcts.PV_EVALUATE_COUNT = 8
    try:
        np.random.seed(0)
        hist = self_play.play(net)
        assert len(hist) > 0 and all(len(h[1]) == 209 for h in hist)
        s = State()
        a = pv_mcts.pv_mcts_action(net, temperature=0)(s)
        assert a in s.legal_actions()
    finally:
        pv_mcts.PV_EVALUATE_COUNT = sims
    N = 5
    p0, p1 = _make_net(24, 1, N, seed=71).to(dev), _make_net(48, 2, N, seed=72).to(dev)
    m = BatchedMatch((p0, p1), 8, sims=8, board_size=N, evaluator="cnn", seed=3)
    pts = m.play()
    assert len(pts) == 8 and all(p in (0.0, 0.5, 1.0) for p in pts)
    assert BatchedMatch((p0, p1), 8, sims=8, board_size=N, evaluator="cnn", seed=3).play() == pts


def test_evaluate_network_on_two_cnn_files(dev, tmp_path, monkeypatch):
    from alphaquoridorgnn_amd import evaluate_network as ev, pv_mcts
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    N = 5
    if ev.BOARD_SIZE != N:
        monkeypatch.setattr(ev, "BOARD_SIZE", N)
        defaults = list(ev.BatchedMatch.__init__.__defaults__)
        defaults[1] = N                                             # (sims, board_size, ...)
        monkeypatch.setattr(ev.BatchedMatch.__init__, "__defaults__", tuple(defaults))
    path = str(tmp_path) + "/"
    torch.save(_make_net(16, 1, N, seed=81).state_dict(), path + "best.pth")
    torch.save(_make_net(24, 1, N, seed=82).state_dict(), path + "latest.pth")
    monkeypatch.setattr(ev, "PV_NETWORK_PATH", path)
    monkeypatch.setattr(ev, "EN_GAME_COUNT", 4)
    monkeypatch.setattr(pv_mcts, "PV_EVALUATE_COUNT", 6)
    promoted = ev.evaluate_network()
    assert promoted in (True, False)
    torch.save(GraphPolicyValueNetwork(6, 32, 2, _A(N)).state_dict(), path + "latest.pth")
    with pytest.raises(ValueError, match="CNN and a GNN"):
        ev.evaluate_network()
