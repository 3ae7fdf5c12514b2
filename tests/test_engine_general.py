"""The engine's any-shape evaluator (evaluator='general', prior_mode 3) and its forward aqg_gcn_forward_boards_general: bit-identity
with the width-generic primitive composition, the fp64 restatement, the active mask, priors and visit counts against oracle.mcts,
whole generations, the evaluation cache, weight updates and host reads."""
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
from tests.test_gnn_any_shape import BAR, _make_net, _params64, _ref_forward   # noqa: E402
from tests.test_gnn_graph_autograd import _sync_count   # noqa: E402
from tests.test_gpu_parity import _board_graphs, _root_children, _small_board_states   # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(6, 64, 2), (6, 65, 1), (6, 256, 4), (6, 2, 3), (6, 1024, 1)]
SID = lambda s: "x".join(map(str, s))                     # noqa: E731


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _states(N, B):
    """B board records (repeated when the pool is smaller)."""
    pool = _small_board_states(N)
    idx = np.arange(B) * max(1, pool.shape[0] // max(B, 1)) % pool.shape[0]
    return np.ascontiguousarray(pool[idx])


def _pack24(recs, N):
    """state72 records -> the engine's 24-byte records (u64 horizontal walls, u64 vertical walls, pawns | walls in hand | plies)."""
    nw = (N - 1) ** 2
    out = np.zeros((recs.shape[0], 3), np.uint64)
    for b, r in enumerate(recs):
        walls = r[4:4 + nw].astype(np.int64)
        out[b, 0] = sum(1 << i for i in range(nw) if walls[i] == 1)
        out[b, 1] = sum(1 << i for i in range(nw) if walls[i] == 2)
        plies = int(r[68]) | (int(r[69]) << 8)
        out[b, 2] = int(r[0]) | (int(r[1]) << 8) | (int(r[2]) << 16) | (int(r[3]) << 24) | (plies << 32)
    return out.view(np.uint8).reshape(-1, 24)


def _composition(net, dev, d72):
    """The primitive composition: aqg_gcn_boards_graph + the width-generic layers (what forward_states of a non-default shape
    runs) -> (policy, value, logits, value_pre, pooled)."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.pv_network_gnn import _general_forward, _param
    lib = _lib.load()
    N = net.board_size
    V, B = N * N, d72.shape[0]
    R = B * V
    x = torch.empty((R, 6), dtype=torch.float32, device=dev)
    idx = torch.empty((R * 5,), dtype=torch.int32, device=dev)
    w = torch.empty((R * 5,), dtype=torch.float32, device=dev)
    _lib.check(lib.aqg_gcn_boards_graph(N, _lib.ptr(d72), B, _lib.ptr(x), _lib.ptr(idx), _lib.ptr(w), _lib.stream_ptr(dev)),
               "aqg_gcn_boards_graph")
    csr = (torch.arange(0, 5 * R + 1, 5, dtype=torch.int32, device=dev), idx, w)
    gptr = torch.arange(0, R + 1, V, dtype=torch.int32, device=dev)
    pf = [_param(p, dev) for _, p in net._ordered_params()]
    policy, value, logits, vpre, acts = _general_forward(lib, dev, net, x, csr, gptr, B, pf)
    return policy, value, logits, vpre, acts[1]


def _fused(net, dev, states, fmt, active=None, fill=None):
    """aqg_gcn_forward_boards_general with LDS poisoned first -> (policy, value, logits, value_pre, pooled)."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, B, A, Hd = net.board_size, states.shape[0], net.policy_output_size, net.hidden_dim
    nws = int(lib.aqg_gcn_boards_general_workspace_floats(N, Hd, A, B))
    ws = torch.empty((nws,), dtype=torch.float32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    outs = [torch.full((B, A), fill if fill is not None else float("nan"), **f32), torch.full((B,), fill or 0.0, **f32),
            torch.empty((B, A), **f32), torch.empty((B,), **f32), torch.empty((B, Hd), **f32)]
    policy, value, logits, vpre, pooled = outs
    net_d = net.general_net(dev)
    _lib.poison_lds(dev)
    _lib.check(lib.aqg_gcn_forward_boards_general(N, _lib.ptr(states), fmt, B, ctypes.byref(net_d), _lib.ptr(active), _lib.ptr(ws), nws,
                                                  _lib.ptr(pooled), _lib.ptr(logits), _lib.ptr(policy), _lib.ptr(vpre), _lib.ptr(value),
                                                  _lib.stream_ptr(dev)), "aqg_gcn_forward_boards_general")
    return policy, value, logits, vpre, pooled


# ------------------------------------------------------------------ the forward
@pytest.mark.parametrize("N", [3, 5, 7, 9])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_forward_boards_general_bit_identical_to_composition(dev, shape, N):
    net = _make_net(shape, _A(N), seed=sum(shape) + N, N=N)
    recs = _states(N, 1000)
    d72 = torch.from_numpy(recs).to(dev)
    d24 = torch.from_numpy(_pack24(recs, N)).to(dev)
    with torch.no_grad():
        want = _composition(net, dev, d72)
        for B in (1, 37, 1000):
            for fmt, d in ((0, d72), (1, d24)):
                got = _fused(net, dev, d[:B].contiguous(), fmt)
                for name, g, w in zip(("policy", "value", "logits", "value_pre", "pooled"), got, want):
                    assert torch.equal(g, w[:B]), f"{SID(shape)} {N}x{N} B={B} fmt={fmt}: {name}"
        # and within the project bar of the fp64 restatement
        sub = recs[:64]
        xn, en, bn = _board_graphs(sub)
        ref = _ref_forward(_params64(net), net.num_gcn_layers, torch.from_numpy(np.asarray(xn, np.float64)), en, bn, len(sub))
        for g, r in zip(want[:4], ref[:4]):
            np.testing.assert_allclose(g[:64].cpu().numpy().reshape(r.shape), r.numpy(), **BAR)


def test_forward_boards_general_active_mask(dev):
    N = 9
    net = _make_net((6, 96, 3), _A(N), seed=11, N=N)
    recs = _states(N, 300)
    d72 = torch.from_numpy(recs).to(dev)
    active = torch.from_numpy((np.random.RandomState(3).rand(300) < 0.4).astype(np.uint8)).to(dev)
    active[5] = 2                                                   # anything but 1 is skipped
    with torch.no_grad():
        full = _fused(net, dev, d72, 0)
        got = _fused(net, dev, d72, 0, active=active, fill=-7.0)
    on = active == 1
    for g, w in zip(got, full):
        assert torch.equal(g[on], w[on])
    assert bool((got[0][~on] == -7.0).all()) and bool((got[1][~on] == -7.0).all())   # a skipped board's policy / value: untouched


# ------------------------------------------------------------------ the engine
class _Fp64Net:
    """predict() (pv_network_cnn.py:117-137) of a GraphPolicyValueNetwork of any shape, in fp64 over the oracle's board graphs."""

    def __init__(self, net):
        self.p, self.L = _params64(net), net.num_gcn_layers

    def predict(self, state, device=None):
        xn, en, bn = _board_graphs(state.rec[None])
        pol, val = _ref_forward(self.p, self.L, torch.from_numpy(np.asarray(xn, np.float64)), en, bn, 1)[:2]
        legal = state.legal_actions()
        pol = pol[0].numpy()[legal].astype(np.float32)
        s = pol.sum()
        return (pol / (s if s else 1)).astype(np.float32), float(np.float32(val[0, 0]))


@pytest.mark.parametrize("N,shape", [(9, (6, 64, 2)), (5, (6, 96, 3))])
def test_engine_general_priors_and_visits_vs_oracle(dev, N, shape):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from oracle import mcts as om, quoridor as oq
    net = _make_net(shape, _A(N), seed=N, N=N)
    oracle = _Fp64Net(net)
    if N == 9:
        g = U.golden("walk_9x9.npz")
        recs = np.stack([g["states"][i] for i in [0, 5, 40, 333, 1200, 2600, 5000, 9000]])
    else:
        pool = _small_board_states(N)
        recs = pool[np.linspace(0, pool.shape[0] - 1, 8).astype(int)]
    recs = recs[[not oq.State(r).is_done() for r in recs]]
    sims = 10
    eng = BatchedSelfPlay(net, num_games=recs.shape[0], sims=sims, board_size=N, evaluator="general", record_history=False)
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


def _check_rows(rows, N, games, sims):
    s, v, z = rows
    assert s.shape[0] > 0 and s.shape[0] == v.shape[0] == z.shape[0]
    assert bool((s[:, 70] == N).all())
    tot = v.long().sum(1)
    assert bool((tot > 0).all()) and bool((tot <= sims).all())
    assert set(z.tolist()) <= {-1, 0, 1}


@pytest.mark.parametrize("N", [5, 9])
def test_engine_general_play_generation(dev, N):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay, MultiSetSelfPlay
    net = _make_net((6, 64, 2), _A(N), seed=20 + N, N=N)
    runs = []
    for _ in range(2):
        eng = BatchedSelfPlay(net, num_games=64, sims=16, board_size=N, evaluator="general", seed=5)
        c = eng.play_generation()
        assert c["finished"] == 64 and c["active"] == 0
        runs.append(_rows(eng))
    _check_rows(runs[0], N, 64, 16)
    assert all(torch.equal(a, b) for a, b in zip(*runs))                   # deterministic
    ms = MultiSetSelfPlay(net, num_games=64, sims=16, num_sets=2, seed=5, board_size=N, evaluator="general")
    c = ms.play_generation()
    assert c["finished"] == 64
    for k, eng_k in enumerate(ms.sets):
        alone = BatchedSelfPlay(net, num_games=eng_k.G, sims=16, board_size=N, evaluator="general", seed=5 * 64 + k)
        alone.play_generation()
        with torch.cuda.stream(ms.streams[k]):
            rows_k = _rows(eng_k)
        assert all(torch.equal(a, b) for a, b in zip(rows_k, _rows(alone))), k


def test_engine_general_eval_cache_bit_identical(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    N = 5
    net = _make_net((6, 80, 2), _A(N), seed=31, N=N)
    off = BatchedSelfPlay(net, num_games=48, sims=24, board_size=N, evaluator="general", seed=9, eval_cache_slots=0)
    off.play_generation()
    on = BatchedSelfPlay(net, num_games=48, sims=24, board_size=N, evaluator="general", seed=9, eval_cache_slots=256)
    c = on.play_generation()
    assert c["cache_hits"] > 0
    assert all(torch.equal(a, b) for a, b in zip(_rows(off), _rows(on)))


def test_engine_general_refresh_after_in_place_update(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    N = 5
    net = _make_net((6, 64, 3), _A(N), seed=41, N=N)
    recs = _states(N, 16)
    kw = dict(num_games=16, sims=24, board_size=N, evaluator="general", eval_cache_slots=128, record_history=False)
    eng = BatchedSelfPlay(net, **kw)
    before = eng.search(recs)[0].clone()
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


def test_engine_general_move_makes_no_host_read(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    net = _make_net((6, 64, 2), _A(9), seed=51)
    eng = BatchedSelfPlay(net, num_games=32, sims=8, evaluator="general", seed=1)
    eng.move()
    torch.cuda.synchronize()
    assert _sync_count(lambda: torch.zeros(1, device=dev).item()) == 1       # the counter sees a read
    assert _sync_count(lambda: (eng.move(), eng.move())) == 0


def test_pv_mcts_general(dev):
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    N = 5
    net = _make_net((6, 48, 2), _A(N), seed=61, N=N)
    recs = _states(N, 6)
    pols = pv_mcts.pv_mcts_policy_batch(net, recs, 1.0, sims=12, board_size=N, evaluator="general")
    assert len(pols) == 6 and all(abs(sum(p) - 1) < 1e-9 for p in pols)
    with torch.no_grad():
        net.policy_head[2].bias.add_(torch.linspace(-2, 2, _A(N), device=dev))
    again = pv_mcts.pv_mcts_policy_batch(net, recs, 1.0, sims=12, board_size=N, evaluator="general")   # cached engine, refreshed
    fresh = BatchedSelfPlay(net, num_games=6, sims=12, board_size=N, evaluator="general", record_history=False)
    visits, _, count = fresh.search(recs)
    visits, count = visits.cpu().numpy(), count.cpu().numpy()
    for b in range(6):
        v = visits[b, :count[b]].astype(np.float64)
        np.testing.assert_allclose(again[b], v / v.sum(), rtol=0, atol=1e-12)
