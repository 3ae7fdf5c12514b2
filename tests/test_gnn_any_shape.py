"""GraphPolicyValueNetwork of any shape, GCNConv.forward and global_mean_pool on the width-generic HIP primitives
(csrc/gcn_general.hip): forward and autograd against an fp64 torch restatement, host reads, the board path, and the
reference's own layer loop against forward(x, edge_index, batch), the default 6/128/3 shape included."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_gnn_graph_autograd import (GRAD_BAR, KINK, _assert_grads_close, _drop_graphs, _gcn_adjacency, _losses,   # noqa: E402
                                           _sync_count, _targets)
from tests.test_gpu_parity import _board_graphs, _pyg_edge_case_batch, _small_board_states, _with_gcn_biases   # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(6, 64, 2), (6, 65, 1), (8, 96, 4), (6, 256, 3), (3, 32, 6), (6, 1024, 1)]
SID = lambda s: "x".join(map(str, s))                     # noqa: E731
BAR = dict(atol=1e-5, rtol=1e-4)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _make_net(shape, A, seed, N=9):
    """A network of `shape` with PyG's initialisation and non-zero GCN biases (zero biases would hide a bias slip)."""
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    torch.manual_seed(seed)
    net = GraphPolicyValueNetwork(*shape, A, board_size=N)
    with torch.no_grad():
        for l, layer in enumerate(net.gcn_layers):
            layer.bias.copy_(torch.linspace(-0.3, 0.5, layer.out_channels) * (1 + 0.5 * l))
    return net.to("cuda").eval()


def _params64(net):
    return {k: v.detach().double().cpu() for k, v in net.state_dict().items()}


def _ref_forward(p, L, x, edge_index, batch, G):
    """fp64 restatement of the reference's forward (pv_network_gnn.py:53-64) at any shape.  Returns (policy, value [G,1], logits,
    value_pre, per-graph kink margin)."""
    n = x.shape[0]
    A = _gcn_adjacency(edge_index, n)
    bt = torch.from_numpy(np.asarray(batch, np.int64))
    h, margin = x, np.full(G, np.inf)
    for l in range(L):
        pre = torch.sparse.mm(A, h @ p[f"gcn_layers.{l}.lin.weight"].T) + p[f"gcn_layers.{l}.bias"]
        a = pre.detach().abs().numpy()
        if n:
            np.minimum.at(margin, np.asarray(batch, np.int64), np.where(a == 0.0, np.inf, a).min(1))
        h = torch.relu(pre)
    cnt = torch.zeros(G, dtype=torch.float64).index_add_(0, bt, torch.ones(n, dtype=torch.float64))
    pooled = torch.zeros((G, h.shape[1]), dtype=torch.float64).index_add_(0, bt, h) / cnt.clamp(min=1.0)[:, None]
    pre_p = pooled @ p["policy_head.0.weight"].T + p["policy_head.0.bias"]
    pre_v = pooled @ p["value_head.0.weight"].T + p["value_head.0.bias"]
    for pre in (pre_p, pre_v):
        a = pre.detach().abs().numpy()
        margin = np.minimum(margin, np.where(a == 0.0, np.inf, a).min(1))
    logits = torch.relu(pre_p) @ p["policy_head.2.weight"].T + p["policy_head.2.bias"]
    vpre = torch.relu(pre_v) @ p["value_head.2.weight"].T + p["value_head.2.bias"]
    return torch.softmax(logits, 1), torch.tanh(vpre), logits, vpre[:, 0], margin


def _to_dev(dev, xn, en, bn):
    return torch.from_numpy(np.asarray(xn)).float().to(dev), torch.from_numpy(en).to(dev), torch.from_numpy(bn).to(dev)


def _edge_cases(F_, seed=0):
    """The PyG edge-case batch with random features of width F_."""
    xn, en, bn, G = _pyg_edge_case_batch(seed)
    return np.random.RandomState(seed + 11).randn(xn.shape[0], F_), en, bn, G


def _check_forward(net, dev, xn, en, bn, G, what):
    from alphaquoridorgnn_amd import _lib
    p = _params64(net)
    with torch.no_grad():
        ref = _ref_forward(p, net.num_gcn_layers, torch.from_numpy(np.asarray(xn, np.float64)), en, bn, G)
    _lib.poison_lds(dev)
    policy, value = net(*_to_dev(dev, xn, en, bn))
    assert policy.shape == (G, net.policy_output_size) and value.shape == (G, 1)
    for got, want, name in ((policy, ref[0], "policy"), (value, ref[1], "value"), (net.last_logits, ref[2], "logits"),
                            (net.last_value_pre, ref[3], "value_pre")):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), err_msg=f"{what}: {name}", **BAR)


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("A", [1, 37, 300])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_any_shape_forward_vs_fp64(dev, shape, A):
    net = _make_net(shape, A, seed=sum(shape) + A)
    xn, en, bn, G = _edge_cases(shape[0])
    _check_forward(net, dev, xn, en, bn, G, "edge cases")
    if shape[0] == 6:
        recs = _small_board_states(9)[::97][:48]
        xn, en, bn = _board_graphs(recs)
        _check_forward(net, dev, xn, en, bn, len(recs), "board graphs")


def test_any_shape_forward_1024_board_graphs(dev):
    net = _make_net((6, 256, 3), 209, seed=5)
    recs = _small_board_states(9)[::13][:1024]
    assert recs.shape[0] == 1024
    xn, en, bn = _board_graphs(recs)
    _check_forward(net, dev, xn, en, bn, 1024, "1,024 board graphs")


# ------------------------------------------------------------------ 2. GCNConv.forward and global_mean_pool alone
def _ref_conv(layer, xn, en):
    A = _gcn_adjacency(en, xn.shape[0])
    W, b = layer.lin.weight.detach().double().cpu(), layer.bias.detach().double().cpu()
    return (torch.sparse.mm(A, torch.from_numpy(np.asarray(xn, np.float64)) @ W.T) + b).numpy()


def test_gcnconv_forward_vs_fp64(dev):
    from alphaquoridorgnn_amd.pv_network_gnn import GCNConv
    xn6, en, bn, G = _pyg_edge_case_batch()                   # repeated self loops, duplicate edges, a 2,100-in-edge hub
    n = xn6.shape[0]
    layers = list(_make_net((8, 96, 4), 37, 1).gcn_layers[:2]) + list(_make_net((6, 128, 3), 209, 2).gcn_layers)
    torch.manual_seed(3)
    layers.append(GCNConv(5, 33).to(dev))
    for layer in layers:
        xn = np.random.RandomState(layer.in_channels).randn(n, layer.in_channels)
        x = torch.from_numpy(xn).float().to(dev)
        want = _ref_conv(layer, xn, en)
        with torch.no_grad():
            out = layer(x, torch.from_numpy(en).to(dev))
            out32 = layer(x, torch.from_numpy(en).int().to(dev))
        assert out.shape == (n, layer.out_channels) and torch.equal(out, out32)
        np.testing.assert_allclose(out.cpu().numpy(), want, **BAR)
        # no edges: every node its own self loop
        with torch.no_grad():
            out = layer(x[:5], torch.zeros((2, 0), dtype=torch.int64, device=dev))
        np.testing.assert_allclose(out.cpu().numpy(), _ref_conv(layer, xn[:5], np.zeros((2, 0), np.int64)), **BAR)
        # n = 0
        out = layer(x[:0], torch.zeros((2, 0), dtype=torch.int64, device=dev))
        assert out.shape == (0, layer.out_channels)
    layer = layers[0]
    x = torch.randn(4, layer.in_channels, device=dev)
    for bad_x, bad_e in ((torch.randn(4, layer.in_channels + 1, device=dev), [[0], [1]]), (x, [[0], [4]]), (x, [[-1], [0]]),
                         (x, [[0.0], [1.0]])):
        with pytest.raises(ValueError):
            layer(bad_x, torch.tensor(bad_e, device=dev))


def test_global_mean_pool_vs_fp64(dev):
    from alphaquoridorgnn_amd.pv_network_gnn import global_mean_pool
    rng = np.random.RandomState(4)
    bn = np.repeat([0, 0, 2, 3, 3, 3, 6], [1, 2, 5, 1, 7, 9, 40])     # ids 1, 4, 5 have no nodes
    for width in (1, 7, 130):
        xn = rng.randn(bn.shape[0], width)
        x, bt = torch.from_numpy(xn).float().to(dev), torch.from_numpy(bn).to(dev)
        want = np.zeros((7, width))
        for g in range(7):
            if (bn == g).any():
                want[g] = xn[bn == g].mean(0)
        out = global_mean_pool(x, bt)
        assert out.shape == (7, width)
        np.testing.assert_allclose(out.cpu().numpy(), want, **BAR)
        assert torch.equal(global_mean_pool(x, bt.int()), out)
        out9 = global_mean_pool(x, bt, size=9)
        assert out9.shape == (9, width) and torch.equal(out9[:7], out) and not out9[7:].any()
        np.testing.assert_allclose(global_mean_pool(x, None).cpu().numpy(), xn.mean(0, keepdims=True), **BAR)
    assert global_mean_pool(torch.zeros((0, 3), device=dev), torch.zeros(0, dtype=torch.int64, device=dev)).shape == (0, 3)
    with pytest.raises(ValueError):
        global_mean_pool(x, bt.flip(0))
    with pytest.raises(ValueError):
        global_mean_pool(x, bt, size=3)


# ------------------------------------------------------------------ 3. the reference's own loop
@pytest.mark.parametrize("shape", [(8, 96, 4), (6, 128, 3)], ids=SID)
def test_reference_layer_loop_reproduces_forward(dev, shape):
    """pv_network_gnn.py:53-64 written out by the caller: relu(layer(x, ei)) over gcn_layers, global_mean_pool, the heads as
    torch modules, against net.forward at a non-default shape and at the default 6/128/3 (the same primitives, composed by the
    caller layer by layer)."""
    from alphaquoridorgnn_amd.pv_network_gnn import global_mean_pool
    net = _make_net(shape, 209, 7)
    assert net.fused == (shape == (6, 128, 3))
    xn, en, bn, G = _edge_cases(shape[0], 1)
    x, ei, bt = _to_dev(dev, xn, en, bn)
    with torch.no_grad():
        policy, value = net(x, ei, bt)
        h = x
        for layer in net.gcn_layers:
            h = F.relu(layer(h, ei))
        g = global_mean_pool(h, bt)
        p2, v2 = net.policy_head(g), net.value_head(g)
    np.testing.assert_allclose(p2.cpu().numpy(), policy.cpu().numpy(), **BAR)
    np.testing.assert_allclose(v2.cpu().numpy(), value.cpu().numpy(), **BAR)


# ------------------------------------------------------------------ 4. autograd
def _ref_grads(net, xn, en, bn, G, loss_fn):
    p = {k: v.clone().requires_grad_(True) for k, v in _params64(net).items()}
    x = torch.tensor(np.asarray(xn, np.float64), requires_grad=True)
    policy, value = _ref_forward(p, net.num_gcn_layers, x, en, bn, G)[:2]
    loss_fn(policy, value).backward()
    g = {k: v.grad.numpy() for k, v in p.items()}
    g["x"] = x.grad.numpy()
    return g


def _hip_grads(net, dev, xn, en, bn, loss_fn):
    net.train()
    net.zero_grad(set_to_none=True)
    x, ei, bt = _to_dev(dev, xn, en, bn)
    x.requires_grad_(True)
    policy, value = net(x, ei, bt)
    assert policy.grad_fn is not None
    loss_fn(policy, value).backward()
    g = {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in net.named_parameters()}
    g["x"] = x.grad.detach().cpu().numpy().astype(np.float64)
    return g


def _kink_filtered(net, xn, en, bn, G):
    with torch.no_grad():
        margin = _ref_forward(_params64(net), net.num_gcn_layers, torch.from_numpy(np.asarray(xn, np.float64)), en, bn, G)[4]
    drop = np.nonzero(margin < KINK)[0]
    assert drop.size < G - 2, drop
    return _drop_graphs(xn, en, bn, drop)


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_any_shape_autograd_vs_fp64(dev, shape):
    net = _make_net(shape, 37, seed=3 * sum(shape))
    xn, en, bn, G = _edge_cases(shape[0], 2)
    xn, en, bn = _kink_filtered(net, xn, en, bn, G)
    pi, z, wp, wv = _targets(G, 37, 5)
    losses = _losses(pi, z, wp, wv)
    for name in ("reference", "weighted"):
        got = _hip_grads(net, dev, xn, en, bn, losses[name])
        _assert_grads_close(got, _ref_grads(net, xn, en, bn, G, losses[name]), GRAD_BAR, f"{SID(shape)} / {name}")
        again = _hip_grads(net, dev, xn, en, bn, losses[name])
        assert all(np.array_equal(got[k], again[k]) for k in got), "two backward passes differ"
    # train-mode forward == eval forward, bit for bit; then an Adam step and a second forward
    x, ei, bt = _to_dev(dev, xn, en, bn)
    net.eval()
    pe, ve = net(x, ei, bt)
    le, vpe = net.last_logits, net.last_value_pre
    net.train()
    pt, vt = net(x, ei, bt)
    assert pt.grad_fn is not None
    for a, b in ((pt, pe), (vt, ve), (net.last_logits, le), (net.last_value_pre, vpe)):
        assert torch.equal(a.detach(), b)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt.zero_grad()
    losses["reference"](pt, vt).backward()
    opt.step()
    net.eval()
    p2, _ = net(x, ei, bt)
    assert torch.isfinite(p2).all() and not torch.equal(p2, pe)
    _check_forward(net, dev, xn, en, bn, G, "after an Adam step")


def test_gcnconv_and_pool_autograd_vs_fp64(dev):
    from alphaquoridorgnn_amd.pv_network_gnn import GCNConv, global_mean_pool
    xn6, en, bn, G = _pyg_edge_case_batch(3)
    n = xn6.shape[0]
    torch.manual_seed(9)
    for cin, cout in ((7, 45), (6, 128), (128, 128)):
        layer = GCNConv(cin, cout).to(dev)
        with torch.no_grad():
            layer.bias.copy_(torch.linspace(-0.2, 0.4, cout))
        xn = np.random.RandomState(cin).randn(n, cin)
        wout = np.random.RandomState(cout).randn(n, cout)
        wpool = np.random.RandomState(1).randn(G, cout)
        # fp64
        W = layer.lin.weight.detach().double().cpu().requires_grad_(True)
        b = layer.bias.detach().double().cpu().requires_grad_(True)
        x64 = torch.tensor(xn, requires_grad=True)
        out = torch.sparse.mm(_gcn_adjacency(en, n), x64 @ W.T) + b
        bt64 = torch.from_numpy(bn)
        cnt = torch.zeros(G, dtype=torch.float64).index_add_(0, bt64, torch.ones(n, dtype=torch.float64)).clamp(min=1)
        pooled = torch.zeros((G, cout), dtype=torch.float64).index_add_(0, bt64, torch.relu(out)) / cnt[:, None]
        ((out * torch.from_numpy(wout)).sum() + (pooled * torch.from_numpy(wpool)).sum()).backward()
        ref = {"w": W.grad.numpy(), "b": b.grad.numpy(), "x": x64.grad.numpy()}
        # HIP
        results = []
        for _ in range(2):
            layer.zero_grad(set_to_none=True)
            x = torch.from_numpy(xn).float().to(dev).requires_grad_(True)
            o = layer(x, torch.from_numpy(en).to(dev))
            pl = global_mean_pool(F.relu(o), torch.from_numpy(bn).to(dev))
            assert o.grad_fn is not None and pl.grad_fn is not None
            ((o * torch.from_numpy(wout).float().to(dev)).sum() + (pl * torch.from_numpy(wpool).float().to(dev)).sum()).backward()
            results.append({"w": layer.lin.weight.grad.cpu().numpy().astype(np.float64),
                            "b": layer.bias.grad.cpu().numpy().astype(np.float64), "x": x.grad.cpu().numpy().astype(np.float64)})
        _assert_grads_close(results[0], ref, GRAD_BAR, f"GCNConv({cin}, {cout})")
        assert all(np.array_equal(results[0][k], results[1][k]) for k in ref)
        opt = torch.optim.Adam(layer.parameters(), lr=1e-3)
        opt.step()
        with torch.no_grad():
            assert torch.isfinite(layer(x, torch.from_numpy(en).to(dev))).all()


# ------------------------------------------------------------------ 5. host reads
def test_any_shape_host_reads(dev):
    net = _make_net((8, 96, 4), 37, 1)
    xn, en, bn, G = _edge_cases(8)
    x, ei, bt = _to_dev(dev, xn, en, bn)
    layer = net.gcn_layers[1]
    h = torch.randn(x.shape[0], 96, device=dev)
    torch.cuda.synchronize()
    assert _sync_count(lambda: torch.zeros(1, device=dev).item()) == 1
    assert _sync_count(lambda: net(x, ei, bt)) == 1
    net.train()
    xg = x.clone().requires_grad_(True)
    out = {}
    assert _sync_count(lambda: out.setdefault("pv", net(xg, ei, bt))) == 1
    assert _sync_count(lambda: out["pv"][0].sum().backward()) == 0
    with torch.no_grad():
        assert _sync_count(lambda: layer(h, ei)) == 1
    assert _sync_count(lambda: layer(h.requires_grad_(True), ei)) == 1


# ------------------------------------------------------------------ 6. boards
@pytest.mark.parametrize("N", [3, 5, 7, 9])
def test_any_shape_forward_states_vs_fp64(dev, N):
    from alphaquoridorgnn_amd import _lib
    A = N * N + 2 * (N - 1) ** 2
    net = _make_net((6, 64, 2), A, seed=N, N=N)
    recs = _small_board_states(N)[::23][:64]
    _lib.poison_lds(dev)
    policy, value, logits, vpre = net.forward_states(torch.from_numpy(recs).to(dev), want_logits=True)
    xn, en, bn = _board_graphs(recs)
    with torch.no_grad():
        ref = _ref_forward(_params64(net), 2, torch.from_numpy(np.asarray(xn, np.float64)), en, bn, len(recs))
    for got, want in ((policy, ref[0]), (value, ref[1]), (logits, ref[2]), (vpre, ref[3])):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), **BAR)
    p2, v2 = net.predict_batch(torch.from_numpy(recs).to(dev))
    assert torch.equal(p2, policy) and torch.equal(v2, value[:, 0])


def test_any_shape_predict_and_self_play(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.game_logic import State
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    net = _make_net((6, 65, 1), 209, seed=2)
    s = State().next(67).next(81 + 20)
    pol, val = net.predict(s, "cuda")
    la = s.legal_actions()
    assert isinstance(pol, np.ndarray) and pol.dtype == np.float32 and pol.shape == (len(la),)
    assert abs(float(pol.sum()) - 1) < 1e-5 and (pol >= 0).all() and isinstance(val, float) and -1 <= val <= 1
    policy, _ = net.forward_states(torch.from_numpy(s.record()).unsqueeze(0).to(dev))
    want = policy[0].cpu().numpy()[la]
    np.testing.assert_allclose(pol, want / want.sum(), atol=1e-6, rtol=1e-5)
    small = _make_net((6, 64, 2), 17, seed=4, N=3)
    eng = BatchedSelfPlay(small, num_games=2, sims=8, board_size=3, evaluator="external", seed=1)
    cnts = eng.play_generation()
    assert cnts["finished"] == 2
    with pytest.raises(ValueError, match="evaluator='external'"):
        BatchedSelfPlay(small, num_games=2, sims=8, board_size=3, evaluator="gnn")
    with pytest.raises(ValueError, match="6 feature planes"):
        GraphPolicyValueNetwork(8, 64, 2, 17, board_size=3).to(dev).forward_states(torch.from_numpy(s.record()).unsqueeze(0).to(dev))
