"""Autograd through GraphPolicyValueNetwork.forward(x, edge_index, batch): train-mode forwards record a graph and backward()
runs the HIP backward composed from the width-generic primitives (csrc/gcn_general.hip).  Checked against a torch-autograd fp64 restatement of the network on
(x, edge_index, batch) (below; its forward is pinned to oracle.gnn.forward_graph first) and against GNNTrainer's fused
gradients."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _util as U                                                            # noqa: E402
from tests.test_gpu_parity import _board_graphs, _net, _pyg_edge_case_batch, _train_batch, _with_gcn_biases   # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ["gcn_layers.0.lin.weight", "gcn_layers.0.bias", "gcn_layers.1.lin.weight", "gcn_layers.1.bias",
        "gcn_layers.2.lin.weight", "gcn_layers.2.bias", "policy_head.0.weight", "policy_head.0.bias",
        "policy_head.2.weight", "policy_head.2.bias", "value_head.0.weight", "value_head.0.bias",
        "value_head.2.weight", "value_head.2.bias"]
POLICY_KEYS = [k for k in KEYS if k.startswith("policy_head")]
GRAD_BAR = 2e-5            # the suite's training bar: |g - g_ref| <= GRAD_BAR * max|g_ref| + 1e-7 per tensor
KINK = 1e-6                # graphs with a non-zero fp64 pre-activation nearer to 0 than this are dropped (ReLU branch = rounding)
EDGE_CASE_SEED = 0         # _pyg_edge_case_batch seed: every graph, the 2,100-in-edge hub too, clears the kink filter (margin 2.1e-6)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


# ------------------------------------------------------------------ fp64 reference (torch autograd, sparse gcn_norm on the CPU)
def _gcn_adjacency(edge_index, n):
    """PyG gcn_norm (add_remaining_self_loops, in-degree, symmetric weights) as a sparse [n, n] fp64 matrix A[dst, src]."""
    src, dst = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    keep = src != dst
    src = np.concatenate([src[keep], np.arange(n)])
    dst = np.concatenate([dst[keep], np.arange(n)])
    deg = np.bincount(dst, minlength=n).astype(np.float64)
    dis = deg ** -0.5
    w = dis[src] * dis[dst]
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([dst, src])), torch.from_numpy(w), (n, n)).coalesce()


def _ref_forward(params, x, edge_index, batch, G):
    """fp64 forward on (x, edge_index, batch) as torch ops.  params: dict of fp64 leaf tensors; x: fp64 tensor.
    Returns (policy, value [G,1], logits, vpre, per-graph kink margin)."""
    n = x.shape[0]
    A = _gcn_adjacency(edge_index, n)
    batch_t = torch.from_numpy(np.asarray(batch, np.int64))
    h, margin = x, np.full(G, np.inf)
    for l in range(3):
        pre = torch.sparse.mm(A, h @ params[f"gcn_layers.{l}.lin.weight"].T) + params[f"gcn_layers.{l}.bias"]
        a = pre.detach().abs().numpy()
        a = np.where(a == 0.0, np.inf, a).min(1)
        np.minimum.at(margin, np.asarray(batch, np.int64), a)
        h = torch.relu(pre)
    cnt = torch.zeros(G, dtype=torch.float64).index_add_(0, batch_t, torch.ones(n, dtype=torch.float64))
    pooled = torch.zeros((G, h.shape[1]), dtype=torch.float64).index_add_(0, batch_t, h) / cnt.clamp(min=1.0)[:, None]
    pre_p = pooled @ params["policy_head.0.weight"].T + params["policy_head.0.bias"]
    pre_v = pooled @ params["value_head.0.weight"].T + params["value_head.0.bias"]
    for pre in (pre_p, pre_v):
        a = pre.detach().abs().numpy()
        margin = np.minimum(margin, np.where(a == 0.0, np.inf, a).min(1))
    logits = torch.relu(pre_p) @ params["policy_head.2.weight"].T + params["policy_head.2.bias"]
    vpre = torch.relu(pre_v) @ params["value_head.2.weight"].T + params["value_head.2.bias"]
    return torch.softmax(logits, 1), torch.tanh(vpre), logits, vpre[:, 0], margin


def _ref_grads(params, xn, en, bn, G, loss_fn):
    """fp64 gradients of loss_fn(policy, value) w.r.t. the 14 parameters and x."""
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in params.items()}
    x = torch.tensor(np.asarray(xn, np.float64), requires_grad=True)
    policy, value, _, _, _ = _ref_forward(p, x, en, bn, G)
    loss_fn(policy, value).backward()
    g = {k: (p[k].grad.numpy() if p[k].grad is not None else np.zeros(p[k].shape)) for k in KEYS}
    g["x"] = x.grad.numpy()
    return g


def _kink_margins(params, xn, en, bn, G):
    p = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    with torch.no_grad():
        return _ref_forward(p, torch.tensor(np.asarray(xn, np.float64)), en, bn, G)[4]


def _drop_graphs(xn, en, bn, drop):
    """The batch without the nodes (and edges) of the graph ids in `drop`; ids stay as they are (a dropped id pools to 0)."""
    keep_node = ~np.isin(bn, drop)
    new_id = np.cumsum(keep_node) - 1
    keep_edge = keep_node[en[0]] & keep_node[en[1]]
    return xn[keep_node], new_id[en[:, keep_edge]], bn[keep_node]


def _kink_filtered_edge_cases(params):
    xn, en, bn, G = _pyg_edge_case_batch(EDGE_CASE_SEED)
    margin = _kink_margins(params, xn, en, bn, G)
    drop = np.nonzero(margin < KINK)[0]
    print(f"edge-case batch: kink filter dropped graphs {drop.tolist()} of {G}")
    assert drop.size <= 2
    # what the batch is for must survive: duplicate edges and a triple self loop (0), edgeless (1), single node (2),
    # single node with two self loops (3), the empty id (4), the 2,100-in-edge hub (5)
    assert not set(drop.tolist()) & {0, 1, 2, 3, 4, 5}, drop
    xn, en, bn = _drop_graphs(xn, en, bn, drop)
    return xn, en, bn, G


def _targets(G, A, seed):
    rng = np.random.RandomState(seed)
    pi = rng.rand(G, A) * (rng.rand(G, A) < 0.3)
    pi[:, 0] += 1e-3
    pi = pi / pi.sum(1, keepdims=True)
    z = rng.choice([-1.0, 0.0, 1.0], G)
    wp, wv = rng.randn(G, A), rng.randn(G, 1)
    return pi, z, wp, wv


def _losses(pi, z, wp, wv):
    """name -> loss(policy, value) for any dtype / device: the reference's loss, a random-weighted sum, value only."""
    def t(a, like):
        return torch.as_tensor(a, dtype=like.dtype, device=like.device)
    return {
        "reference": lambda p, v: F.cross_entropy(p, t(pi, p)) + F.mse_loss(v.squeeze(), t(z, v)),
        "weighted": lambda p, v: (p * t(wp, p)).sum() + (v * t(wv, v)).sum(),
        "value only": lambda p, v: F.mse_loss(v.squeeze(), t(z, v)),
    }


def _hip_grads(model, dev, xn, en, bn, loss_fn):
    from alphaquoridorgnn_amd import _lib
    model.train()
    model.zero_grad(set_to_none=True)
    x = torch.from_numpy(np.asarray(xn)).float().to(dev).requires_grad_(True)
    _lib.poison_lds(dev)
    policy, value = model(x, torch.from_numpy(en).to(dev), torch.from_numpy(bn).to(dev))
    assert policy.grad_fn is not None and value.grad_fn is not None
    loss_fn(policy, value).backward()
    sd = dict(model.named_parameters())
    g = {k: (sd[k].grad.detach().cpu().numpy().astype(np.float64) if sd[k].grad is not None else None) for k in KEYS}
    g["x"] = x.grad.detach().cpu().numpy().astype(np.float64)
    return g


def _assert_grads_close(got, ref, bar, what):
    for k, r in ref.items():
        gk = got[k]
        assert gk is not None, f"{what}: {k} has no gradient"
        tol = bar * np.abs(r).max() + 1e-7
        err = np.abs(gk - r).max()
        assert err <= tol, f"{what}: {k} off by {err:.3g} (tolerance {tol:.3g})"


def _check_batch_against_fp64(model, params, dev, xn, en, bn, G, seed, what):
    from oracle import gnn as og
    # the restatement is pinned to the oracle's forward before its gradients are trusted
    p = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    with torch.no_grad():
        _, _, logits, vpre, _ = _ref_forward(p, torch.tensor(np.asarray(xn, np.float64)), en, bn, G)
    want = og.forward_graph(params, xn, en, bn, G)
    np.testing.assert_allclose(logits.numpy(), want["logits"], atol=1e-12, rtol=1e-10)
    np.testing.assert_allclose(vpre.numpy(), want["value_pre"], atol=1e-12, rtol=1e-10)
    pi, z, wp, wv = _targets(G, model.policy_output_size, seed)
    for name, loss in _losses(pi, z, wp, wv).items():
        got = _hip_grads(model, dev, xn, en, bn, loss)
        ref = _ref_grads(params, xn, en, bn, G, loss)
        if name == "value only":
            for k in POLICY_KEYS:
                assert got[k] is not None and not np.any(got[k]), f"{what}: {k} must be exactly 0 for a value-only loss"
                ref.pop(k)
        _assert_grads_close(got, ref, GRAD_BAR, f"{what} / {name} loss")


# ------------------------------------------------------------------ 1. gradients against fp64 autograd
def test_graph_autograd_gradients_vs_fp64(dev):
    """All 14 parameter gradients and x.grad against the fp64 restatement: the PyG edge-case batch (non-zero GCN biases,
    randn features, an empty graph id, a 2,100-in-edge hub) and 160 kink-filtered board graphs; the reference's loss, a
    random-weighted sum of both outputs, and a value-only loss (policy-head gradients exactly 0)."""
    from oracle import gnn as og
    params = _with_gcn_biases(og.init_params(1))
    model = _net(params)
    xn, en, bn, G = _kink_filtered_edge_cases(params)
    _check_batch_against_fp64(model, params, dev, xn, en, bn, G, 0, "edge cases")
    params2 = _with_gcn_biases(og.init_params(2))
    recs, _, _ = _train_batch(160, 3, params=params2)
    xn, en, bn = _board_graphs(recs)
    _check_batch_against_fp64(_net(params2), params2, dev, xn, en, bn, len(recs), 1, "board graphs")


# ------------------------------------------------------------------ 2. cross-check with the fused trainer
def test_graph_autograd_matches_fused_trainer(dev):
    """Board positions through forward(x, edge_index, batch) in train mode with the reference's loss against
    GNNTrainer.step(update=False): two independent fp32 implementations of one gradient."""
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    from alphaquoridorgnn_amd.train_network import GNNTrainer
    from oracle import gnn as og
    params = og.init_params(5)
    recs, pi, z = _train_batch(64, 7, params=params)
    m = GNNNetwork()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m = m.to(dev).eval()
    tr = GNNTrainer(m, max_batch=64)
    tr.step(torch.from_numpy(recs).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev), update=False)
    fused = {k: g.detach().cpu().numpy().astype(np.float64) for k, g in zip(KEYS, tr.grads)}
    xn, en, bn = _board_graphs(recs)
    loss = _losses(pi, z, None, None)["reference"]
    got = _hip_grads(_net(params), dev, xn, en, bn, loss)
    got.pop("x")
    _assert_grads_close(got, fused, 4e-5, "generic autograd vs GNNTrainer")


# ------------------------------------------------------------------ 3. recording does not change the forward
def test_graph_autograd_forward_bit_identical(dev):
    from oracle import gnn as og
    params = _with_gcn_biases(og.init_params(1))
    model = _net(params)
    xn, en, bn, G = _pyg_edge_case_batch()
    x, ei, bt = torch.from_numpy(xn).float().to(dev), torch.from_numpy(en).to(dev), torch.from_numpy(bn).to(dev)
    model.eval()
    pe, ve = model(x, ei, bt)
    le, vpe = model.last_logits, model.last_value_pre
    assert not pe.requires_grad and not ve.requires_grad
    model.train()
    with torch.no_grad():
        pn, vn = model(x, ei, bt)
    assert not pn.requires_grad and not vn.requires_grad and pn.grad_fn is None
    with torch.inference_mode():
        pi_, vi_ = model(x, ei, bt)
    assert pi_.grad_fn is None
    pt, vt = model(x, ei, bt)
    assert pt.grad_fn is not None and vt.grad_fn is not None
    for a, b in ((pt, pe), (vt, ve), (model.last_logits, le), (model.last_value_pre, vpe), (pn, pe), (vn, ve), (pi_, pe)):
        assert torch.equal(a.detach(), b)


# ------------------------------------------------------------------ 4. host reads
def _sync_count(call):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            call()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("called a synchronizing" in str(w.message) for w in caught)


def test_graph_autograd_host_reads(dev):
    """A recording forward reads the device once (_prepare_graph's read); backward() never."""
    from oracle import gnn as og
    params = _with_gcn_biases(og.init_params(1))
    model = _net(params).train()
    xn, en, bn, G = _pyg_edge_case_batch()
    x = torch.from_numpy(xn).float().to(dev).requires_grad_(True)
    ei, bt = torch.from_numpy(en).to(dev), torch.from_numpy(bn).to(dev)
    pi, z, _, _ = _targets(G, model.policy_output_size, 0)
    loss_fn = _losses(pi, z, None, None)["reference"]
    model(x, ei, bt)                       # weights packed
    torch.cuda.synchronize()
    out = {}

    def fwd():
        out["pv"] = model(x, ei, bt)
    calib = _sync_count(lambda: torch.zeros(1, device=dev).item())
    n_fwd = _sync_count(fwd)
    loss = loss_fn(*out["pv"])
    torch.cuda.synchronize()
    n_bwd = _sync_count(loss.backward)
    assert (calib, n_fwd, n_bwd) == (1, 1, 0), (calib, n_fwd, n_bwd)
    assert x.grad is not None


# ------------------------------------------------------------------ 5. determinism
def test_graph_autograd_deterministic(dev):
    """Two backward passes (LDS poisoned before each) give bit-identical gradients."""
    from oracle import gnn as og
    params = _with_gcn_biases(og.init_params(1))
    model = _net(params)
    xn, en, bn, G = _pyg_edge_case_batch()
    pi, z, wp, wv = _targets(G, model.policy_output_size, 0)
    loss = _losses(pi, z, wp, wv)["weighted"]
    a = _hip_grads(model, dev, xn, en, bn, loss)
    b = _hip_grads(model, dev, xn, en, bn, loss)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_graph_autograd_empty_and_double_backward(dev):
    """n = 0 gives zero gradients; a graph id without nodes still feeds its heads; double backward raises."""
    from oracle import gnn as og
    model = _net(og.init_params(1)).train()
    A = model.policy_output_size
    x = torch.zeros((0, 6), device=dev, requires_grad=True)
    policy, value = model(x, torch.zeros((2, 0), dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev))
    assert policy.shape == (0, A) and value.shape == (0, 1)
    (policy.sum() + value.sum()).backward()
    for p in model.parameters():
        assert p.grad is not None and not torch.any(p.grad)
    model.zero_grad(set_to_none=True)
    # graph 0 has no nodes: pooled = 0, so the heads' biases (and the value head's hidden weights) still get gradients
    x = torch.randn((5, 6), device=dev)
    policy, value = model(x, torch.tensor([[0, 1], [1, 2]], device=dev), torch.ones(5, dtype=torch.long, device=dev))
    g = torch.autograd.grad(value[0, 0], [model.value_head[2].bias, model.gcn_layers[0].bias], allow_unused=True)
    assert g[0] is not None and float(g[0].abs().sum()) > 0
    assert g[1] is not None and not torch.any(g[1])          # graph 0 contributes nothing to the trunk
    policy, value = model(x, torch.tensor([[0, 1], [1, 2]], device=dev), torch.ones(5, dtype=torch.long, device=dev))
    (gw,) = torch.autograd.grad(value.sum(), [model.value_head[2].weight], create_graph=True)
    with pytest.raises(RuntimeError):
        gw.sum().backward()


# ------------------------------------------------------------------ 6. optimiser step
@pytest.mark.parametrize("N", [9, 5])
def test_graph_autograd_adam_step_repacks(dev, N):
    """One torch.optim.Adam step on the generic path; the next forward must run the updated weights (the packed buffer is
    keyed on the parameters' version counters, which the optimiser bumps): against oracle.gnn.forward_graph on the model's
    updated state_dict.  9x9 and 5x5 (policy size 57)."""
    from oracle import gnn as og
    params = _with_gcn_biases(og.init_params(3, N=N))
    model = _net(params, N=N).train()
    recs = U.golden(f"walk_{N}x{N}.npz")["states"][:48]
    xn, en, bn = _board_graphs(recs)
    x, ei, bt = torch.from_numpy(xn).float().to(dev), torch.from_numpy(en).to(dev), torch.from_numpy(bn).to(dev)
    pi, z, _, _ = _targets(len(recs), model.policy_output_size, 2)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.zero_grad()
    policy, value = model(x, ei, bt)
    before = model.last_logits.detach().clone()
    _losses(pi, z, None, None)["reference"](policy, value).backward()
    opt.step()
    model.eval()
    with torch.no_grad():
        model(x, ei, bt)
    after = model.last_logits.cpu().numpy()
    assert not np.allclose(after, before.cpu().numpy(), atol=1e-4)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    want = og.forward_graph(sd, xn, en, bn, len(recs))
    np.testing.assert_allclose(after, want["logits"], atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(model.last_value_pre.cpu().numpy(), want["value_pre"], atol=2e-5, rtol=1e-4)


# ------------------------------------------------------------------ 7. scale
def test_graph_autograd_at_scale(dev):
    """4,096 9x9 board graphs (331,776 nodes), gradients against the sparse fp64 reference on the CPU (reference loss)."""
    from oracle import gnn as og
    params = _with_gcn_biases(og.init_params(11))
    model = _net(params)
    states = U.golden("walk_9x9.npz")["states"]
    idx = np.random.RandomState(4096).randint(0, states.shape[0], size=4600)
    xn, en, bn = _board_graphs(states[idx])
    margin = _kink_margins(params, xn, en, bn, len(idx))
    keep = np.nonzero(margin >= KINK)[0]
    print(f"scale: kink filter dropped {len(idx) - keep.size} of {len(idx)} board graphs")
    assert keep.size >= 4096
    recs = states[idx[keep[:4096]]]
    xn, en, bn = _board_graphs(recs)
    assert xn.shape[0] == 331776
    pi, z, _, _ = _targets(4096, model.policy_output_size, 4)
    loss = _losses(pi, z, None, None)["reference"]
    got = _hip_grads(model, dev, xn, en, bn, loss)
    ref = _ref_grads(params, xn, en, bn, 4096, loss)
    _assert_grads_close(got, ref, GRAD_BAR, "4,096 board graphs")
