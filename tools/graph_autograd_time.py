#!/usr/bin/env python3
"""Developer timing: autograd through forward(x, edge_index, batch) at 4,096 9x9 board graphs (331,776 nodes).

Prints, in ms per call (HIP events, median of REPS after warm-up):
  hip forward (recording)  -- train-mode forward that keeps H1..H3 (host preparation included: one device-to-host read)
  hip backward             -- loss.backward() through the width-generic primitives (csrc/gcn_general.hip)
  torch eager fwd+bwd      -- the same network restated in fp32 torch ops on the GPU (index_add_ aggregation), for comparison
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from alphaquoridorgnn_amd import _lib
from tests import _util as U
from tests.test_gpu_parity import _board_graphs, _net, _with_gcn_biases
from oracle import gnn as og

REPS = int(os.environ.get("REPS", "10"))
B = int(os.environ.get("GRAPHS", "4096"))


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def eager(params, x, src, dst, w, batch, G):
    """fp32 torch restatement: gcn_norm weights given, aggregation by index_add_, mean pool by index_add_."""
    n = x.shape[0]
    h = x
    for l in range(3):
        xw = h @ params[f"gcn_layers.{l}.lin.weight"].T
        h = torch.relu(torch.zeros((n, xw.shape[1]), device=x.device).index_add_(0, dst, w[:, None] * xw[src])
                       + params[f"gcn_layers.{l}.bias"])
    cnt = torch.zeros(G, device=x.device).index_add_(0, batch, torch.ones(n, device=x.device))
    pooled = torch.zeros((G, h.shape[1]), device=x.device).index_add_(0, batch, h) / cnt.clamp(min=1.0)[:, None]
    logits = torch.relu(pooled @ params["policy_head.0.weight"].T + params["policy_head.0.bias"]) @ params["policy_head.2.weight"].T \
        + params["policy_head.2.bias"]
    vpre = torch.relu(pooled @ params["value_head.0.weight"].T + params["value_head.0.bias"]) @ params["value_head.2.weight"].T \
        + params["value_head.2.bias"]
    return torch.softmax(logits, 1), torch.tanh(vpre)


def main():
    dev = _lib.require_gpu("cuda:0")
    params = _with_gcn_biases(og.init_params(11))
    model = _net(params).train()
    states = U.golden("walk_9x9.npz")["states"]
    recs = states[np.random.RandomState(4096).randint(0, states.shape[0], size=B)]
    xn, en, bn = _board_graphs(recs)
    x = torch.from_numpy(xn).float().to(dev)
    ei, bt = torch.from_numpy(en).to(dev), torch.from_numpy(bn).to(dev)
    rng = np.random.RandomState(0)
    pi = torch.from_numpy(rng.dirichlet(np.ones(model.policy_output_size), B)).float().to(dev)
    z = torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], B)).float().to(dev)

    def loss_of(p, v):
        return F.cross_entropy(p, pi) + F.mse_loss(v.squeeze(), z)

    state = {}

    def fwd():
        state["loss"] = loss_of(*model(x, ei, bt))

    def bwd():
        state["loss"].backward()

    t_fwd = timed(fwd)
    # backward alone: a fresh recorded forward before every timed backward
    ts = []
    for i in range(REPS + 3):
        model.zero_grad(set_to_none=True)
        fwd()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        bwd()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    t_bwd = float(np.median(ts))
    with torch.no_grad():
        model.eval()
        t_eval = timed(lambda: model(x, ei, bt))
        model.train()

    # torch eager restatement (same gcn_norm entries as the kernels: _prepare_graph's CSR)
    ptr, src, w, gptr, G = model._prepare_graph(x, ei, bt)
    dst = torch.repeat_interleave(torch.arange(x.shape[0], device=dev), (ptr[1:] - ptr[:-1]).long())
    tp = {k: torch.from_numpy(np.asarray(v)).float().to(dev).requires_grad_(True) for k, v in params.items()}
    src_l, bt_l = src.long(), bt.long()

    def eager_step():
        for t in tp.values():
            t.grad = None
        loss_of(*eager(tp, x, src_l, dst, w, bt_l, G)).backward()
    t_eager = timed(eager_step)

    def eager_fwd():
        with torch.no_grad():
            eager(tp, x, src_l, dst, w, bt_l, G)
    t_eager_fwd = timed(eager_fwd)
    print(f"graphs {B}, nodes {x.shape[0]}, edges {en.shape[1]}")
    print(f"hip eval forward (no_grad):        {t_eval:8.3f} ms")
    print(f"hip forward (recording) + loss:    {t_fwd:8.3f} ms")
    print(f"hip backward:                      {t_bwd:8.3f} ms")
    print(f"hip forward + backward:            {t_fwd + t_bwd:8.3f} ms")
    print(f"torch eager fp32 forward (no_grad):{t_eager_fwd:8.3f} ms")
    print(f"torch eager fp32 forward+backward: {t_eager:8.3f} ms")


if __name__ == "__main__":
    main()
