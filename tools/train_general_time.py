"""Times one optimisation step at batch 128 on 9x9 boards, per network shape (6/128/3, 6/256/3, 6/64/2), in one process with the
forms taking turns (median of REPS rounds of STEPS steps each, after WARMUP rounds):
  general   train_network.GeneralTrainer.step (aqg_gcn_train_step_general: forward, losses, backward, Adam on HIP kernels)
  autograd  the route it replaces: forward(x, edge_index, batch) over the same boards in train mode, the reference's two losses,
            backward() through the library's kernels, torch.optim.Adam.  The graphs (x, edge_index, batch) are built once
            before timing, from the library's featuriser: the host-side graph building a user would add per step is NOT counted
  gnn       train_network.GNNTrainer.step (the fused 6/128/3 step), at 6/128/3 only
Prints one JSON line: ms per step of each form and shape."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.train_network import GeneralTrainer, GNNTrainer   # noqa: E402

B, N = 128, 9
REPS, WARMUP, STEPS = int(os.environ.get("REPS", "7")), int(os.environ.get("WARMUP", "2")), int(os.environ.get("STEPS", "20"))
SHAPES = [(6, 128, 3), (6, 256, 3), (6, 64, 2)]


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / STEPS


def alternating(fns):
    for _ in range(WARMUP):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for i, f in enumerate(fns):
            ts[i].append(events_ms(f))
    return [float(np.median(t)) for t in ts]


def batch(dev):
    from tests.test_gpu_parity import _small_board_states
    rng = np.random.RandomState(0)
    recs = _small_board_states(N)
    recs = torch.from_numpy(recs[rng.randint(0, recs.shape[0], B)]).to(dev)
    A = N * N + 2 * (N - 1) ** 2
    pi = rng.rand(B, A) * (rng.rand(B, A) < 0.2) + 1e-3
    pi = torch.from_numpy((pi / pi.sum(1, keepdims=True)).astype(np.float32)).to(dev)
    z = torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], B).astype(np.float32)).to(dev)
    return recs, pi, z


def graphs(recs, dev):
    """(x, edge_index, batch) of the board records: the featuriser's node features and its ELL rows as an edge list (the self
    loop, entry 0 of each row, is GCNConv's own and is left out)."""
    lib = _lib.load()
    R = B * N * N
    x = torch.empty((R, 6), dtype=torch.float32, device=dev)
    idx = torch.empty((R, 5), dtype=torch.int32, device=dev)
    w = torch.empty((R, 5), dtype=torch.float32, device=dev)
    _lib.check(lib.aqg_gcn_boards_graph(N, _lib.ptr(recs), B, _lib.ptr(x), _lib.ptr(idx), _lib.ptr(w), _lib.stream_ptr(dev)),
               "aqg_gcn_boards_graph")
    dst = torch.arange(R, device=dev).unsqueeze(1).expand(R, 4)
    src = idx[:, 1:].long()
    keep = src >= 0
    edge_index = torch.stack([src[keep], dst[keep]])
    bt = torch.arange(B, device=dev).repeat_interleave(N * N)
    return x, edge_index, bt


def main():
    dev = _lib.require_gpu()
    recs, pi, z = batch(dev)
    x, ei, bt = graphs(recs, dev)
    ce, mse = torch.nn.CrossEntropyLoss(), torch.nn.MSELoss()
    out = {"batch": B, "board": N, "steps_per_sample": STEPS, "reps": REPS, "ms_per_step": {}}
    for shape in SHAPES:
        torch.manual_seed(0)
        net_g = P.GraphPolicyValueNetwork(*shape, 209).to(dev)
        net_a = P.GraphPolicyValueNetwork(*shape, 209).to(dev).train()
        net_a.load_state_dict(net_g.state_dict())
        tr = GeneralTrainer(net_g, max_batch=B)
        opt = torch.optim.Adam(net_a.parameters(), lr=1e-3)

        def general():
            tr.step(recs, pi, z, lr=1e-4)

        def autograd():
            policy, value = net_a(x, ei, bt)
            loss = ce(policy, pi) + mse(value.squeeze(), z)
            opt.zero_grad()
            loss.backward()
            opt.step()

        fns, names = [general, autograd], ["general", "autograd"]
        if shape == (6, 128, 3):
            net_f = P.GNNNetwork().to(dev)
            net_f.load_state_dict(net_g.state_dict())
            trf = GNNTrainer(net_f, max_batch=B)
            fns.append(lambda: trf.step(recs, pi, z, lr=1e-4))
            names.append("gnn")
        ms = alternating(fns)
        out["ms_per_step"]["x".join(map(str, shape))] = {n: round(t, 4) for n, t in zip(names, ms)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
