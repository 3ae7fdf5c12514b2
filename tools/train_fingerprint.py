#!/usr/bin/env python3
"""Fingerprint of what the three trainers compute, for comparing two builds of the library (refactoring check).

    AQG_LIB_PATH=/path/to/old.so python tools/train_fingerprint.py > old.txt
    AQG_LIB_PATH=/path/to/new.so python tools/train_fingerprint.py > new.txt  &&  diff old.txt new.txt

The training kernels use no atomics on results and are run-to-run identical, so equal builds print equal lines: one SHA-256 per
case over every parameter, adam_m, adam_v and the returned loss sums.  Inputs and weights are seeded on the CPU.  Cases: run_epoch
over 5 positions at max_batch 2 (steps of 2, 2 and the short 1) under train_fused 1 / 2 / 3 on 9x9 and on 3x3 (padding rows); one
step(update=False) followed by the Adam-only call (mode 2); a GeneralTrainer on a 6/8/1 network at 5x5; a CNNTrainer on
CNNNetwork(8, 1, board_size=5)."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from alphaquoridorgnn_amd import _lib
from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer
from oracle import quoridor as oq

dev = _lib.require_gpu("cuda:0")


def positions(N, count, seed):
    """`count` records of random legal play on the oracle's rules, with probability targets and outcomes"""
    rng = np.random.RandomState(seed)
    recs = []
    while len(recs) < count:
        s = oq.State(N=N)
        for _ in range(12):
            if s.is_done():
                break
            recs.append(s.rec.copy())
            la = s.legal_actions()
            s = s.next(la[rng.randint(len(la))])
    A = N * N + 2 * (N - 1) ** 2
    pi = rng.rand(count, A).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    z = rng.choice([-1.0, 0.0, 1.0], count).astype(np.float32)
    return torch.from_numpy(np.stack(recs[:count])), torch.from_numpy(pi), torch.from_numpy(z)


def digest(tr, sums):
    h = hashlib.sha256()
    for group in (tr.params, tr.adam_m, tr.adam_v, [sums]):
        for x in group:
            h.update(x.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def graph_net(N, hidden=128, layers=3, seed=0):
    torch.manual_seed(seed)
    return GraphPolicyValueNetwork(6, hidden, layers, N * N + 2 * (N - 1) ** 2, board_size=N).to(dev)


def epoch(tr, N):
    st, pi, z = positions(N, 5, 40 + N)
    sums = tr.run_epoch(st, pi, z, torch.tensor([3, 0, 4, 1, 2]), lr=1e-3)
    torch.cuda.synchronize()
    return digest(tr, sums)


for N in (9, 3):
    for fused in (1, 2, 3):
        _lib.set_option("train_fused", fused)
        print(f"run_epoch {N}x{N} train_fused={fused}: {epoch(GNNTrainer(graph_net(N), max_batch=2), N)}")
_lib.set_option("train_fused", 2)
tr = GNNTrainer(graph_net(9, seed=1), max_batch=4)
st, pi, z = (x.to(dev) for x in positions(9, 4, 7))
losses = torch.stack(tr.step(st, pi, z, lr=1e-3, update=False))
tr.step_count += 1
tr.t.step = tr.step_count
tr._call(st, pi, z, 2)                                              # Adam only, on the gradients of the call before
torch.cuda.synchronize()
print(f"step(update=False) + mode 2 9x9: {digest(tr, losses)}")
print(f"GeneralTrainer 6/8/1 5x5: {epoch(GeneralTrainer(graph_net(5, hidden=8, layers=1, seed=2), max_batch=2), 5)}")
torch.manual_seed(3)
print(f"CNNTrainer CNNNetwork(8, 1) 5x5: {epoch(CNNTrainer(CNNNetwork(8, 1, board_size=5).to(dev), max_batch=2), 5)}")
print("fallbacks:", _lib.load().aqg_gcn_train_fallbacks(1))
