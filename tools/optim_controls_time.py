#!/usr/bin/env python3
"""Time the optimiser controls (weight decay, global-norm clipping) inside the three HIP training steps, and the gradient-norm
kernels alone against torch.linalg.vector_norm.

Per trainer -- the fused 6/128/3 step, a general shape (6/64/2) and the CNN (128 filters x 16 blocks), 9x9 at batch 128 -- five
forms take turns, `--rounds` times; each turn times `--steps` steps between two events; the median over the rounds is reported:
    off, off2   two trainers with every control off: their difference is the spread a form has to leave to count as a cost
    decay       weight_decay=1e-4, decoupled: the same launches as off
    clip        max_grad_norm=1.0: + the norm's partials launch (fused step: + compute / clip / update as separate launches)
    both        decay and clip
The norm alone: aqg_grad_norm (two launches: partials, combine) against torch.linalg.vector_norm on the same buffer, at the
6/128/3 parameter count and at 4.76 M floats.  Prints one JSON line.

Usage: python tools/optim_controls_time.py [--batch 128] [--board 9] [--steps 50] [--rounds 9]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    from alphaquoridorgnn_amd import _lib, constants, game_logic
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer, grad_norm
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    dev = _lib.require_gpu()
    N, B = args.board, args.batch
    A = N * N + 2 * (N - 1) ** 2
    rng = np.random.RandomState(0)
    new = lambda: game_logic.State(board_size=N, num_walls=constants.board_params(N)[0])   # noqa: E731
    recs, s = [], new()
    while len(recs) < B:
        recs.append(s.record())
        la = s.legal_actions()
        s = s.next(la[rng.randint(len(la))])
        if s.is_done():
            s = new()
    pi = rng.rand(B, A).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    S = torch.from_numpy(np.stack(recs)).to(dev)
    P = torch.from_numpy(pi).to(dev)
    Z = torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], B).astype(np.float32)).to(dev)
    kinds = {"fused_6x128x3": lambda kw: GNNTrainer(GraphPolicyValueNetwork(6, 128, 3, A, board_size=N).to(dev), max_batch=B, **kw),
             "general_6x64x2": lambda kw: GeneralTrainer(GraphPolicyValueNetwork(6, 64, 2, A, board_size=N).to(dev), max_batch=B, **kw),
             "cnn_128x16": lambda kw: CNNTrainer(CNNNetwork(128, 16, board_size=N).to(dev), max_batch=B, **kw)}
    forms = {"off": {}, "off2": {}, "decay": dict(weight_decay=1e-4), "clip": dict(max_grad_norm=1.0),
             "both": dict(weight_decay=1e-4, max_grad_norm=1.0)}
    out = dict(board=N, batch=B, steps=args.steps, rounds=args.rounds, step_ms={}, norm_us={})
    for kind, make in kinds.items():
        torch.manual_seed(0)
        trainers = {f: make(kw) for f, kw in forms.items()}
        for tr in trainers.values():
            for _ in range(3):
                tr.step(S, P, Z)
        torch.cuda.synchronize()
        series = {f: [] for f in forms}
        for _ in range(args.rounds):
            for f, tr in trainers.items():
                series[f].append(timed(lambda: tr.step(S, P, Z), args.steps))
        out["step_ms"][kind] = {f: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))
                                for f, v in series.items()}
        print(kind, out["step_ms"][kind], file=sys.stderr, flush=True)
        del trainers
    sizes = {"6x128x3_params": sum(p.numel() for p in GraphPolicyValueNetwork(6, 128, 3, A, board_size=N).parameters()),
             "4.76M": 4760000}
    for name, n in sizes.items():
        x = torch.randn(n, device=dev)
        for fn in (lambda: grad_norm(x), lambda: torch.linalg.vector_norm(x)):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ours, theirs = [], []
        for _ in range(args.rounds):
            ours.append(timed(lambda: grad_norm(x), 200) * 1e3)
            theirs.append(timed(lambda: torch.linalg.vector_norm(x), 200) * 1e3)
        out["norm_us"][name] = dict(n=n, aqg_grad_norm=round(float(np.median(ours)), 2),
                                    torch_vector_norm=round(float(np.median(theirs)), 2))
        print(name, out["norm_us"][name], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
