#!/usr/bin/env python3
"""Time weight averaging (train_network.WeightAverage) inside the three HIP training steps, and the averaging launch alone against
torch's foreach operations.

Per trainer -- the fused 6/128/3 step, a general shape (6/64/2) and the CNN (128 filters x 16 blocks), 9x9 at batch 128 -- four
forms take turns, `--rounds` times; each turn times `--steps` steps between two events; the median over the rounds is reported:
    off, off2   two trainers without an average: their difference is the spread a form has to leave to count as a cost
    k1          an average updated behind every step (one more launch per step)
    k8          an average updated behind every eighth step
The launch alone: WeightAverage.update() (one launch over all tensors) against torch._foreach_mul_(avg, d) followed by
torch._foreach_add_(avg, params, alpha=1 - d) over the same tensors, at the 6/128/3 and the 128 x 16 CNN parameter counts (the CNN's
running statistics included).  Prints one JSON line.

Usage: python tools/weight_average_time.py [--batch 128] [--board 9] [--steps 50] [--rounds 9]
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
    from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer, WeightAverage
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
    kinds = {"fused_6x128x3": lambda: GNNTrainer(GraphPolicyValueNetwork(6, 128, 3, A, board_size=N).to(dev), max_batch=B),
             "general_6x64x2": lambda: GeneralTrainer(GraphPolicyValueNetwork(6, 64, 2, A, board_size=N).to(dev), max_batch=B),
             "cnn_128x16": lambda: CNNTrainer(CNNNetwork(128, 16, board_size=N).to(dev), max_batch=B)}
    forms = {"off": None, "off2": None, "k1": 1, "k8": 8}
    out = dict(board=N, batch=B, steps=args.steps, rounds=args.rounds, step_ms={}, launch_us={})
    for kind, make in kinds.items():
        torch.manual_seed(0)
        trainers = {f: make() for f in forms}
        for f, every in forms.items():
            if every is not None:
                WeightAverage(trainers[f], decay=0.999, every=every)
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
        if kind != "general_6x64x2":
            avg = trainers["k1"].average
            shadows, sources, d = avg.tensors(), avg.sources, 0.999

            def foreach():
                torch._foreach_mul_(shadows, d)
                torch._foreach_add_(shadows, sources, alpha=1.0 - d)

            for fn in (avg.update, foreach):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            ours, theirs = [], []
            for _ in range(args.rounds):
                ours.append(timed(avg.update, 200) * 1e3)
                theirs.append(timed(foreach, 200) * 1e3)
            out["launch_us"][kind] = dict(tensors=len(shadows), n=sum(x.numel() for x in shadows),
                                          aqg_weight_average_update=round(float(np.median(ours)), 2),
                                          torch_foreach_mul_add=round(float(np.median(theirs)), 2))
            print(kind, out["launch_us"][kind], file=sys.stderr, flush=True)
        del trainers
    print(json.dumps(out))


if __name__ == "__main__":
    main()
