#!/usr/bin/env python3
"""Time the loss form (include/aqgnn.h "loss form") inside the three HIP training steps, and bench.py's headline on two trees.

Per trainer -- the fused 6/128/3 step, a general shape (6/64/2) and the CNN (128 filters x 16 blocks), 9x9 at batch 128 -- five
forms take turns, `--rounds` times; each turn times `--steps` steps between two events; the median over the rounds is reported:
    off, off2   two trainers with the option off: their difference is the spread a form has to leave to count as a cost or a saving
    ce          policy_loss='cross_entropy': the fused step's second board instantiation; one loss launch in place of two elsewhere
    ce_w        the same with value_loss_weight=0.25
    ref_w       the reference's form with value_loss_weight=0.25 (the fused step's third instantiation; one more launch elsewhere)
With --parent DIR (a built tree of the parent commit), bench.py --gpus 1 is run in DIR and in this tree as child processes, taking
turns in both orders (parent, this, this, parent, ...), and both series of headline values are reported.  Prints one JSON line.

Usage: python tools/policy_loss_time.py [--batch 128] [--board 9] [--steps 50] [--rounds 9] [--parent DIR --bench-turns 2]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def headline(tree, steps, warmup):
    """bench.py's headline value in `tree`, one child process."""
    run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree}: {run.stderr[-2000:]}")
    return float(json.loads(run.stdout.strip().splitlines()[-1])["value"])


def main():
    from alphaquoridorgnn_amd import _lib, constants, game_logic
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: bench.py's headline there and here, taking turns")
    ap.add_argument("--bench-turns", type=int, default=2, help="pairs of bench.py runs (each pair in the other order than the last)")
    ap.add_argument("--bench-steps", type=int, default=2)
    ap.add_argument("--bench-warmup", type=int, default=1)
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
    forms = {"off": {}, "off2": {}, "ce": dict(policy_loss="cross_entropy"),
             "ce_w": dict(policy_loss="cross_entropy", value_loss_weight=0.25), "ref_w": dict(value_loss_weight=0.25)}
    out = dict(board=N, batch=B, steps=args.steps, rounds=args.rounds, step_ms={})
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
    if args.parent:
        torch.cuda.synchronize()
        values = {"parent": [], "this": []}
        for turn in range(args.bench_turns):
            for name in (("parent", "this") if turn % 2 == 0 else ("this", "parent")):
                values[name].append(headline(args.parent if name == "parent" else HERE, args.bench_steps, args.bench_warmup))
                print("bench", name, values[name][-1], file=sys.stderr, flush=True)
        out["bench_headline"] = {k: dict(values=[round(x, 2) for x in v], median=round(float(np.median(v)), 2)) for k, v in values.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
