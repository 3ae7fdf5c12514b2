#!/usr/bin/env python3
"""Time the residual CNN's training step on HIP (train_network.CNNTrainer) against the stock PyTorch-ROCm step on the same GPU.

  * HIP: CNNTrainer.step (one library call: forward with every BatchNorm in train mode, both losses, backward, Adam) and
    run_epoch (every step of an epoch in one call), per step;
  * stock: what the reference's train_network.py:84-92 runs -- the module in train mode, autograd, torch.optim.Adam(lr=0.001) --
    on [B,6,N,N] planes of the same positions (featurised once, outside the timing: the reference's DataLoader hands it planes).

Per shape, the step's share of the f32 matrix peak (157.3 TFLOP/s) counts 3 x the convs' forward FLOP (forward, dX, dW; the stem's
dX is not computed but is counted, as for stock).  Default shapes: 128 filters x 16 blocks (the reference's) and 64 x 6, on 9x9 at
batch 128.  Prints one JSON line.

Usage: python tools/cnn_train_time.py [--shapes 128x16,64x6] [--board 9] [--batch 128] [--steps 20] [--epoch-positions 1024]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MATRIX = 157.3e12


def step_flop(F, L, N, B):
    V = N * N
    convs = [(6, F)] + [(F, F)] * (2 * L)
    return 3 * sum(2 * B * V * 9 * ci * co for ci, co in convs)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / reps


def main():
    from alphaquoridorgnn_amd import _lib, constants, game_logic
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16,64x6")
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--epoch-positions", type=int, default=1024)
    args = ap.parse_args()
    dev = _lib.require_gpu()
    N, B = args.board, args.batch
    rng = np.random.RandomState(0)
    n = max(args.epoch_positions, B)
    new = lambda: game_logic.State(board_size=N, num_walls=constants.board_params(N)[0])   # noqa: E731
    recs, s = [], new()
    while len(recs) < n:
        recs.append(s.record())
        la = s.legal_actions()
        s = s.next(la[rng.randint(len(la))])
        if s.is_done():
            s = new()
    recs = np.stack(recs)
    A = N * N + 2 * (N - 1) ** 2
    pi = rng.rand(n, A).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    z = rng.choice([-1.0, 0.0, 1.0], n).astype(np.float32)
    S, P, Z = torch.from_numpy(recs).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev)
    out = dict(board=N, batch=B, rows={})
    for shape in args.shapes.split(","):
        F, L = (int(v) for v in shape.split("x"))
        torch.manual_seed(0)
        net = CNNNetwork(F, L, board_size=N).to(dev)
        tr = CNNTrainer(net, max_batch=B)
        hip = timed(lambda: tr.step(S[:B], P[:B], Z[:B]), args.steps)
        order = torch.arange(n, device=dev)
        steps = (n + B - 1) // B
        epoch = timed(lambda: tr.run_epoch(S, P, Z, order), 2, warmup=1) / steps
        ref = CNNNetwork(F, L, board_size=N).to(dev).train()
        x = torch.from_numpy(ref.preprocess_input([(
            (int(r[0]), int(r[1])), (int(r[2]), int(r[3])), [int(w) for w in r[4:4 + (N - 1) ** 2]]) for r in recs[:B]])).to(dev)
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
        ce, mse = torch.nn.CrossEntropyLoss(), torch.nn.MSELoss()

        def stock():
            opt.zero_grad()
            policy, value = ref(x)
            (ce(policy, P[:B]) + mse(value.squeeze(), Z[:B])).backward()
            opt.step()

        st = timed(stock, args.steps)
        fl = step_flop(F, L, N, B)
        out["rows"][shape] = dict(hip_step_ms=round(hip * 1e3, 3), hip_epoch_step_ms=round(epoch * 1e3, 3),
                                  stock_step_ms=round(st * 1e3, 3), speedup=round(st / hip, 3),
                                  hip_peak_share=round(fl / hip / PEAK_F32_MATRIX, 4),
                                  stock_peak_share=round(fl / st / PEAK_F32_MATRIX, 4))
        print(shape, out["rows"][shape], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
