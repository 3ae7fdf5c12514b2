#!/usr/bin/env python3
"""Time the residual CNN (pv_network_cnn.CNNNetwork, 9x9, 128 filters x 16 blocks by default) on the GPU.

  * the HIP forward (forward_states on board records) at several batch sizes, with its share of the f32 matrix peak computed from
    the shape (2 V 9 Cin Cout FLOP per conv: about 0.77 GFLOP per board at 128/16, so at most ~205 k boards/s at 157.3 TFLOP/s);
  * the stock PyTorch-ROCm eval forward of the same module on [B,6,9,9] planes, in the same process;
  * self-play moves/s on the engine with evaluator='cnn', without and with the evaluation cache;
  * evaluator='external' (model.predict per leaf from the host) with the same model at a small size.

Prints one JSON line.  Usage: python tools/cnn_time.py [--batches 256,4096,16384] [--games 1024] [--sims 50] [--moves 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MATRIX = 157.3e12


def gflop_per_board(F, L, N):
    V = N * N
    convs = [(6, F)] + [(F, F)] * (2 * L)
    return sum(2 * V * 9 * ci * co for ci, co in convs) / 1e9


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps / 1e3          # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--batches", default="256,4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--moves", type=int, default=4)
    ap.add_argument("--cache-slots", type=int, default=1024)
    ap.add_argument("--skip-stock", action="store_true")
    args = ap.parse_args()

    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from tests import _util as U
    dev = _lib.require_gpu("cuda:0")
    torch.manual_seed(0)
    N = 9
    net = CNNNetwork(args.filters, args.blocks, board_size=N).to(dev).eval()
    gf = gflop_per_board(args.filters, args.blocks, N)
    pool = U.golden("walk_9x9.npz")["states"]
    out = dict(filters=args.filters, blocks=args.blocks, board=N, gflop_per_board=round(gf, 4), forward={})
    for B in [int(b) for b in args.batches.split(",")]:
        recs = torch.from_numpy(np.ascontiguousarray(pool[np.arange(B) % pool.shape[0]])).to(dev)
        with torch.no_grad():
            s = timed(lambda: net.forward_states(recs), args.reps)
        row = dict(hip_ms=round(s * 1e3, 3), hip_boards_per_s=round(B / s), hip_peak_share=round(B * gf * 1e9 / s / PEAK_F32_MATRIX, 4))
        if not args.skip_stock:
            planes = torch.from_numpy(net.preprocess_input([((int(r[0]), int(r[1])), (int(r[2]), int(r[3])), list(r[4:68]))
                                                            for r in recs.cpu().numpy()])).to(dev)
            with torch.no_grad():
                s2 = timed(lambda: net._forward_stock(planes), args.reps)
            row.update(stock_ms=round(s2 * 1e3, 3), stock_boards_per_s=round(B / s2))
        out["forward"][str(B)] = row
        del recs
        torch.cuda.empty_cache()

    def moves_per_s(G, sims, moves, **kw):
        eng = BatchedSelfPlay(net, num_games=G, sims=sims, seed=1, record_history=False, **kw)
        eng.move()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(moves):
            eng.move()
        torch.cuda.synchronize()
        return G * moves / (time.perf_counter() - t)

    out["selfplay"] = dict(games=args.games, sims=args.sims,
                           cnn_moves_per_s=round(moves_per_s(args.games, args.sims, args.moves, evaluator="cnn", eval_cache_slots=0), 1),
                           cnn_cache_moves_per_s=round(moves_per_s(args.games, args.sims, args.moves, evaluator="cnn",
                                                                   eval_cache_slots=args.cache_slots), 1))
    out["external"] = dict(games=4, sims=8, moves_per_s=round(moves_per_s(4, 8, 1, evaluator="external"), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
