"""Times a self-play move with and without root exploration noise on one GPU: GAMES games x SIMS simulations on 9x9 with the default
6/128/3 network (evaluator='gnn'), root_noise_eps 0 against 0.25 in generator mode, with and without the evaluation cache.  Per
configuration: WARMUP moves (graph capture, caches), then the median, fastest and slowest of MOVES moves, each timed with a pair of
events; the engines take turns move by move, so drift hits all of them alike.  Every engine plays from the same seed.
Prints one line per configuration and the cost of the noise as a percentage of the noise-free move."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402

GAMES, SIMS = int(os.environ.get("GAMES", "2048")), int(os.environ.get("SIMS", "200"))
MOVES, WARMUP = int(os.environ.get("MOVES", "5")), int(os.environ.get("WARMUP", "2"))
CACHE_SLOTS = int(os.environ.get("CACHE_SLOTS", "1024"))


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        for slots in (0, CACHE_SLOTS):
            engines = {eps: BatchedSelfPlay(net, num_games=GAMES, sims=SIMS, seed=1, record_history=False, eval_cache_slots=slots,
                                            root_noise_eps=eps) for eps in (0.0, 0.25)}
            times = {eps: [] for eps in engines}
            for m in range(WARMUP + MOVES):
                for eps, eng in engines.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    eng.move()
                    b.record()
                    b.synchronize()
                    if m >= WARMUP:
                        times[eps].append(a.elapsed_time(b))
            med = {eps: float(np.median(t)) for eps, t in times.items()}
            for eps, t in times.items():
                print(f"cache {slots:5d}  eps {eps:4.2f}  move median {med[eps]:8.2f} ms  min {min(t):8.2f}  max {max(t):8.2f}  "
                      f"({GAMES} games x {SIMS} sims, {MOVES} moves after {WARMUP})", flush=True)
            print(f"cache {slots:5d}  noise on costs {100.0 * (med[0.25] / med[0.0] - 1.0):+.2f} % of the noise-free move", flush=True)
            del engines


if __name__ == "__main__":
    main()
