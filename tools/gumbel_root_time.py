"""Times a self-play move with the Gumbel root search against the two PUCT forms on one GPU: GAMES games on 9x9 with the default
6/128/3 network (evaluator='gnn'), at every simulation count of SIMS_LIST --
    gumbel   gumbel_considered = CONSIDERED (the three-launch simulation form around the root launch),
    puct3    the three-launch PUCT form (option step_heads 0): the difference is the two extra launches and the new scoring,
    fused    the default form (the heads inside the step, the forms beside it): the difference is what not fusing costs.
Per form: WARMUP moves (graph capture, caches), then the median, fastest and slowest of MOVES moves, each timed with a pair of
events; the forms take turns move by move, so drift hits all of them alike (the step_heads option is set in front of every move: it
is part of the captured graph's key).  Every engine plays from the same seed.
Then GENERATION = 1: games/s of one whole GAMES-slot generation at the first simulation count with the Gumbel search beside one at the
last simulation count with PUCT (throughput only: nothing here says which games are better)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay, MultiSetSelfPlay   # noqa: E402

GAMES = int(os.environ.get("GAMES", "2048"))
SIMS_LIST = [int(x) for x in os.environ.get("SIMS_LIST", "32,200").split(",")]
CONSIDERED = int(os.environ.get("CONSIDERED", "16"))
MOVES, WARMUP = int(os.environ.get("MOVES", "9")), int(os.environ.get("WARMUP", "2"))
GENERATION = int(os.environ.get("GENERATION", "1"))


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        for sims in SIMS_LIST:
            kw = dict(num_games=GAMES, sims=sims, seed=1, record_history=False)
            forms = {"gumbel": (BatchedSelfPlay(net, gumbel_considered=CONSIDERED, **kw), 1),
                     "puct3": (BatchedSelfPlay(net, **kw), 0),
                     "fused": (BatchedSelfPlay(net, **kw), 1)}
            times = {name: [] for name in forms}
            for m in range(WARMUP + MOVES):
                for name, (eng, step_heads) in forms.items():
                    _lib.set_option("step_heads", step_heads)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    eng.move()
                    b.record()
                    b.synchronize()
                    if m >= WARMUP:
                        times[name].append(a.elapsed_time(b))
            _lib.set_option("step_heads", 1)
            med = {name: float(np.median(t)) for name, t in times.items()}
            for name, t in times.items():
                print(f"sims {sims:4d}  {name:7s} move median {med[name]:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                      f"({GAMES} games, considered {CONSIDERED}, {MOVES} moves after {WARMUP})", flush=True)
            print(f"sims {sims:4d}  gumbel against puct3 {100.0 * (med['gumbel'] / med['puct3'] - 1.0):+.2f} %   against fused "
                  f"{100.0 * (med['gumbel'] / med['fused'] - 1.0):+.2f} %   puct3 against fused {100.0 * (med['puct3'] / med['fused'] - 1.0):+.2f} %",
                  flush=True)
            del forms
    if GENERATION:
        for name, sims, kw in (("gumbel", SIMS_LIST[0], dict(gumbel_considered=CONSIDERED)), ("puct", SIMS_LIST[-1], {})):
            eng = MultiSetSelfPlay(net, num_games=GAMES, sims=sims, seed=1, device=dev, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = eng.play_generation()
            eng.sync()
            dt = time.perf_counter() - t0
            print(f"generation  {name:7s} sims {sims:4d}  {c['finished']} games in {dt:7.3f} s = {c['finished'] / dt:9.1f} games/s  "
                  f"({len(eng.sets)} sets)", flush=True)
            del eng


if __name__ == "__main__":
    main()
