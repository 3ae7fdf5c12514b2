"""Times a self-play move with and without tree reuse on one GPU: GAMES games x SIMS simulations on 9x9 with the default 6/128/3
network (evaluator='gnn'), tree_reuse off against on (tree_reuse_visits = SIMS).  WARMUP moves (graph capture, caches; the first move
of a game has nothing to keep), then the median, fastest and slowest of MOVES moves, each timed with a pair of events; the two engines
take turns move by move, so drift hits both alike.  Both play from the same seed.  Then, on the reuse engine: the keep launch alone,
one launch timed on the pools of a SIMS-simulation search from the positions its games stand at, with the most visited child as the
chosen one; and, on a fresh engine, a whole generation's share of moves that started from a kept subtree with their mean kept visits.
Prints one line per figure."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402

GAMES, SIMS = int(os.environ.get("GAMES", "2048")), int(os.environ.get("SIMS", "200"))
MOVES, WARMUP = int(os.environ.get("MOVES", "7")), int(os.environ.get("WARMUP", "3"))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        engines = {on: BatchedSelfPlay(net, num_games=GAMES, sims=SIMS, seed=1, tree_reuse=on) for on in (False, True)}
        for on, eng in engines.items():
            print(f"reuse {'on ' if on else 'off'}  pool {eng.node_cap * 32 / 2 ** 20:6.2f} MiB per game ({eng.node_cap} records), path "
                  f"{eng.t['path'].shape[1]} entries", flush=True)
        times = {on: [] for on in engines}
        for m in range(WARMUP + MOVES):
            for on, eng in engines.items():
                t = timed(eng.move)
                if m >= WARMUP:
                    times[on].append(t)
        med = {on: float(np.median(t)) for on, t in times.items()}
        for on, t in times.items():
            print(f"reuse {'on ' if on else 'off'}  move median {med[on]:8.2f} ms  min {min(t):8.2f}  max {max(t):8.2f}  "
                  f"({GAMES} games x {SIMS} sims, {MOVES} moves after {WARMUP})", flush=True)
        print(f"reuse on costs {100.0 * (med[True] / med[False] - 1.0):+.2f} % of the move without it (keep launch + larger pool under the step)", flush=True)
        eng = engines[True]
        s = eng.tree_reuse_stats()
        print(f"after {WARMUP + MOVES} moves: {s['moves_kept']} of {GAMES * (WARMUP + MOVES)} moves left a kept subtree to the next, mean kept "
              f"visits {s['mean_kept_visits']:.1f}", flush=True)
        # the keep launch alone
        roots = eng.root_states72()
        live = eng.t["game_active"].clone()
        _lib.check(eng.lib.aqg_engine_search(ctypes.byref(eng.e), _lib.ptr(roots), eng._stream()), "aqg_engine_search")
        eng.t["game_active"].copy_(live)
        visits = torch.empty((GAMES, _lib.MAX_LEGAL), dtype=torch.int32, device=dev)
        actions = torch.empty((GAMES, _lib.MAX_LEGAL), dtype=torch.uint8, device=dev)
        count = torch.empty((GAMES,), dtype=torch.int32, device=dev)
        _lib.check(eng.lib.aqg_engine_root_visits(ctypes.byref(eng.e), _lib.ptr(visits), _lib.ptr(actions), _lib.ptr(count), eng._stream()), "root_visits")
        index = visits.argmax(dim=1).to(torch.int32).contiguous()
        used = float(eng.t["node_count"].float().mean().item())
        t = timed(lambda: _lib.check(eng.lib.aqg_engine_keep_subtrees(ctypes.byref(eng.e), ctypes.byref(eng.reuse), _lib.ptr(index), eng._stream()), "keep"))
        kept = int(eng.t["kept"].sum().item())
        after = float(eng.t["node_count"][eng.t["kept"] != 0].float().mean().item()) if kept else 0.0
        print(f"keep launch alone: {t:8.3f} ms for {GAMES} slots ({kept} kept; {used:.0f} used records per slot before, {after:.0f} after where kept) "
              f"= {100.0 * t / med[False]:.2f} % of the move without reuse", flush=True)
        del engines
        # a whole generation
        eng = BatchedSelfPlay(net, num_games=GAMES, sims=SIMS, seed=1, tree_reuse=True)
        c = eng.play_generation()
        s = eng.tree_reuse_stats()
        moves = int(eng.t["game_plies"].sum().item())
        later = moves - c['finished']                 # moves that have a predecessor in their game
        print(f"generation: {c['finished']} games, {moves} moves, {s['moves_kept']} of the {later} behind a game's first started from a kept "
              f"subtree ({100.0 * s['moves_kept'] / max(later, 1):.1f} %), mean kept visits {s['mean_kept_visits']:.1f} on top of which "
              f"{SIMS} simulations ran", flush=True)


if __name__ == "__main__":
    main()
