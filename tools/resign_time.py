"""Resignation on one GPU: what the option costs and what it saves (include/aqgnn.h, "resignation").

  cost     GAMES games x SIMS simulations on 9x9 with the default 6/128/3 network (evaluator='gnn'): a move with the option off against
           the same move with it on at a threshold of 1.0, which never triggers -- and against a SECOND engine with the option off,
           whose distance from the first is the spread any difference has to be read against.  WARMUP moves, then the median, fastest
           and slowest of MOVES moves, each timed with a pair of events; the three engines take turns move by move and play from the
           same seed.
  bench    bench.py --gpus 1 --steps K --warmup W of this tree and of the tree at --parent, taking turns, ROUNDS times each: games/s.
  benefit  one self_play() generation of --games games on --slots slots (refill) with the network at PV_NETWORK_PATH/best.pth, on the
           board of AQG_BOARD_SIZE: the option off, then 'auto' at --bound -- a collecting generation (every game played out, nothing
           resigns) and the generation at the threshold it suggests, if it suggests one; --fixed T adds a generation at T.  Plies
           per game, games/s, the threshold, the false-positive rate.

Prints one line per figure."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cost(args):
    from alphaquoridorgnn_amd import pv_network_gnn as P
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        forms = {"off  ": {}, "on   ": dict(resign_threshold=1.0), "off-2": {}}
        engines = {k: BatchedSelfPlay(net, num_games=args.games, sims=args.sims, seed=1, **kw) for k, kw in forms.items()}
        times = {k: [] for k in engines}
        for m in range(args.warmup + args.moves):
            for k, eng in engines.items():
                t = timed(eng.move)
                if m >= args.warmup:
                    times[k].append(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k, t in times.items():
            print(f"resign {k}  move median {med[k]:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                  f"({args.games} games x {args.sims} sims, {args.moves} moves after {args.warmup})", flush=True)
        spread = 100.0 * abs(med["off-2"] / med["off  "] - 1.0)
        diff = 100.0 * (med["on   "] / med["off  "] - 1.0)
        print(f"off against off: {spread:.2f} % apart (the spread)", flush=True)
        print(f"on (threshold 1.0, never resigns) against off: {diff:+.2f} % -- {'inside' if abs(diff) <= spread else 'OUTSIDE'} the spread", flush=True)
        on = engines["on   "]
        same = all(torch.equal(on.t[k], engines["off  "].t[k]) for k in ("hist_visits", "hist_action", "root_state"))
        lo = on.t["resign_min"]
        print(f"the games of on and off are {'the same bytes' if same else 'DIFFERENT'}; resign_min after {args.warmup + args.moves} moves: "
              f"lowest {float(lo.min().item()):+.4f} (random-init values stay near 0: nothing would resign)", flush=True)


def bench(args):
    def run(tree):
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.bench_warmup)],
                             cwd=tree, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit(f"bench.py failed in {tree}:\n{out.stderr[-2000:]}")
        line = [x for x in out.stdout.splitlines() if x.startswith("{")][-1]
        return float(json.loads(line)["value"])
    got = {"parent": [], "new": []}
    for _ in range(args.rounds):
        for name, tree in (("parent", args.parent), ("new", ROOT)):
            got[name].append(run(tree))
            print(f"bench.py --gpus 1 --steps {args.steps} --warmup {args.bench_warmup}  {name:6s} {got[name][-1]:9.2f} games/s", flush=True)
    for name, v in got.items():
        print(f"{name:6s} median {float(np.median(v)):9.2f}  min {min(v):9.2f}  max {max(v):9.2f} games/s", flush=True)


def benefit(args):
    from alphaquoridorgnn_amd import constants, pv_mcts, self_play as sp
    from alphaquoridorgnn_amd.pv_network_gnn import load_network
    dev = torch.device("cuda", torch.cuda.current_device())
    weights = args.weights or constants.PV_NETWORK_PATH + "best.pth"
    model = load_network(weights).to(dev).eval()
    print(f"weights: {weights}", flush=True)
    pv_mcts.PV_EVALUATE_COUNT = args.sims
    sp.SP_SLOTS, sp.SP_RESIGN_MAX_FALSE_POSITIVE, sp.SP_RESIGN_MIN_PLY = args.slots, args.bound, args.min_ply
    print(f"{constants.BOARD_SIZE}x{constants.BOARD_SIZE}, {args.games} games on {args.slots} slots, {args.sims} simulations, seed {args.seed}", flush=True)

    def generation(title, threshold):
        sp.SP_RESIGN_THRESHOLD = threshold
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        path = sp.self_play(model, games=args.games, seed=args.seed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        import pickle
        with open(path, "rb") as f:
            rows = len(pickle.load(f))
        os.remove(path)
        print(f"{title}: {rows / args.games:6.2f} plies per game, {args.games / dt:8.1f} games/s ({dt:.2f} s with the file)", flush=True)
        return rows, dt

    generation("warm-up (off)        ", None)
    off = generation("off                  ", None)
    sp.SP_RESIGN_AUTO = {"threshold": None, "parts": []}
    generation("auto, collecting     ", "auto")
    chosen = sp.SP_RESIGN_AUTO["threshold"]
    if args.fixed is not None:
        on = generation(f"fixed threshold {args.fixed:.3f}", args.fixed)
        s = sp.SP_RESIGN_LAST["stats"]
        print(f"fixed threshold {args.fixed:.4f}: {s['games_resigned']} of {s['games']} games resigned; plies {on[0]} against {off[0]} "
              f"({100.0 * (on[0] / off[0] - 1.0):+.1f} %), time {100.0 * (on[1] / off[1] - 1.0):+.1f} %; played out {s['disabled_games']} games: "
              f"{s['would_resign']} sides would have resigned, {s['false_positives']} of them did not lose (false-positive rate "
              f"{s['false_positive_rate']:.3f})", flush=True)
    if chosen is None:
        print(f"auto: no threshold keeps the false-positive rate at or under {100 * args.bound:.0f} % with enough resigning sides to say so: "
              "the next generation would collect again", flush=True)
        return
    sp.SP_RESIGN_AUTO["threshold"] = chosen
    on = generation(f"auto, threshold {chosen:.3f}", "auto")
    s = sp.SP_RESIGN_LAST["stats"]
    print(f"threshold {chosen:.4f} at a {100 * args.bound:.0f} % bound; {s['games_resigned']} of {s['games']} games resigned; plies {on[0]} against "
          f"{off[0]} ({100.0 * (on[0] / off[0] - 1.0):+.1f} %), time {100.0 * (on[1] / off[1] - 1.0):+.1f} %; played out {s['disabled_games']} games: "
          f"{s['would_resign']} sides would have resigned, {s['false_positives']} of them did not lose (false-positive rate "
          f"{s['false_positive_rate']:.3f})", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="what", required=True)
    c = sub.add_parser("cost")
    c.add_argument("--games", type=int, default=2048)
    c.add_argument("--sims", type=int, default=200)
    c.add_argument("--moves", type=int, default=7)
    c.add_argument("--warmup", type=int, default=3)
    b = sub.add_parser("bench")
    b.add_argument("--parent", required=True, help="a built checkout of the parent commit")
    b.add_argument("--steps", type=int, default=2)
    b.add_argument("--bench-warmup", type=int, default=1)
    b.add_argument("--rounds", type=int, default=3)
    f = sub.add_parser("benefit")
    f.add_argument("--games", type=int, default=1024)
    f.add_argument("--slots", type=int, default=256)
    f.add_argument("--sims", type=int, default=50)
    f.add_argument("--bound", type=float, default=0.05)
    f.add_argument("--min-ply", type=int, default=0)
    f.add_argument("--seed", type=int, default=11)
    f.add_argument("--fixed", type=float, default=None, help="also play a generation at this fixed threshold")
    f.add_argument("--weights", default=None, help="a .pth file (default: PV_NETWORK_PATH/best.pth)")
    args = ap.parse_args(argv)
    {"cost": cost, "bench": bench, "benefit": benefit}[args.what](args)


if __name__ == "__main__":
    main()
