"""Times what starting games from a table costs, and what a paired match buys, on one GPU.

1. The move: GAMES games x SIMS simulations on 9x9 with the default 6/128/3 network (evaluator='gnn'), three engines from the same
   seed taking turns move by move, so drift hits all alike: the keyword absent, a SECOND engine with the keyword absent -- the difference
   of these two is the spread of the measurement itself --, a table of TABLE_ROWS copies of the opening record as start_states -- the
   SAME games as the first two, so only the launches differ -- and a TABLE_ROWS-row random_book, whose games are other games (four
   plies deep, walls on the board).  The engines have GAMES slots and a quota of twice that, so every move ends in a refill launch: with
   the finish-move instantiation the one launch that differs.  WARMUP moves
   (graph capture, caches), then the median, fastest and slowest of MOVES moves, each timed with a pair of events.
2. The checker and random_book at every n of RECORDS: the launch alone (median of REPEATS), and the whole book call (wall clock, one call).
3. How much pairing narrows the error: two random-weight 5x5 networks, MATCH_GAMES games at MATCH_SIMS simulations; pair_report's se
   from a book of MATCH_GAMES / 2 openings at T = 0 beside the plain standard error of the mean points of the T = 1 match from the opening.
Prints one line per figure.  PARTS (default 1,2,3) selects."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, game_logic, openings, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402

GAMES, SIMS = int(os.environ.get("GAMES", "2048")), int(os.environ.get("SIMS", "200"))
MOVES, WARMUP = int(os.environ.get("MOVES", "7")), int(os.environ.get("WARMUP", "3"))
TABLE_ROWS = int(os.environ.get("TABLE_ROWS", "1024"))
RECORDS = [int(x) for x in os.environ.get("RECORDS", "1024,65536").split(",")]
REPEATS = int(os.environ.get("REPEATS", "21"))
MATCH_GAMES, MATCH_SIMS = int(os.environ.get("MATCH_GAMES", "512")), int(os.environ.get("MATCH_SIMS", "50"))
PARTS = {int(x) for x in os.environ.get("PARTS", "1,2,3").split(",")}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def moves(dev):
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    book = openings.random_book(9, 4, TABLE_ROWS, seed=1)
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        same = torch.from_numpy(openings.opening_record(9)).to(dev).unsqueeze(0).repeat(TABLE_ROWS, 1)
        names = ("off", "off (second engine)", f"table of {TABLE_ROWS} opening records (the same games)", f"book of {TABLE_ROWS} rows (other games)")
        engines = [BatchedSelfPlay(net, num_games=GAMES, sims=SIMS, seed=1, quota=2 * GAMES, start_states=table)
                   for table in (None, None, same, book)]
        times = [[] for _ in engines]
        for m in range(WARMUP + MOVES):
            for t, eng in zip(times, engines):
                ms = timed(eng.move)
                if m >= WARMUP:
                    t.append(ms)
        for name, t in zip(names, times):
            print(f"move {GAMES} games x {SIMS} sims, {name}: median {np.median(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f}) over {MOVES} moves",
                  flush=True)
        off = abs(np.median(times[0]) - np.median(times[1]))
        mean = (np.median(times[0]) + np.median(times[1])) / 2
        print(f"off against off: {off:.2f} ms; opening table against the mean of the two: {np.median(times[2]) - mean:+.2f} ms; "
              f"book against it: {np.median(times[3]) - mean:+.2f} ms", flush=True)


def checker_and_book(dev):
    for n in RECORDS:
        book = openings.random_book(9, 6, n, seed=2)
        fn = lambda: game_logic.check_states_batch(book, 9)        # noqa: E731
        fn(), fn()
        print(f"checker, {n} records (9x9): median {np.median([timed(fn) for _ in range(REPEATS)]) * 1000:.1f} us per launch", flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        openings.random_book(9, 6, n, seed=3)
        torch.cuda.synchronize()
        print(f"random_book(9, plies=6, count={n}): {(time.perf_counter() - t0) * 1000:.1f} ms for the whole call", flush=True)


def pairing(dev):
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    N, A = 5, 25 + 2 * 16
    nets = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        nets.append(P.GraphPolicyValueNetwork(6, 128, 3, A, board_size=N).to(dev).eval())
    book = openings.random_book(N, 4, MATCH_GAMES // 2, seed=4)
    paired = BatchedMatch(nets, MATCH_GAMES, sims=MATCH_SIMS, board_size=N, temperature=0.0, evaluator="general", openings=book)
    paired.play()
    r = paired.report()
    plain = np.asarray(BatchedMatch(nets, MATCH_GAMES, sims=MATCH_SIMS, board_size=N, temperature=1.0, evaluator="general", seed=7).play())
    se = plain.std(ddof=1) / np.sqrt(len(plain))
    print(f"paired, {r['pairs']} openings x 2 at T = 0: mean {r['mean']:.4f}, se {r['se']:.4f} (elo {r['elo']:+.1f} +- {r['elo_se']:.1f}, los {r['los']:.3f})", flush=True)
    print(f"plain, {len(plain)} games from the opening at T = 1: mean {plain.mean():.4f}, se {se:.4f}", flush=True)


if __name__ == "__main__":
    device = _lib.require_gpu()
    if 1 in PARTS:
        moves(device)
    if 2 in PARTS:
        checker_and_book(device)
    if 3 in PARTS:
        pairing(device)
