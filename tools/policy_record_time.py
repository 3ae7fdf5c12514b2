"""Times what recording completed-Q policy targets costs a self-play move on one GPU, and the policy append beside the counts append.

The move: GAMES games x SIMS simulations on 9x9 with the default 6/128/3 network (evaluator='gnn'), three engines from the same seed
taking turns move by move, so drift hits all alike: policy_target='visits', a SECOND engine with policy_target='visits' -- the
difference of these two is the spread of the measurement itself -- and policy_target='completed_q'.  WARMUP moves (graph capture,
caches), then the median, fastest and slowest of MOVES moves, each timed with a pair of events.  Then the record launch alone on the
third engine's pools.

The append: at every n of APPEND_ROWS, aqg_replay_append_policy against the counts form and against a composition of torch operations
that writes the same ring (an index_copy_ per ring and a dtype conversion); the three rings of the policy append are checked against
the composition's bit for bit.  Median of REPEATS launches, each timed with a pair of events, after two that are not timed.
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
APPEND_ROWS = [int(x) for x in os.environ.get("APPEND_ROWS", "4000,163840").split(",")]
REPEATS = int(os.environ.get("REPEATS", "21"))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_of(fn, repeats=REPEATS):
    fn(), fn()
    return float(np.median([timed(fn) for _ in range(repeats)]))


def moves(dev):
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        names = ("off", "off (second engine)", "on")
        engines = [BatchedSelfPlay(net, num_games=GAMES, sims=SIMS, seed=1, policy_target="completed_q" if name == "on" else "visits")
                   for name in names]
        print(f"hist_policy: {engines[2].t['hist_policy'].numel() * 4 / 2 ** 20:.1f} MiB beside hist_visits "
              f"{engines[2].t['hist_visits'].numel() * 2 / 2 ** 20:.1f} MiB ({GAMES} games x {engines[2].max_plies} plies x {engines[2].A} actions)",
              flush=True)
        times = [[] for _ in engines]
        for m in range(WARMUP + MOVES):
            for t, eng in zip(times, engines):
                ms = timed(eng.move)
                if m >= WARMUP:
                    t.append(ms)
        med = [float(np.median(t)) for t in times]
        for name, t, md in zip(names, times, med):
            print(f"record {name:20s} move median {md:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  ({GAMES} games x {SIMS} sims, {MOVES} moves "
                  f"after {WARMUP})", flush=True)
        spread, cost = med[1] - med[0], med[2] - med[0]
        print(f"off against off: {1000.0 * spread:+9.1f} us ({100.0 * spread / med[0]:+.3f} %)   on against off: {1000.0 * cost:+9.1f} us "
              f"({100.0 * cost / med[0]:+.3f} %)   the cost lies {'inside' if abs(cost) <= abs(spread) else 'outside'} the off-against-off spread",
              flush=True)
        same = all(torch.equal(engines[0].t[k], engines[2].t[k]) for k in ("hist_visits", "hist_action", "hist_state72", "game_plies"))
        print(f"the games of 'on' are the games of 'off': {same}", flush=True)
        eng = engines[2]
        launch = lambda: _lib.check(eng.lib.aqg_engine_record_improved_policy(ctypes.byref(eng.e), ctypes.byref(eng.policy_record),   # noqa: E731
                                                                              eng._stream()), "aqg_engine_record_improved_policy")
        print(f"record launch alone: {1000.0 * median_of(launch):8.1f} us over {GAMES} roots ({int(eng.t['game_active'].sum().item())} active)", flush=True)


def appends(dev, N=9):
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    A = N * N + 2 * (N - 1) ** 2
    for n in APPEND_ROWS:
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        capacity, head = n + 1000, 700
        S = torch.randint(0, 256, (n, 72), dtype=torch.uint8, device=dev, generator=g)
        V = torch.randint(0, 40, (n, A), dtype=torch.int16, device=dev, generator=g)
        Pi = torch.rand((n, A), dtype=torch.float32, device=dev, generator=g)
        Z = torch.randint(-1, 2, (n,), dtype=torch.int8, device=dev, generator=g)
        rings = lambda: (torch.zeros((capacity, 72), dtype=torch.uint8, device=dev), torch.zeros((capacity, A), dtype=torch.float32, device=dev),   # noqa: E731
                         torch.zeros((capacity,), dtype=torch.float32, device=dev))
        rp, rc, rt = rings(), rings(), rings()
        slots = (head + torch.arange(n, device=dev)) % capacity

        def policy():
            _lib.check(lib.aqg_replay_append_policy(N, A, _lib.ptr(S), _lib.ptr(Pi), _lib.ptr(Z), None, 0.0, n, capacity, head,
                                                    *(_lib.ptr(x) for x in rp), st), "aqg_replay_append_policy")

        def counts():
            _lib.check(lib.aqg_replay_append(N, A, _lib.ptr(S), _lib.ptr(V), _lib.ptr(Z), None, None, n, capacity, head,
                                             *(_lib.ptr(x) for x in rc), st), "aqg_replay_append")

        def composed():
            rt[0].index_copy_(0, slots, S)
            rt[1].index_copy_(0, slots, Pi)
            rt[2].index_copy_(0, slots, Z.to(torch.float32))

        t = [median_of(f) for f in (policy, counts, composed)]
        equal = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(rp, rt))
        moved = n * (72 + 4 * A + 1) + n * (72 + 4 * A + 4)
        print(f"append n = {n:7d} (9x9): policy {1000.0 * t[0]:8.1f} us ({moved / t[0] / 1e6:7.1f} GB/s)   counts {1000.0 * t[1]:8.1f} us   "
              f"torch composition {1000.0 * t[2]:8.1f} us   rings equal: {equal}", flush=True)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    appends(dev)
    moves(dev)


if __name__ == "__main__":
    main()
