"""Times the self-play target options on one GPU.

(a) One move: GAMES games x SIMS simulations on 9x9 with the default 6/128/3 network (evaluator='gnn'), history on, one capturable
stream (graph replay) -- the options off (two engines, "off" and "off again": their difference is the spread of the run) against on:
"values" records the search value and sets a schedule that never turns within the timed moves (temperature_plies = LATE_PLIES), so it
plays the games of "off"; "schedule" turns at ply 1, so its games differ from move 1 on.  The engines take turns move by move; WARMUP
moves, then the median, fastest and slowest of MOVES moves, each timed with a pair of events.  Every engine plays from the same seed.

(b) The append: one aqg_replay_append_blend launch against the plain aqg_replay_append launch and against the torch composition of the
same arithmetic (the plain composition of tools/replay_window_time.py with keep * z.float() + blend * q for the value) at 9x9 with
n = GAMES9 x PLIES9 (4,000) and LARGE9 (163,840) rows, the write wrapping; the forms take turns, median / fastest / slowest of ROUNDS
(9) after WARMUP_ROUNDS (2).  Bytes per second count the plain append's 2A + 73 read and 4A + 76 written per row, plus 4 for the value."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402
from tools.replay_window_time import generation, report, timed   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
GAMES, SIMS, MOVES, WARMUP, LATE_PLIES = E("GAMES", "2048"), E("SIMS", "200"), E("MOVES", "7"), E("WARMUP", "2"), E("LATE_PLIES", "1000")
ROUNDS, WARMUP_ROUNDS = E("ROUNDS", "9"), E("WARMUP_ROUNDS", "2")
SIZES = [(9, E("GAMES9", "50") * E("PLIES9", "80")), (9, E("LARGE9", "163840"))]
BLEND = float(os.environ.get("BLEND", "0.5"))


def moves(dev):
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        options = {"off": {}, "off again": {}, "values": dict(temperature_plies=LATE_PLIES, record_search_value=True),
                   "schedule": dict(temperature_plies=1, record_search_value=True)}
        engines = {k: BatchedSelfPlay(net, num_games=GAMES, sims=SIMS, seed=1, eval_cache_slots=0, **kw) for k, kw in options.items()}
        times = timed({k: eng.move for k, eng in engines.items()}, MOVES, WARMUP)
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k, t in times.items():
            rel = "" if k == "off" else f"  {100.0 * (med[k] / med['off'] - 1.0):+.2f} % against off"
            print(f"move  {k:10s} median {med[k]:8.2f} ms  min {min(t):8.2f}  max {max(t):8.2f}  ({GAMES} games x {SIMS} sims, {MOVES} moves "
                  f"after {WARMUP}){rel}", flush=True)
        rows = {k: tuple(eng.t[n] for n in ("hist_state72", "hist_visits", "hist_action")) for k, eng in engines.items()}
        print(f"move  'values' recorded the rows of 'off': {all(torch.equal(a, b) for a, b in zip(rows['off'], rows['values']))}; "
              f"'schedule' played other games: {not torch.equal(rows['off'][2], rows['schedule'][2])}; search values recorded: "
              f"{int((engines['values'].t['hist_value'] != 0).sum())}", flush=True)


def appends(dev):
    lib = _lib.load()
    for N, n in SIZES:
        s, v, z = generation(N, n, dev)
        q = (torch.rand((n,), generator=torch.Generator(device="cpu").manual_seed(n)) * 2 - 1).to(dev)
        A = v.shape[1]
        capacity = n + n // 2
        head = capacity - n // 3                          # the write wraps
        names = ("plain append kernel", "blend append kernel", "torch composition, blend")
        rings = {k: (torch.zeros((capacity, 72), dtype=torch.uint8, device=dev), torch.zeros((capacity, A), device=dev),
                     torch.zeros((capacity,), device=dev)) for k in names}
        slots = (head + torch.arange(n, device=dev)) % capacity
        keep = float(np.float32(1.0) - np.float32(BLEND))

        def plain():
            r72, rpi, rz = rings[names[0]]
            _lib.check(lib.aqg_replay_append(N, A, _lib.ptr(s), _lib.ptr(v), _lib.ptr(z), None, None, n, capacity, head, _lib.ptr(r72),
                                             _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(dev)), names[0])

        def blend():
            r72, rpi, rz = rings[names[1]]
            _lib.check(lib.aqg_replay_append_blend(N, A, _lib.ptr(s), _lib.ptr(v), _lib.ptr(z), _lib.ptr(q), BLEND, n, capacity, head,
                                                   _lib.ptr(r72), _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(dev)), names[1])

        def composition():
            r72, rpi, rz = rings[names[2]]
            vd = v.double()
            tot = vd.sum(1, keepdim=True)
            rpi.index_copy_(0, slots, (vd / tot.clamp_min(1.0)).float())
            r72.index_copy_(0, slots, s)
            rz.index_copy_(0, slots, keep * z.float() + BLEND * q)

        nbytes = n * (2 * A + 73 + 4 * A + 76 + 4)
        label = f"append  {N}x{N} n {n:7d} ({nbytes / 1e6:7.1f} MB read + written)"
        report(label, timed({names[0]: plain, names[1]: blend, names[2]: composition}, ROUNDS, WARMUP_ROUNDS), names[0], nbytes)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(rings[names[1]], rings[names[2]]))
        rest = all(torch.equal(a, b) for a, b in zip(rings[names[0]][:2], rings[names[1]][:2]))
        print(f"append  {N}x{N} n {n:7d} blend kernel and composition give equal rings: {same}; records and pi equal the plain append's: {rest}",
              flush=True)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    moves(dev)
    appends(dev)


if __name__ == "__main__":
    main()
