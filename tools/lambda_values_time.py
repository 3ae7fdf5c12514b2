"""Times the lambda-return value targets on one GPU.

(a) The launch: one aqg_lambda_values launch against the torch composition of the same result -- a backward loop over the hp columns
with the three f32 operations of a ply and the masks of the skip rules, a handful of elementwise launches per column -- at 9x9's
max_plies with GAMES (2,048) and LARGE (16,384) games and at 5x5's with SMALL (1,024) games.  The games' lengths are uniform in
1 .. max_plies, one game in sixteen is not done, q is uniform in [-1, 1].  The forms take turns, median / fastest / slowest of ROUNDS
(9) after WARMUP_ROUNDS (2), each timed with a pair of events; both write into NaN-filled tensors, which must come out equal bit for
bit.  Bytes count the row read and the row written of every processed game, at its own length.

(b) One move: GAMES games x SIMS simulations on 9x9 with the default 6/128/3 network (evaluator='gnn'), history on, one capturable
stream (graph replay), SP_VALUE_LAMBDA unset -- two engines, "off" and "off again", which take turns move by move: the option adds
nothing to a move, so their difference is the spread of the run.  WARMUP moves, then the median, fastest and slowest of MOVES moves."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.constants import board_params   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402
from tools.replay_window_time import report, timed   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
GAMES, SIMS, MOVES, WARMUP = E("GAMES", "2048"), E("SIMS", "200"), E("MOVES", "7"), E("WARMUP", "2")
ROUNDS, WARMUP_ROUNDS = E("ROUNDS", "9"), E("WARMUP_ROUNDS", "2")
SIZES = [(9, GAMES), (9, E("LARGE", "16384")), (5, E("SMALL", "1024"))]
LAMBDA = float(np.float32(os.environ.get("LAMBDA", "0.95")))


def launches(dev):
    lib = _lib.load()
    for N, quota in SIZES:
        hp = board_params(N)[1]
        gen = torch.Generator(device="cpu").manual_seed(quota + N)
        plies = torch.randint(1, hp + 1, (quota,), generator=gen, dtype=torch.int32).to(dev)
        result = torch.randint(-1, 2, (quota,), generator=gen, dtype=torch.int8).to(dev)
        done = (torch.arange(quota) % 16 != 5).to(torch.uint8).to(dev)
        q = (torch.rand((quota, hp), generator=gen) * 2 - 1).to(dev)
        names = ("lambda kernel", "torch composition")
        outs = {k: torch.full((quota, hp), float("nan"), device=dev) for k in names}
        a = float(np.float32(1.0) - np.float32(LAMBDA))

        def kernel():
            _lib.check(lib.aqg_lambda_values(quota, hp, _lib.ptr(plies), _lib.ptr(result), _lib.ptr(done), _lib.ptr(q), LAMBDA,
                                             _lib.ptr(outs[names[0]]), _lib.stream_ptr(dev)), names[0])

        def composition():
            out = outs[names[1]]
            live = (done != 0) & (plies >= 1) & (plies <= hp)
            last = plies - 1
            r = result.float()
            z_last = torch.where(last % 2 == 0, r, -r)
            after = torch.zeros((quota,), device=dev)
            for t in range(hp - 1, -1, -1):
                after = torch.where(last == t, z_last, after)
                g = a * q[:, t] + LAMBDA * after          # three elementwise launches: each product and the sum rounded
                out[:, t] = torch.where(live & (last >= t), g, out[:, t])
                after = -g

        rows = int(plies[done != 0].sum().item())
        label = f"lambda-return  {N}x{N} hp {hp:3d} games {quota:6d} ({8 * rows / 1e6:6.2f} MB read + written)"
        report(label, timed({names[0]: kernel, names[1]: composition}, ROUNDS, WARMUP_ROUNDS), names[0], 8 * rows)
        torch.cuda.synchronize()
        same = torch.equal(outs[names[0]].view(torch.int32), outs[names[1]].view(torch.int32))
        print(f"lambda-return  {N}x{N} hp {hp:3d} games {quota:6d} kernel and composition leave equal tensors: {same}; floats written: "
              f"{int((~outs[names[0]].isnan()).sum())} of {quota * hp}, {rows} expected", flush=True)


def moves(dev):
    torch.manual_seed(0)
    net = P.GNNNetwork().to(dev).eval()
    stream = torch.cuda.Stream(device=dev)            # a capturable stream: the move replays its hipGraph, as in self-play
    with torch.cuda.stream(stream):
        engines = {k: BatchedSelfPlay(net, num_games=GAMES, sims=SIMS, seed=1, eval_cache_slots=0) for k in ("off", "off again")}
        times = timed({k: eng.move for k, eng in engines.items()}, MOVES, WARMUP)
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k, t in times.items():
            rel = "" if k == "off" else f"  {100.0 * (med[k] / med['off'] - 1.0):+.2f} % against off"
            print(f"move  {k:10s} median {med[k]:8.2f} ms  min {min(t):8.2f}  max {max(t):8.2f}  ({GAMES} games x {SIMS} sims, {MOVES} moves "
                  f"after {WARMUP}){rel}", flush=True)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    launches(dev)
    moves(dev)


if __name__ == "__main__":
    main()
