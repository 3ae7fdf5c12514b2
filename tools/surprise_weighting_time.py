"""Times policy surprise weighting (replay.surprise_index, csrc/replay_surprise.hip) on one GPU, on the rows of real self-play
generations, and writes profiles/surprise_weighting.log (OUT=<path> writes elsewhere).

Input: generations played here by the engine with a random-weight network (SIMS simulations a move, default 200) and appended to a
ReplayWindow until it holds n rows -- 9x9 at n = 4,000 (generations of GAMES_SMALL = 16 games) and n = 163,840 (GAMES_LARGE = 1,024), 5x5
at n = 1,000 (16 games, a 6/16/2 network) -- the sizes of tools/merge_positions_time.py.  The network whose policy the surprise is
taken against is the one that played.

Timed, per size, WARMUP rounds and then the median, fastest and slowest of ROUNDS = 9 rounds, the forms of a group taking turns round
by round, a 512 MB buffer filled in front of every timed call, outside the timing:
  the rows launch alone (a pair of events; the network's policy of all n rows computed outside the timing):
    aqg_replay_surprise_rows;  the torch composition of the same k -- index_select of the targets, xlogy(t, t) - t * log(clamp(p,
    2^-126)) in float64, a float64 row sum, clamp, float32 -- which leaves out the row predicates;
  the counts launch alone: aqg_replay_surprise_counts;  the torch composition of the same counts with torch's own uniforms in place of
    the counter-based draw (so it is not the same draw, and cannot be keyed by ring slot);
  a whole surprise_index (host wall-clock around a synchronise, the network's forward included), beside one run_epoch of the trainer
    over the same n rows at batch 128 with a learning rate of 0 -- the update has NUM_EPOCH = 100 of those.
Bytes per second of the rows launch count 8A + 8 bytes read and 8 written per row."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P, train_network as tn   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402
from alphaquoridorgnn_amd.replay import ReplayWindow, surprise_index   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
ROUNDS, WARMUP, SIMS = E("ROUNDS", "9"), E("WARMUP", "2"), E("SIMS", "200")
SIZES = [(9, E("SMALL9", "4000"), E("GAMES_SMALL", "16")), (9, E("LARGE9", "163840"), E("GAMES_LARGE", "1024")),
         (5, E("SMALL5", "1000"), E("GAMES_SMALL", "16"))]
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "surprise_weighting.log"))
LOG = []
FLUSH = []                                  # one 512 MB device buffer, twice the Infinity Cache


def say(line):
    print(line, flush=True)
    LOG.append(line)


def window_of(N, n, games, dev):
    """(network, window of exactly n rows): whole generations of `games` games, seeds 1, 2, ..., the oldest rows of the first dropped."""
    torch.manual_seed(7)
    if N == 9:
        net, evaluator = P.GNNNetwork().to(dev).eval(), "gnn"
    else:
        net, evaluator = P.GraphPolicyValueNetwork(6, 16, 2, N * N + 2 * (N - 1) ** 2, board_size=N).to(dev).eval(), "general"
    gens, rows, seed = [], 0, 0
    while rows < n:
        seed += 1
        eng = BatchedSelfPlay(net, num_games=games, sims=SIMS, board_size=N, evaluator=evaluator, seed=seed)
        eng.play_generation()
        gens.append(tuple(x.clone() for x in eng.history_tensors()))
        rows += int(gens[-1][0].shape[0])
        del eng
    skip = rows - n
    gens[0] = tuple(x[skip:].contiguous() for x in gens[0])
    w = ReplayWindow(N, max_generations=len(gens), capacity_rows=n + n // 2, device=dev)
    w._start = n // 3                                   # the valid interval wraps the ring, as it does in a long run
    for g in gens:
        w.append_counts(*g)
    assert len(w) == n and len(w.generations) == len(gens)
    return net, w


def timed(forms, wall=False):
    times = {k: [] for k in forms}
    for r in range(WARMUP + ROUNDS):
        for k, f in forms.items():
            FLUSH[0].fill_(r & 1)                       # outside the timing: every form starts with the caches full of something else
            if wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
            if r >= WARMUP:
                times[k].append(ms)
    return times


def report(label, times, base, nbytes=None):
    med = {k: float(np.median(t)) for k, t in times.items()}
    for k, t in times.items():
        rel = "" if k == base else f"  {100.0 * (med[k] / med[base] - 1.0):+.1f} % against {base}"
        rate = "" if nbytes is None else f"  {nbytes / (med[k] * 1e-3) / 1e12:5.2f} TB/s"
        say(f"{label}  {k:32s} median {med[k] * 1e3:11.1f} us  min {min(t) * 1e3:11.1f}  max {max(t) * 1e3:11.1f}{rate}{rel}")


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    FLUSH.append(torch.zeros((512 << 20,), dtype=torch.uint8, device=dev))
    say(f"surprise weighting: rows of real self-play generations (random-weight network, {SIMS} simulations a move), ROUNDS={ROUNDS} WARMUP={WARMUP}")
    for N, n, games in SIZES:
        net, w = window_of(N, n, games, dev)
        s, p, z = w.tensors()
        index, rows = w.index(), int(s.shape[0])
        A = p.shape[1]
        tag = f"{N}x{N} n {n:7d}"
        stats = {}
        expanded, k_ref, count_ref = surprise_index(net, s, p, index, seed=1, update=0, stats=stats)
        say(f"{tag}  generations {w.generations} of {games} games: {stats['rows']} rows -> {stats['expanded']} rows, {stats['left_out']} left "
            f"out, most copies {stats['most_copies']}, mean KL {stats['mean_kl']:.4f}, largest {float(k_ref.max()):.4f}, share of positive "
            f"target entries {float((p.index_select(0, index) > 0).float().mean()):.3f}")
        with torch.no_grad():
            policy = torch.cat([net.forward_states(s.index_select(0, index[o:o + 16384]).contiguous())[0] for o in range(0, n, 16384)])
        k, q = torch.empty((n,), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        kept = {}

        def rows_launch():
            _lib.check(lib.aqg_replay_surprise_rows(N, A, _lib.ptr(policy), _lib.ptr(p), _lib.ptr(index), rows, n, 0, n, _lib.ptr(k),
                                                    _lib.ptr(q), st), "aqg_replay_surprise_rows")

        def rows_torch():
            t = p.index_select(0, index).double()
            kl = (torch.xlogy(t, t) - t * torch.log(policy.double().clamp(min=2.0 ** -126))).sum(dim=1)
            kept["k"] = kl.clamp(min=0.0, max=88.0).float()

        nbytes = n * (8 * A + 8 + 8)
        report(f"{tag}  rows launch ({nbytes / 1e6:7.1f} MB)", timed({"xlogy - t log p, float64 sum": rows_torch, "aqg_replay_surprise_rows": rows_launch}),
               "xlogy - t log p, float64 sum", nbytes)
        torch.cuda.synchronize()
        say(f"{tag}  the launch against surprise_index: k equal {torch.equal(k, k_ref)}; against the composition: largest |k| difference "
            f"{float((kept['k'] - k).abs().max()):.3g}")
        total = q.sum(dtype=torch.int64).reshape(1)

        def counts_launch():
            _lib.check(lib.aqg_replay_surprise_counts(_lib.ptr(q), _lib.ptr(index), _lib.ptr(total), n, n, 0.5, 8, 1, 0, _lib.ptr(count), st),
                       "aqg_replay_surprise_counts")

        def counts_torch():
            f = (n * 0.5) / n + ((n * 0.5) * q.double()) / total.double()
            whole = torch.floor(f)
            kept["count"] = (whole + (torch.rand((n,), dtype=torch.float64, device=dev) < f - whole)).clamp(max=8.0).to(torch.int32)

        report(f"{tag}  counts launch", timed({"torch: f, floor, rand, clamp": counts_torch, "aqg_replay_surprise_counts": counts_launch}),
               "torch: f, floor, rand, clamp")
        torch.cuda.synchronize()
        say(f"{tag}  the launch against surprise_index: counts equal {torch.equal(count, count_ref)}; the composition's own draw gives "
            f"{int(kept['count'].sum())} rows against {int(count.sum())}")
        trainer = tn.trainer_for(net, max_batch=128)

        def whole():
            kept["whole"] = surprise_index(net, s, p, index, seed=1, update=0)

        def epoch():
            trainer.run_epoch(s, p, z, index[torch.randperm(n, device=dev)], lr=0.0)

        report(f"{tag}  whole (host wall-clock)", timed({"one run_epoch, batch 128": epoch, "surprise_index": whole}, wall=True),
               "one run_epoch, batch 128")
        say(f"{tag}  whole: index equal {torch.equal(kept['whole'][0], expanded)}")
        del w, s, p, z, net, trainer
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
