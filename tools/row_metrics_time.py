"""Times held-out validation (validation.row_metrics, csrc/row_metrics.hip) on one GPU, on the rows of real self-play generations, and
writes profiles/row_metrics.log (OUT=<path> writes elsewhere).

Input: generations played here by the engine with a random-weight network (SIMS simulations a move, default 200) and appended to a
ReplayWindow until it holds n rows -- 9x9 at n = 4,000 (generations of GAMES_SMALL = 16 games) and n = 163,840 (GAMES_LARGE = 1,024), 5x5
at n = 1,000 (16 games, a 6/16/2 network) -- the sizes of tools/surprise_weighting_time.py.  The network measured is the one that played.

Timed, per size, WARMUP rounds and then the median, fastest and slowest of ROUNDS = 9 rounds, the forms of a group taking turns round
by round, a 512 MB buffer filled in front of every timed call, outside the timing:
  the metrics alone (a pair of events; the network's outputs for all n rows computed outside the timing):
    form one, aqg_replay_row_metrics + aqg_row_metrics_reduce;  form two, the torch composition of the same numbers -- index_select of
    the targets, xlogy(t, t), t * log(clamp(p, 2^-126)), logsumexp, the float64 row sums, the first maximum, the bucket from the two
    ply bytes, and index_add_ by bucket -- which leaves out the row predicates.  Both must leave equal tables within the tests' bar
    (tests/_row_metrics.py: the rows' bars added up per bucket, plus the reduction's depth);
  a whole row_metrics (host wall-clock around a synchronise, the network's forward included), beside one run_epoch of the trainer over
    NINE times as many rows at batch 128 with a learning rate of 0 -- a held-out share of 0.1 -- so that the cost of --holdout-every 1
    is stated as a share of an update.
Bytes per second of form one count 8A + 8 + 4 + 2 bytes read a row by the rows launch, 36 written, and 36 read again by the reduction."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P, train_network as tn   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402
from alphaquoridorgnn_amd.replay import ReplayWindow   # noqa: E402
from alphaquoridorgnn_amd.validation import Metrics, row_metrics   # noqa: E402
from tests._row_metrics import ULP_DEVICE, U, bars, reduce_depth   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
ROUNDS, WARMUP, SIMS = E("ROUNDS", "9"), E("WARMUP", "2"), E("SIMS", "200")
SIZES = [(9, E("SMALL9", "4000"), E("GAMES_SMALL", "16")), (9, E("LARGE9", "163840"), E("GAMES_LARGE", "1024")),
         (5, E("SMALL5", "1000"), E("GAMES_SMALL", "16"))]
BUCKET_PLIES, BUCKETS = 8, 16
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "row_metrics.log"))
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
        rate = "" if nbytes is None or k == base else f"  {nbytes / (med[k] * 1e-3) / 1e12:5.2f} TB/s"
        say(f"{label}  {k:34s} median {med[k] * 1e3:11.1f} us  min {min(t) * 1e3:11.1f}  max {max(t) * 1e3:11.1f}{rate}{rel}")
    return med


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    FLUSH.append(torch.zeros((512 << 20,), dtype=torch.uint8, device=dev))
    say(f"row metrics: rows of real self-play generations (random-weight network, {SIMS} simulations a move), ROUNDS={ROUNDS} WARMUP={WARMUP}, "
        f"{BUCKETS} buckets of {BUCKET_PLIES} plies")
    for N, n, games in SIZES:
        net, w = window_of(N, n, games, dev)
        s, p, z = w.tensors()
        index, rows = w.index(), int(s.shape[0])
        A = p.shape[1]
        tag = f"{N}x{N} n {n:7d}"
        whole_ref = row_metrics(net, s, p, z, index, bucket_plies=BUCKET_PLIES, buckets=BUCKETS)
        say(f"{tag}  generations of {games} games, {len(w.generations)} of them: " + " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}"
                                                                                             for k, v in whole_ref.totals().items()))
        with torch.no_grad():
            outs = [net.forward_states(s.index_select(0, index[o:o + 16384]).contiguous()) for o in range(0, n, 16384)]
            policy = torch.cat([o[0] for o in outs]).contiguous()
            value = torch.cat([o[1][:, 0] for o in outs]).contiguous()
        vals = torch.empty((n, 4), dtype=torch.float64, device=dev)
        word = torch.empty((n,), dtype=torch.int32, device=dev)
        tables = torch.empty((2, BUCKETS + 1, 4), dtype=torch.int64, device=dev)
        partial = torch.empty((int(lib.aqg_row_metrics_workspace_doubles(n, BUCKETS)),), dtype=torch.float64, device=dev)
        kept = {}

        def launches():
            _lib.check(lib.aqg_replay_row_metrics(N, A, _lib.ptr(policy), _lib.ptr(value), _lib.ptr(s), _lib.ptr(p), _lib.ptr(z), _lib.ptr(index),
                                                  rows, n, 0, n, BUCKET_PLIES, BUCKETS, _lib.ptr(vals), _lib.ptr(word), st), "aqg_replay_row_metrics")
            _lib.check(lib.aqg_row_metrics_reduce(_lib.ptr(vals), _lib.ptr(word), n, BUCKETS, _lib.ptr(partial), _lib.ptr(tables[0]),
                                                  _lib.ptr(tables[1]), st), "aqg_row_metrics_reduce")

        def composition():
            t = p.index_select(0, index).double()
            pd = policy.double()
            zz, vv = z.index_select(0, index).double(), value.double()
            rec = s.index_select(0, index)
            ce = -(t * torch.log(pd.clamp(min=2.0 ** -126))).sum(dim=1)
            ent = -torch.xlogy(t, t).sum(dim=1)
            lp = t.sum(dim=1) * torch.logsumexp(pd, dim=1) - (t * pd).sum(dim=1)
            se = (vv - zz) ** 2
            hit = t.gather(1, pd.argmax(dim=1, keepdim=True))[:, 0] == t.max(dim=1).values
            counted = zz != 0
            agrees = counted & (vv * zz > 0)
            bucket = ((rec[:, 68].long() | rec[:, 69].long() << 8) // BUCKET_PLIES).clamp(max=BUCKETS - 1)
            sums = torch.zeros((BUCKETS + 1, 4), dtype=torch.float64, device=dev)
            sums.index_add_(0, bucket, torch.stack((ce, ent, lp, se), dim=1))
            counts = torch.zeros((BUCKETS + 1, 4), dtype=torch.int64, device=dev)
            counts.index_add_(0, bucket, torch.stack((torch.ones_like(bucket), hit.long(), counted.long(), agrees.long()), dim=1))
            kept["sums"], kept["counts"] = sums, counts

        nbytes = n * (8 * A + 8 + 4 + 2 + 36 + 36)
        report(f"{tag}  metrics ({nbytes / 1e6:7.1f} MB)", timed({"torch composition, index_add_": composition, "rows launch + reduce": launches}),
               "torch composition, index_add_", nbytes)
        torch.cuda.synchronize()
        host = tables.cpu().numpy()
        got = Metrics(host[0].view(np.float64), host[1], BUCKET_PLIES, BUCKETS)
        other = kept["sums"].cpu().numpy()
        t_host, p_host = p.index_select(0, index).cpu().numpy(), policy.cpu().numpy()
        bucket_host = word.cpu().numpy() & 255
        inside = True
        for col, bar in enumerate(bars(t_host, p_host, ULP_DEVICE, ULP_DEVICE)):
            per_bucket, mass = np.zeros(BUCKETS + 1), np.zeros(BUCKETS + 1)
            np.add.at(per_bucket, bucket_host, bar)
            np.add.at(mass, bucket_host, np.abs(vals[:, col].cpu().numpy()))
            inside = inside and bool(np.all(np.abs(got.sums[:, col] - other[:, col]) <= per_bucket + reduce_depth(n) * U * mass))
        mass = np.zeros(BUCKETS + 1)
        np.add.at(mass, bucket_host, vals[:, 3].cpu().numpy())
        inside = inside and bool(np.all(np.abs(got.sums[:, 3] - other[:, 3]) <= reduce_depth(n) * U * mass))
        say(f"{tag}  the launches against row_metrics: tables equal {got.sums.tobytes() == whole_ref.sums.tobytes() and np.array_equal(got.counts, whole_ref.counts)}; "
            f"against the composition: counts equal {np.array_equal(got.counts, kept['counts'].cpu().numpy())}, sums within the bar {inside}, "
            f"largest difference {float(np.abs(got.sums - other).max()):.3g}")
        trainer = tn.trainer_for(net, max_batch=128)
        nine = index.repeat(9)

        def whole():
            kept["whole"] = row_metrics(net, s, p, z, index, bucket_plies=BUCKET_PLIES, buckets=BUCKETS)

        def epoch():
            trainer.run_epoch(s, p, z, nine[torch.randperm(9 * n, device=dev)], lr=0.0)

        med = report(f"{tag}  whole (host wall-clock)", timed({f"one run_epoch over {9 * n} rows, batch 128": epoch, "row_metrics": whole}, wall=True),
                     f"one run_epoch over {9 * n} rows, batch 128")
        say(f"{tag}  whole: tables equal {kept['whole'].sums.tobytes() == whole_ref.sums.tobytes()}; --holdout-every 1 at a held-out share of 0.1 "
            f"adds {100.0 * med['row_metrics'] / med[f'one run_epoch over {9 * n} rows, batch 128']:.1f} % to an update")
        del w, s, p, z, net, trainer
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
