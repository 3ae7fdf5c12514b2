"""Times the position merge (replay.merge_positions, csrc/replay_merge.hip) on one GPU, on the rows of real self-play generations, and
writes profiles/merge_positions.log (OUT=<path> writes elsewhere).

Input: generations played here by the engine with a random-weight network (SIMS simulations a move, default 200) and appended to a
ReplayWindow until it holds n rows -- 9x9 at n = 4,000 (generations of GAMES_SMALL = 16 games) and n = 163,840 (GAMES_LARGE = 1,024), 5x5
at n = 1,000 (16 games, a 6/16/2 network).  Per size the log gives the share of rows that repeat an older row of the window, (n - u) / n,
the longest run and the number of runs of more than 64 rows.

Timed, per size, WARMUP rounds and then the median, fastest and slowest of ROUNDS = 9 rounds, the forms of a group taking turns round
by round.  In front of every timed call, outside the timing, a 512 MB buffer is filled: without it the form that ran behind another
one that had just read the same 260 MB was 9 to 15 % faster for that alone, whichever form it was:
  the merge launch alone (a pair of events; perm, starts and the torch composition's index prepared outside the timing):
    aqg_replay_merge_runs;  the torch composition of the same result -- index_add_ of the gathered policy rows and values into u rows,
    a division by the count, an index_select of the records --;  and as the floor the plain aqg_augment_gather of the same n rows;
  a whole merge (host wall-clock around a synchronise: a merge reads the run starts back):
    replay.merge_positions;  the torch composition from the records on -- torch.unique over the key bytes (dim 0, with inverse and
    counts), the groups put in first-occurrence order, then the same index_add_ and division.
ALT_LIB=<path to another build of the library> times that build's aqg_replay_merge_runs beside the shipped one (an A/B of the kernel:
csrc/build.sh with AQG_REPLACE="replay_merge=..." and OUT).
Bytes per second of the launch count 4A + 76 + 8 bytes read per input row and 4A + 80 written per output row."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402
from alphaquoridorgnn_amd.replay import KEY_BYTES, ReplayWindow, merge_positions   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
ROUNDS, WARMUP, SIMS = E("ROUNDS", "9"), E("WARMUP", "2"), E("SIMS", "200")
SIZES = [(9, E("SMALL9", "4000"), E("GAMES_SMALL", "16")), (9, E("LARGE9", "163840"), E("GAMES_LARGE", "1024")),
         (5, E("SMALL5", "1000"), E("GAMES_SMALL", "16"))]
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "merge_positions.log"))
ALT_LIB = os.environ.get("ALT_LIB")
LOG = []
FLUSH = []                                  # one 512 MB device buffer, twice the Infinity Cache


def say(line):
    print(line, flush=True)
    LOG.append(line)


def window_of(N, n, games, dev):
    """A window of exactly n rows: whole generations of `games` games, seeds 1, 2, ..., the oldest rows of the first one dropped."""
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
    return w


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
        say(f"{label}  {k:30s} median {med[k] * 1e3:11.1f} us  min {min(t) * 1e3:11.1f}  max {max(t) * 1e3:11.1f}{rate}{rel}")


def composition(s, p, z, src, starts_rows, dest, count, u):
    """index_add_ of the gathered rows, then a division: (out72, out_pi, out_z)."""
    A = p.shape[1]
    by = count.to(torch.float32)
    out_pi = torch.zeros((u, A), device=p.device).index_add_(0, dest, p.index_select(0, src)) / by[:, None]
    out_z = torch.zeros((u,), device=p.device).index_add_(0, dest, z.index_select(0, src)) / by
    return s.index_select(0, starts_rows), out_pi, out_z


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    key_bytes = torch.from_numpy(KEY_BYTES).to(dev)
    FLUSH.append(torch.zeros((512 << 20,), dtype=torch.uint8, device=dev))
    alt = None
    if ALT_LIB:
        alt = ctypes.CDLL(ALT_LIB).aqg_replay_merge_runs
        alt.restype, alt.argtypes = _lib.SIGNATURES["aqg_replay_merge_runs"]
        say(f"ALT_LIB = {os.path.basename(ALT_LIB)}")
    say(f"position merge: rows of real self-play generations (random-weight network, {SIMS} simulations a move), ROUNDS={ROUNDS} WARMUP={WARMUP}")
    for N, n, games in SIZES:
        w = window_of(N, n, games, dev)
        s, p, z = w.tensors()
        index = w.index()
        A = p.shape[1]
        out72, out_pi, out_z, count = merge_positions(s, p, z, index=index, board_size=N)
        u = int(out72.shape[0])
        longest, over = int(count.max()), int((count > 64).sum())
        tag = f"{N}x{N} n {n:7d}"
        say(f"{tag}  generations {w.generations} of {games} games: {u} positions, repeated rows {n - u} = {100.0 * (n - u) / n:.2f} % of the "
            f"rows, longest run {longest}, runs of more than 64 rows: {over}")
        # perm and starts as merge_positions builds them, here from the torch composition's own grouping (the result says which rows
        # go together): places of the input sorted by output row, stable
        _, inverse, counts_u = torch.unique(s.index_select(0, index)[:, key_bytes], dim=0, return_inverse=True, return_counts=True)
        first = torch.full((counts_u.shape[0],), n, dtype=torch.int64, device=dev).scatter_reduce_(
            0, inverse, torch.arange(n, device=dev), "amin")
        rank = torch.empty_like(first)
        rank[torch.sort(first).indices] = torch.arange(first.shape[0], device=dev)
        dest_of_place = rank[inverse]                                       # output row of every input place
        order = torch.sort(dest_of_place, stable=True).indices
        src, dest = index[order].contiguous(), dest_of_place[order].contiguous()
        cnt = torch.bincount(dest, minlength=u)
        starts = (torch.cumsum(cnt, 0) - cnt).contiguous()
        assert u == int(first.shape[0]) and torch.equal(cnt.to(torch.int32), count)
        starts_rows = src[starts]
        outs = (torch.empty_like(out72), torch.empty_like(out_pi), torch.empty_like(out_z), torch.empty_like(count))
        floats = int(lib.aqg_replay_merge_workspace_floats(N, n, u))
        work = torch.empty((max(floats, 1),), device=dev)
        g72, gpi, gz = torch.empty((n, 72), dtype=torch.uint8, device=dev), torch.empty((n, A), device=dev), torch.empty((n,), device=dev)
        kept = {}

        def launch(entry=lib.aqg_replay_merge_runs):
            _lib.check(entry(N, A, _lib.ptr(s), _lib.ptr(p), _lib.ptr(z), _lib.ptr(src), _lib.ptr(starts), n, u,
                                                 *(_lib.ptr(x) for x in outs), _lib.ptr(work), floats, st), "aqg_replay_merge_runs")

        def torch_launch():
            kept["composition"] = composition(s, p, z, src, starts_rows, dest, cnt, u)

        def floor():
            _lib.check(lib.aqg_augment_gather(N, A, _lib.ptr(s), _lib.ptr(p), _lib.ptr(z), _lib.ptr(src), None, 0, 0, 0, n, _lib.ptr(g72),
                                              _lib.ptr(gpi), _lib.ptr(gz), st), "aqg_augment_gather")

        nbytes = n * (4 * A + 76 + 8) + u * (4 * A + 80)
        forms = {"index_add_ + division": torch_launch, "aqg_replay_merge_runs": launch}
        if alt is not None:
            forms["aqg_replay_merge_runs, ALT_LIB"] = lambda: launch(alt)
        forms["aqg_augment_gather (floor)"] = floor
        report(f"{tag}  launch ({nbytes / 1e6:7.1f} MB)", timed(forms), "index_add_ + division", nbytes)
        torch.cuda.synchronize()
        c72, cpi, cz = kept["composition"]
        say(f"{tag}  the launch against merge_positions: equal {all(torch.equal(a, b) for a, b in zip(outs, (out72, out_pi, out_z, count)))}; "
            f"against the composition: records equal {torch.equal(c72, out72)}, largest |pi| difference "
            f"{float((cpi - out_pi).abs().max()):.3g}, largest |z| difference {float((cz - out_z).abs().max()):.3g}")

        def whole():
            kept["whole"] = merge_positions(s, p, z, index=index, board_size=N)

        def torch_whole():
            _, inv, c = torch.unique(s.index_select(0, index)[:, key_bytes], dim=0, return_inverse=True, return_counts=True)
            f = torch.full((c.shape[0],), n, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, torch.arange(n, device=dev), "amin")
            by_first = torch.sort(f).indices
            r = torch.empty_like(f)
            r[by_first] = torch.arange(f.shape[0], device=dev)
            kept["torch whole"] = composition(s, p, z, index, index[f[by_first]], r[inv], c[by_first], int(c.shape[0]))

        report(f"{tag}  whole merge (host wall-clock)", timed({"torch.unique + index_add_": torch_whole, "merge_positions": whole}, wall=True),
               "torch.unique + index_add_")
        say(f"{tag}  whole: records equal {torch.equal(kept['torch whole'][0], kept['whole'][0])}, largest |pi| difference "
            f"{float((kept['torch whole'][1] - kept['whole'][1]).abs().max()):.3g}")
        del w, s, p, z
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
