"""Times the reanalyse stage on one GPU.

The kernel: one aqg_replay_refresh launch -- n searched roots in legal order (i32 visit counts, u8 action ids, their number, the
search value) written into n scattered slots of a ring, value blend 0.25 -- against the torch composition of the same result: the
mask by the count, the sums, (v.double() / tot).float(), zeros + scatter_add_ into an [n, A] f32 array, index_copy_ into the ring,
and the blend by gather, two products, a sum and index_copy_.  Sizes as tools/replay_window_time.py: 9x9 at n = GAMES9 x PLIES9
(default 50 x 80 = 4,000) and at LARGE9 (163,840), 5x5 at n = GAMES5 x PLIES5 (1,000).  Per size: WARMUP rounds, then the median,
fastest and slowest of ROUNDS rounds, each form timed with a pair of events, the forms taking turns round by round, a 512 MB fill
in front of every timed call so that each starts with the caches full of something else.  Both forms are applied the same number
of times and must leave equal rings.  Bytes per second count 4 * 136 + 136 + 4 + 8 + 4 bytes read and 4A + 8 read or written per row.

The stage, 9x9 with the default network: two self-play generations of STAGE_GAMES games at STAGE_SIMS simulations go into a window;
reanalyse() then searches STAGE_ROWS (4,000) rows of the older one again at STAGE_SIMS simulations.  Host wall-clock around a
synchronise, STAGE_ROUNDS rounds, beside the wall-clock of the self-play generations and their row counts."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib   # noqa: E402
from alphaquoridorgnn_amd.replay import ReplayWindow   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
ROUNDS, WARMUP = E("ROUNDS", "9"), E("WARMUP", "2")
SIZES = [(9, E("GAMES9", "50") * E("PLIES9", "80")), (9, E("LARGE9", "163840")), (5, E("GAMES5", "50") * E("PLIES5", "20"))]
STAGE_GAMES, STAGE_SIMS, STAGE_ROWS, STAGE_ROUNDS = E("STAGE_GAMES", "50"), E("STAGE_SIMS", "50"), E("STAGE_ROWS", "4000"), E("STAGE_ROUNDS", "3")
BLEND = 0.25
ML = _lib.MAX_LEGAL
FLUSH = []                                  # one 512 MB device buffer, twice the Infinity Cache


def searched(N, n, capacity, dev):
    """n roots as a 50-simulation search leaves them: a legal list of 4 .. min(A, 136) distinct actions, counts that sum to 50, 0 and
    0xFF behind the count, a search value; and n distinct slots scattered over the ring."""
    A = N * N + 2 * (N - 1) ** 2
    g = torch.Generator(device="cpu").manual_seed(N * 1000003 + n)
    count = torch.randint(4, min(A, ML) + 1, (n,), generator=g, dtype=torch.int32)
    order = torch.rand((n, A), generator=g).argsort(1)[:, :ML]                        # distinct ids per row
    if order.shape[1] < ML:
        order = torch.cat((order, torch.zeros((n, ML - order.shape[1]), dtype=order.dtype)), 1)
    inside = torch.arange(ML)[None, :] < count[:, None]
    actions = torch.where(inside, order, torch.full_like(order, 0xFF)).to(torch.uint8)
    pick = (torch.rand((n, 50), generator=g) * count[:, None]).long()
    visits = torch.zeros((n, ML), dtype=torch.int32)
    visits.scatter_add_(1, pick, torch.ones((n, 50), dtype=torch.int32))
    q = torch.rand((n,), generator=g) * 2 - 1
    slots = torch.randperm(capacity, generator=g)[:n]
    return tuple(x.to(dev).contiguous() for x in (visits, actions, count, q, slots))


def timed(forms, rounds, warmup, wall=False):
    """forms: {name: callable}.  The forms take turns; returns {name: [ms per timed round]}."""
    times = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, f in forms.items():
            FLUSH[0].fill_(r & 1)                       # outside the timing
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
            if r >= warmup:
                times[k].append(ms)
    return times


def report(label, times, base, nbytes=None):
    med = {k: float(np.median(t)) for k, t in times.items()}
    for k, t in times.items():
        rel = "" if k == base else f"  {100.0 * (med[k] / med[base] - 1.0):+.1f} % against {base}"
        rate = "" if nbytes is None else f"  {nbytes / (med[k] * 1e-3) / 1e12:5.2f} TB/s"
        print(f"{label}  {k:22s} median {med[k] * 1e3:11.1f} us  min {min(t) * 1e3:11.1f}  max {max(t) * 1e3:11.1f}{rate}{rel}", flush=True)


def kernel_sizes(dev):
    lib = _lib.load()
    for N, n in SIZES:
        A = N * N + 2 * (N - 1) ** 2
        capacity = n + n // 2
        visits, actions, count, q, slots = searched(N, n, capacity, dev)
        g = torch.Generator(device="cpu").manual_seed(n)
        first = (torch.rand((capacity, A), generator=g).to(dev), (torch.rand((capacity,), generator=g) * 2 - 1).to(dev))
        rings = {k: tuple(x.clone() for x in first) for k in ("torch composition", "refresh kernel")}
        j = torch.arange(ML, device=dev)[None, :]
        keep = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(BLEND, dtype=torch.float32)

        def launch():
            rpi, rz = rings["refresh kernel"]
            _lib.check(lib.aqg_replay_refresh(N, A, _lib.ptr(visits), _lib.ptr(actions), _lib.ptr(count), _lib.ptr(q), BLEND, _lib.ptr(slots),
                                              n, capacity, _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(dev)), "aqg_replay_refresh")

        def composition():
            rpi, rz = rings["torch composition"]
            inside = j < count[:, None]
            vd = torch.where(inside, visits, 0).double()
            tot = vd.sum(1, keepdim=True)
            dense = torch.zeros((n, A), dtype=torch.float32, device=dev)
            dense.scatter_add_(1, torch.where(inside, actions.long(), 0), (vd / tot.clamp_min(1.0)).float())
            rpi.index_copy_(0, slots, dense)
            rz.index_copy_(0, slots, float(keep) * rz.index_select(0, slots) + BLEND * q)

        nbytes = n * (4 * ML + ML + 16 + 4 * A + 8)
        forms = {"torch composition": composition, "refresh kernel": launch}
        report(f"refresh  {N}x{N} n {n:7d} ({nbytes / 1e6:7.1f} MB read + written)", timed(forms, ROUNDS, WARMUP), "torch composition", nbytes)
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*rings.values()))
        moved = not torch.equal(rings["refresh kernel"][0], first[0])
        print(f"refresh  {N}x{N} n {n:7d} the rings of both forms are equal: {same} (and not what they were: {moved})", flush=True)


def stage(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    from alphaquoridorgnn_amd.reanalyse import eligible_rows, reanalyse
    N = 9
    torch.manual_seed(1)
    model = GNNNetwork().to(dev).eval()
    model.packed_weights(dev)
    window = ReplayWindow(N, max_generations=2, capacity_rows=200000, device=dev)
    for k in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng = MultiSetSelfPlay(model, num_games=STAGE_GAMES, quota=STAGE_GAMES, sims=STAGE_SIMS, num_sets=1, board_size=N, seed=11 + k, device=dev)
        eng.play_generation()
        rows = eng.history_tensors()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        window.append_counts(*rows)
        del eng
        print(f"stage    9x9 self-play generation {k}: {STAGE_GAMES} games, {STAGE_SIMS} simulations, {int(rows[0].shape[0])} rows in "
              f"{ms:10.1f} ms host wall-clock ({ms * 1e3 / max(int(rows[0].shape[0]), 1):8.1f} us per row)", flush=True)
    eligible = eligible_rows(window)
    done = []
    update = [0]

    def one_pass():
        done.append(reanalyse(window, model, STAGE_ROWS, sims=STAGE_SIMS, seed=3, update=update[0]))
        update[0] += 1

    times = timed({"reanalyse": one_pass}, STAGE_ROUNDS, 1, wall=True)["reanalyse"]
    print(f"stage    9x9 reanalyse of {done[-1]} of {eligible} rows at {STAGE_SIMS} simulations, engine build included: median "
          f"{float(np.median(times)):10.1f} ms  min {min(times):10.1f}  max {max(times):10.1f} host wall-clock "
          f"({float(np.median(times)) * 1e3 / max(done[-1], 1):8.1f} us per row)", flush=True)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    FLUSH.append(torch.zeros((512 << 20,), dtype=torch.uint8, device=dev))
    kernel_sizes(dev)
    if STAGE_ROUNDS > 0:
        stage(dev)


if __name__ == "__main__":
    main()
