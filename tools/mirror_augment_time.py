"""Times the preparation of one training epoch on one GPU: the three index_select gathers of an epoch without the mirror augmentation
against the one fused launch (aqg_augment_gather) with flips off (a plain gather) and with flips on (seeded draw), over n positions
with a fresh shuffle.  Sizes: 9x9 at n = GAMES9 x PLIES9 (default 50 x 80 = 4,000: the reference's SP_GAME_COUNT of 50 times a typical
9x9 game) and at LARGE9 (default 163,840 = the 2,048 games of the benchmark x 80), 5x5 at n = GAMES5 x PLIES5 (50 x 20 = 1,000).
Per size: WARMUP rounds, then the median, fastest and slowest of ROUNDS rounds, each form timed with a pair of events, the forms taking
turns round by round so drift hits all of them alike.  Then a whole run_epoch of the default networks (GNNTrainer at 9x9,
GeneralTrainer 6/64/2 at 5x5) without and with mirror=(seed, epoch), the same way, on trainers of equal weights."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import train_network as tn   # noqa: E402
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
ROUNDS, WARMUP = E("ROUNDS", "5"), E("WARMUP", "2")
SIZES = [(9, E("GAMES9", "50") * E("PLIES9", "80")), (9, E("LARGE9", "163840")), (5, E("GAMES5", "50") * E("PLIES5", "20"))]
EPOCH_SIZES = [(9, E("GAMES9", "50") * E("PLIES9", "80")), (5, E("GAMES5", "50") * E("PLIES5", "20"))]


def rows(N, n, dev):
    A = N * N + 2 * (N - 1) ** 2
    g = torch.Generator(device="cpu").manual_seed(N * 1000003 + n)
    s = torch.randint(0, 3, (n, 72), generator=g, dtype=torch.uint8)
    s[:, 0], s[:, 2] = torch.randint(0, N * N, (n,), generator=g), torch.randint(0, N * N, (n,), generator=g)
    s[:, 1], s[:, 3], s[:, 68:] = 3, 3, 0
    s[:, 4 + (N - 1) ** 2:68] = 0
    s[:, 70] = N
    p = torch.rand((n, A), generator=g)
    p = p / p.sum(1, keepdim=True)
    z = torch.randint(-1, 2, (n,), generator=g).float()
    return s.to(dev), p.to(dev), z.to(dev)


def timed(forms, rounds, warmup):
    """forms: {name: callable}.  The forms take turns; returns {name: [ms per timed round]}."""
    times = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, f in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    return times


def report(label, times, base):
    med = {k: float(np.median(t)) for k, t in times.items()}
    for k, t in times.items():
        rel = "" if k == base else f"  {100.0 * (med[k] / med[base] - 1.0):+.1f} % against {base}"
        print(f"{label}  {k:28s} median {med[k] * 1e3:9.1f} us  min {min(t) * 1e3:9.1f}  max {max(t) * 1e3:9.1f}{rel}", flush=True)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    for N, n in SIZES:
        s, p, z = rows(N, n, dev)
        A = p.shape[1]
        order = torch.randperm(n, device=dev)
        forms = {
            "three index_select": lambda: [x.index_select(0, order).contiguous() for x in (s, p, z)],
            "fused launch, flips off": lambda: tn._augment_launch(N, s, p, z, order, None),
            "fused launch, flips on": lambda: tn._augment_launch(N, s, p, z, order, (7, 3)),
        }
        mb = 2 * n * (72 + 4 * A + 4) / 1e6
        report(f"prepare {N}x{N} n {n:7d} ({mb:7.1f} MB read + written)", timed(forms, ROUNDS, WARMUP), "three index_select")
    for N, n in EPOCH_SIZES:
        s, p, z = rows(N, n, dev)
        order = torch.randperm(n, device=dev)
        shape = (6, 128, 3) if N == 9 else (6, 64, 2)
        trainers = {}
        for name in ("run_epoch, mirror off", "run_epoch, mirror on"):
            torch.manual_seed(1)
            trainers[name] = tn.trainer_for(GraphPolicyValueNetwork(*shape, p.shape[1], board_size=N).to(dev).eval())
        forms = {
            "run_epoch, mirror off": lambda: trainers["run_epoch, mirror off"].run_epoch(s, p, z, order),
            "run_epoch, mirror on": lambda: trainers["run_epoch, mirror on"].run_epoch(s, p, z, order, mirror=(7, 3)),
        }
        steps = (n + tn.BATCH_SIZE - 1) // tn.BATCH_SIZE
        report(f"epoch   {N}x{N} n {n:7d} ({steps:4d} steps of {tn.BATCH_SIZE}, {type(trainers['run_epoch, mirror on']).__name__})",
               timed(forms, ROUNDS, WARMUP), "run_epoch, mirror off")


if __name__ == "__main__":
    main()
