"""Times the replay window's append on one GPU.

The kernel: one aqg_replay_append launch of a generation in the counts form (u16 visit counts, i8 z -> f32 targets in the ring)
against the torch composition of the same arithmetic -- (v.double() / tot).float(), the casts, and three index_copy_ into the rings --
over n rows written at a head that makes the write wrap.  Sizes as tools/mirror_augment_time.py: 9x9 at n = GAMES9 x PLIES9 (default
50 x 80 = 4,000) and at LARGE9 (163,840), 5x5 at n = GAMES5 x PLIES5 (1,000).  ALT_LIB=<path to another build of the library> times
that build's aqg_replay_append beside the shipped one (an A/B of the kernel: csrc/build.sh with AQG_REPLACE="replay=..." and OUT).
Per size: WARMUP rounds, then the median, fastest and slowest of ROUNDS rounds, each form timed with a pair of events, the forms taking
turns round by round.  Bytes per second count 2A + 73 bytes read and 4A + 76 written per row.

The hand-over, 9x9 at n = 4,000: a generation from the engine's device tensors to training rows on the same GPU, by the file
(self_play._history_rows, pickle to a file, load, the conversion of train_network._training_rows) and by ReplayWindow.append_counts;
host wall-clock around a synchronise, the same rounds."""
import ctypes
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib   # noqa: E402
from alphaquoridorgnn_amd.pv_network_gnn import pack_states   # noqa: E402
from alphaquoridorgnn_amd.replay import ReplayWindow   # noqa: E402
from alphaquoridorgnn_amd.self_play import _history_rows   # noqa: E402

E = lambda k, d: int(os.environ.get(k, d))   # noqa: E731
ROUNDS, WARMUP = E("ROUNDS", "9"), E("WARMUP", "2")
SIZES = [(9, E("GAMES9", "50") * E("PLIES9", "80")), (9, E("LARGE9", "163840")), (5, E("GAMES5", "50") * E("PLIES5", "20"))]
HANDOVER = (9, E("GAMES9", "50") * E("PLIES9", "80"))
ALT_LIB = os.environ.get("ALT_LIB")


def generation(N, n, dev):
    """n rows as a 200-simulation search leaves them: records, counts that sum to 200 over a dozen actions, outcomes."""
    A = N * N + 2 * (N - 1) ** 2
    g = torch.Generator(device="cpu").manual_seed(N * 1000003 + n)
    s = torch.randint(0, 3, (n, 72), generator=g, dtype=torch.uint8)
    s[:, 0], s[:, 2] = torch.randint(0, N * N, (n,), generator=g), torch.randint(0, N * N, (n,), generator=g)
    s[:, 1], s[:, 3], s[:, 68:] = 3, 3, 0
    s[:, 4 + (N - 1) ** 2:68] = 0
    s[:, 70] = N
    v = torch.zeros((n, A), dtype=torch.int16)
    v.scatter_add_(1, torch.randint(0, min(A, 12), (n, 200), generator=g), torch.ones((n, 200), dtype=torch.int16))
    z = torch.randint(-1, 2, (n,), generator=g).to(torch.int8)
    return s.to(dev), v.to(dev), z.to(dev)


def timed(forms, rounds, warmup, wall=False):
    """forms: {name: callable}.  The forms take turns; returns {name: [ms per timed round]}."""
    times = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, f in forms.items():
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
        print(f"{label}  {k:28s} median {med[k] * 1e3:11.1f} us  min {min(t) * 1e3:11.1f}  max {max(t) * 1e3:11.1f}{rate}{rel}", flush=True)


def entry(lib):
    fn = lib.aqg_replay_append
    fn.restype, fn.argtypes = _lib.SIGNATURES["aqg_replay_append"]
    return fn


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    entries = {"append kernel": entry(_lib.load())}
    if ALT_LIB:
        entries["append kernel, ALT_LIB"] = entry(ctypes.CDLL(ALT_LIB))
        print(f"ALT_LIB = {os.path.basename(ALT_LIB)}")
    for N, n in SIZES:
        s, v, z = generation(N, n, dev)
        A = v.shape[1]
        capacity = n + n // 2
        head = capacity - n // 3                          # the write wraps
        rings = {k: (torch.zeros((capacity, 72), dtype=torch.uint8, device=dev), torch.zeros((capacity, A), device=dev),
                     torch.zeros((capacity,), device=dev)) for k in list(entries) + ["torch composition"]}
        slots = (head + torch.arange(n, device=dev)) % capacity

        def launch(k):
            r72, rpi, rz = rings[k]
            _lib.check(entries[k](N, A, _lib.ptr(s), _lib.ptr(v), _lib.ptr(z), None, None, n, capacity, head, _lib.ptr(r72),
                                  _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(dev)), k)

        def composition():
            r72, rpi, rz = rings["torch composition"]
            vd = v.double()
            tot = vd.sum(1, keepdim=True)
            rpi.index_copy_(0, slots, (vd / tot.clamp_min(1.0)).float())
            r72.index_copy_(0, slots, s)
            rz.index_copy_(0, slots, z.float())

        forms = {"torch composition": composition}
        forms.update({k: (lambda k=k: launch(k)) for k in entries})
        nbytes = n * (2 * A + 73 + 4 * A + 76)
        report(f"append  {N}x{N} n {n:7d} ({nbytes / 1e6:7.1f} MB read + written)", timed(forms, ROUNDS, WARMUP), "torch composition", nbytes)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for k in entries for a, b in zip(rings[k], rings["torch composition"]))
        print(f"append  {N}x{N} n {n:7d} the rings of all forms are equal: {same}", flush=True)

    N, n = HANDOVER
    s, v, z = generation(N, n, dev)
    window = ReplayWindow(N, max_generations=1, capacity_rows=n, device=dev)
    tmp = tempfile.mkdtemp()
    kept = {}

    def by_file():
        path = os.path.join(tmp, "generation.history")
        with open(path, "wb") as f:
            pickle.dump(_history_rows(s, v, z, N), f)
        with open(path, "rb") as f:
            history = pickle.load(f)
        hs, hp, hv = zip(*history)
        kept["file"] = (torch.from_numpy(pack_states(hs, N)).to(dev), torch.tensor(np.array(hp), dtype=torch.float32, device=dev),
                        torch.tensor(np.array(hv), dtype=torch.float32, device=dev))

    forms = {"_history_rows + file + load": by_file, "append_counts": lambda: window.append_counts(s, v, z)}
    report(f"handover {N}x{N} n {n:7d} (host wall-clock)", timed(forms, ROUNDS, WARMUP, wall=True), "_history_rows + file + load")
    same = all(torch.equal(a, b) for a, b in zip(window.rows()[1:], kept["file"][1:]))
    print(f"handover {N}x{N} n {n:7d} pi and z of both routes are equal: {same}", flush=True)
    os.remove(os.path.join(tmp, "generation.history"))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
