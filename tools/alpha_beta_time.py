"""Times the alpha-beta agent (max_depth 2) served by the kernel against the native host search on a pool of THREADS threads, on
9x9 and 5x5 boards:
  (a) one call on 5 / 64 / 256 / 1,024 positions -- agents.alpha_beta_action_batch(backend='hip') against backend='host' on the
      same records (the actions are compared as well).  The positions come from seeded random walks of 0-12 plies from the opening
      (agents.draw_uniforms), so both sides still hold walls;
  (b) one whole BatchedAgentMatch of GAMES games per backend (hash evaluator, SIMS simulations), wall time.
Every time is the median of REPS runs after WARMUP runs, with the fastest and the slowest run beside it; device calls are bracketed
by a device synchronisation and include the copy of the records in and of the actions out.  Prints one line per measurement."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, agents   # noqa: E402
from alphaquoridorgnn_amd.constants import board_params   # noqa: E402
from alphaquoridorgnn_amd.evaluate_agents import BatchedAgentMatch   # noqa: E402
from alphaquoridorgnn_amd.game_logic import State   # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "5")), int(os.environ.get("WARMUP", "1"))
THREADS = int(os.environ.get("THREADS", "16"))
GAMES, SIMS = int(os.environ.get("GAMES", "256")), int(os.environ.get("SIMS", "16"))
BATCHES = (5, 64, 256, 1024)
DEPTH = 2


def positions(N, count):
    """Walk w plays w % 13 plies from the opening with the draws agents.draw_uniforms(2, w, .) and contributes where it stands
    (earlier if the game would end or the last wall in hand would be placed: 5x5 has two walls a side)."""
    walls = board_params(N)[0]
    out = []
    for w in range(count):
        s, u = State(board_size=N, num_walls=walls), agents.draw_uniforms(2, w, 12)
        for i in range(w % 13):
            la = agents._legal(s)
            t = s.next(la[min(len(la) - 1, int(u[i] * len(la)))])
            if t.is_done() or (t.player[1] == 0 and t.enemy[1] == 0):      # the walk ends before the last wall leaves the hands
                break
            s = t
        out.append(s.record())
    out = np.stack(out)
    assert ((out[:, 1] > 0) | (out[:, 3] > 0)).all()
    return out


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    _lib.load()
    dev = _lib.require_gpu()
    print(f"device {torch.cuda.get_device_name(dev)}  host threads {THREADS}  reps {REPS}  warm-up {WARMUP}  max_depth {DEPTH}", flush=True)
    for N in (9, 5):
        pool = positions(N, max(BATCHES))
        legal = [len(agents._legal(r)) for r in pool[:64]]
        print(f"{N}x{N}: legal actions of the first 64 positions: mean {np.mean(legal):.0f}, min {min(legal)}, max {max(legal)}", flush=True)
        for B in BATCHES:
            recs = pool[:B]
            got = {}

            def hip():
                got["hip"] = agents.alpha_beta_action_batch(recs, max_depth=DEPTH, backend="hip")

            def host():
                got["host"] = agents.alpha_beta_action_batch(recs, max_depth=DEPTH, threads=THREADS, backend="host")
            d, dlo, dhi = timed(hip)
            h, hlo, hhi = timed(host)
            same = bool(np.array_equal(got["hip"], got["host"]))
            print(f"{N}x{N} B={B:5d}  hip {d * 1e3:9.2f} ms [{dlo * 1e3:.2f} .. {dhi * 1e3:.2f}]   host {h * 1e3:9.2f} ms "
                  f"[{hlo * 1e3:.2f} .. {hhi * 1e3:.2f}]   host / hip {h / d:7.1f}   same actions {same}", flush=True)
        points = {}
        for backend in ("hip", "host"):
            m = BatchedAgentMatch(7, "alpha_beta", GAMES, sims=SIMS, board_size=N, evaluator="fake",
                                  agent_kwargs={"backend": backend, "threads": THREADS, "max_depth": DEPTH})
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            points[backend] = m.play()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            print(f"{N}x{N} match of {GAMES} games, {SIMS} simulations, backend {backend}: {t:8.2f} s, network's points "
                  f"{sum(points[backend]) / GAMES:.3f}", flush=True)
            del m
        print(f"{N}x{N} match: same points per game {points['hip'] == points['host']}", flush=True)


if __name__ == "__main__":
    main()
