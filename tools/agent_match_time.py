"""Times the batched baseline agents and whole network-vs-agent matches on one GPU, on 9x9 and 5x5 boards:
  (a) mcts_action_batch (100 evaluations) at 64 / 256 / 1,024 positions, positions/s, against the host loop agents.mcts_action on
      HOST_POSITIONS of the same positions (one core; extrapolated per position);
  (b) playout_batch at 1,024 / 8,192 positions, playouts/s;
  (c) whole matches of GAMES games per opponent with a random-init 6/128/3 network at SIMS simulations: games/s and the share of
      wall time spent on the agent's plies.
GPU times are medians of REPS runs after WARMUP runs, bracketed by a device synchronisation; every run draws from a new seed.
Prints one line per measurement."""
import os
import random
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
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork   # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "5")), int(os.environ.get("WARMUP", "1"))
HOST_POSITIONS = int(os.environ.get("HOST_POSITIONS", "4"))
GAMES, SIMS = int(os.environ.get("GAMES", "256")), int(os.environ.get("SIMS", "50"))
EVALUATIONS = 100


def positions(N, count):
    """Positions of random games from the initial position (agents.draw_uniforms, so the set is the same on every run)."""
    out, game = [], 0
    draw = board_params(N)[1]
    while len(out) < count:
        s, u = State(board_size=N, num_walls=board_params(N)[0]), agents.draw_uniforms(1, game, draw)
        for i in range(draw):
            if s.is_done():
                break
            out.append(s.record())
            la = agents._legal(s)
            s = s.next(la[min(len(la) - 1, int(u[i] * len(la)))])
        game += 1
    return np.stack(out[:count])


def timed(fn):
    for i in range(WARMUP):
        fn(i)
    ts = []
    for i in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(WARMUP + i)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def section_a(N, dev):
    pool = positions(N, 1024)
    random.seed(0)
    t0 = time.perf_counter()
    for r in pool[:HOST_POSITIONS]:
        agents.mcts_action(State.from_record(r), EVALUATIONS)
    host = (time.perf_counter() - t0) / HOST_POSITIONS
    print(f"(a) {N}x{N} host agents.mcts_action, {EVALUATIONS} evaluations: {host:8.3f} s per position "
          f"({1 / host:8.2f} positions/s, one core, {HOST_POSITIONS} positions)")
    for B in (64, 256, 1024):
        d = torch.from_numpy(pool[:B]).to(dev)
        med, lo, hi = timed(lambda i: agents.mcts_action_device(d, N, EVALUATIONS, seed=i))
        print(f"(a) {N}x{N} mcts_action_batch  B={B:5d}: {1e3 * med:9.2f} ms (min {1e3 * lo:.2f}, max {1e3 * hi:.2f})  "
              f"{B / med:10.1f} positions/s  = {B / med * host:8.1f} x the host loop per position")


def section_b(N, dev):
    for B in (1024, 8192):
        pool = positions(N, 1024)
        d = torch.from_numpy(pool[np.arange(B) % 1024]).to(dev)

        def run(i):
            agents.playout_batch(d, seed=i)
        med, lo, hi = timed(run)
        print(f"(b) {N}x{N} playout_batch      B={B:5d}: {1e3 * med:9.2f} ms (min {1e3 * lo:.2f}, max {1e3 * hi:.2f})  "
              f"{B / med:10.0f} playouts/s")


def section_c(N, dev):
    A = N * N + 2 * (N - 1) ** 2
    torch.manual_seed(0)
    net = GraphPolicyValueNetwork(6, 128, 3, A).to(dev).eval()
    for agent in ("random", "alpha_beta", "mcts"):
        match = BatchedAgentMatch(net, agent, GAMES, sims=SIMS, board_size=N, evaluator="general", seed=3)
        spent = [0.0]
        plain = match._agent_actions

        def timed_agent(eng, first, ply, table):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = plain(eng, first, ply, table)
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t0
            return out
        match._agent_actions = timed_agent
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        points = match.play()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        print(f"(c) {N}x{N} {GAMES} games vs {agent:10s} ({SIMS} simulations): {wall:8.2f} s  {GAMES / wall:8.2f} games/s  "
              f"agent plies {100 * spent[0] / wall:5.1f} % of wall time  network's average point {sum(points) / len(points):.3f}")
        del match


def main():
    dev = _lib.require_gpu()
    which = os.environ.get("SECTIONS", "abc")
    for N in (9, 5):
        if "a" in which:
            section_a(N, dev)
        if "b" in which:
            section_b(N, dev)
        if "c" in which:
            section_c(N, dev)


if __name__ == "__main__":
    main()
