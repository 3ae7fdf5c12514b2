"""Baseline Quoridor agents -- drop-in for the reference's agents.py (random, alpha-beta, rollout MCTS).

They are CPU opponents for strength tracking (evaluate_agents.py:62-89), CPU code in the reference too.  Each is a function
of the game state that returns an action (agents.py:1-4).  The rules they walk -- legal_actions(), next(), the jump-aware
shortest path -- come from the host build of the SAME rule header the GPU kernels compile (csrc/host_agents.cpp over
csrc/quoridor_core.hpp, inside libaqgnn_hip.so), so no GPU launch per call and no second copy of the rules.
The random streams are consumed exactly like the reference's: `random.randint` once per random move (agents.py:17).

The *_batch functions serve many states per call -- what a match of a network against a baseline agent asks for every ply
(evaluate_agents.BatchedAgentMatch): random moves, random playouts and the rollout MCTS on HIP kernels (csrc/agents.hip, one
wavefront per state; GPU required), alpha-beta on the native host search from a thread pool or, with backend='hip', on the
kernel of the same file (one wavefront per state and root action).  The kernels cannot replay Python's
`random` stream; their draws come from a caller-supplied table of uniforms or from the counter-based generator `draw_uniforms`
mirrors (include/aqgnn.h).  The single-state functions above them are untouched.
"""
import ctypes
import functools
import math
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .constants import NUM_PLIES_FOR_DRAW, NUM_WALLS, board_params
from .counter_rng import MASK64, counter_uniform, stream_key

MAX_DIST_FROM_GOAL = NUM_PLIES_FOR_DRAW // 2 - NUM_WALLS   # agents.py:11


def _rec(state):
    return np.ascontiguousarray(state.record() if hasattr(state, "record") else state, dtype=np.uint8)


def _legal(state):
    """State.legal_actions() on the host (ordered like the reference: pawn moves, then per slot H, V)."""
    rec = _rec(state)
    out = (ctypes.c_uint8 * _lib.MAX_LEGAL)()
    n = _lib.load().aqg_host_legal_actions(int(rec[70]), rec.ctypes.data_as(ctypes.c_void_p), out)
    if n < 0:
        raise _lib.HipLibraryError("aqg_host_legal_actions failed")
    return [int(out[i]) for i in range(n)]


def _board(state):
    return int(state.N) if hasattr(state, "N") else int(_rec(state)[70])


def _max_dist(state):
    walls, draw = board_params(_board(state))
    return draw // 2 - walls


def _draw(state):
    return board_params(_board(state))[1]


# ------------------------------------------------------------------ random (agents.py:14-18)
def random_action(state):
    """Selects a uniformly random legal action."""
    legal_actions = _legal(state)
    return legal_actions[random.randint(0, len(legal_actions) - 1)]


# ------------------------------------------------------------------ alpha-beta (agents.py:22-108)
def shortest_path(state):
    """Plies the mover needs to reach its goal row with the other pawn frozen (jumps allowed); -1 if walled in (agents.py:27-41)."""
    rec = _rec(state)
    return int(_lib.load().aqg_host_shortest_path(int(rec[70]), rec.ctypes.data_as(ctypes.c_void_p)))


def heuristic_eval(state):
    """(enemy's shortest path - mover's shortest path) / MAX_DIST_FROM_GOAL (agents.py:22-54)."""
    rec = _rec(state)
    return float(_lib.load().aqg_host_heuristic_eval(int(rec[70]), rec.ctypes.data_as(ctypes.c_void_p), _max_dist(state)))


def alpha_beta_action(state, max_depth=2):
    """The action with the maximum depth-limited negamax value, first best wins (agents.py:90-108).  The whole search runs
    natively: the reference's pure-Python version needs ~131^3 evaluations per move on an open 9x9 board."""
    rec = _rec(state)
    a = int(_lib.load().aqg_host_alpha_beta_action(int(rec[70]), rec.ctypes.data_as(ctypes.c_void_p), _draw(state), _max_dist(state), int(max_depth)))
    return None if a < 0 else a


# ------------------------------------------------------------------ rollout MCTS (agents.py:112-214)
def playout(state):
    """Random playout to the end of the game: -1 loss, 0 draw, from the point of view of `state`'s mover (agents.py:112-122)."""
    sign = 1
    while True:                                   # (the reference recurses; a loop keeps 116-ply games off the Python stack)
        if state.is_lose():
            return -sign
        if state.is_draw():
            return 0
        state = state.next(random_action(state))
        sign = -sign


def argmax(collection):
    return collection.index(max(collection))


class _Tree:
    """The reference's recursive Node.evaluate (agents.py:133-197) as an arena walked iteratively: nodes are rows of parallel
    lists (state, w, n, first child, child count), children of a node are consecutive rows, one simulation = one descent that
    records its path + one backup loop with the sign flipping per ply.  Same decisions in the same order, hence the same
    consumption of the `random` stream (the goldens replay it): an untried child first, else the first maximum of UCB1
    (agents.py:177-196); a playout at a childless node, which is expanded on its tenth visit (:153-163)."""

    def __init__(self, state):
        self.state, self.w, self.n, self.first, self.count = [state], [0], [0], [-1], [0]
        self.expand(0)

    def expand(self, i):
        self.first[i] = len(self.state)
        for a in _legal(self.state[i]):
            self.state.append(self.state[i].next(a))
            self.w.append(0); self.n.append(0); self.first.append(-1); self.count.append(0)
        self.count[i] = len(self.state) - self.first[i]

    def select(self, i):
        kids = range(self.first[i], self.first[i] + self.count[i])
        t = 0
        for k in kids:
            if self.n[k] == 0:
                return k
            t += self.n[k]
        best, best_k = None, -1
        for k in kids:
            u = -self.w[k] / self.n[k] + 2 * (2 * math.log(t) / self.n[k]) ** 0.5
            if best is None or u > best:          # strict: the first maximum wins, like list.index(max(...))
                best, best_k = u, k
        return best_k

    def simulate(self):
        path = [0]
        while True:
            i = path[-1]
            st = self.state[i]
            if st.is_done():
                value = -1 if st.is_lose() else 0
                break
            if self.count[i] == 0:
                value = playout(st)
                if self.n[i] + 1 == 10:
                    self.expand(i)
                break
            path.append(self.select(i))
        for i in reversed(path):                  # value is the leaf's own view; every step up the path negates it (:167)
            self.w[i] += value
            self.n[i] += 1
            value = -value


def mcts_action(state, evaluations=100):
    """Plain Monte-Carlo tree search with random playouts; the most visited root action (agents.py:130-214)."""
    tree = _Tree(state)
    for _ in range(evaluations):
        tree.simulate()
    visits = tree.n[tree.first[0]:tree.first[0] + tree.count[0]]
    return _legal(state)[argmax(visits)]


# ------------------------------------------------------------------ batched agents (csrc/agents.hip, include/aqgnn.h)
def draw_uniforms(seed, b, n):
    """The first n draws of state / game b of a call seeded with `seed`: float64 in [0, 1), a pure function of (seed, b, i) -- the
    generator the kernels use when no table is given (include/aqgnn.h):
    key = mix(seed + G (b + 1)); u_i = (mix(key + G (i + 1)) >> 11) 2^-53."""
    return counter_uniform(stream_key(int(seed), int(b)), np.arange(int(n)))


def default_threads():
    """Threads of the alpha-beta pool: the CPUs this process may run on, at most 16 (never the machine's CPU count)."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _records(states72):
    """[B,72] uint8 records from an array, a tensor, or a sequence of States / records (host or device, as given)."""
    if isinstance(states72, torch.Tensor):
        return states72.to(torch.uint8).reshape(-1, 72)
    if isinstance(states72, np.ndarray):
        return np.ascontiguousarray(states72, dtype=np.uint8).reshape(-1, 72)
    return np.stack([_rec(s) for s in states72]).reshape(-1, 72) if len(states72) else np.zeros((0, 72), np.uint8)


def _device_batch(states72, device):
    dev = _lib.require_gpu(device)
    recs = _records(states72)
    d = (recs if isinstance(recs, torch.Tensor) else torch.from_numpy(recs)).to(dev).contiguous()
    if d.shape[0] == 0:
        raise ValueError("no states")
    return dev, d, int(d[0, 70].item())


def _draw_source(uniforms, B, dev):
    """(table tensor or None, stride) of a call.  uniforms: None = the generator; else float64 [B, n], row b = the draws of state b."""
    if uniforms is None:
        return None, 0
    u = torch.as_tensor(np.asarray(uniforms, dtype=np.float64) if not isinstance(uniforms, torch.Tensor) else uniforms,
                        dtype=torch.float64).to(dev).contiguous()
    if u.dim() == 1:
        u = u.view(B, -1)
    if u.dim() != 2 or u.shape[0] != B:
        raise ValueError(f"uniforms must be [B, n] with B = {B}, got {tuple(u.shape)}")
    return u, int(u.shape[1])


def _check_draws(draws, stride, what):
    m = int(draws.max().item()) if draws.numel() else 0
    if m > stride:
        raise ValueError(f"{what}: a state consumed {m} draws, the uniforms table holds {stride} per state")


def random_action_device(states, N, seed=0, uniforms=None):
    """aqg_agent_random on device records [B,72]: int32 [B] device tensor, -1 where a state has no legal action."""
    dev = states.device
    B = int(states.shape[0])
    u, stride = _draw_source(uniforms, B, dev)
    out = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().aqg_agent_random(N, _lib.ptr(states), B, _lib.ptr(u), stride, int(seed) & MASK64, _lib.ptr(out),
                                            _lib.stream_ptr(dev)), "aqg_agent_random")
    return out


def random_action_batch(states72, seed=0, uniforms=None, device=None):
    """random_action for every state at once: legal_actions()[min(count - 1, int(u * count))] with one draw u per state -- from
    `uniforms` ([B] or [B,1] float64) or from draw_uniforms(seed, b, 1).  Returns int32 [B] (numpy), -1 = no legal action."""
    dev, d, N = _device_batch(states72, device)
    return random_action_device(d, N, seed, uniforms).cpu().numpy()


def playout_batch(states72, seed=0, uniforms=None, return_final=False, device=None):
    """playout() from every state at once (aqg_playouts): (value, plies, draws) int32 [B] numpy arrays -- the value from the START
    state's mover's view, the moves played, the draws consumed -- and the final records uint8 [B,72] with return_final.  Draws:
    row b of `uniforms` [B, n] in order, or draw_uniforms(seed, b, .)."""
    dev, d, N = _device_batch(states72, device)
    B = int(d.shape[0])
    u, stride = _draw_source(uniforms, B, dev)
    value, plies, draws = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    final = torch.empty((B, 72), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().aqg_playouts(N, _lib.ptr(d), B, board_params(N)[1], _lib.ptr(u), stride, int(seed) & MASK64,
                                        _lib.ptr(value), _lib.ptr(plies), _lib.ptr(draws), _lib.ptr(final), _lib.stream_ptr(dev)),
               "aqg_playouts")
    if u is not None:
        _check_draws(draws, stride, "playout_batch")
    out = (value.cpu().numpy(), plies.cpu().numpy(), draws.cpu().numpy())
    return out + (final.cpu().numpy(),) if return_final else out


MCTS_MAX_EVALUATIONS = 2048     # AQG_AGENT_MCTS_MAX_EVALUATIONS: the table below is (evaluations + 1)^2 doubles, 32 MiB at the cap


@functools.lru_cache(maxsize=4)
def explore_table(evaluations):
    """UCB1's exploration term 2 * (2 * log(t) / n) ** 0.5 for 1 <= n <= t <= evaluations, as CPython evaluates the reference's
    expression (agents.py:196), float64 [(evaluations + 1), (evaluations + 1)] indexed [t][n]: the kernel looks it up instead of
    calling a log and a pow of its own, which are not the host's bit for bit."""
    E = int(evaluations)
    if not 0 <= E <= MCTS_MAX_EVALUATIONS:
        raise ValueError(f"evaluations must be 0..{MCTS_MAX_EVALUATIONS}, got {E}")
    out = np.zeros((E + 1, E + 1), dtype=np.float64)
    for t in range(1, E + 1):
        lt = math.log(t)
        for n in range(1, t + 1):
            out[t, n] = 2 * (2 * lt / n) ** 0.5
    return out


_explore_dev = {}


def mcts_action_device(states, N, evaluations=100, seed=0, uniforms=None):
    """aqg_agent_mcts on device records [B,72]: (action i32 [B], visits i32 [B,MAX_LEGAL], actions u8 [B,MAX_LEGAL], count i32 [B],
    draws i32 [B]) device tensors."""
    dev = states.device
    lib = _lib.load()
    B, E = int(states.shape[0]), int(evaluations)
    u, stride = _draw_source(uniforms, B, dev)
    key = (E, str(dev))
    if key not in _explore_dev:
        while len(_explore_dev) >= 4:                      # a few evaluation counts at most stay resident
            _explore_dev.pop(next(iter(_explore_dev)))
        _explore_dev[key] = torch.from_numpy(explore_table(E)).to(dev).contiguous()
    ws = torch.empty((int(lib.aqg_agent_mcts_workspace_bytes(N, B, E)),), dtype=torch.uint8, device=dev)
    action, count, draws = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    visits = torch.empty((B, _lib.MAX_LEGAL), dtype=torch.int32, device=dev)
    actions = torch.empty((B, _lib.MAX_LEGAL), dtype=torch.uint8, device=dev)
    _lib.check(lib.aqg_agent_mcts(N, _lib.ptr(states), B, E, board_params(N)[1], _lib.ptr(_explore_dev[key]), _lib.ptr(u), stride,
                                  int(seed) & MASK64, _lib.ptr(ws), ws.numel(), _lib.ptr(action), _lib.ptr(visits), _lib.ptr(actions),
                                  _lib.ptr(count), _lib.ptr(draws), _lib.stream_ptr(dev)), "aqg_agent_mcts")
    ws.record_stream(torch.cuda.current_stream(dev))
    return action, visits, actions, count, draws


def mcts_action_batch(states72, evaluations=100, seed=0, uniforms=None, return_visits=False, device=None):
    """mcts_action for every state at once (aqg_agent_mcts; the semantics of _Tree): int32 [B] actions (numpy, -1 = no legal
    action); with return_visits also the root children's (visits i32 [B,MAX_LEGAL], actions u8 [B,MAX_LEGAL], count i32 [B]) in the
    layout of aqg_engine_root_visits.  Draws of state b are consumed in evaluation order, one per random move of each playout: row b
    of `uniforms` [B, n], or draw_uniforms(seed, b, .)."""
    dev, d, N = _device_batch(states72, device)
    u, stride = _draw_source(uniforms, int(d.shape[0]), dev)
    action, visits, actions, count, draws = mcts_action_device(d, N, evaluations, seed, u)
    if u is not None:
        _check_draws(draws, stride, "mcts_action_batch")
    if return_visits:
        return action.cpu().numpy(), visits.cpu().numpy(), actions.cpu().numpy(), count.cpu().numpy()
    return action.cpu().numpy()


AB_MAX_DEPTH = _lib.AGENT_AB_MAX_DEPTH     # the deepest search aqg_agent_alpha_beta serves
# BatchedAgentMatch's 'auto' backend: slots per engine from which the alpha-beta agent is served by the kernel -- the smallest
# 9x9 batch at which tools/alpha_beta_time.py measured the device call faster than the 16-thread host pool.  That is the smallest
# batch of the run in profiles/alpha_beta_device.log (5 positions: 3.6 ms against 18.0 ms); nothing below 5 was measured.
ALPHA_BETA_DEVICE_MIN_STATES = 5


def shortest_paths_batch(states72, device=None):
    """shortest_path of every state and of its flipped state (aqg_agent_shortest_paths): int32 [B,2] (numpy), column 0 the
    mover's plies to its goal row, column 1 the other side's; -1 = walled in."""
    dev, d, N = _device_batch(states72, device)
    out = torch.empty((int(d.shape[0]), 2), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().aqg_agent_shortest_paths(N, _lib.ptr(d), int(d.shape[0]), _lib.ptr(out), _lib.stream_ptr(dev)),
               "aqg_agent_shortest_paths")
    return out.cpu().numpy()


def heuristic_eval_batch(states72, device=None):
    """heuristic_eval of every state: float64 [B] (numpy).  The paths come from the kernel, the one division is done here in
    float64 as the host does it, so the values are heuristic_eval's bit for bit."""
    recs = _records(states72)
    if recs.shape[0] == 0:
        raise ValueError("no states")
    walls, draw = board_params(int(recs[0, 70]))
    p = shortest_paths_batch(recs, device).astype(np.int64)
    return (p[:, 1] - p[:, 0]).astype(np.float64) / np.float64(draw // 2 - walls)


def _check_depth(max_depth):
    if not 0 <= int(max_depth) <= AB_MAX_DEPTH:
        raise ValueError(f"the alpha-beta kernel serves max_depth 0..{AB_MAX_DEPTH}, got {max_depth}")
    return int(max_depth)


def alpha_beta_action_device(states, N, max_depth=2, active=None, return_nodes=False):
    """aqg_agent_alpha_beta on device records [B,72]: int32 [B] device tensor, -1 where a state has no legal action, 0 where
    `active` (uint8 [B] device tensor, an engine's game_active) is 0.  No host synchronisation.  With return_nodes also the
    positions visited per state, int64 [B]."""
    dev = states.device
    lib = _lib.load()
    B, depth = int(states.shape[0]), _check_depth(max_depth)
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    nodes = torch.empty((B,), dtype=torch.int64, device=dev) if return_nodes else None
    if B > 0:
        if active is not None and (active.dtype != torch.uint8 or active.numel() != B):
            raise ValueError("active must be a uint8 tensor with one entry per state")
        walls, draw = board_params(N)
        ws = torch.empty((int(lib.aqg_agent_alpha_beta_workspace_bytes(N, B, depth)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.aqg_agent_alpha_beta(N, _lib.ptr(states), B, _lib.ptr(active), draw, draw // 2 - walls, depth, _lib.ptr(ws),
                                            ws.numel(), _lib.ptr(action), _lib.ptr(nodes), _lib.stream_ptr(dev)),
                   "aqg_agent_alpha_beta")
        ws.record_stream(torch.cuda.current_stream(dev))
    return (action, nodes) if return_nodes else action


def alpha_beta_action_batch(states72, max_depth=2, threads=None, backend="host", device=None):
    """alpha_beta_action for every state, in input order.  Returns int32 [B] (numpy), -1 = no action.
    backend 'host' (the default; no GPU needed): the native host search from a pool of `threads` threads (default
    default_threads(); ctypes releases the GIL during a search).  backend 'hip': the kernel (aqg_agent_alpha_beta, max_depth up to
    AB_MAX_DEPTH, one board size per call); the same actions."""
    if backend not in ("host", "hip"):
        raise ValueError(f"backend must be 'host' or 'hip', got {backend!r}")
    if backend == "hip":
        _check_depth(max_depth)
        if len(states72) == 0:
            return np.zeros((0,), dtype=np.int32)
        dev, d, N = _device_batch(states72, device)
        return alpha_beta_action_device(d, N, max_depth).cpu().numpy()
    recs = _records(states72)
    if isinstance(recs, torch.Tensor):
        recs = recs.cpu().numpy()
    recs = np.ascontiguousarray(recs, dtype=np.uint8)
    lib = _lib.load()
    threads = default_threads() if threads is None else max(1, int(threads))

    def one(i):
        r = recs[i]
        N = int(r[70])
        walls, draw = board_params(N)
        return int(lib.aqg_host_alpha_beta_action(N, r.ctypes.data_as(ctypes.c_void_p), draw, draw // 2 - walls, int(max_depth)))

    n = recs.shape[0]
    if threads == 1 or n <= 1:
        out = [one(i) for i in range(n)]
    else:
        with ThreadPoolExecutor(max_workers=min(threads, n)) as pool:
            out = list(pool.map(one, range(n)))
    return np.asarray(out, dtype=np.int32)


if __name__ == '__main__':
    from .game_logic import State
    s = State()
    while not s.is_done():
        s = s.next(random_action(s))
    print(s)
