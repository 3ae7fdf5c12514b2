"""Strength tracking -- drop-in for the reference's evaluate_agents.py: the best network against the random, alpha-beta and
rollout-MCTS agents, with the games of a match played CONCURRENTLY on the batched HIP engine.

Call surface kept (evaluate_agents.py:15-89): EP_GAME_COUNT, first_player_point, play(next_actions), evaluate_algorithm_of,
evaluate_best_player().  `play` / `evaluate_algorithm_of` are the reference's host loops for any two action functions (without its
per-ply print of the board).  `evaluate_best_player()` plays its three matches with BatchedAgentMatch: the network's plies are
searched by the engine as in self-play, the agent's plies are served for all games at once -- random moves and the rollout MCTS by
the kernels of csrc/agents.hip, alpha-beta by its kernel there too (or, for a handful of slots, by the native host search on a thread
pool: `backend` below) -- and applied to the engine without a search
(aqg_engine_apply_actions).  Per game this is the reference's loop: colours alternate with the game index
(evaluate_agents.py:46-51) and the network moves at temperature 0 (:73).  The kernels' random draws are their own stream
(agents.draw_uniforms), not Python's `random`.
"""
import numpy as np
import torch

from . import agents, constants
from . import pv_mcts
from .constants import BOARD_SIZE, board_params
from .engine import BatchedSelfPlay
from .evaluators import BINDINGS
from .game_logic import State
from .selfplay_options import refuse_self_play_options
from .two_engine_match import TwoEngineMatch

EP_GAME_COUNT = 10  # Number of games per evaluation (evaluate_agents.py:15)


def first_player_point(ended_state):
    """1: first player wins, 0: first player loses, 0.5: draw (evaluate_agents.py:18-22)."""
    if ended_state.is_lose():
        return 0 if ended_state.is_first_player() else 1
    return 0.5


def play(next_actions, board_size=None):
    """Execute one game with two action functions (evaluate_agents.py:25-40); host loop."""
    state = State() if board_size is None else State(board_size=board_size, num_walls=board_params(board_size)[0])
    while not state.is_done():
        next_action = next_actions[0] if state.is_first_player() else next_actions[1]
        action = next_action(state)
        state = state.next(action)
    return first_player_point(state)


def evaluate_algorithm_of(label, next_actions, games=None, board_size=None):
    """Evaluation of any algorithm (evaluate_agents.py:43-59): EP_GAME_COUNT games, colours alternating; prints and returns the
    average point of next_actions[0]."""
    games = EP_GAME_COUNT if games is None else int(games)
    total_point = 0
    for i in range(games):
        if i % 2 == 0:
            total_point += play(next_actions, board_size)
        else:
            total_point += 1 - play(list(reversed(next_actions)), board_size)
        print('\rEvaluate {}/{}'.format(i + 1, games), end='')
    print('')
    average_point = total_point / games
    print(label, average_point)
    return average_point


AGENTS = ("random", "alpha_beta", "mcts")


class BatchedAgentMatch(TwoEngineMatch):
    """`num_games` games of a network against a baseline agent on the batched engine; the network moves first in game i when i is
    even (evaluate_agents.py:46-51).  Two engines, as BatchedMatch has them: the network-first games and the agent-first games.
    Each ply, each engine either searches (`move`) or reads its roots, asks the agent for one action per slot and applies them.

    agent: 'random' / 'mcts' / 'alpha_beta' (HIP kernels), or any callable state -> action, served game by game on the host (the
    slow, general path; while it is called, `self.current` = (engine index, slot, ply)).
    agent_kwargs: evaluations (mcts, default 100); max_depth / threads / backend (alpha_beta).  backend 'hip': the positions go
    from the engine to aqg_agent_alpha_beta and the actions back into the engine without leaving the device; 'host': the records
    are copied out, searched natively from a thread pool and copied back; 'auto' (the default): 'hip' for engines of at least
    agents.ALPHA_BETA_DEVICE_MIN_STATES slots and a max_depth the kernel serves, else 'host'.  The games are the same either way.
    evaluator: 'gnn' (the default 6/128/3 network), 'general' (a GraphPolicyValueNetwork of any shape), 'cnn', 'external' (any
    model with predict) or 'fake' (`model` is the integer bias of the parity tests' hash evaluator)."""

    def __init__(self, model, agent, num_games, sims=None, board_size=BOARD_SIZE, temperature=0.0, evaluator="gnn", seed=0,
                 device=None, agent_kwargs=None, root_noise_eps=None, root_noise_alpha=None, root_noise_seed=None,
                 tree_reuse=None, tree_reuse_visits=None, resign_threshold=None, resign_min_ply=None,
                 resign_disable_fraction=None, resign_seed=None, gumbel_considered=None, gumbel_scale=None, gumbel_seed=None):
        # (a strength measurement plays the network as it is: root exploration noise is a self-play option and is refused)
        refuse_self_play_options("BatchedAgentMatch", root_noise_eps=root_noise_eps, root_noise_alpha=root_noise_alpha, root_noise_seed=root_noise_seed,
                                 tree_reuse=tree_reuse, tree_reuse_visits=tree_reuse_visits, resign_threshold=resign_threshold,
                                 resign_min_ply=resign_min_ply, resign_disable_fraction=resign_disable_fraction, resign_seed=resign_seed,
                                 gumbel_considered=gumbel_considered, gumbel_scale=gumbel_scale, gumbel_seed=gumbel_seed)
        if not callable(agent) and agent not in AGENTS:
            raise ValueError(f"agent must be one of {AGENTS} or a callable state -> action")
        if evaluator not in BINDINGS:
            raise ValueError(f"evaluator must be one of {', '.join(BINDINGS)}")
        self.model, self.agent, self.evaluator = model, agent, evaluator
        self.agent_kwargs = dict(agent_kwargs or {})
        if self.agent_kwargs.get("backend", "auto") not in ("auto", "hip", "host"):
            raise ValueError("agent_kwargs['backend'] must be 'auto', 'hip' or 'host'")
        self.N, self.seed = int(board_size), int(seed)
        self.current = None
        self._build_engines(num_games, self.seed, sims=pv_mcts.PV_EVALUATE_COUNT if sims is None else sims, board_size=board_size,
                            temperature=temperature, device=device)

    def _engine(self, first, **kw):
        return BatchedSelfPlay(self.model, evaluator=self.evaluator, **kw)      # ('fake': the model is the integer bias)

    def _alpha_beta_on_device(self, eng):
        backend = self.agent_kwargs.get("backend", "auto")
        if backend == "auto":
            return (eng.G >= agents.ALPHA_BETA_DEVICE_MIN_STATES
                    and 0 <= int(self.agent_kwargs.get("max_depth", 2)) <= agents.AB_MAX_DEPTH)
        return backend == "hip"

    # ------------------------------------------------------------------ the agent's ply
    def _call_seed(self, first, ply):
        return (self.seed * 1000003 + 2 * ply + first) & ((1 << 64) - 1)

    def _agent_actions(self, eng, first, ply, table):
        """One action per slot (int32 [G], device or host) for the positions engine `eng` stands in."""
        states = eng.root_states72()
        if self.agent == "random":
            table, width = agents._draw_source(table, eng.G, eng.dev)
            if table is not None and width < 1:                              # a table that is too short must not pass silently
                raise ValueError("agent_uniforms: the random agent takes one draw per slot and ply")
            return agents.random_action_device(states, self.N, self._call_seed(first, ply), table)
        if self.agent == "mcts":
            table, width = agents._draw_source(table, eng.G, eng.dev)
            out = agents.mcts_action_device(states, self.N, int(self.agent_kwargs.get("evaluations", 100)),
                                            self._call_seed(first, ply), table)
            if table is not None:
                agents._check_draws(out[4], width, "agent_uniforms (mcts)")
            return out[0]
        if self.agent == "alpha_beta" and self._alpha_beta_on_device(eng):
            return agents.alpha_beta_action_device(states, self.N, int(self.agent_kwargs.get("max_depth", 2)),
                                                   active=eng.t["game_active"])
        recs = states.cpu().numpy()
        active = eng.t["game_active"].cpu().numpy() != 0
        out = np.zeros((eng.G,), dtype=np.int32)
        if self.agent == "alpha_beta":
            idx = np.nonzero(active)[0]
            if len(idx):
                out[idx] = agents.alpha_beta_action_batch(recs[idx], max_depth=int(self.agent_kwargs.get("max_depth", 2)),
                                                          threads=self.agent_kwargs.get("threads"))
            return out
        for g in np.nonzero(active)[0]:
            self.current = (first, int(g), ply)
            a = self.agent(State.from_record(recs[g]))
            out[g] = -1 if a is None else int(a)
        self.current = None
        return out

    # ------------------------------------------------------------------ the match
    def play(self, uniforms=None, agent_uniforms=None):
        """Play every game to the end; returns the network's points per game in game order.
        uniforms: optional pair (per engine) of float64 [max_plies, G_engine], the engine's own draw per searched move (unused at
        temperature 0).  agent_uniforms: optional pair of float64 [max_plies, G_engine, n]: [ply][g] is the table of draws of slot
        g's agent move at that ply ('random': n >= 1; 'mcts': n >= evaluations * plies to the draw limit); default: the generator,
        seeded per engine and ply from `seed`.
        fp16-range guard ('gnn'): the match is replayed from ply 0 on the exact f32-input kernels (TwoEngineMatch._play)."""
        for eng in filter(None, self.engines):
            if eng.moves_done:          # a second play() on the same object plays the match again
                eng.reset()
        return self._play(uniforms, agent_uniforms)

    def _ply(self, eng, first, ply, uniforms, agent_uniforms):
        if (ply % 2 == 0) == (first == 0):                       # the network's ply
            eng.move(None if uniforms is None else uniforms[first][ply])
        else:
            table = None if agent_uniforms is None else agent_uniforms[first][ply]
            eng.apply_actions(self._agent_actions(eng, first, ply, table))


_LABELS = {"random": "VS_Random", "alpha_beta": "VS_AlphaBeta", "mcts": "VS_MCTS"}
_BOARD_OF_POLICY = {n * n + 2 * (n - 1) * (n - 1): n for n in (3, 5, 7, 9)}


def evaluate_best_player(games=None, agents=AGENTS, seed=None, root_noise_eps=None, root_noise_alpha=None, root_noise_seed=None,
                         tree_reuse=None, tree_reuse_visits=None, resign_threshold=None, resign_min_ply=None,
                         resign_disable_fraction=None, resign_seed=None, gumbel_considered=None, gumbel_scale=None, gumbel_seed=None):
    """Evaluation of the best player (evaluate_agents.py:62-89): best.pth -- a GNN of any shape or the residual CNN, on the board its
    policy head is sized for -- against each of `agents`, `games` games each (default EP_GAME_COUNT), all games of a match at once.
    Prints the reference's lines (label, average point) and returns {label: average point}."""
    refuse_self_play_options("evaluate_best_player", root_noise_eps=root_noise_eps, root_noise_alpha=root_noise_alpha, root_noise_seed=root_noise_seed,
                             tree_reuse=tree_reuse, tree_reuse_visits=tree_reuse_visits, resign_threshold=resign_threshold,
                             resign_min_ply=resign_min_ply, resign_disable_fraction=resign_disable_fraction, resign_seed=resign_seed,
                             gumbel_considered=gumbel_considered, gumbel_scale=gumbel_scale, gumbel_seed=gumbel_seed)
    from .pv_network_cnn import CNNNetwork
    from .pv_network_gnn import GNNNetwork, load_network
    games = EP_GAME_COUNT if games is None else int(games)
    model = load_network(constants.PV_NETWORK_PATH + 'best.pth')
    board = _BOARD_OF_POLICY.get(int(model.policy_output_size), BOARD_SIZE)
    # by class: the board follows the file's policy head here, and load_network makes a GNNNetwork only of 6/128/3 WITH the 9x9 head
    evaluator = "cnn" if isinstance(model, CNNNetwork) else "gnn" if isinstance(model, GNNNetwork) else "general"
    seed = int(np.random.randint(0, 2 ** 30)) if seed is None else int(seed)
    out = {}
    for k, agent in enumerate(agents):                 # (the parameter, not the module: this function needs only the names)
        match = BatchedAgentMatch(model, agent, games, board_size=board, temperature=0.0, evaluator=evaluator, seed=seed + k)
        points = match.play()
        print('Evaluate {}/{}'.format(games, games))
        label = _LABELS.get(agent, str(agent))
        out[label] = sum(points) / games
        print(label, out[label])
        del match
    del model
    torch.cuda.empty_cache()
    return out


if __name__ == '__main__':
    evaluate_best_player()
