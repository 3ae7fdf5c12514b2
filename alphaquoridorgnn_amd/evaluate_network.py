"""New-parameter evaluation -- drop-in for the reference's evaluate_network.py, on the batched HIP engine.

Call surface kept (evaluate_network.py:13-94): EN_GAME_COUNT, EN_TEMPERATURE, first_player_point, play(next_actions),
update_best_player, evaluate_network().  `evaluate_network()` plays the EN_GAME_COUNT games of latest vs best
CONCURRENTLY: the games in which `latest` moves first form one engine batch, the games in which `best` moves first a
second one, and before every ply each batch is pointed at the weights of the model whose turn it is -- per game exactly
the reference's loop, in which the mover's own model searches from a fresh tree (pv_mcts.py:98-104) and the colours
alternate with the game index (evaluate_network.py:69-74).
"""
from shutil import copy

import numpy as np
import torch

from . import _lib
from . import pv_mcts
from .constants import PV_NETWORK_PATH, BOARD_SIZE
from .engine import BatchedSelfPlay
from .evaluators import BINDINGS
from .game_logic import State
from .pv_network_gnn import GNNNetwork, load_network
from .pv_network_cnn import CNNNetwork
from .selfplay_options import refuse_self_play_options
from .two_engine_match import TwoEngineMatch

EN_GAME_COUNT = 15    # Number of games per evaluation (evaluate_network.py:14; originally 400)
EN_TEMPERATURE = 1.0  # Temperature of the Boltzmann distribution (evaluate_network.py:15)
# Paired-opening evaluation (the reference has none; openings.random_book, BatchedMatch(openings=)): EN_OPENING_PLIES K > 0 (even) plays
# the match from a book of EN_GAME_COUNT // 2 positions K random plies deep, each opening twice with the colours exchanged, at
# EN_OPENING_TEMPERATURE, and prints openings.pair_report.  The promotion rule stays average > 0.5.
EN_OPENING_PLIES = 0         # 0 = off: every game from the opening record, at EN_TEMPERATURE
EN_OPENING_SEED = 0
EN_OPENING_TEMPERATURE = 0.0


def first_player_point(ended_state):
    """1: first player wins, 0: first player loses, 0.5: draw (evaluate_network.py:18-22)."""
    if ended_state.is_lose():
        return 0 if ended_state.is_first_player() else 1
    return 0.5


def play(next_actions):
    """Execute one game with two action functions (evaluate_network.py:25-44); host loop, reference-shaped."""
    state = State()
    while True:
        if state.is_done():
            break
        next_action = next_actions[0] if state.is_first_player() else next_actions[1]
        action = next_action(state)
        state = state.next(action)
    return first_player_point(state)


def update_best_player():
    """Replace the best player (evaluate_network.py:47-49)."""
    copy(PV_NETWORK_PATH + 'latest.pth', PV_NETWORK_PATH + 'best.pth')
    print('Latest model is better than current best. Replacing best model with latest.')


def check_opening_options(plies, games):
    """EN_OPENING_PLIES against the game count: 0 = off; else even, >= 2, and an even number of games (ValueError otherwise)."""
    if isinstance(plies, bool) or int(plies) != plies or plies < 0 or plies % 2:
        raise ValueError(f"the opening depth must be an even number of plies >= 0, not {plies!r}: a start record has an even ply counter")
    if plies and (games < 2 or games % 2):
        raise ValueError(f"paired openings need an even number of games (every opening is played twice), not {games}")
    return int(plies)


class BatchedMatch(TwoEngineMatch):
    """`num_games` games of player 0 vs player 1 on the batched engine; game i has player (i % 2) moving first
    (evaluate_network.py:69-74).  Players are models (evaluator='gnn': the default 6/128/3 network; evaluator='general':
    GraphPolicyValueNetworks of any shape with 6 input features, the two players' shapes may differ; evaluator='cnn': two
    CNNNetworks, whose shapes may differ too) or integer biases of the parity tests' hash evaluator (evaluator='fake')."""

    def __init__(self, players, num_games, sims=None, board_size=BOARD_SIZE, temperature=EN_TEMPERATURE,
                 evaluator="gnn", seed=0, device=None, root_noise_eps=None, root_noise_alpha=None, root_noise_seed=None,
                 tree_reuse=None, tree_reuse_visits=None, resign_threshold=None, resign_min_ply=None,
                 resign_disable_fraction=None, resign_seed=None, gumbel_considered=None, gumbel_scale=None, gumbel_seed=None,
                 openings=None):
        """openings (None = off: the match as it always was): a uint8 [S, 72] book (openings.random_book); num_games must then be
        even, games 2j and 2j + 1 both start from openings[j % S] -- game 2j with player 0 moving first, game 2j + 1 with player 1 --
        and report() is openings.pair_report of the last play().  `temperature` stays the caller's (0 = no sampling noise)."""
        # (an evaluation match measures the networks as they are: root exploration noise is a self-play option and is refused)
        refuse_self_play_options("BatchedMatch", root_noise_eps=root_noise_eps, root_noise_alpha=root_noise_alpha, root_noise_seed=root_noise_seed,
                                 tree_reuse=tree_reuse, tree_reuse_visits=tree_reuse_visits, resign_threshold=resign_threshold,
                                 resign_min_ply=resign_min_ply, resign_disable_fraction=resign_disable_fraction, resign_seed=resign_seed,
                                 gumbel_considered=gumbel_considered, gumbel_scale=gumbel_scale, gumbel_seed=gumbel_seed)
        if evaluator == "external":
            raise ValueError("BatchedMatch has no evaluator='external': an engine asks one model, eng.model, from the host")
        self.players, self.evaluator, self.binding = players, evaluator, BINDINGS[evaluator]
        self.openings, self.points = openings, None
        if openings is not None and int(num_games) % 2:
            raise ValueError("BatchedMatch: with openings num_games must be even (every opening is played twice, colours exchanged)")
        # the split puts game 2j on engine 0 and game 2j + 1 on engine 1, both as local game j: both take the same table and the
        # default index j % S
        start = {} if openings is None else dict(start_states=openings)
        # (no evaluation cache here: the two players' weights take turns on one engine, a table would mix their outputs)
        self._build_engines(num_games, seed, sims=pv_mcts.PV_EVALUATE_COUNT if sims is None else sims, board_size=board_size,
                            temperature=temperature, device=device, eval_cache_slots=0, **start)
        eng = self.engines[0]      # (there unless the match has no game at all); the handles are what _ply points an engine at
        self._handles = [] if eng is None else [self.binding.handle(m, eng.dev, (eng.N, eng.A)) for m in players]

    def _engine(self, first, **kw):
        # built with the player whose workspace is the larger, then pointed at the mover's handle before every ply
        return BatchedSelfPlay(self.binding.sizing_player(self.players), evaluator=self.evaluator, **kw)

    @property
    def _flags(self):
        """evaluator='gnn': the gnn_flags each player's evaluations carry."""
        return [h[1] for h in self._handles]

    def _ply(self, eng, first, ply, uniforms):
        self.binding.point(eng, self._handles[first if ply % 2 == 0 else 1 - first])
        eng.move(None if uniforms is None else uniforms[first][ply])

    def play(self, uniforms=None):
        """Play every game to the end.  uniforms: optional pair of float64 arrays [max_plies, G_first] (parity tests).  Returns the
        per-game points of player 0 in game order.  fp16-range guard (TwoEngineMatch._play): BOTH players are marked (mark_saturated) before
        the replay -- the promotion decision (evaluate_network.py:90-94) is never taken on evaluations that are not the networks'."""
        if self.points is not None:              # played before: every game starts again (a first play() finds the engines reset)
            for eng in filter(None, self.engines):
                eng.reset()
        self.points = self._play(uniforms)
        return self.points

    def report(self):
        """openings.pair_report of the last play(): pairs, mean, se, elo, elo_se, los.  Needs openings."""
        from .openings import pair_report
        if self.openings is None or self.points is None:
            raise ValueError("report() is the paired report of a played match: build the match with openings and play() it")
        return pair_report(self.points)

    def _switch_to_exact_kernels(self):
        for m in self.players:
            if hasattr(m, "mark_saturated"):
                m.mark_saturated(self.engines[0].dev)
        self._handles = [(packed, _lib.GNN_EXACT_F32) for packed, _ in self._handles]
        super()._switch_to_exact_kernels()


def evaluate_network(root_noise_eps=None, root_noise_alpha=None, root_noise_seed=None, tree_reuse=None, tree_reuse_visits=None, resign_threshold=None,
                     resign_min_ply=None, resign_disable_fraction=None, resign_seed=None, gumbel_considered=None, gumbel_scale=None,
                     gumbel_seed=None):
    """Network evaluation (evaluate_network.py:52-94): latest vs best, promote when the average point exceeds 0.5.  Two
    default 6/128/3 networks play on the engine's fused evaluator ('gnn'); when either file holds another shape, both play on
    its any-shape evaluator ('general').  Two CNNs (pv_network_cnn.py) play on the engine's CNN evaluator ('cnn'); a CNN against
    a GNN is refused (ValueError)."""
    refuse_self_play_options("evaluate_network", root_noise_eps=root_noise_eps, root_noise_alpha=root_noise_alpha, root_noise_seed=root_noise_seed,
                             tree_reuse=tree_reuse, tree_reuse_visits=tree_reuse_visits, resign_threshold=resign_threshold,
                             resign_min_ply=resign_min_ply, resign_disable_fraction=resign_disable_fraction, resign_seed=resign_seed,
                             gumbel_considered=gumbel_considered, gumbel_scale=gumbel_scale, gumbel_seed=gumbel_seed)
    model0 = load_network(PV_NETWORK_PATH + 'latest.pth')
    model1 = load_network(PV_NETWORK_PATH + 'best.pth')
    cnn = [isinstance(m, CNNNetwork) for m in (model0, model1)]
    if any(cnn) and not all(cnn):
        raise ValueError("evaluate_network: latest.pth and best.pth hold different networks (a CNN and a GNN); matches between "
                         "a CNN and a GNN are not supported")
    fused = all(isinstance(m, GNNNetwork) for m in (model0, model1))      # (by class, as evaluate_agents does: both files, or neither)
    if fused and torch.cuda.is_available():
        for m in (model0, model1):
            m.packed_weights(torch.device("cuda", torch.cuda.current_device()))
    evaluator = "cnn" if all(cnn) else "gnn" if fused else "general"
    plies = check_opening_options(EN_OPENING_PLIES, EN_GAME_COUNT)
    if plies:
        from .openings import random_book
        book = random_book(BOARD_SIZE, plies, EN_GAME_COUNT // 2, EN_OPENING_SEED)
        match = BatchedMatch((model0, model1), EN_GAME_COUNT, temperature=EN_OPENING_TEMPERATURE,
                             seed=int(np.random.randint(0, 2 ** 30)), evaluator=evaluator, openings=book)
    else:
        match = BatchedMatch((model0, model1), EN_GAME_COUNT, temperature=EN_TEMPERATURE,
                             seed=int(np.random.randint(0, 2 ** 30)), evaluator=evaluator)
    points = match.play()
    print('Evaluating latest model against current best ({} games, concurrent)'.format(EN_GAME_COUNT))
    average_point = sum(points) / EN_GAME_COUNT
    print('Average points of latest model against current best:', average_point)
    if plies:
        r = match.report()
        print(f'paired openings ({plies} plies, {r["pairs"]} pairs, T = {EN_OPENING_TEMPERATURE}): mean {r["mean"]:.4f} +- {r["se"]:.4f}, '
              f'elo {r["elo"]:+.1f} +- {r["elo_se"]:.1f}, likelihood of superiority {r["los"]:.3f}')
    del model0
    del model1
    del match
    torch.cuda.empty_cache()
    if average_point > 0.5:
        update_best_player()
        return True
    return False


if __name__ == '__main__':
    evaluate_network()
