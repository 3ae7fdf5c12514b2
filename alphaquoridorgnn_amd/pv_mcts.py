"""Policy-Value MCTS -- drop-in for the reference's pv_mcts.py on top of the batched HIP engine.

Same call surface (pv_mcts.py:18-109): PV_EVALUATE_COUNT, pv_mcts_policy(model, state, temperature, device),
pv_mcts_action(model, temperature=0, device='cpu'), boltzman(xs, temperature).  A single-state call is a batch
of one game on the GPU engine (csrc/mcts.hip); thousands of states go through `pv_mcts_policy_batch`.
"""
import numpy as np
import torch

from . import _lib
from .engine import BatchedSelfPlay

PV_EVALUATE_COUNT = 50  # Number of simulations per inference (pv_mcts.py:18; "original is 1600")

_engines = {}


def _engine_for(model, num_games, sims, board_size, evaluator="gnn", fake_bias=0):
    key = (id(model), num_games, sims, board_size, evaluator, fake_bias)
    eng = _engines.get(key)
    if eng is None:
        if len(_engines) > 4:
            _engines.clear()
        eng = _engines[key] = BatchedSelfPlay(model, num_games=num_games, sims=sims, board_size=board_size,
                                              evaluator=evaluator, fake_bias=fake_bias, record_history=False)
    else:
        eng.refresh_weights()          # (a network evaluator's weights may have changed since; nothing to do for the others)
    return eng


def _drop_engine(eng):
    """Forget a cached engine (reanalyse: its tree pool must not stay resident beside the next generation's self-play engine)."""
    for key in [k for k, v in _engines.items() if v is eng]:
        del _engines[key]


def boltzman(xs, temperature):
    """Boltzmann distribution (pv_mcts.py:106-109)."""
    xs = [x ** (1 / temperature) for x in xs]
    return [x / sum(xs) for x in xs]


def _policy_from_visits(visits, temperature):
    if temperature == 0:                               # pv_mcts.py:89-92
        pol = np.zeros(len(visits))
        pol[int(np.argmax(visits))] = 1
        return pol
    return boltzman(visits, temperature)               # pv_mcts.py:93-95


def pv_mcts_policy_batch(model, states72, temperature, sims=None, board_size=None, evaluator="gnn", fake_bias=0,
                         tree_reuse=None, tree_reuse_visits=None, resign_threshold=None, resign_min_ply=None,
                         resign_disable_fraction=None, resign_seed=None):
    """states72: uint8 [B,72] -> list of B policies (each aligned with that state's legal_actions()).
    evaluator: 'gnn' (the default 6/128/3 network), 'general' (a GraphPolicyValueNetwork of any shape with 6 input features, on
    the library's kernels), 'cnn' (the reference's CNNNetwork, pv_network_cnn.py, on the library's kernels), 'external'
    (model.predict per leaf) or 'fake'.  Every call searches caller-given roots from fresh trees: the self-play options that ask for
    tree reuse are refused (ValueError)."""
    from .selfplay_options import refuse_self_play_options
    refuse_self_play_options("pv_mcts_policy_batch", tree_reuse=tree_reuse, tree_reuse_visits=tree_reuse_visits, resign_threshold=resign_threshold,
                             resign_min_ply=resign_min_ply, resign_disable_fraction=resign_disable_fraction, resign_seed=resign_seed)
    states72 = torch.as_tensor(states72, dtype=torch.uint8)
    B = states72.shape[0]
    N = int(states72[0, 70]) if board_size is None else board_size
    eng = _engine_for(model, B, PV_EVALUATE_COUNT if sims is None else sims, N, evaluator, fake_bias)
    visits, actions, count = eng.search(states72)
    visits, count = visits.cpu().numpy(), count.cpu().numpy()
    return [_policy_from_visits([int(v) for v in visits[b, :count[b]]], temperature) for b in range(B)]


def pv_mcts_improved_policy_batch(model, states72, sims=None, board_size=None, evaluator="gnn", fake_bias=0, c_visit=50.0, c_scale=1.0):
    """states72: uint8 [B,72] -> (pi' float32 [B, A], vmix float32 [B]) on the engine's device: the completed-Q improved policy of a
    fresh search of every position, pi' = softmax(log p + sigma(completedQ)) over its legal actions (Danihelka et al., ICLR 2022;
    engine.improved_policy_reference), as dense rows over the board's A actions -- 0 at the others -- and the mixed value of each root.
    Non-zero on unvisited legal actions, unlike the visit counts of pv_mcts_policy_batch.  evaluator, sims and fake_bias as there."""
    from .selfplay_options import check_completed_q
    c_visit, c_scale = check_completed_q(c_visit, c_scale)
    states72 = torch.as_tensor(states72, dtype=torch.uint8)
    B = states72.shape[0]
    N = int(states72[0, 70]) if board_size is None else board_size
    eng = _engine_for(model, B, PV_EVALUATE_COUNT if sims is None else sims, N, evaluator, fake_bias)
    eng.search(states72)
    policy, actions, count, vmix = eng.root_improved_policy(c_visit, c_scale)
    A = N * N + 2 * (N - 1) ** 2
    inside = (torch.arange(_lib.MAX_LEGAL, device=policy.device).unsqueeze(0) < count.unsqueeze(1)) & (actions < A)
    dense = torch.zeros((B, A + 1), dtype=torch.float32, device=policy.device)       # column A takes what lies past the count
    dense.scatter_(1, torch.where(inside, actions.long(), A), torch.where(inside, policy, 0.0))
    return dense[:, :A].contiguous(), vmix


def evaluator_of(model):
    """'gnn' for the GNN the HIP kernels evaluate themselves (the default 6/128/3 shape); 'cnn' for the reference's CNNNetwork
    (pv_network_cnn.py, self_play.py:16,78), which they evaluate too; 'external' for any other object with the reference's
    predict(state, device) (BaseNetwork.py:36-40), e.g. a GraphPolicyValueNetwork of another shape or a stock CNN module."""
    from .pv_network_cnn import CNNNetwork
    if isinstance(model, CNNNetwork):
        return "cnn"
    # (another GNN shape stays 'external', not 'general': this surface serves ANY object through its predict, as the reference does)
    return "gnn" if hasattr(model, "packed_weights") and getattr(model, "fused", True) else "external"


def pv_mcts_policy(model, state, temperature, device=None):
    """PUCT MCTS from `state`; returns the improved policy over state.legal_actions() (pv_mcts.py:20-95)."""
    rec = torch.from_numpy(state.record()).unsqueeze(0)
    return pv_mcts_policy_batch(model, rec, temperature, PV_EVALUATE_COUNT, state.N, evaluator=evaluator_of(model))[0]


def pv_mcts_action(model, temperature=0, device='cpu', root_noise_eps=None, root_noise_alpha=None, root_noise_seed=None,
                   tree_reuse=None, tree_reuse_visits=None, resign_threshold=None, resign_min_ply=None,
                   resign_disable_fraction=None, resign_seed=None):
    """Returns a function of the game state that selects an action based on PV-MCTS (pv_mcts.py:98-103).  A player for matches:
    it never adds root exploration noise, and the self-play options that ask for it are refused (ValueError)."""
    from .selfplay_options import refuse_self_play_options
    refuse_self_play_options("pv_mcts_action", root_noise_eps=root_noise_eps, root_noise_alpha=root_noise_alpha, root_noise_seed=root_noise_seed,
                             tree_reuse=tree_reuse, tree_reuse_visits=tree_reuse_visits, resign_threshold=resign_threshold,
                             resign_min_ply=resign_min_ply, resign_disable_fraction=resign_disable_fraction, resign_seed=resign_seed)
    def pv_mcts_action(state):
        policy = pv_mcts_policy(model, state, temperature, device)
        return np.random.choice(state.legal_actions(), p=policy)
    return pv_mcts_action
