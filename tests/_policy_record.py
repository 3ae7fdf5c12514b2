"""Shared by tests/test_policy_record_cpu.py and tests/test_policy_record.py: policy rows with the bit patterns a verbatim copy must
keep, the file route of such rows, and the host statement of the rows a self-play engine records with policy_target='completed_q'
(include/aqgnn.h, "recording completed-Q targets during self-play").

The host statement follows a game as it was played: per ply the oracle's PV-MCTS (FakeModel) searches the root -- from the kept
subtree where tree reuse keeps one -- engine.improved_policy_reference turns the root's children into pi', and the row is pi'
scattered by the legal action ids over zeros.  The move is the one the game recorded, so the statement needs no uniform."""
import pickle

import numpy as np
import torch

from oracle import mcts as om, quoridor as oq
from tests import _tree_reuse as T
from tests._improved_policy import oracle_children


def policy_size(N):
    return N * N + 2 * (N - 1) ** 2


def recorded_rows(N, n, seed):
    """Policy rows as the engine records them, float32 [n, A]: a softmax over a random legal subset, zeros elsewhere -- with a
    denormal, a -0.0, the smallest normal and a 1.0 planted where there is room: a verbatim copy keeps every one of them."""
    rng = np.random.RandomState(seed)
    A = policy_size(N)
    P = np.zeros((n, A), dtype=np.float32)
    for i in range(n):
        k = int(rng.randint(1, A + 1))
        ids = rng.permutation(A)[:k]
        P[i, ids] = rng.dirichlet(np.full(k, 0.3)).astype(np.float32)
    special = np.asarray([1e-42, -0.0, 1.1754944e-38, 1.0], dtype=np.float32)
    for i in range(min(n, 4)):
        P[i, i % A] = special[i]
    if n > 4:
        P[4] = 0                                                 # a move that was applied, not searched
    return P


def policy_file_route(S, V, Z, P, N, tmp_path, values=None, blend=0.0):
    """self_play._history_rows(policy=) -> pickle -> the conversion of the trainers' loader; numpy (s, p, v)."""
    from alphaquoridorgnn_amd.pv_network_gnn import pack_states
    from alphaquoridorgnn_amd.self_play import _history_rows
    path = tmp_path / f"policy_rows{N}.history"
    with open(path, "wb") as f:
        pickle.dump(_history_rows(torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z), N,
                                  None if values is None else torch.from_numpy(values), blend, policy=torch.from_numpy(P)), f)
    with open(path, "rb") as f:
        history = pickle.load(f)
    s, p, v = zip(*history)
    return (pack_states(s, N), torch.tensor(np.array(p), dtype=torch.float32).numpy(),
            torch.tensor(np.array(v), dtype=torch.float32).numpy())


def root_row(root, N, c_visit=50.0, c_scale=1.0):
    """The dense row of one searched oracle root: improved_policy_reference over its children, scattered by legal action id."""
    from alphaquoridorgnn_amd.engine import improved_policy_reference
    row = np.zeros((policy_size(N),), dtype=np.float32)
    if root.children:
        pi, _ = improved_policy_reference(*oracle_children(root), c_visit, c_scale)
        row[list(root.state.legal_actions())] = pi
    return row


def statement_rows(N, sims, bias, recs, actions, keep_visits=None, c_visit=50.0, c_scale=1.0):
    """The rows of ONE game: recs uint8 [plies, 72] its recorded positions, actions uint8 [plies] its recorded moves (0xFF = the
    mover resigned: the game ends behind that row).  keep_visits: the engine's tree_reuse_visits (None = a fresh tree every move).
    Returns float32 [plies, A]; the replay checks every recorded position on the way."""
    model, state, clock = om.FakeModel(bias), oq.State(N=N), T.Clock()
    root = T.Node(state, 0)
    out = []
    for ply in range(recs.shape[0]):
        assert np.array_equal(np.asarray(state.rec)[:68], recs[ply][:68]) and state.plies_played == ply
        T.search_from(model, root, sims, clock)
        out.append(root_row(root, N, c_visit, c_scale))
        if actions[ply] == 0xFF:
            assert ply == recs.shape[0] - 1
            break
        legal = list(state.legal_actions())
        child = root.children[legal.index(int(actions[ply]))]
        state = child.state
        kept = keep_visits is not None and T.keeps(child, state.is_done(), keep_visits)
        root = T.reroot(child) if kept else T.Node(state, 0)
    return np.stack(out)
