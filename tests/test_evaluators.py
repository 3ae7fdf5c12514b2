"""GPU test of the evaluator bindings' pointing (alphaquoridorgnn_amd/evaluators.py): BatchedMatch points each engine at the
mover's weights before every ply; every position a match recorded must have been searched with exactly the mover's network."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_cnn import _make_net as _cnn   # noqa: E402
from tests.test_gnn_any_shape import _make_net as _gnn   # noqa: E402

pytestmark = pytest.mark.gpu

N, SIMS, GAMES, SEED = 5, 8, 4, 11
A = N * N + 2 * (N - 1) ** 2      # 57: the policy head every player of a 5x5 match must have (the engine refuses another)


def _players(kind):
    if kind == "gnn":          # the default trunk with the 5x5 head: the fused kernels, two initialisations
        return _gnn((6, 128, 3), A, seed=1, N=N), _gnn((6, 128, 3), A, seed=2, N=N)
    if kind == "general":
        return _gnn((6, 32, 2), A, seed=3, N=N), _gnn((6, 64, 1), A, seed=4, N=N)
    return _cnn(16, 1, N, seed=5).to("cuda"), _cnn(24, 2, N, seed=6).to("cuda")


@pytest.mark.parametrize("kind", ["gnn", "general", "cnn"])
def test_match_searches_every_ply_with_the_movers_network(kind):
    """Two games per first-mover engine, so both engines exist and the pointing alternates on each.  The visit counts recorded at
    every ply equal -- exactly: a game's searches are bit-identical whatever else is in the batch -- those of
    an engine that was built with the mover's model alone and is never re-pointed."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    players = _players(kind)
    match = BatchedMatch(players, GAMES, sims=SIMS, board_size=N, evaluator=kind, seed=SEED)
    points = match.play()
    assert len(points) == GAMES and all(e is not None and e.G == 2 for e in match.engines)
    alone = [BatchedSelfPlay(m, num_games=1, sims=SIMS, board_size=N, evaluator=kind, record_history=False) for m in players]
    for first, eng in enumerate(match.engines):
        c = eng.counters()
        assert c["finished"] == 2 and c["active"] == 0
        if kind == "gnn":      # a silent fallback to the exact kernels would make the comparison vacuous
            assert c["gnn_saturated"] == 0 and not any(f & _lib.GNN_EXACT_F32 for f in match._flags)
        plies = eng.t["game_plies"].cpu().numpy()
        assert plies.max() >= 3
        hs, hv = eng.t["hist_state72"].cpu().numpy(), eng.t["hist_visits"].cpu().numpy()
        for k in range(2):
            for ply in range(int(plies[k])):
                visits, actions, count = (x.cpu().numpy() for x in alone[(first + ply) % 2].search(hs[k, ply:ply + 1]))
                dense = np.zeros(A, dtype=np.int64)
                dense[actions[0, :count[0]]] = visits[0, :count[0]]
                assert dense.sum() > 0 and np.array_equal(hv[k, ply].astype(np.int64), dense), (first, k, ply)
    if kind == "gnn":
        assert not any(e.e.gnn_flags & _lib.GNN_EXACT_F32 for e in alone)
