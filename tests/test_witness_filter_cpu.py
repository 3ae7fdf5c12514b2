"""Host side of the wall searches (no GPU).  (1) The rule header's host build -- with the one-fill-per-lane search can_reach1_w3 in
wall_keeps_paths' cross-check -- against oracle/quoridor.py, lists and counts exactly, on random play at every board size and on
hand-built positions.  (2) The witness-path filter, a documented experiment that does not ship (tests/hostcheck/witnesscheck.cpp,
DESIGN 4 K3): it must never clear a candidate that a search rejects.  (3) The candidate counts that the GPU layout tests rely on."""
import numpy as np
import pytest

from tests import _util as U
from tests import witness_cases as W


def _same_as_oracle(N, recs):
    from oracle import quoridor as oq
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 72)
    a, c, _ = oq.legal_actions_batch(recs)
    out, cnt = U.hc_legal(N, recs)
    assert np.array_equal(cnt, c)
    for i in range(recs.shape[0]):
        assert np.array_equal(out[i, :c[i]], a[i, :c[i]]), i
        assert (out[i, c[i]:] == -1).all()


@pytest.mark.parametrize("N", [3, 5, 7, 9])
def test_random_play_matches_oracle(N):
    recs = W.random_walk_states(N, 400, seed=100 + N)
    _same_as_oracle(N, recs)
    assert sum(W.wrongly_cleared(N, r) for r in recs) == 0


@pytest.mark.parametrize("N", [5, 9])
def test_hand_built_positions_match_oracle(N):
    pos = W.hand_positions(N)
    # what each position is for, checked on the host build of the filter itself (plain-path bits: 1 mover, 2 enemy)
    pre, post, paths = W.survivors(N, pos["plugged_corridor"])
    assert paths == 0 and post == pre and pre > 0                   # no plain path: the filter is off, every candidate is searched
    for name in ("adjacent_diagonal_jump", "border_path", "last_gap"):
        pre, post, paths = W.survivors(N, pos[name])
        assert paths == 3 and 0 < post < pre, name                   # both paths found, some candidates cleared, some left
    assert W.survivors(N, pos["no_walls_in_hand"])[2] == 3
    from oracle import quoridor as oq
    assert all(a < N * N for a in oq.legal_actions(pos["no_walls_in_hand"]))
    # last_gap: the walls that close the line's only gap are among the survivors and are illegal
    S = N - 1
    legal = set(oq.legal_actions(pos["last_gap"]))
    assert N * N + 1 * S + (S - 1) not in legal                      # H at slot (1, S-1) completes the line
    _same_as_oracle(N, np.stack(list(pos.values())))
    assert sum(W.wrongly_cleared(N, r) for r in pos.values()) == 0


def test_crowded_position_for_the_interleaved_layout():
    """The batch the GPU test uses for the interleaved layout: more than 32 (and at most 64) candidates to search."""
    r32 = W.crowded(9, 32, seed=1)
    assert 32 < W.survivors(9, r32)[0] <= 64
    _same_as_oracle(9, r32)


def test_most_crowded_position():
    """A batch with MORE THAN 64 candidates to search in one position (a second round of the interleaved layout) cannot be built:
    tools/crowded_search.cpp ends at 63 in every run, prefilter alone, and with wall sets that the placement rules would not allow.
    What is checked instead is the fullest single round: 63 candidates, 63 of the 64 task lanes of the interleaved layout."""
    r = W.most_crowded()
    pre, post, paths = W.survivors(9, r)
    assert pre == post == 63 and paths != 3
    assert W.wrongly_cleared(9, r) == 0
    _same_as_oracle(9, r)
