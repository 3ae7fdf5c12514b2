"""CPU tests of the pawn-jump fixtures tests/golden/jumps_NxN.npz (tools/gen_golden_jumps.py: the reference's own lists, paths and
flags on every jump class, case by case): the fixtures hold what they promise, and the C oracle, the host build of the rule header
(csrc/quoridor_core.hpp) and the host agents (csrc/host_agents.cpp) reproduce them bit for bit.  tests/test_jump_cases.py runs the
same cases through the kernels."""
import numpy as np
import pytest

from tests import _jump_cases as J
from tests import _util as U

BOARDS = [3, 5, 9]
FAMILY_A = {3: 156, 5: 940, 9: 4524}
FAMILY_B = {3: 0, 5: 432, 9: 1869}


@pytest.mark.parametrize("N", BOARDS)
def test_fixture_holds_every_class(N):
    """The classifier and the pawn rule of tests/_jump_cases.py read the walls as blocked edges, on their own."""
    c = J.cases(N)
    a = c.family == 0
    assert int(a.sum()) == FAMILY_A[N] and int((~a).sum()) == FAMILY_B[N] and not a[FAMILY_A[N]:].any()
    assert c.states.dtype == np.uint8 and c.legal.dtype == np.int16 and c.counts.dtype == np.int32 and c.paths.dtype == np.int16
    assert (c.states[:, 70] == N).all() and (c.legal.shape[1], c.paths.shape[1]) == (136, 2)
    in_a = [c.cls[i] for i in np.flatnonzero(a)]
    assert None not in in_a and set(in_a) == J.ALL_CLASSES                     # 68 of 68
    assert sorted(set(c.npawn[a].tolist())) == [0, 1, 2, 3, 4, 5]
    assert (c.paths[a] == -1).any() and (c.paths >= -1).all()
    assert (c.paths[~a] >= 0).all()                                            # family B was filtered on it
    assert np.array_equal(J.enumerate_family_a(N), c.states[a])                # the tests' enumerator is the generator's
    assert c.one_per_class_counts == J.ONE_PER_CLASS[N]
    assert len(c.first_of_class) == 68
    assert np.array_equal(c.counts, (c.legal >= 0).sum(1))
    assert np.array_equal(c.status, ((c.states[:, 2] < N) * 1 + ((c.states[:, 68] | (c.states[:, 69].astype(int) << 8)) >= J.DRAW[N]) * 2))
    for i, rec in enumerate(c.states):
        assert J.pawn_moves(rec) == c.legal[i, :c.npawn[i]].tolist(), (N, i, c.cls[i])
        assert (c.legal[i, c.npawn[i]:c.counts[i]] >= N * N).all() and (c.legal[i, c.counts[i]:] == -1).all()


def test_seven_by_seven_enumeration_holds_every_class():
    recs = J.enumerate_family_a(7)
    assert {J.classify(r) for r in recs} == J.ALL_CLASSES
    assert sorted({len(J.pawn_moves(r)) for r in recs}) == [0, 1, 2, 3, 4, 5]


def _pawn_pairs(c):
    """(state index, action) of every legal pawn action of every state."""
    rows, cols = np.nonzero((c.legal >= 0) & (c.legal < c.N * c.N))
    return rows, c.legal[rows, cols].astype(np.int32)


@pytest.mark.parametrize("N", BOARDS)
def test_oracle_and_rule_header_equal_fixture(N):
    from oracle import quoridor as oq
    c = J.cases(N)
    a, cnt, mask = oq.legal_actions_batch(c.states)
    assert np.array_equal(cnt, c.counts)
    want = c.legal.copy()
    got = a[:, :136].copy()
    got[np.arange(136)[None, :] >= cnt[:, None]] = -1
    assert np.array_equal(got, want)
    A = N * N + 2 * (N - 1) ** 2
    assert np.array_equal(mask[:, :A], c.mask()) and not mask[:, A:].any()
    h, hcnt = U.hc_legal(N, c.states)
    h[np.arange(136)[None, :] >= hcnt[:, None]] = -1
    assert np.array_equal(hcnt, c.counts) and np.array_equal(h, want)
    assert np.array_equal(oq.status_batch(c.states, J.DRAW[N]), c.status)
    assert np.array_equal(U.hc_status(N, c.states, J.DRAW[N]), c.status)
    rows, acts = _pawn_pairs(c)
    assert len(rows) == int(c.npawn.sum())
    want_next = J.pawn_next(c.states[rows], acts)
    assert np.array_equal(oq.next_batch(c.states[rows], acts), want_next)
    assert np.array_equal(U.hc_next(N, c.states[rows], acts), want_next)


@pytest.mark.parametrize("N", BOARDS)
def test_no_walls_in_hand_leaves_the_pawn_prefix(N):
    from oracle import quoridor as oq
    c = J.cases(N)
    recs = c.states.copy()
    recs[:, 1] = 0
    want = c.legal.copy()
    want[np.arange(136)[None, :] >= c.npawn[:, None]] = -1
    a, cnt, _ = oq.legal_actions_batch(recs)
    got = a[:, :136].copy()
    got[np.arange(136)[None, :] >= cnt[:, None]] = -1
    assert np.array_equal(cnt, c.npawn) and np.array_equal(got, want)
    h, hcnt = U.hc_legal(N, recs)
    h[np.arange(136)[None, :] >= hcnt[:, None]] = -1
    assert np.array_equal(hcnt, c.npawn) and np.array_equal(h, want)


@pytest.mark.parametrize("N", BOARDS)
def test_host_paths_and_heuristic_equal_fixture(N):
    from alphaquoridorgnn_amd import agents
    c = J.cases(N)
    flip = J.flipped(c.states)
    max_dist = J.DRAW[N] // 2 - J.WALLS[N]
    for i, rec in enumerate(c.states):
        assert (agents.shortest_path(rec), agents.shortest_path(flip[i])) == (int(c.paths[i, 0]), int(c.paths[i, 1])), (N, i, c.cls[i])
        assert agents.heuristic_eval(rec) == (int(c.paths[i, 1]) - int(c.paths[i, 0])) / max_dist, (N, i)
    # the host agents' own legal lists (csrc/host_agents.cpp) on one state per class, lost ones and the mover on row 0 included
    for i in np.concatenate([c.first_of_class, c.one_per_class]):
        assert agents._legal(c.states[i]) == c.legal[i, :c.counts[i]].tolist(), (N, i, c.cls[i])
