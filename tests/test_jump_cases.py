"""GPU tests of the pawn rule on every device path, jump class by jump class (tests/golden/jumps_NxN.npz, tests/_jump_cases.py): the
wave list of csrc/legal_wave.hpp behind aqg_legal_actions, the transition and status kernels, the MCTS step kernel's expansion from
both of its call sites (evaluation cache off / on), the jump-aware flood fills behind wall legality and behind
agent_shortest_paths_kernel, the alpha-beta, playout and rollout-MCTS kernels of csrc/agents.hip, and the mirror.  Every comparison is
exact: against the reference's recordings, the C oracle, or the host build of the same rules (tests/test_jump_cases_cpu.py pins those
three to each other on the same cases).

"One per class" is Cases.one_per_class: the first live state of each class of family A with the mover off row 0, and of each class
present in family B; every test that uses it asserts how many classes it holds (tests/_jump_cases.ONE_PER_CLASS)."""
import numpy as np
import pytest
import torch

from tests import _jump_cases as J
from tests._agent_replay import _check_mcts, _check_playouts

pytestmark = pytest.mark.gpu

ONE_BELOW = float(np.nextafter(1.0, 0.0))
MCTS_CHUNK = 14              # 9x9 roots per case of the rollout-MCTS test: the host replay of one costs a quarter of a second


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _one_per_class(N):
    c = J.cases(N)
    assert c.one_per_class_counts == J.ONE_PER_CLASS[N] and len(c.one_per_class) == sum(J.ONE_PER_CLASS[N])
    return c, c.one_per_class


def _legal_on_device(dev, N, recs):
    """(mask, order as int16 with -1 for 0xFF, count) of a batch, as numpy arrays."""
    from alphaquoridorgnn_amd import game_logic as gl
    mask, order, count = gl.legal_actions_batch(torch.from_numpy(np.ascontiguousarray(recs)).to(dev), N)
    order = order.cpu().numpy().astype(np.int16)
    order[order == 255] = -1
    return mask.cpu().numpy(), order, count.cpu().numpy()


def _padded(lists, keep):
    out = lists.copy()
    out[np.arange(out.shape[1])[None, :] >= np.asarray(keep)[:, None]] = -1
    return out


def _mask_of(lists, A):
    m = np.zeros((len(lists), A + 1), dtype=np.uint8)
    m[np.arange(len(lists))[:, None], np.where(lists >= 0, lists, A)] = 1
    return m[:, :A]


# ---------------------------------------------------------------------------------------------- 1. the legal list
@pytest.mark.parametrize("N", [3, 5, 9])
def test_legal_actions_equal_fixture(dev, N):
    """The whole file as one shuffled batch: mask, ordered list (0xFF past the count) and count; then with no wall in the mover's
    hand: the pawn prefix alone."""
    c = J.cases(N)
    A = N * N + 2 * (N - 1) ** 2
    perm = np.random.RandomState(N).permutation(len(c.states))
    mask, order, count = _legal_on_device(dev, N, c.states[perm])
    assert np.array_equal(count, c.counts[perm])
    assert np.array_equal(order, c.legal[perm])
    assert mask.shape == (len(perm), A) and np.array_equal(mask, c.mask()[perm])
    bare = c.states[perm].copy()
    bare[:, 1] = 0
    want = _padded(c.legal, c.npawn)[perm]
    mask, order, count = _legal_on_device(dev, N, bare)
    assert np.array_equal(count, c.npawn[perm]) and np.array_equal(order, want) and np.array_equal(mask, _mask_of(want, A))


def test_legal_actions_7x7_equal_oracle(dev):
    """No reference constants for 7x7: the same enumeration (68 classes: tests/test_jump_cases_cpu.py) against the oracle."""
    from oracle import quoridor as oq
    N, A = 7, 121
    recs = J.enumerate_family_a(N)
    perm = np.random.RandomState(7).permutation(len(recs))
    for bare in (False, True):
        batch = recs[perm].copy()
        if bare:
            batch[:, 1] = 0
        a, cnt, m = oq.legal_actions_batch(batch)
        want = _padded(a[:, :136], cnt)
        mask, order, count = _legal_on_device(dev, N, batch)
        assert np.array_equal(count, cnt) and np.array_equal(order, want) and np.array_equal(mask, m[:, :A])
        if bare:
            assert [order[i, :count[i]].tolist() for i in range(len(batch))] == [J.pawn_moves(r) for r in batch]


# ---------------------------------------------------------------------------------------------- 2. transitions and flags
@pytest.mark.parametrize("N", [3, 5, 7, 9])
def test_next_and_status_on_every_pawn_action(dev, N):
    from alphaquoridorgnn_amd import game_logic as gl
    from oracle import quoridor as oq
    if N == 7:
        recs = J.enumerate_family_a(N)
        a, cnt, _ = oq.legal_actions_batch(recs)
        legal = _padded(a[:, :136], cnt)
        status = oq.status_batch(recs, J.DRAW[N])
    else:
        c = J.cases(N)
        recs, legal, status = c.states, c.legal, c.status
    rows, cols = np.nonzero((legal >= 0) & (legal < N * N))
    acts = legal[rows, cols].astype(np.int32)
    assert len(rows) == int(J.pawn_count(N, legal).sum()) > len(recs)
    d = torch.from_numpy(np.ascontiguousarray(recs[rows])).to(dev)
    got = gl.next_batch(d, torch.from_numpy(acts), N).cpu().numpy()
    assert np.array_equal(got, oq.next_batch(recs[rows], acts))
    assert np.array_equal(got, J.pawn_next(recs[rows], acts))
    assert np.array_equal(gl.status_batch(torch.from_numpy(recs).to(dev), N, J.DRAW[N]).cpu().numpy(), status)
    assert (status & 1).any() and not (status & 2).any()                     # lost positions are among them; 4 plies are no draw


# ---------------------------------------------------------------------------------------------- 3. the State API
@pytest.mark.parametrize("N", [3, 5, 9])
def test_state_api_on_one_state_per_class(dev, N):
    """State.legal_actions() and State.legal_actions_pos(pos) launch the same kernel on a rewritten record.  One per class, and the
    first state of each of the 68 classes whatever its status (the lists are defined on lost positions too)."""
    from alphaquoridorgnn_amd.game_logic import State
    c, picked = _one_per_class(N)
    every = np.union1d(picked, c.first_of_class)
    assert {c.cls[i] for i in every if c.family[i] == 0} == J.ALL_CLASSES
    for i in every:
        s = State.from_record(c.states[i])
        assert s.legal_actions() == c.legal[i, :c.counts[i]].tolist(), (N, i, c.cls[i])
        assert s.legal_actions_pos(int(c.states[i, 0])) == c.legal[i, :c.npawn[i]].tolist(), (N, i, c.cls[i])


# ---------------------------------------------------------------------------------------------- 4. the step kernel, lock-step
@pytest.mark.parametrize("N", [5, 9])
def test_search_equals_oracle_search(dev, N):
    """Thirty simulations from each root walk children in which the pawns still touch or have just jumped."""
    from alphaquoridorgnn_amd.pv_mcts import pv_mcts_policy_batch
    from oracle import mcts as om, quoridor as oq
    c, picked = _one_per_class(N)
    roots = c.states[picked]
    pols = pv_mcts_policy_batch(None, roots, 1.0, sims=30, board_size=N, evaluator="fake", fake_bias=11)
    for b, i in enumerate(picked):
        ref = om.pv_mcts_policy(om.FakeModel(11), oq.State(roots[b]), 1.0, 30)
        assert len(pols[b]) == c.counts[i] and np.array_equal(np.asarray(pols[b]), np.asarray(ref)), (N, i, c.cls[i])


# ---------------------------------------------------------------------------------------------- 5. both call sites of the wave list
def _gnn_search(dev, roots, step_heads, slots):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    from oracle import gnn as og
    model = GNNNetwork()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in og.init_params(3).items()})
    _lib.set_option("step_heads", step_heads)
    try:
        eng = BatchedSelfPlay(model.to(dev).eval(), num_games=len(roots), sims=30, seed=11, record_history=False, eval_cache_slots=slots)
        assert eng.eval_cache_slots == (slots or 0)
        out = tuple(x.cpu().numpy() for x in eng.search(roots))
        if slots:                              # the same roots again: the same tree, now expanded from the table's rows (64 entries
            again = tuple(x.cpu().numpy() for x in eng.search(roots))         # per game hold the 30 leaves of the first search)
            assert all(np.array_equal(x, y) for x, y in zip(out, again))
        return out, eng.counters()
    finally:
        _lib.set_option("step_heads", 1)


def test_search_with_and_without_the_evaluation_cache(dev):
    """The step kernel builds a leaf's list from two places, by whether the evaluation cache is on, and with the cache on a repeated
    leaf takes its list from the table.  83 roots, 8 games per workgroup: every workgroup mixes classes."""
    c, picked = _one_per_class(9)
    roots = c.states[picked]
    runs = {(heads, slots): _gnn_search(dev, roots, heads, slots) for heads in (1, 0) for slots in (None, 64)}
    first = runs[(1, None)][0]
    for key, ((visits, actions, count), counters) in runs.items():
        assert np.array_equal(count, c.counts[picked]), key
        lists = actions.astype(np.int16)
        lists[lists == 255] = -1
        assert np.array_equal(lists, c.legal[picked]), key
        assert (visits.sum(1) > 0).all() and counters["leaf_evals"] > 0
        assert np.array_equal(visits, first[0]), key
    assert runs[(1, 64)][1]["cache_hits"] > 0 and runs[(0, 64)][1]["cache_hits"] > 0


# ---------------------------------------------------------------------------------------------- 6. shortest paths
@pytest.mark.parametrize("N", [3, 5, 9])
def test_shortest_paths_equal_fixture(dev, N):
    from alphaquoridorgnn_amd import agents
    c = J.cases(N)
    got = agents.shortest_paths_batch(c.states)
    assert got.dtype == np.int32 and np.array_equal(got, c.paths.astype(np.int32))
    assert (got == -1).any()
    h = agents.heuristic_eval_batch(c.states)
    p = c.paths.astype(np.int64)
    assert h.dtype == np.float64 and np.array_equal(h, (p[:, 1] - p[:, 0]) / np.float64(J.DRAW[N] // 2 - J.WALLS[N]))
    for i in np.union1d(c.one_per_class, np.flatnonzero((c.paths < 0).any(1))):
        assert h[i] == agents.heuristic_eval(c.states[i]), (N, i)


# ---------------------------------------------------------------------------------------------- 7. alpha-beta
@pytest.mark.parametrize("N,depth", [(9, 1), (5, 1), (5, 2), (3, 1), (3, 2)])
def test_alpha_beta_equals_host(dev, N, depth):
    from alphaquoridorgnn_amd import agents
    c, picked = _one_per_class(N)
    recs = c.states[picked]
    got = agents.alpha_beta_action_batch(recs, max_depth=depth, backend="hip")
    want = agents.alpha_beta_action_batch(recs, max_depth=depth, backend="host")
    for b, i in enumerate(picked):
        assert int(got[b]) == int(want[b]), (N, depth, i, c.cls[i])


# ---------------------------------------------------------------------------------------------- 8. playouts, rollout MCTS
@pytest.mark.parametrize("N", [3, 5, 9])
def test_playouts_equal_host_replay(dev, N):
    from alphaquoridorgnn_amd import agents
    c, picked = _one_per_class(N)
    states = c.states[picked]
    tables = np.stack([agents.draw_uniforms(1700 + N, b, J.DRAW[N]) for b in range(len(states))])
    tables[::5, ::3] = 0.0
    tables[1::5, 1::4] = ONE_BELOW
    got = agents.playout_batch(states, uniforms=tables, return_final=True)
    _check_playouts(N, states, tables, got)


@pytest.mark.parametrize("N,chunk", [(5, None)] + [(9, k) for k in range(-(-sum(J.ONE_PER_CLASS[9]) // MCTS_CHUNK))])
def test_rollout_mcts_equals_host_tree(dev, monkeypatch, N, chunk):
    """(3x3 is left to the playout test: a random playout from some of its jump positions reaches a mover without a legal action,
    where the reference's mcts_action raises.)"""
    from alphaquoridorgnn_amd import agents
    c, picked = _one_per_class(N)
    rows = np.arange(len(picked)) if chunk is None else np.arange(len(picked))[chunk * MCTS_CHUNK:(chunk + 1) * MCTS_CHUNK]
    assert len(rows) > 0
    states, E = c.states[picked[rows]], 100
    tables = np.stack([agents.draw_uniforms(1800 + N, int(b), E * J.DRAW[N]) for b in rows])
    got = agents.mcts_action_batch(states, evaluations=E, uniforms=tables, return_visits=True)
    _check_mcts(monkeypatch, N, states, tables, E, got, need_expansion=False)


# ---------------------------------------------------------------------------------------------- 9. the mirror
@pytest.mark.parametrize("N", [5, 9])
def test_mirror_permutes_the_legal_mask(dev, N):
    from alphaquoridorgnn_amd import game_logic as gl
    c = J.cases(N)
    a = c.family == 0
    A = N * N + 2 * (N - 1) ** 2
    d = torch.from_numpy(np.ascontiguousarray(c.states[a])).to(dev)
    mirrored = gl.mirror_batch(d, N)
    assert np.array_equal(mirrored.cpu().numpy(), gl.mirror_record(c.states[a]))
    mask, _, count = gl.legal_actions_batch(mirrored, N)
    want = np.zeros((int(a.sum()), A), dtype=np.uint8)
    want[:, gl.mirror_actions(np.arange(A), N)] = c.mask()[a]
    assert np.array_equal(mask.cpu().numpy(), want) and np.array_equal(count.cpu().numpy(), c.counts[a])
    assert {J.classify(r) for r in mirrored.cpu().numpy()} == J.ALL_CLASSES   # the mirror maps the set of classes onto itself
