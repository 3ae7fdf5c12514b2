"""GPU tests of the alpha-beta agent's kernels (csrc/agents.hip: aqg_agent_shortest_paths, aqg_agent_alpha_beta) and of the match
that serves its agent with them.  Every comparison is exact: against the reference's recordings (agents_*.npz, ab_walls_*.npz) and
against the native host search (aqg_host_shortest_path, aqg_host_alpha_beta_action) on positions built for the kernel's edges."""

import functools

import numpy as np
import pytest

from tests import _util as U

pytestmark = pytest.mark.gpu

DRAW = {3: 14, 5: 28, 7: 70, 9: 116}
WALLS = {3: 1, 5: 2, 7: 6, 9: 10}
FIXTURES = ["agents_3x3.npz", "agents_5x5.npz", "agents_9x9.npz", "ab_walls_5x5.npz", "ab_walls_9x9.npz"]


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _State():
    from alphaquoridorgnn_amd.game_logic import State
    return State


def _initial(N):
    return _State()(board_size=N, num_walls=WALLS[N]).record()


def _with(rec, **kw):
    """A copy of a record with some fields replaced: ppos, pwl, epos, ewl, plies, walls={slot: 1 (H) / 2 (V)}."""
    r = rec.copy()
    for k, i in (("ppos", 0), ("pwl", 1), ("epos", 2), ("ewl", 3)):
        if k in kw:
            r[i] = kw[k]
    if "plies" in kw:
        r[68], r[69] = kw["plies"] & 0xFF, kw["plies"] >> 8
    for slot, o in kw.get("walls", {}).items():
        r[4 + slot] = o
    return r


def _flipped(rec):
    """The position seen by the other side without a move (agents.py:46-47): the walls rotated, the pawns swapped."""
    N = int(rec[70])
    nw = (N - 1) ** 2
    r = rec.copy()
    r[4:4 + nw] = rec[4:4 + nw][::-1]
    r[0], r[1], r[2], r[3] = rec[2], rec[3], rec[0], rec[1]
    return r


def _walk(N, count, seed):
    """Positions of host random walks from the opening (draws: agents.draw_uniforms(seed, game, .))."""
    from alphaquoridorgnn_amd import agents
    out, game = [], 0
    while len(out) < count:
        s, u = _State()(board_size=N, num_walls=WALLS[N]), agents.draw_uniforms(seed, game, DRAW[N])
        for i in range(DRAW[N]):
            if s.is_done():
                break
            out.append(s.record())
            la = agents._legal(s)
            s = s.next(la[min(len(la) - 1, int(u[i] * len(la)))])
        game += 1
    return np.stack(out[:count])


WALLED_IN_5 = dict(ppos=20, walls={12: 1, 13: 2})      # the mover in the corner (4,0): H at slot (3,0) above it, V at (3,1) beside (4,1)


@functools.lru_cache(maxsize=None)
def _edge_states(N):
    """The positions on which the kernel can go wrong (see the tests below), as a tuple of (label, record)."""
    from alphaquoridorgnn_amd import agents
    V, mid = N * N, N // 2
    start = _initial(N)
    out = [("opening", start),
           ("mover without walls", _with(start, pwl=0)),
           ("other without walls", _with(start, ewl=0)),
           ("mover one step from its goal", _with(start, ppos=N + mid)),
           ("other one step from its goal", _with(start, epos=N + mid)),
           ("both one step from their goals", _with(start, ppos=N + mid - 1, epos=N + mid))]
    for k in (1, 2, 3):
        out.append((f"draw - {k}", _with(start, plies=DRAW[N] - k)))
    if N >= 5:
        me, other = (mid + 1) * N + mid, mid * N + mid                       # the other pawn straight ahead of the mover
        adj = _with(start, ppos=me, epos=V - 1 - other)
        behind = (mid - 1) * (N - 1) + mid                                   # the H slot whose wall closes the edge behind it
        out += [("adjacent", adj), ("adjacent, wall behind", _with(adj, walls={behind: 1}, ewl=WALLS[N] - 1)),
                ("adjacent, wall behind, no walls", _with(adj, walls={behind: 1}, pwl=0, ewl=0))]
        assert any(abs(t % N - mid) == 1 for t in agents._legal(out[-1][1]))                 # the jump has gone diagonal
    else:
        out += [(f"3x3 walk {i}", r) for i, r in enumerate(_walk(3, 12, 33))]                # many root actions tie on 3x3
    if N == 5:
        out.append(("walled in", _with(start, **WALLED_IN_5)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _host_actions(N, depth):
    from alphaquoridorgnn_amd import agents
    return agents.alpha_beta_action_batch(np.stack([r for _, r in _edge_states(N)]), max_depth=depth)


# ---------------------------------------------------------------------------------------------- shortest paths
@pytest.mark.parametrize("name", FIXTURES)
def test_shortest_paths_equal_recordings(dev, name):
    from alphaquoridorgnn_amd import agents
    g = U.golden(name)
    states = g["states"]
    got = agents.shortest_paths_batch(states)
    assert got.dtype == np.int32 and got.shape == (len(states), 2)
    if "paths" in g:
        assert np.array_equal(got, g["paths"].astype(np.int32))
    for i, rec in enumerate(states):
        assert (int(got[i, 0]), int(got[i, 1])) == (agents.shortest_path(rec), agents.shortest_path(_flipped(rec))), (name, i)
    h = agents.heuristic_eval_batch(states)
    assert h.dtype == np.float64 and np.array_equal(h, g["heuristic"])
    assert np.array_equal(h, np.asarray([agents.heuristic_eval(r) for r in states]))


def test_shortest_paths_7x7_walk_and_walled_in(dev):
    from alphaquoridorgnn_amd import agents
    states = _walk(7, 70, 71)[3::4][:16]
    assert len(states) == 16 and (states[:, 4:68] != 0).any()
    got = agents.shortest_paths_batch(states)
    for i, rec in enumerate(states):
        assert (int(got[i, 0]), int(got[i, 1])) == (agents.shortest_path(rec), agents.shortest_path(_flipped(rec))), i
    boxed = _with(_initial(5), **WALLED_IN_5)
    assert agents.shortest_path(boxed) == -1
    both = agents.shortest_paths_batch(np.stack([boxed, _flipped(boxed), _initial(5)]))
    assert both.tolist() == [[-1, 4], [4, -1], [4, 4]]
    for N in (3, 5, 7, 9):
        recs = np.stack([r for _, r in _edge_states(N)])
        got = agents.shortest_paths_batch(recs)
        want = [[agents.shortest_path(r), agents.shortest_path(_flipped(r))] for r in recs]
        assert got.tolist() == want, N


# ---------------------------------------------------------------------------------------------- actions
@pytest.mark.parametrize("name", FIXTURES)
def test_actions_equal_recordings(dev, name):
    from alphaquoridorgnn_amd import agents
    g = U.golden(name)
    states = g["states"]
    assert np.array_equal(agents.alpha_beta_action_batch(states, max_depth=1, backend="hip"), g["ab1"].astype(np.int32))
    deep = g["ab2_index"] if "ab2_index" in g else np.arange(len(states))
    assert np.array_equal(agents.alpha_beta_action_batch(states[deep], max_depth=2, backend="hip"), g["ab2"].astype(np.int32))


@pytest.mark.parametrize("N,depth", [(N, d) for N in (3, 5, 7, 9) for d in (0, 1, 2)] + [(3, 3), (5, 3)])
def test_actions_equal_host_on_the_edges(dev, N, depth):
    """The opening (9x9: 131 legal actions, three rounds of 64 lanes and one action past 128; 7x7: 75, two rounds; 5x5 and 3x3: one
    round), one side without walls, a pawn one step from its goal (a loss inside the tree), the draw limit inside the tree,
    adjacent pawns with and without a wall behind, 3x3 positions where many root actions tie, a walled-in mover."""
    from alphaquoridorgnn_amd import agents
    edges = _edge_states(N)
    recs = np.stack([r for _, r in edges])
    counts = {label: len(agents._legal(r)) for label, r in edges}
    assert counts["opening"] == {3: 11, 5: 35, 7: 75, 9: 131}[N]
    got = agents.alpha_beta_action_batch(recs, max_depth=depth, backend="hip")
    want = _host_actions(N, depth)
    for i, (label, _) in enumerate(edges):
        assert int(got[i]) == int(want[i]), (N, depth, label, counts[label])


def test_sentinel_and_no_action(dev):
    """A mover without a legal action gives -1, as the host does; so does every depth."""
    from alphaquoridorgnn_amd import agents
    # 3x3, the mover in the corner (2,0) under an H wall at slot (1,0); the other pawn beside it on (2,1) with a V wall at (1,1) behind:
    # no step, no jump, no wall in hand
    rec = _with(_initial(3), ppos=6, pwl=0, epos=8 - 7, ewl=0, walls={2: 1, 3: 2})
    assert agents._legal(rec) == []
    for depth in (0, 1, 2):
        host = agents.alpha_beta_action_batch(rec[None], max_depth=depth)
        assert int(host[0]) == -1
        assert np.array_equal(agents.alpha_beta_action_batch(np.stack([rec, _initial(3)]), max_depth=depth, backend="hip"),
                              agents.alpha_beta_action_batch(np.stack([rec, _initial(3)]), max_depth=depth))


# ---------------------------------------------------------------------------------------------- batch shapes
@functools.lru_cache(maxsize=None)
def _mixed_70():
    from alphaquoridorgnn_amd import agents
    pool = list(U.golden("ab_walls_5x5.npz")["states"]) + list(U.golden("agents_5x5.npz")["states"]) + [r for _, r in _edge_states(5)]
    recs = np.stack([pool[(7 * i) % len(pool)] for i in range(70)])
    return recs, agents.alpha_beta_action_batch(recs, max_depth=2)


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 70])
def test_batch_shapes(dev, B):
    from alphaquoridorgnn_amd import agents
    recs, want = _mixed_70()
    assert np.array_equal(agents.alpha_beta_action_batch(recs[:B], max_depth=2, backend="hip"), want[:B])


def test_empty_batch_and_active_mask(dev):
    import torch
    from alphaquoridorgnn_amd import agents
    empty = agents.alpha_beta_action_batch(np.zeros((0, 72), np.uint8), backend="hip")
    assert empty.shape == (0,) and empty.dtype == np.int32
    none = agents.alpha_beta_action_device(torch.zeros((0, 72), dtype=torch.uint8, device=dev), 5)
    assert none.shape == (0,) and none.dtype == torch.int32
    recs, want = _mixed_70()
    d = torch.from_numpy(recs).to(dev)
    active = torch.ones((70,), dtype=torch.uint8, device=dev)
    masked = [0, 3, 63, 64, 69]
    active[masked] = 0
    garbage = d.clone()
    garbage[masked] = 0xEE                                  # what a masked slot holds is never read as a position
    got = agents.alpha_beta_action_device(garbage, 5, 2, active=active).cpu().numpy()
    expect = want.copy()
    expect[masked] = 0
    assert np.array_equal(got, expect)
    with pytest.raises(ValueError, match="active"):
        agents.alpha_beta_action_device(d, 5, 2, active=active.to(torch.int32))


def test_same_call_twice_same_bytes(dev):
    import torch
    from alphaquoridorgnn_amd import agents
    recs, want = _mixed_70()
    d = torch.from_numpy(recs).to(dev)
    a1, n1 = agents.alpha_beta_action_device(d, 5, 2, return_nodes=True)
    a2, n2 = agents.alpha_beta_action_device(d, 5, 2, return_nodes=True)
    assert np.array_equal(a1.cpu().numpy(), want)
    assert a1.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes()
    assert n1.dtype == torch.int64 and n1.cpu().numpy().tobytes() == n2.cpu().numpy().tobytes()
    counts = np.asarray([len(agents._legal(r)) for r in recs])
    assert (n1.cpu().numpy() >= counts).all()              # every root child is a position visited
    nine = torch.from_numpy(np.stack([_initial(9), _with(_initial(9), pwl=0)])).to(dev)
    b1, m1 = agents.alpha_beta_action_device(nine, 9, 2, return_nodes=True)
    b2, m2 = agents.alpha_beta_action_device(nine, 9, 2, return_nodes=True)
    assert torch.equal(b1, b2) and torch.equal(m1, m2)


# ---------------------------------------------------------------------------------------------- the match
def _records_of(match):
    return [tuple(eng.t[n].cpu().numpy().copy() for n in ("hist_state72", "hist_action", "game_plies", "game_result", "game_done"))
            for eng in match.engines]


@pytest.mark.parametrize("N,games", [(5, 6), (9, 2)])
def test_match_hip_equals_host(dev, N, games):
    from alphaquoridorgnn_amd.evaluate_agents import BatchedAgentMatch
    played = {}
    for backend in ("hip", "host"):
        m = BatchedAgentMatch(7, "alpha_beta", games, sims=16, board_size=N, evaluator="fake", agent_kwargs={"backend": backend})
        played[backend] = (m.play(), _records_of(m))
    assert played["hip"][0] == played["host"][0]
    for ea, eb in zip(played["hip"][1], played["host"][1]):
        assert np.array_equal(ea[2], eb[2]) and np.array_equal(ea[3], eb[3]) and np.array_equal(ea[4], eb[4])
        assert ea[4].all()
        for k, n in enumerate(ea[2]):
            assert np.array_equal(ea[0][k, :n], eb[0][k, :n]) and np.array_equal(ea[1][k, :n], eb[1][k, :n])
