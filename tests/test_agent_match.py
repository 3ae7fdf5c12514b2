"""GPU tests of the batched baseline agents (csrc/agents.hip) and of the network-vs-agent match built on them
(evaluate_agents.BatchedAgentMatch).  Every comparison is exact: the kernels against a host replay by the reference-pinned rules
(agents._legal + State.next) and against agents._Tree, driven by the same tables of uniforms."""

import numpy as np
import pytest
import torch

from tests import _util as U
from tests._agent_replay import _State, _TableDraw, _check_mcts, _check_playouts, _pick

pytestmark = pytest.mark.gpu

DRAW = {3: 14, 5: 28, 7: 70, 9: 116}
WALLS = {3: 1, 5: 2, 7: 6, 9: 10}
ONE_BELOW = float(np.nextafter(1.0, 0.0))       # the largest double below 1


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _initial(N):
    return _State()(board_size=N, num_walls=WALLS[N]).record()


def _walk_7x7(count):
    """7x7 has no fixture: positions of host random walks from the initial position (draws: agents.draw_uniforms(70, game, .))."""
    from alphaquoridorgnn_amd import agents
    out, game = [], 0
    while len(out) < count:
        s, u = _State()(board_size=7, num_walls=WALLS[7]), agents.draw_uniforms(70, game, DRAW[7])
        for i in range(DRAW[7]):
            if s.is_done():
                break
            out.append(s.record())
            s = s.next(_pick(agents._legal(s), u[i]))
        game += 1
    return np.stack(out[:count])


def _special(rec, N):
    """An already lost state, an already drawn state and a state one ply from the draw limit, made from a live record."""
    lost, drawn, last = rec.copy(), rec.copy(), rec.copy()
    lost[2] = N // 2                                             # the enemy stands on its goal row: the mover has lost
    drawn[68], drawn[69] = DRAW[N] & 0xFF, DRAW[N] >> 8
    last[68], last[69] = (DRAW[N] - 1) & 0xFF, (DRAW[N] - 1) >> 8
    return [lost, drawn, last]


def _states(N, walk_count):
    """agents_NxN states + the initial position + `walk_count` states of walk_NxN.npz at a fixed stride (len // walk_count)
    + the three special states; 7x7: the initial position, host walks and the special states."""
    if N == 7:
        w = _walk_7x7(walk_count + 30)
        return np.stack([_initial(7)] + list(w) + _special(w[5], 7))
    a = U.golden(f"agents_{N}x{N}.npz")["states"]
    w = U.golden(f"walk_{N}x{N}.npz")["states"]
    stride = len(w) // walk_count
    ws = w[::stride][:walk_count]
    return np.stack(list(a) + [_initial(N)] + list(ws) + _special(ws[walk_count // 2], N))


# ---------------------------------------------------------------------------------------------- 6. random
@pytest.mark.parametrize("N", [3, 5, 9])
def test_random_action_equals_host_pick(dev, N):
    """Every 7th state of walk_NxN.npz (3x3: every state), each with a uniform from a cycle holding 0, the largest double below 1,
    the k / count boundaries of the state's own count (and their neighbours below), and generator draws."""
    from alphaquoridorgnn_amd import agents
    g = U.golden(f"walk_{N}x{N}.npz")
    states = g["states"] if N == 3 else g["states"][::7]
    counts = g["counts"] if N == 3 else g["counts"][::7]
    legal = g["legal"] if N == 3 else g["legal"][::7]
    extra = agents.draw_uniforms(6, N, len(states))
    u = np.empty(len(states), dtype=np.float64)
    for i, c in enumerate(counts):
        c, k = int(c), i // 6
        u[i] = [0.0, ONE_BELOW, (k % c) / c, float(np.nextafter(((k % c) + 1) / c, 0.0)), (c - 1) / c, extra[i]][i % 6]
    got = agents.random_action_batch(states, uniforms=u)
    for i in range(len(states)):
        c = int(counts[i])
        la = [int(x) for x in legal[i, :c]]
        if i % 97 == 0:
            assert la == agents._legal(states[i])
        assert int(got[i]) == la[min(c - 1, int(u[i] * c))], (N, i, u[i])


# ---------------------------------------------------------------------------------------------- 7. playouts
@pytest.mark.parametrize("N", [3, 5, 7, 9])
def test_playouts_equal_host_replay(dev, N):
    """>= 64 states per board size: see _states (walk stride = len // 48)."""
    from alphaquoridorgnn_amd import agents
    states = _states(N, 48)
    assert len(states) >= 64
    tables = np.stack([agents.draw_uniforms(700 + N, b, DRAW[N]) for b in range(len(states))])
    tables[::5, ::3] = 0.0
    tables[1::5, 1::4] = ONE_BELOW
    got = agents.playout_batch(states, uniforms=tables, return_final=True)
    _check_playouts(N, states, tables, got)
    n = len(states)
    assert int(got[2][n - 3]) == 0 and int(got[0][n - 3]) == -1 and int(got[1][n - 3]) == 0      # already lost
    assert int(got[2][n - 2]) == 0 and int(got[0][n - 2]) == 0                                   # already drawn
    assert int(got[1][n - 1]) == 1                                                               # one ply from the draw limit
    # 9. the generator path equals the table path fed from agents.draw_uniforms
    gen = agents.playout_batch(states, seed=4242 + N, return_final=True)
    tab = agents.playout_batch(states, uniforms=np.stack([agents.draw_uniforms(4242 + N, b, DRAW[N]) for b in range(n)]),
                               return_final=True)
    for x, y in zip(gen, tab):
        assert np.array_equal(x, y)
    again = agents.playout_batch(states, seed=4242 + N, return_final=True)
    for x, y in zip(gen, again):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="draws"):
        agents.playout_batch(_initial(N)[None], uniforms=np.zeros((1, 1)))


# ---------------------------------------------------------------------------------------------- 8. rollout MCTS
def _mcts_states(N):
    a = U.golden(f"agents_{N}x{N}.npz")["states"]
    w = U.golden(f"walk_{N}x{N}.npz")["states"]
    ws = w[::len(w) // 16][:16]                                  # 16 walk states at stride len // 16
    return np.stack(list(a) + [_initial(N)] + list(ws))


@pytest.mark.parametrize("N,E", [(3, 100), (5, 100), (9, 100), (3, 400), (5, 400)])
def test_mcts_equals_host_tree(dev, monkeypatch, N, E):
    from alphaquoridorgnn_amd import agents
    states = _mcts_states(N)
    B, n = len(states), E * DRAW[N]
    tables = np.stack([agents.draw_uniforms(800 + N + E, b, n) for b in range(B)])
    got = agents.mcts_action_batch(states, evaluations=E, uniforms=tables, return_visits=True)
    _check_mcts(monkeypatch, N, states, tables, E, got, need_expansion=(E == 400))
    # 9. the generator path equals the table path fed from agents.draw_uniforms
    gen = agents.mcts_action_batch(states, evaluations=E, seed=800 + N + E, return_visits=True)
    for x, y in zip(gen, got):
        assert np.array_equal(x, y)
    assert np.array_equal(agents.mcts_action_batch(states, evaluations=E, seed=800 + N + E), got[0])


@pytest.mark.parametrize("N", [5, 9])
def test_mcts_answer_does_not_depend_on_the_batch(dev, N):
    """A state's answer alone == at position 37 of a batch of 64 (same table of draws)."""
    from alphaquoridorgnn_amd import agents
    states = _mcts_states(N)
    E, n = 100, 100 * DRAW[N]
    batch = np.stack([states[i % len(states)] for i in range(64)])
    tables = np.stack([agents.draw_uniforms(900 + N, b, n) for b in range(64)])
    full = agents.mcts_action_batch(batch, evaluations=E, uniforms=tables, return_visits=True)
    alone = agents.mcts_action_batch(batch[37:38], evaluations=E, uniforms=tables[37:38], return_visits=True)
    for x, y in zip(full, alone):
        assert np.array_equal(x[37], y[0])
    again = agents.mcts_action_batch(batch, evaluations=E, uniforms=tables, return_visits=True)
    for x, y in zip(full, again):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------- 10. applying moves
@pytest.mark.parametrize("N", [5, 9])
def test_apply_actions_replays_recorded_games(dev, N):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.evaluate_agents import first_player_point
    State = _State()
    g = U.golden(f"eval_{N}x{N}.npz")
    games = [[int(a) for a in g[f"e{i}_actions"]] for i in range(int(g["count"][0]))]
    G, A = len(games), N * N + 2 * (N - 1) ** 2
    eng = BatchedSelfPlay(None, num_games=G, sims=4, board_size=N, evaluator="fake")
    chain = [State(board_size=N, num_walls=WALLS[N]) for _ in range(G)]
    recorded = [[] for _ in range(G)]
    for ply in range(max(len(x) for x in games)):
        roots = eng.root_states72().cpu().numpy()
        acts = np.zeros(G, dtype=np.int32)
        for k in range(G):
            if ply < len(games[k]):
                assert np.array_equal(roots[k], chain[k].record()), (k, ply)
                acts[k] = games[k][ply]
                recorded[k].append(chain[k].record())
                chain[k] = chain[k].next(games[k][ply])
        eng.apply_actions(acts)
        roots = eng.root_states72().cpu().numpy()
        for k in range(G):
            assert np.array_equal(roots[k], chain[k].record()), (k, ply)
    c = eng.counters()
    assert c["active"] == 0 and c["finished"] == G and c["dead_ends"] == 0
    hs, ha, hv = (eng.t[n].cpu().numpy() for n in ("hist_state72", "hist_action", "hist_visits"))
    plies, done, result = (eng.t[n].cpu().numpy() for n in ("game_plies", "game_done", "game_result"))
    for k in range(G):
        n = len(games[k])
        assert int(plies[k]) == n and int(done[k]) == 1 and chain[k].is_done()
        assert np.array_equal(hs[k, :n], np.stack(recorded[k]))
        assert [int(a) for a in ha[k, :n]] == games[k]
        want = np.zeros((n, A), dtype=hv.dtype)
        want[np.arange(n), games[k]] = 1
        assert np.array_equal(hv[k, :n], want)
        point = (float(result[k]) + 1.0) / 2.0
        assert point == first_player_point(chain[k]) == float(g[f"e{k}_point"][0])


@pytest.mark.parametrize("N", [5, 9])
def test_apply_actions_between_searched_moves(dev, N):
    """move(), apply_actions, move() on one engine: the third ply's searched visits are those of a fresh engine search()ed from
    that position; a -1 action ends its slot as a draw and raises counters[2]."""
    from alphaquoridorgnn_amd import agents
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    State = _State()
    G, sims = 6, 24
    eng = BatchedSelfPlay(None, num_games=G, sims=sims, board_size=N, evaluator="fake", fake_bias=3, temperature=0.0)
    eng.move()
    roots = eng.root_states72().cpu().numpy()
    acts = np.array([agents._legal(roots[k])[(3 * k) % len(agents._legal(roots[k]))] for k in range(G)], dtype=np.int32)
    acts[G - 1] = -1
    eng.apply_actions(acts)
    c = eng.counters()
    assert c["dead_ends"] == 1 and c["active"] == G - 1 and c["finished"] == 1
    assert int(eng.t["game_done"][G - 1]) == 1 and int(eng.t["game_result"][G - 1]) == 0 and int(eng.t["game_plies"][G - 1]) == 1
    third = eng.root_states72().cpu().numpy()
    for k in range(G - 1):
        assert np.array_equal(third[k], State.from_record(roots[k]).next(int(acts[k])).record())
    eng.move()
    hv = eng.t["hist_visits"].cpu().numpy()
    fresh = BatchedSelfPlay(None, num_games=G, sims=sims, board_size=N, evaluator="fake", fake_bias=3, temperature=0.0,
                            record_history=False)
    visits, actions, count = (x.cpu().numpy() for x in fresh.search(third))
    for k in range(G - 1):
        dense = np.zeros(hv.shape[2], dtype=np.int64)
        dense[actions[k, :count[k]]] = visits[k, :count[k]]
        assert np.array_equal(hv[k, 2].astype(np.int64), dense), k
        assert int(eng.t["game_plies"][k]) == 3
    assert int(eng.t["game_plies"][G - 1]) == 1                  # the ended slot stayed out of the third ply


@pytest.mark.parametrize("N", [3, 5])
def test_apply_actions_records_games_as_move_does(dev, N):
    """The one transition behind engine_finish_move_kernel and engine_apply_actions_kernel (csrc/mcts_move.hip engine_transition),
    pinned from both sides: engine A plays a quota of 12 games on 8 slots with move(); engine B, built alike, is handed A's
    recorded action of every active slot ply by ply through apply_actions.  After every ply the two agree in every slot's position,
    game_active, slot_game and the counters; at the end in every game's record.  The refill runs behind both kernels.
    (`leaf_evals` and `terminal_sims` of counters() are statistics of the search, which B never runs: every other entry and the
    whole counters tensor are compared.  oracle/mcts.py's FakeModel plays this setup -- sims 8, temperature 0, bias 0 -- to a decisive
    game on both boards: 2 plies and z = -1 on 3x3, 7 plies and z = +1 on 5x5, so the quota outlasts the first eight games.)"""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    G, Q = 8, 12
    kw = dict(num_games=G, sims=8, board_size=N, evaluator="fake", temperature=0.0, quota=Q)
    a, b = BatchedSelfPlay(None, **kw), BatchedSelfPlay(None, **kw)
    host = lambda eng, name: eng.t[name].cpu().numpy()
    engine_counters = lambda eng: {k: v for k, v in eng.counters().items() if k not in ("leaf_evals", "terminal_sims")}
    moves = 0
    while a.counters()["active"] > 0:
        assert moves < 2 * Q * a.max_plies
        active, slot_game, plies = host(a, "game_active"), host(a, "slot_game"), host(a, "game_plies")
        a.move()
        recorded = host(a, "hist_action")
        acts = np.zeros(G, dtype=np.int32)
        for g in range(G):
            if active[g]:
                acts[g] = recorded[slot_game[g], plies[slot_game[g]]]
        b.apply_actions(acts)
        moves += 1
        assert np.array_equal(b.root_states72().cpu().numpy(), a.root_states72().cpu().numpy()), moves
        for name in ("game_active", "slot_game", "counters"):
            assert np.array_equal(host(b, name), host(a, name)), (name, moves)
        assert engine_counters(b) == engine_counters(a), moves
    c = a.counters()
    assert c["finished"] == Q and c["started"] == Q and c["dead_ends"] == 0
    for name in ("game_plies", "game_done", "game_result", "game_first_move", "hist_state72", "hist_action"):
        assert np.array_equal(host(b, name), host(a, name)), name
    plies, actions, visits = host(a, "game_plies"), host(a, "hist_action"), host(b, "hist_visits")
    for k in range(Q):
        n = int(plies[k])
        want = np.zeros((n, visits.shape[2]), dtype=visits.dtype)
        want[np.arange(n), actions[k, :n]] = 1
        assert np.array_equal(visits[k, :n], want), k
    assert (host(a, "game_result") != 0).any()                   # a decisive game went through lose / z
    assert (host(a, "game_first_move") > 0).any()                # a slot was refilled


# ---------------------------------------------------------------------------------------------- 11. whole matches
def _match(agent, N, games, seed=5, **kw):
    from alphaquoridorgnn_amd.evaluate_agents import BatchedAgentMatch
    return BatchedAgentMatch(7, agent, games, sims=16, board_size=N, evaluator="fake", seed=seed, **kw)


def _records_of(match):
    out = []
    for eng in match.engines:
        out.append(tuple(eng.t[n].cpu().numpy().copy()
                         for n in ("hist_state72", "hist_action", "game_plies", "game_result", "game_done", "hist_visits")))
    return out


def _same_records(a, b):
    for ea, eb in zip(a, b):
        plies = ea[2]
        assert np.array_equal(plies, eb[2]) and np.array_equal(ea[3], eb[3]) and np.array_equal(ea[4], eb[4])
        for k, n in enumerate(plies):
            assert np.array_equal(ea[0][k, :n], eb[0][k, :n]) and np.array_equal(ea[1][k, :n], eb[1][k, :n])


def _check_match_records(match, points, N):
    from alphaquoridorgnn_amd import agents
    assert all(p in (0.0, 0.5, 1.0) for p in points) and len(points) == match.num_games
    for first, eng in enumerate(match.engines):
        hs, ha, plies, result, done, hv = _records_of(match)[first]
        assert done.all()
        for k, n in enumerate(plies):
            for j in range(int(n)):
                assert int(ha[k, j]) in agents._legal(hs[k, j]), (first, k, j)
                assert (int(hs[k, j, 68]) | (int(hs[k, j, 69]) << 8)) == j
                searched = (j % 2 == 0) == (first == 0)                          # the network's plies carry a search's visit counts,
                assert (int(hv[k, j].sum()) > 1) == searched, (first, k, j)      # the agent's a single 1 at its action
                if not searched:
                    assert int(hv[k, j, int(ha[k, j])]) == 1
            fp = (float(result[k]) + 1.0) / 2.0
            assert points[2 * k + first] == (fp if first == 0 else 1.0 - fp)     # game 2k + first: the network first iff first == 0


@pytest.mark.parametrize("N,games", [(5, 24), (9, 8)])
@pytest.mark.parametrize("agent", ["random", "mcts"])
def test_match_gpu_agent_equals_host_closure(dev, monkeypatch, N, games, agent):
    from alphaquoridorgnn_amd import agents
    E = 20
    n = 1 if agent == "random" else E * DRAW[N]
    sizes = [(games + 1) // 2, games // 2]
    rng = np.random.RandomState(11)
    uniforms = [rng.random_sample((DRAW[N], g)) for g in sizes]
    agent_uniforms = [np.stack([np.stack([agents.draw_uniforms(1000 + first, ply * 64 + g, n) for g in range(sizes[first])])
                                for ply in range(DRAW[N])]) for first in range(2)]
    kw = dict(evaluations=E) if agent == "mcts" else {}
    gpu = _match(agent, N, games, agent_kwargs=kw)
    points = gpu.play(uniforms, agent_uniforms)
    _check_match_records(gpu, points, N)

    host = _match(lambda state: None, N, games)          # placeholder agent, replaced below (the closure needs the match)

    def closure(state):
        first, g, ply = host.current
        table = agent_uniforms[first][ply][g]
        if agent == "random":
            return _pick(agents._legal(state), table[0])
        monkeypatch.setattr(agents, "random_action", _TableDraw(table))
        return agents.mcts_action(state, E)
    host.agent = closure
    assert host.play(uniforms, agent_uniforms) == points
    _same_records(_records_of(gpu), _records_of(host))


@pytest.mark.parametrize("N,games", [(5, 24), (9, 8)])
def test_match_alpha_beta_batch_equals_callable(dev, N, games):
    from alphaquoridorgnn_amd import agents
    batch = _match("alpha_beta", N, games)
    points = batch.play()
    _check_match_records(batch, points, N)
    host = _match(agents.alpha_beta_action, N, games)
    assert host.play() == points
    _same_records(_records_of(batch), _records_of(host))


@pytest.mark.parametrize("agent", ["random", "mcts"])
def test_match_same_seed_same_games(dev, agent):
    kw = dict(evaluations=20) if agent == "mcts" else {}
    a = _match(agent, 5, 10, seed=9, agent_kwargs=kw)
    pa = a.play()
    b = _match(agent, 5, 10, seed=9, agent_kwargs=kw)
    assert b.play() == pa
    _same_records(_records_of(a), _records_of(b))
    _check_match_records(a, pa, 5)
    assert a.play() == pa                                        # and a second play() of the same match object


# ---------------------------------------------------------------------------------------------- 12. real networks
@pytest.mark.parametrize("kind", ["gnn_6_128_3", "gnn_6_64_2", "cnn_32x2"])
def test_evaluate_best_player_on_real_networks(dev, tmp_path, monkeypatch, capsys, kind):
    """Completes and returns three values in [0, 1]; 5x5 board.  No strength is asserted: a random-init network has none."""
    from alphaquoridorgnn_amd import constants, evaluate_agents as ea, pv_mcts
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    N, A = 5, 57
    torch.manual_seed(3)
    if kind == "cnn_32x2":
        model = CNNNetwork(32, 2, N)
    else:
        hidden, layers = (128, 3) if kind == "gnn_6_128_3" else (64, 2)
        model = GraphPolicyValueNetwork(6, hidden, layers, A)
    path = str(tmp_path) + "/"
    torch.save(model.state_dict(), path + "best.pth")
    monkeypatch.setattr(constants, "PV_NETWORK_PATH", path)
    monkeypatch.setattr(pv_mcts, "PV_EVALUATE_COUNT", 8)
    out = ea.evaluate_best_player(games=4, seed=1)
    assert list(out) == ["VS_Random", "VS_AlphaBeta", "VS_MCTS"]
    assert all(0.0 <= v <= 1.0 and (v * 8) == int(v * 8) for v in out.values())
    text = capsys.readouterr().out
    for label in out:
        assert label in text
