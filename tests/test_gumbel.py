"""The Gumbel root search on the device (csrc/mcts_step.hip GUMBEL, csrc/mcts_gumbel.hip; include/aqgnn.h "Gumbel root search"): the
root launch alone on narrowed pools, between sentinels; whole search trees bit for bit against the reference search of
tests/_gumbel.py, fed the device's own logits and evaluations; the finish launch alone and whole games of move() against a host loop;
the option off = the engine as it was; refusals; self_play() end to end."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _gumbel as TG, _tree_parity as TP

pytestmark = pytest.mark.gpu
REPO = TP.REPO
MAX_LEGAL = TG.MAX_LEGAL
SENTINEL = np.float32(-12345.5)          # what every cp word holds in front of the root launch
COUNTS = (1, 63, 64, 65, 127, 128, 129, 136)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _engine(G, sims, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    kw.setdefault("record_history", False)
    kw.setdefault("fake_bias", 3)
    return BatchedSelfPlay(kw.pop("model", None), num_games=G, sims=sims, board_size=N, **kw)


def _pools(eng):
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    torch.cuda.synchronize()
    return eng.t["node_rec"].cpu().numpy().view(NODE_DTYPE).reshape(eng.G, eng.node_cap).copy(), eng.t["node_count"].cpu().numpy().copy()


def _write_pools(eng, pools):
    eng.t["node_rec"].copy_(torch.from_numpy(np.ascontiguousarray(pools).view(np.float64).reshape(eng.G * eng.node_cap, 4)))


@functools.lru_cache(maxsize=None)
def _roots(N, count):
    """`count` roots of board N: the opening first, then positions a few plies deep and later ones from the recorded walk."""
    recs, _ = TP.pick_roots(N, count)
    assert TP.plies(recs)[0] == 0
    return recs


def _one_ulp(got, want):
    """got within one f32 ulp of want (finite entries), and -inf / +inf exactly where want has them."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    fin = np.isfinite(want)
    same_inf = np.array_equal(got[~fin], want[~fin])
    lo, hi = np.nextafter(want[fin], np.float32(-np.inf)), np.nextafter(want[fin], np.float32(np.inf))
    return same_inf and bool(((got[fin] >= lo) & (got[fin] <= hi)).all())


# ------------------------------------------------------------------ 1. the root launch alone
def _priors(cnt, seed):
    """Priors of `cnt` children with a zero, a negative value and a NaN among them (where there is room)."""
    p = np.random.RandomState(seed).dirichlet(np.ones(cnt)).astype(np.float32)
    if cnt >= 63:
        p[[2, cnt // 2, cnt - 1]] = [0.0, -0.125, np.nan]
    return p


def _launch_root(eng):
    from alphaquoridorgnn_amd import _lib
    _lib.check(eng.lib.aqg_engine_gumbel_root(ctypes.byref(eng.e), ctypes.byref(eng.gumbel), eng._stream()), "aqg_engine_gumbel_root")


@pytest.mark.parametrize("source", ["table", "generator"])
@pytest.mark.parametrize("N,G", [(3, 1), (5, 4), (5, 5), (9, 9)])
def test_root_launch_alone(dev, N, G, source):
    """gl within one f32 ulp of gumbel_logits_reference -- the float64 values differ by at most 4 ulp of float64 between the device's
    log and the host's, so the two roundings to float32 differ only beside a rounding boundary --, -inf exactly where stated, m_g
    exact, and every other word of the pool, every slot not launched and every word around m untouched (the launch is given m inside a
    padded buffer with sentinels on both sides)."""
    from alphaquoridorgnn_amd import gumbel as GB
    M, scale = 16, 1.5
    eng = _engine(G, 2, N, gumbel_considered=M, gumbel_scale=scale, gumbel_seed=77)
    eng.search(np.repeat(TG.opening(N)[None], G, 0))           # real expanded roots
    base, _ = _pools(eng)
    assert TP.kids_of(base[0][0])[1] == len(_legal(TG.opening(N)))
    padded = torch.full((G + 32,), -7, dtype=torch.int32, device=dev)      # m = padded[16 : 16 + G]
    eng.gumbel.m = padded[16:].data_ptr()
    table = np.random.RandomState(5).standard_normal((G, MAX_LEGAL)) * 3.0
    table[:, 7], table[:, 9] = np.nan, np.inf                  # read as 0
    idle = G - 1 if G > 1 else None                            # one slot is not launched: inactive
    for shift in range(len(COUNTS) if G < len(COUNTS) else 1):
        pools = base.copy()
        pools["cp"] = SENTINEL
        counts = [COUNTS[(g + shift * G) % len(COUNTS)] for g in range(G)]
        priors = [_priors(c, 100 * shift + g) for g, c in enumerate(counts)]
        for g, c in enumerate(counts):
            pools["kids"][g, 0] = 1 | (c << 24)
            pools["p"][g, 1:1 + c] = priors[g]
        _write_pools(eng, pools)
        padded.fill_(-7)
        if idle is not None:
            eng.t["game_active"][idle] = 0
        eng._set_gumbel(table if source == "table" else None)
        _launch_root(eng)
        got, _ = _pools(eng)
        words = padded.cpu().numpy()
        m = words[16:16 + G]
        assert (words[:16] == -7).all() and (words[16 + G:] == -7).all()
        for g, c in enumerate(counts):
            if g == idle:
                assert got[g].tobytes() == pools[g].tobytes() and m[g] == -7
                continue
            variates = table[g] if source == "table" else GB.draw_gumbel(77, g, 0, c)
            want = GB.gumbel_logits_reference(priors[g], variates, scale)
            gl = got[g][1:1 + c]["cp"]
            assert _one_ulp(gl, want), (g, c)
            assert np.array_equal(np.isneginf(gl), ~(priors[g] > 0)), (g, c)
            assert m[g] == min(M, int((priors[g] > 0).sum())), (g, c)
            rest = got[g].copy()
            rest["cp"][1:1 + c] = SENTINEL
            assert rest.tobytes() == pools[g].tobytes(), (g, c)         # every other word of the pool
        eng.t["game_active"].fill_(1)


def _legal(rec):
    from oracle import quoridor as oq
    return list(oq.State(rec).legal_actions())


def test_root_launch_guards_and_slot_independence(dev):
    """A count above MAX_LEGAL or a child range that leaves the pool writes nothing and sets m_g = 0; the generator's row of a game
    does not depend on the slot the game sits in."""
    eng = _engine(4, 2, 5, gumbel_considered=8, gumbel_seed=5)
    eng.search(np.repeat(TG.opening(5)[None], 4, 0))
    pools, _ = _pools(eng)
    pools["cp"] = SENTINEL
    cap = eng.node_cap
    pools["kids"][0, 0] = 1 | (137 << 24)                       # above MAX_LEGAL
    pools["kids"][1, 0] = (cap - 10) | (64 << 24)               # leaves the pool
    pools["kids"][2, 0] = 0                                     # not expanded
    _write_pools(eng, pools)
    eng.t["gumbel_m"].fill_(-7)
    _launch_root(eng)
    got, _ = _pools(eng)
    m = eng.t["gumbel_m"].cpu().numpy()
    for g in range(3):
        assert got[g].tobytes() == pools[g].tobytes() and m[g] == 0, g
    assert m[3] == 8 and not (got[3][1:1 + 35]["cp"] == SENTINEL).any()
    # game 9 in slot 0, then in slot 3: the same row
    rows = []
    for slot in (0, 3):
        pools["kids"][slot, 0] = 1 | (35 << 24)
        _write_pools(eng, pools)
        eng.t["slot_game"].copy_(torch.tensor([1, 2, 3, 4], dtype=torch.int32))
        eng.t["slot_game"][slot] = 9
        _launch_root(eng)
        rows.append(_pools(eng)[0][slot][1:36]["cp"].copy())
    from alphaquoridorgnn_amd import gumbel as GB
    assert rows[0].tobytes() == rows[1].tobytes()
    assert _one_ulp(rows[0], GB.gumbel_logits_reference(pools[0][1:36]["p"], GB.draw_gumbel(5, 9, 0, 35), 1.0))


# ------------------------------------------------------------------ 2. selection, exactly
def _check_search(eng, recs, sims, M, table=None, c_visit=TG.C_VISIT, c_scale=TG.C_SCALE):
    """search() then every slot's whole tree against the reference search fed the device's own gl row; returns the pools."""
    eng.search(recs, gumbel=table)
    gl, m, win = (x.cpu().numpy() for x in eng.root_gumbel())
    pools, counts = _pools(eng)
    for g in range(eng.G):
        cnt = TP.kids_of(pools[g][0])[1]
        assert cnt == len(_legal(recs[g])) and np.isneginf(gl[g, cnt:]).all()
        root = TG.check_tree(pools[g], counts[g], recs[g], sims, gl[g, :cnt], M, c_visit, c_scale)
        assert m[g] == root.m == min(M, int((gl[g, :cnt] > -np.inf).sum())), g
        assert win[g] == TG.winner(root, c_visit, c_scale), g
        assert pools[g][1:1 + cnt]["cp"].tobytes() == gl[g, :cnt].tobytes()
    return pools, gl


@pytest.mark.parametrize("sims", [2, 3, 9, 17, 50])
@pytest.mark.parametrize("N", [3, 5, 9])
def test_search_trees_bit_exact(dev, N, sims):
    """The opening (9x9: 131 children, three lane rounds) and roots a few plies deep and later; M above the legal count on 3x3."""
    recs = _roots(N, 6)
    for M in (1, 2, 4, 16):
        eng = _engine(6, sims, N, gumbel_considered=M, gumbel_seed=1000 + M)
        _check_search(eng, recs, sims, M)
        if N == 9:
            assert TP.kids_of(_pools(eng)[0][0][0])[1] == 131


def test_search_largest_logit_in_every_lane_round(dev):
    """Variate tables that put the largest gl on child 0, 63, 64, 127, 128 and 130 of the 9x9 opening: that child is sampled first."""
    peaks = (0, 63, 64, 127, 128, 130)
    recs = np.repeat(TG.opening(9)[None], len(peaks), 0)
    table = np.stack([TG.table_with_peak(1, p, seed=p)[0] for p in peaks])
    for sims, M in ((17, 4), (9, 16), (2, 1)):
        eng = _engine(len(peaks), sims, 9, gumbel_considered=M)
        pools, gl = _check_search(eng, recs, sims, M, table=table)
        for g, p in enumerate(peaks):
            assert int(np.argmax(gl[g, :131])) == p and pools[g][1 + p]["n"] >= 1, (g, p)
            if M == 1:
                assert pools[g][1 + p]["n"] == sims - 1


@pytest.mark.parametrize("N", [5, 9])
def test_search_hand_over_to_memory(dev, N):
    """step_fast_depth 0 and 1: the reloaded copies of the root's children are scored the same way -- identical pools."""
    from alphaquoridorgnn_amd import _lib
    recs = _roots(N, 6)
    want = None
    try:
        for depth in (61, 0, 1):
            _lib.set_option("step_fast_depth", depth)
            eng = _engine(6, 50, N, gumbel_considered=4, gumbel_seed=3)
            pools, _ = _check_search(eng, recs, 50, 4)
            if want is None:
                want = pools
            for g in range(6):
                used = int(_pools(eng)[1][g])
                assert pools[g][:used].tobytes() == want[g][:used].tobytes(), (depth, g)
    finally:
        _lib.set_option("step_fast_depth", 61)


def test_search_graph_capture_on_and_off(dev):
    """On a capturable stream the search is a replayed hipGraph whose key holds the Gumbel struct: the same trees as plain launches,
    for two tables in turn (one buffer, the replay reads the new content) and for the generator (another key)."""
    from alphaquoridorgnn_amd import _lib
    recs = _roots(5, 4)
    tables = [np.random.RandomState(s).standard_normal((4, MAX_LEGAL)) for s in (1, 2)]
    results = {}
    side = torch.cuda.Stream()
    try:
        for use_graph in (0, 1):
            _lib.set_option("use_graph", use_graph)
            with torch.cuda.stream(side):
                eng = _engine(4, 17, 5, gumbel_considered=4, gumbel_seed=8)
                out = []
                for table in (tables[0], tables[1], None, tables[0]):
                    pools, _ = _check_search(eng, recs, 17, 4, table=table)
                    out.append(b"".join(pools[g][:int(_pools(eng)[1][g])].tobytes() for g in range(4)))
                results[use_graph] = out
            side.synchronize()
    finally:
        _lib.set_option("use_graph", 1)
    assert results[0] == results[1]
    assert results[0][0] == results[0][3] and len(set(results[0][:3])) == 3


def _general_net(dev):
    return TP.general_net((6, 32, 2), 5, seed=5, factor=8.0).to(dev)


def test_search_general_network_and_evaluation_cache(dev):
    """One 'general' 6/32/2 network on 5x5: the whole tree against the reference search, and the evaluation cache on and off give
    identical trees."""
    net = _general_net(dev)
    recs = _roots(5, 4)
    pools = {}
    for slots in (0, 64):
        eng = _engine(4, 50, 5, evaluator="general", model=net, gumbel_considered=4, gumbel_seed=2, eval_cache_slots=slots)
        pools[slots], _ = _check_search(eng, recs, 50, 4)
        used = _pools(eng)[1]
        pools[slots] = [pools[slots][g][:int(used[g])] for g in range(4)]
    for g in range(4):
        for f in ("n", "w", "kids", "action", "p"):
            assert pools[0][g][f].tobytes() == pools[64][g][f].tobytes(), (g, f)


@pytest.mark.parametrize("N,kind", [(9, "gnn"), (3, "general"), (7, "general")])
def test_search_cached_step_kernels(dev, N, kind):
    """The CACHE instantiations of the GUMBEL step kernel on the other boards: 9x9 with the default network, 3x3 and 7x7 with a small
    'general' one -- the whole tree against the reference search, and the trees of the cache-less engine."""
    if kind == "gnn":
        from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
        from oracle import gnn as og
        net = GNNNetwork()
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in og.init_params(4).items()})
        net = net.to(dev).eval()
    else:
        net = TP.general_net((6, 32, 2), N, seed=N, factor=8.0).to(dev)
    recs = _roots(N, 4)
    trees = {}
    for slots in (0, 64):
        eng = _engine(4, 17, N, evaluator=kind, model=net, gumbel_considered=4, gumbel_seed=6, eval_cache_slots=slots)
        pools, _ = _check_search(eng, recs, 17, 4)
        used = _pools(eng)[1]
        trees[slots] = [pools[g][:int(used[g])] for g in range(4)]
    for g in range(4):
        for f in ("n", "w", "kids", "action", "p"):
            assert trees[0][g][f].tobytes() == trees[64][g][f].tobytes(), (g, f)


# ------------------------------------------------------------------ 3. the move
def _finish(eng):
    from alphaquoridorgnn_amd import _lib
    _lib.check(eng.lib.aqg_engine_finish_move_gumbel(ctypes.byref(eng.e), None, 0, None, None, None, None, None, ctypes.byref(eng.gumbel),
                                                     eng._stream()), "aqg_engine_finish_move_gumbel")


def test_finish_launch_alone(dev):
    """On pools whose counts and q the test overwrites: ties in S take the first, a winner in each lane round, cnt = 0 is the dead
    end -- and the read-out names the same child."""
    from alphaquoridorgnn_amd import gumbel as GB
    G = 6
    eng = _engine(G, 2, 9, gumbel_considered=16, record_history=True)
    eng.search(np.repeat(TG.opening(9)[None], G, 0))
    pools, _ = _pools(eng)
    rng = np.random.RandomState(4)
    want = []
    for g, (winner, tie) in enumerate(((5, None), (70, None), (129, None), (64, 127), (3, 66), (None, None))):
        kids = pools[g][1:132]
        kids["cp"] = rng.uniform(-6, -2, 131).astype(np.float32)
        kids["cp"][rng.permutation(131)[:40]] = -np.inf             # not sampled
        kids["n"] = 0
        kids["q"] = 0
        kids["w"] = 0
        if winner is None:
            pools["kids"][g, 0] = 0                                  # the dead end
            want.append(-1)
            continue
        sampled = [winner] + ([tie] if tie is not None else []) + [i for i in (10, 90, 120) if i not in (winner, tie)]
        for i in sampled:                                            # the survivors of the last phase: the largest visit count
            kids["n"][i], kids["q"][i], kids["cp"][i] = 7, np.float32(-0.5), np.float32(-3.0)
        kids["n"][20], kids["q"][20], kids["cp"][20] = 3, np.float32(1.0), np.float32(5.0)      # a larger S at a smaller count: not it
        kids["n"][21], kids["q"][21] = 9, np.float32(1.0)            # the largest count of all, never sampled (gl = -inf beside it)
        kids["cp"][21] = -np.inf
        kids["q"][winner] = np.float32(0.25)
        if tie is not None:
            kids["q"][tie] = np.float32(0.25)                        # the same S further on: the first is taken
        kids["w"] = -kids["q"].astype(np.float64) * kids["n"]
        assert GB.gumbel_winner_reference(kids["cp"], kids["n"], kids["q"], 50.0, 1.0) == winner
        want.append(winner)
    _write_pools(eng, pools)
    win = eng.root_gumbel()[2].cpu().numpy()
    assert list(win) == want
    before = eng.counters()
    _finish(eng)
    torch.cuda.synchronize()
    after = eng.counters()
    acts = eng.t["hist_action"].cpu().numpy()
    for g, w in enumerate(want[:5]):
        assert acts[g, 0] == pools[g][1 + w]["action"], g
    assert after["dead_ends"] == before["dead_ends"] + 1 and eng.t["game_done"][5].item() == 1 and eng.t["game_result"][5].item() == 0
    assert list(eng.t["game_plies"].cpu().numpy()) == [1, 1, 1, 1, 1, 0]
    vis = eng.t["hist_visits"].cpu().numpy()
    assert vis[0, 0, pools[0][1 + 5]["action"]] == 7 and vis[0, 0].sum() == 7 * 4 + 3 + 9


def _host_game(N, sims, M, seed, k, start=None, c_visit=20.0, c_scale=1.0, bias=3):
    """One game of move() on the host: the reference search at every ply with the generator's variates of (seed, game k, the
    record's ply), rule 4's move.  -> (records, visit rows, completed-Q rows, search values, z of ply 0, plies)."""
    from alphaquoridorgnn_amd import gumbel as GB
    from oracle import mcts as om, quoridor as oq
    from tests._policy_record import root_row
    model = om.FakeModel(bias)
    state = oq.State(start) if start is not None else oq.State(N=N)
    A = TP.action_count(N)
    recs, visits, rows, values = [], [], [], []
    while not state.is_done():
        legal = _legal(state.rec)
        g = GB.draw_gumbel(seed, k, state.plies_played, len(legal))
        root = TG.search(model, state, sims, lambda p: GB.gumbel_logits_reference(p, g, 1.0), M, c_visit, c_scale)
        v = np.zeros(A, np.int16)
        v[legal] = [c.n for c in root.children]
        recs.append(np.asarray(state.rec).copy())
        visits.append(v)
        rows.append(root_row(root, N, c_visit, c_scale))
        values.append(np.float32(root.w / root.n))
        state = state.next(legal[TG.winner(root, c_visit, c_scale)])
    return np.stack(recs), np.stack(visits), np.stack(rows), np.array(values, np.float32), om.first_player_value(state), len(recs)


@pytest.mark.parametrize("N,start", [(3, False), (5, False), (5, True)])
def test_whole_games_against_the_host_loop(dev, N, start):
    """5 games on 2 slots, with refill (and with a start table): history_tensors(), game_result, game_plies, the recorded completed-Q
    rows and hist_value against the host loop on the reference search."""
    from tests._improved_policy import pi_close
    sims, M, seed = 9, 4, 31
    kw, starts = {}, [None] * 5
    if start:
        table = np.stack([r for r in TP.walk_states(N) if TP.plies(r)[0] % 2 == 0 and TP.plies(r)[0] <= 8][:3])
        kw = dict(start_states=table)
        starts = [table[k % 3] for k in range(5)]
    eng = _engine(2, sims, N, quota=5, record_history=True, gumbel_considered=M, gumbel_seed=seed, policy_target="completed_q",
                  policy_c_visit=20.0, record_search_value=True, **kw)
    c = eng.play_generation()
    assert c["finished"] == 5
    S, V, Z = (x.cpu().numpy() for x in eng.history_tensors())
    P, Q = eng.history_policies().cpu().numpy(), eng.history_values().cpu().numpy()
    plies, result = eng.t["game_plies"].cpu().numpy(), eng.t["game_result"].cpu().numpy()
    at = 0
    for k in range(5):
        recs, visits, rows, values, z0, n = _host_game(N, sims, M, seed, k, starts[k])
        assert plies[k] == n and result[k] == z0, k
        sl = slice(at, at + n)
        at += n
        assert np.array_equal(S[sl][:, :68], recs[:, :68]) and np.array_equal(V[sl], visits), k
        assert list(Z[sl]) == [z0 * (1 if i % 2 == 0 else -1) for i in range(n)], k
        assert Q[sl].tobytes() == values.tobytes(), k
        assert pi_close(P[sl], rows) and np.array_equal(P[sl] > 0, rows > 0), k
    assert at == S.shape[0]


def test_two_sets_against_one(dev):
    """A game's variates do not depend on the set count: MultiSetSelfPlay with two sets plays the games of one set."""
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    out = []
    for sets in (1, 2):
        eng = MultiSetSelfPlay(None, num_games=4, sims=9, num_sets=sets, seed=6, board_size=3, evaluator="fake", fake_bias=3,
                               gumbel_considered=4, policy_target="completed_q")
        assert eng.play_generation()["finished"] == 4
        out.append([x.cpu().numpy().tobytes() for x in eng.history_tensors() + (eng.history_policies(),)])
    assert out[0] == out[1]


def test_option_off_is_the_engine_as_it_was(dev):
    a = _engine(4, 8, 3, record_history=True, seed=9)
    b = _engine(4, 8, 3, record_history=True, seed=9, gumbel_considered=0, gumbel_scale=3.0, gumbel_seed=1)
    assert b.gumbel is None and "gumbel_m" not in b.t and "gumbel_schedule" not in b.t
    for eng in (a, b):
        assert eng.play_generation()["finished"] == 4
    for x, y in zip(a.history_tensors(), b.history_tensors()):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert a.t["node_rec"].cpu().numpy().tobytes() == b.t["node_rec"].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="gumbel_considered"):
        b.root_gumbel()
    with pytest.raises(ValueError, match="gumbel_considered"):
        b.move(gumbel=np.zeros((4, MAX_LEGAL)))
    c = _engine(2, 8, 3, record_history=True, gumbel_considered=4)
    with pytest.raises(ValueError, match="no uniform"):
        c.move(uniforms=np.zeros(2))
    with pytest.raises(ValueError, match="no uniform"):
        c.play_generation(uniforms=np.zeros((4, 2)))
    assert c.moves_done == 0


# ------------------------------------------------------------------ 4. refusals
def test_engine_refusals(dev):
    for kw, word in ((dict(sims=1), "sims >= 2"), (dict(gumbel_considered=65), "1..64"), (dict(gumbel_scale=-1.0), "gumbel_scale"),
                     (dict(gumbel_scale=float("nan")), "gumbel_scale"), (dict(root_noise_eps=0.25), "root noise"),
                     (dict(tree_reuse=True), "tree_reuse"), (dict(resign_threshold=0.9, record_history=True), "resignation"),
                     (dict(temperature_plies=2), "temperature_plies"), (dict(evaluator="external"), "external")):
        args = dict(gumbel_considered=4, sims=8)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            _engine(2, args.pop("sims"), 3, **args)
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    with pytest.raises(ValueError, match="root noise"):
        MultiSetSelfPlay(None, num_games=2, sims=8, board_size=3, evaluator="fake", gumbel_considered=4, root_noise_eps=0.25)


def test_library_refusals(dev):
    """The library refuses in the stated order, before any launch: the pool and the words are untouched."""
    from alphaquoridorgnn_amd import _lib
    eng = _engine(2, 8, 3, gumbel_considered=4, record_history=True)
    eng.search(np.repeat(TG.opening(3)[None], 2, 0))
    before = _pools(eng)[0].tobytes(), eng.t["gumbel_m"].cpu().numpy().tobytes()
    lib, e, st = eng.lib, ctypes.byref(eng.e), eng._stream()

    def move(gb, plies=0, reuse=None, resign=None):
        return lib.aqg_engine_move_gumbel(e, None, plies, None, reuse, resign, None, None, ctypes.byref(gb), st)

    def variant(**kw):
        gb = _lib.GumbelStruct()
        ctypes.memmove(ctypes.byref(gb), ctypes.byref(eng.gumbel), ctypes.sizeof(gb))
        for k, v in kw.items():
            setattr(gb, k, v)
        return gb
    reuse, resign = _lib.TreeReuseStruct(), _lib.ResignStruct()
    cases = [(lambda: move(variant(considered=0)), "considered"), (lambda: move(variant(considered=65)), "considered"),
             (lambda: move(variant(scale=-1.0)), "scale"), (lambda: move(variant(scale=float("inf"))), "scale"),
             (lambda: move(variant(), reuse=ctypes.byref(reuse)), "tree reuse"), (lambda: move(variant(), resign=ctypes.byref(resign)), "resignation"),
             (lambda: move(variant(), plies=3), "temperature_plies"),
             (lambda: move(variant(considered=0, scale=-1.0), plies=3, reuse=ctypes.byref(reuse)), "considered"),       # the order
             (lambda: lib.aqg_engine_search_gumbel(e, _lib.ptr(eng._roots), ctypes.byref(variant(scale=float("nan"))), st), "scale"),
             (lambda: lib.aqg_engine_gumbel_root(e, ctypes.byref(variant(considered=-1)), st), "considered"),
             (lambda: lib.aqg_engine_move_gumbel(e, None, 0, None, None, None, None, None, None, st), "null")]
    for call, word in cases:
        assert call() != 0 and word in lib.aqg_last_error().decode(), word
    eng.e.sims = 1
    assert move(variant()) != 0 and "sims" in lib.aqg_last_error().decode()
    eng.e.sims = 8
    eng.e.root_noise_eps, eng.e.root_noise_alpha = 0.25, 0.3
    assert move(variant()) != 0 and "root noise" in lib.aqg_last_error().decode()
    eng.e.root_noise_eps, eng.e.root_noise_alpha = 0.0, 0.0
    mode, eng.e.prior_mode = eng.e.prior_mode, 2
    assert move(variant()) != 0 and "prior_mode 2" in lib.aqg_last_error().decode()
    eng.e.prior_mode = mode
    assert (_pools(eng)[0].tobytes(), eng.t["gumbel_m"].cpu().numpy().tobytes()) == before


# ------------------------------------------------------------------ 5. self_play() end to end
_LOOP = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, pv_mcts, self_play as sp, train_network as tn
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork

assert constants.BOARD_SIZE == 3
torch.manual_seed(3)
dev = aqd.device()
net = GraphPolicyValueNetwork(6, 16, 2, 17, board_size=3)
os.makedirs(constants.PV_NETWORK_PATH)
torch.save(net.state_dict(), constants.PV_NETWORK_PATH + "best.pth")
model = net.to(dev).eval()
pv_mcts.PV_EVALUATE_COUNT = 8
sp.SP_POLICY_TARGET, sp.SP_GUMBEL_CONSIDERED = "completed_q", 4
path = sp.self_play(model, games=6, seed=17)
again = sp.self_play(model, games=6, seed=17)
with open(path, "rb") as f:
    rows = pickle.load(f)
with open(again, "rb") as f:
    rows2 = pickle.load(f)
print("DETERMINISTIC", path == again or rows == rows2)
history = tn.load_data()
s, p, v = zip(*history)
pi = np.array(p, dtype=np.float64)
print("LOADER_READS_IT", len(history) == len(rows) >= 6 * 2, pi.shape[1] == 17, bool(np.abs(pi.sum(1) - 1.0).max() < 1e-5), set(v) <= {-1, 0, 1})
sp.SP_POLICY_TARGET = "visits"
try:
    sp.self_play(model, games=2, seed=1)
    print("REFUSED False")
except ValueError as err:
    print("REFUSED", "completed_q" in str(err))
'''


def test_self_play_with_the_option(dev, tmp_path):
    """One child process on the 3x3 board: self_play() with the option writes a .history file train_network.load_data() reads; the
    progress line names the search."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="3")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("DETERMINISTIC True", "LOADER_READS_IT True True True True", "REFUSED True"):
        assert line in r.stdout, (line, r.stdout[-2000:])
    assert "search: Gumbel root, 4 considered" in r.stdout
