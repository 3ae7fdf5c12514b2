"""Resignation on the GPU (include/aqgnn.h "resignation"; engine_finish_move_kernel in csrc/mcts_move.hip): whole games bit for bit against
the host statement of tests/_resign.py -- rows, visit rows, values, hist_action with its 0xFF, game_plies, game_result, game_resigned and
resign_min -- on 1, 4 and 5 slots, with and without graph capture, with min_ply on either side of a first crossing and with none, all
or some of the games disabled; a threshold of 1.0 against the option off; independence from slots, refill and sets; tree reuse, the
temperature schedule and table root noise beside it; the network evaluators with the evaluation cache on and off and the external
one; the refusals; self_play() with the options.  tests/test_resign_cpu.py asserts what the case lists contain."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _resign as R   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _engine(G, sims, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    return BatchedSelfPlay(kw.pop("model", None), num_games=G, sims=sims, board_size=N, **kw)


def _game_rows(eng):
    """Per game: (plies, result, resigned, resign_min bytes, states, visit rows, actions, values) of its recorded plies."""
    plies = eng.t["game_plies"].cpu().numpy()
    hs, hv, ha, hq = (eng.t[k].cpu().numpy() for k in ("hist_state72", "hist_visits", "hist_action", "hist_value"))
    res = eng.t["game_result"].cpu().numpy()
    if eng.resign is not None:
        flag, lo = eng.t["game_resigned"].cpu().numpy(), eng.t["resign_min"].cpu().numpy()
    else:
        flag, lo = np.zeros(eng.quota, np.uint8), np.full((eng.quota, 2), np.inf, dtype=np.float32)
    assert bool((eng.t["game_done"].cpu().numpy() != 0).all())
    return [(int(plies[k]), int(res[k]), int(flag[k]), lo[k].tobytes(), hs[k, :plies[k], :70].tobytes(), hv[k, :plies[k]].tobytes(),
             ha[k, :plies[k]].tobytes(), hq[k, :plies[k]].tobytes()) for k in range(eng.quota)]


def _play_quota(G, quota, U_game, N, sims=R.SIMS, tables=None, **kw):
    """Play `quota` games on G slots; game k's move at ply j is drawn with U_game[k, j] (and mixed with tables[j, k]) whatever slot it
    sits in.  Returns the engine."""
    from alphaquoridorgnn_amd import _lib
    kw.setdefault("fake_bias", 2)
    kw.setdefault("record_search_value", True)
    eng = _engine(G, sims, N, quota=quota, **kw)
    for _ in range(eng.max_plies * quota + 1):
        active = eng.t["game_active"].cpu().numpy()
        if not active.any():
            break
        sg, gp = eng.t["slot_game"].cpu().numpy(), eng.t["game_plies"].cpu().numpy()
        u = np.zeros(G)
        noise = None if tables is None else np.ones((G, _lib.MAX_LEGAL))
        for g in range(G):
            if active[g]:
                u[g] = U_game[sg[g], gp[sg[g]]]
                if noise is not None:
                    noise[g] = tables[gp[sg[g]], sg[g]]
        eng.move(torch.from_numpy(u), None if noise is None else torch.from_numpy(noise))
    c = eng.counters()
    assert c["finished"] == quota and c["active"] == 0 and c["dead_ends"] == 0
    return eng


def _assert_statement(eng, want):
    got = _game_rows(eng)
    for k in range(eng.quota):
        assert got[k] == R.game_rows_of(want, k), k
    # the flat history: z follows from game_result, and a resigning row reads -1 with the action 0xFF
    st, vis, z = (x.cpu().numpy() for x in eng.history_tensors())
    act = eng.t["hist_action"][eng._history_valid()[0]].cpu().numpy()
    assert vis.tobytes() == want["visits"].tobytes() and z.tobytes() == want["z"].tobytes() and act.tobytes() == want["actions"].tobytes()
    last = np.cumsum(want["plies"]) - 1
    for k in range(eng.quota):
        assert (act[last[k]] == 0xFF) == bool(want["resigned"][k])
        assert not want["resigned"][k] or z[last[k]] == -1
    assert int((act == 0xFF).sum()) == int(want["resigned"].sum())
    lo, res, enabled, flag, plies, done = eng.resign_arrays()
    assert enabled.tolist() == want["enabled"].tolist() and flag.tobytes() == want["resigned"].tobytes()
    assert lo.tobytes() == want["minima"].tobytes() and res.tobytes() == want["result"].tobytes() and plies.tobytes() == want["plies"].tobytes()
    stats = eng.resign_stats()
    assert stats["games"] == eng.quota and stats["games_resigned"] == int(want["resigned"].sum()) and stats["plies"] == int(want["plies"].sum())
    assert stats["disabled_games"] == int((~want["enabled"]).sum())


# ------------------------------------------------------------------ 1. whole games against the statement
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("slots", [1, 4, 5])
@pytest.mark.parametrize("N", [3, 5])
def test_whole_games_match_the_statement(dev, N, slots, graph):
    from alphaquoridorgnn_amd import _lib
    want = R.generation(N)
    assert want["resigned"].any() and not want["resigned"].all()
    side = torch.cuda.Stream(device=dev)                             # a capturable stream: the move is replayed from a hipGraph
    _lib.set_option("use_graph", graph)
    try:
        with torch.cuda.stream(side):
            eng = _play_quota(slots, R.G, want["u"], N, resign_threshold=R.THRESHOLD, resign_disable_fraction=0.0, resign_seed=R.RESIGN_SEED)
            _assert_statement(eng, want)
    finally:
        _lib.set_option("use_graph", 1)


@pytest.mark.parametrize("N", [3, 5])
def test_min_ply_on_either_side_of_the_first_crossing(dev, N):
    on = R.generation(N)
    g = int(np.flatnonzero(on["resigned"])[0])
    cross = int(on["plies"][g]) - 1
    for min_ply in (cross, cross + 1):
        want = R.generation(N, min_ply=min_ply)
        eng = _play_quota(4, R.G, want["u"], N, resign_threshold=R.THRESHOLD, resign_min_ply=min_ply, resign_disable_fraction=0.0,
                          resign_seed=R.RESIGN_SEED)
        _assert_statement(eng, want)
        assert (eng.t["game_plies"][g].item() == cross + 1) == (min_ply == cross)


@pytest.mark.parametrize("fraction", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N", [3, 5])
def test_disabled_games_play_on(dev, N, fraction):
    from alphaquoridorgnn_amd.engine import draw_resign_enabled
    want = R.generation(N, disable_fraction=fraction)
    eng = _play_quota(5, R.G, want["u"], N, resign_threshold=R.THRESHOLD, resign_disable_fraction=fraction, resign_seed=R.RESIGN_SEED)
    _assert_statement(eng, want)
    enabled = draw_resign_enabled(R.RESIGN_SEED, np.arange(R.G), fraction)
    assert eng.resign_arrays()[2].tolist() == enabled.tolist()
    flag = eng.t["game_resigned"].cpu().numpy().astype(bool)
    assert not flag[~enabled].any() and (fraction == 1.0 or flag.any())
    stats = eng.resign_stats()
    if fraction == 1.0:                                               # every game was played out: the count is the statement's
        lose = np.stack([want["result"] < 0, want["result"] > 0], axis=1)
        would = want["minima"] < -np.float32(R.THRESHOLD)
        assert (stats["would_resign"], stats["false_positives"]) == (int(would.sum()), int((would & ~lose).sum()))
        assert stats["would_resign"] > 0


# ------------------------------------------------------------------ 2. a threshold of 1.0 = the engine without the option
@pytest.mark.parametrize("kind", ["fake", "general"])
def test_threshold_one_changes_nothing(dev, kind):
    N, G, sims = 5, 8, 12
    kw = dict(seed=6, record_search_value=True, temperature_plies=4, quota=12)
    if kind == "general":
        from tests.test_gnn_any_shape import _make_net
        kw.update(model=_make_net((6, 16, 2), R.T.action_count(N), seed=11, N=N), evaluator="general")
    else:
        kw.update(fake_bias=2)
    a = _engine(G, sims, N, **kw)
    a.play_generation()
    b = _engine(G, sims, N, resign_threshold=1.0, resign_disable_fraction=0.3, **kw)
    b.play_generation()
    ra, rb = _game_rows(a), _game_rows(b)
    assert [r[:3] + r[4:] for r in ra] == [r[:3] + r[4:] for r in rb]
    assert all(torch.equal(a.t[k], b.t[k]) for k in ("hist_state72", "hist_visits", "hist_action", "hist_value", "root_state", "counters"))
    assert not bool(b.t["game_resigned"].any())
    lo = b.t["resign_min"].cpu().numpy()
    assert np.isfinite(lo).all() and (lo >= -1).all() and b.resign_stats()["games_resigned"] == 0      # ... while the statistics are kept
    hv, plies = a.t["hist_value"].cpu().numpy(), a.t["game_plies"].cpu().numpy()
    for k in range(12):                                               # m >= v_root: the minimum is bounded by the recorded values
        for s in (0, 1):
            assert lo[k, s] >= hv[k, s:plies[k]:2].min()


# ------------------------------------------------------------------ 3. independence from slots, refill and sets
def test_a_games_rows_do_not_depend_on_its_slot(dev):
    N, G, quota = 5, 4, 12
    U_game = np.random.RandomState(78).random_sample(size=(quota, 28))
    kw = dict(resign_threshold=R.THRESHOLD, resign_disable_fraction=0.3, resign_seed=11, seed=9)
    refill = _play_quota(G, quota, U_game, N, **kw)                   # three games per slot
    wide = _play_quota(quota, quota, U_game, N, **kw)                 # one slot per game
    assert _game_rows(refill) == _game_rows(wide) and refill.resign_stats() == wide.resign_stats()
    flag, enabled = wide.t["game_resigned"].cpu().numpy().astype(bool), wide.resign_arrays()[2]
    assert flag.any() and not flag.all() and not enabled.all() and not flag[~enabled].any()
    plain = _play_quota(quota, quota, U_game, N, seed=9)
    assert [r[0] for r in _game_rows(plain)] != [r[0] for r in _game_rows(wide)]


def test_two_sets_play_the_single_sets_games(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay, draw_resign_enabled
    N, sims, G = 5, R.SIMS, 8
    kw = dict(board_size=N, evaluator="fake", fake_bias=2, record_search_value=True, resign_threshold=R.THRESHOLD, resign_disable_fraction=0.4)
    ms = MultiSetSelfPlay(None, num_games=G, sims=sims, num_sets=2, seed=3, quota=3 * G, resign_seed=77, **kw)
    ms.play_generation()
    ms.sync()
    parts = []
    for i, s in enumerate(ms.sets):                       # set i is a stand-alone engine of seed 3 * 64 + i and the set's resignation seed
        alone = _engine(s.G, sims, N, seed=3 * 64 + i, quota=s.quota, resign_seed=s.resign_seed,
                        **{k: v for k, v in kw.items() if k not in ("board_size", "evaluator")})
        alone.play_generation()
        assert _game_rows(alone) == _game_rows(s)
        parts.append(alone.resign_arrays())
    total = ms.resign_arrays()
    assert all(np.concatenate([p[i] for p in parts]).tobytes() == total[i].tobytes() for i in range(6))
    # the sets' games are numbered through: the enabled set is the draw of (resign_seed, game index over the whole engine)
    assert total[2].tolist() == draw_resign_enabled(77, np.arange(3 * G), 0.4).tolist()
    stats = ms.resign_stats()
    assert stats["games"] == 3 * G and 0 < stats["games_resigned"] < 3 * G and stats["disabled_games"] == int((~total[2]).sum()) > 0
    assert ms.suggest_resign_threshold(0.05, min_sides=50) is None   # 24 games have 48 sides: too few to say


# ------------------------------------------------------------------ 4. beside tree reuse, the schedule and root noise
@pytest.mark.parametrize("slots", [8, 3])
def test_with_tree_reuse_schedule_and_table_noise(dev, slots):
    """The statement extended the same way.  On 3 slots a resigned slot takes a new game: its rows are those of a game started from a
    fresh tree, which is what the statement plays."""
    N, keep, K, eps = 5, 6, 3, 0.25
    want = R.generation(N, disable_fraction=0.3, keep=keep, K=K, noise_seed=41, eps=eps)
    assert want["resigned"].any() and not want["resigned"].all()
    assert any(r["kept"] for rows in want["games"] for r in rows)
    assert want["visits"].tobytes() != R.generation(N, disable_fraction=0.3)["visits"].tobytes()
    eng = _play_quota(slots, R.G, want["u"], N, tables=want["tables"], resign_threshold=R.THRESHOLD, resign_disable_fraction=0.3,
                      resign_seed=R.RESIGN_SEED, tree_reuse=True, tree_reuse_visits=keep, temperature_plies=K, root_noise_eps=eps)
    _assert_statement(eng, want)
    assert eng.tree_reuse_stats()["moves_kept"] == sum(r["kept"] for rows in want["games"] for r in rows)
    # no slot is left marked, and no child index is left behind a game that ended
    assert not bool(eng.t["kept"].any()) and bool((eng.t["child_index"] == -1).all())


# ------------------------------------------------------------------ 5. the other evaluators
def _net(kind, N, dev):
    if kind == "general":
        from tests.test_gnn_any_shape import _make_net
        return _make_net((6, 16, 2), R.T.action_count(N), seed=11, N=N)
    if kind == "cnn":
        from tests.test_cnn import _make_net
        return _make_net(8, 1, N, seed=12).to(dev)
    from tests.test_gpu_parity import _model
    return _model(2)[0]


def _played(eng, limit=40):
    for _ in range(min(limit, eng.max_plies)):
        eng.move()
    keys = ("hist_state72", "hist_visits", "hist_action", "hist_value", "game_plies", "game_result", "game_done", "root_state", "resign_min",
            "game_resigned")
    return tuple(eng.t[k].cpu() for k in keys if k in eng.t)


@pytest.mark.parametrize("kind,N", [("gnn", 9), ("general", 5), ("cnn", 5)])
def test_network_evaluators(dev, kind, N):
    """Random weights give values near 0: the threshold is chosen from the played-out run's own minima so that some games resign and
    some do not, and the resigned games then are the played-out ones cut at their first crossing."""
    net = _net(kind, N, dev)
    G, sims = 8, 8
    kw = dict(model=net, evaluator=kind, seed=4, record_search_value=True, resign_seed=5, resign_disable_fraction=0.25,
              resign_min_ply=2)                                       # (ply 0 is the same position, with the same value, in every game)
    full = _engine(G, sims, N, eval_cache_slots=0, resign_threshold=1.0, **kw)
    base = _played(full)
    lo = base[8].numpy()
    low = np.sort(lo.min(axis=1))
    assert low[2] < low[5] < 0                                        # games differ in how bad they ever looked
    thr = float(-(low[2] + low[5]) / 2)
    on = _played(_engine(G, sims, N, eval_cache_slots=0, resign_threshold=thr, **kw))
    cached = _engine(G, sims, N, eval_cache_slots=64, resign_threshold=thr, **kw)
    assert all(torch.equal(x, y) for x, y in zip(_played(cached), on))
    print(f"{kind}: threshold {thr:.4f}, {int(on[9].sum())} of {G} games resigned, {cached.counters()['cache_hits']} evaluation-cache hits")
    flag, plies, act = on[9].numpy().astype(bool), on[4].numpy(), on[2].numpy()
    enabled = cached.resign_arrays()[2]
    assert flag.any() and not flag[~enabled].any()
    for k in range(G):
        n = int(plies[k])
        if flag[k]:                                                   # the played-out game up to the resigning row, whose action is 0xFF
            assert act[k, n - 1] == 0xFF and n <= int(base[4][k])
            assert torch.equal(on[1][k, :n], base[1][k, :n]) and torch.equal(on[3][k, :n], base[3][k, :n])
            assert torch.equal(on[2][k, :n - 1], base[2][k, :n - 1])
            side = (n - 1) & 1
            assert on[8][k, side] < -np.float32(thr) and on[6][k] == 1 and on[5][k] == (-1 if side == 0 else 1)
        else:
            assert torch.equal(on[1][k], base[1][k]) and torch.equal(on[2][k], base[2][k]) and torch.equal(on[8][k], base[8][k])
            assert not enabled[k] or lo[k].min() >= -np.float32(thr)          # enabled and played out: it never crossed


def test_external_evaluator_plays_the_statement(dev):
    from tests.test_gpu_parity import _OracleFakeAdapter
    N = 3
    want = R.generation(N, disable_fraction=0.5)
    eng = _engine(R.G, R.SIMS, N, model=_OracleFakeAdapter(2), evaluator="external", record_search_value=True, resign_threshold=R.THRESHOLD,
                  resign_disable_fraction=0.5, resign_seed=R.RESIGN_SEED)
    for m in range(eng.max_plies):
        eng.move(torch.from_numpy(np.ascontiguousarray(want["u"][:, m])))
    assert eng.counters()["active"] == 0
    _assert_statement(eng, want)


# ------------------------------------------------------------------ 6. refusals on a live engine
def test_refusals(dev):
    import ctypes
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    eng = _engine(4, 8, 5, resign_threshold=0.5)
    with pytest.raises(ValueError, match="resign_threshold"):
        eng.apply_actions(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="resign_threshold"):
        eng.search(np.zeros((4, 72), np.uint8))
    with pytest.raises(ValueError, match="resign"):
        eng.set_resign_threshold(0.0)
    with pytest.raises(ValueError, match="never resigns a game"):
        BatchedMatch((0, 1), 2, sims=4, board_size=5, evaluator="fake", resign_threshold=0.5)
    with pytest.raises(ValueError, match="resign_threshold"):
        _engine(4, 8, 5).resign_stats()
    before = {k: v.clone() for k, v in eng.t.items()}
    u = torch.zeros(4, dtype=torch.float64, device=dev)
    e, rs = ctypes.byref(eng.e), eng.resign

    def refused(word, **fields):
        bad = _lib.ResignStruct()
        ctypes.memmove(ctypes.byref(bad), ctypes.byref(rs), ctypes.sizeof(bad))
        for k, v in fields.items():
            setattr(bad, k, v)
        for call in (lambda: eng.lib.aqg_engine_move_resign(e, _lib.ptr(u), 0, None, None, ctypes.byref(bad), eng._stream()),
                     lambda: eng.lib.aqg_engine_finish_move_resign(e, _lib.ptr(u), 0, None, None, ctypes.byref(bad), eng._stream()),
                     lambda: eng.lib.aqg_engine_reset_resign(e, ctypes.byref(bad), eng._stream())):
            assert call() != 0 and word in eng.lib.aqg_last_error().decode()
    refused("threshold", threshold=0.0)
    refused("threshold", threshold=1.5)
    refused("min_ply", min_ply=-1)
    refused("disable_fraction", disable_fraction=1.5)
    refused("required", resign_min=None)
    refused("required", game_resigned=None)
    nohist = _engine(4, 8, 5, record_history=False)
    assert nohist.lib.aqg_engine_move_resign(ctypes.byref(nohist.e), _lib.ptr(u), 0, None, None, ctypes.byref(rs), nohist._stream()) != 0
    assert "max_plies" in nohist.lib.aqg_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(v, eng.t[k]) for k, v in before.items())    # nothing was launched
    eng.set_resign_threshold(0.75)
    assert eng.resign.threshold == 0.75 and eng.resign_options[0] == 0.75


def test_reset_clears_the_statistics(dev):
    eng = _engine(8, R.SIMS, 5, fake_bias=2, resign_threshold=R.THRESHOLD, resign_disable_fraction=0.0, seed=2, record_search_value=True)
    eng.play_generation()
    first = _game_rows(eng)
    assert bool(eng.t["game_resigned"].any()) and bool(torch.isfinite(eng.t["resign_min"]).any())
    eng.reset()
    assert not bool(eng.t["game_resigned"].any()) and bool(torch.isinf(eng.t["resign_min"]).all()) and bool((eng.t["resign_min"] > 0).all())
    eng.gen.manual_seed(2)
    eng.play_generation()
    assert _game_rows(eng) == first


# ------------------------------------------------------------------ 7. self_play() end to end
_LOOP = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, engine, pv_mcts, self_play as sp
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
from alphaquoridorgnn_amd.replay import ReplayWindow

assert constants.BOARD_SIZE == 5
torch.manual_seed(3)
dev = aqd.device()
model = GraphPolicyValueNetwork(6, 16, 2, 57, board_size=5).to(dev).eval()
pv_mcts.PV_EVALUATE_COUNT = 8
GAMES, SEED = 12, 17


def generation(threshold, slots, fraction=0.25):
    sp.SP_RESIGN_THRESHOLD, sp.SP_SLOTS, sp.SP_RESIGN_DISABLE_FRACTION, sp.SP_RESIGN_MIN_PLY = threshold, slots, fraction, 2
    sp.SP_REPLAY = ReplayWindow(5, max_generations=1, capacity_rows=4096, device=dev)
    path = sp.self_play(model, games=GAMES, seed=SEED)
    with open(path, "rb") as f:
        rows = pickle.load(f)
    os.remove(path)
    return rows, [x.cpu().numpy() for x in sp.SP_REPLAY.rows()]


def engine_rows(slots, **kw):
    """An engine built as self_play() builds its own."""
    eng = engine.MultiSetSelfPlay(model, num_games=slots, quota=GAMES, sims=8, num_sets=1, board_size=5, temperature=sp.SP_TEMPERATURE,
                                  seed=SEED % (2 ** 31 - 1), device=dev, evaluator="general", **kw)
    eng.play_generation()
    return eng, [x.cpu().numpy() for x in eng.history_tensors()]


off_rows, off_ring = generation(None, None)
print("OFF_KEEPS_NO_STATISTICS", sp.SP_RESIGN_LAST is None)
eng, want = engine_rows(GAMES)
print("OFF_IS_THE_ENGINE", np.array_equal(off_ring[0][:, :70], want[0][:, :70]), len(off_rows) == len(want[0]))
slot_rows, slot_ring = generation(None, 3)
eng, want = engine_rows(3)
print("SLOTS_IS_THE_REFILL_ENGINE", np.array_equal(slot_ring[0][:, :70], want[0][:, :70]), len(slot_rows) == len(want[0]),
      eng.sets[0].G == 3 and eng.sets[0].quota == GAMES)

# collect first: the played-out minima say which threshold resigns some games and not others
all_rows, _ = generation(1.0, 3, 1.0)
last = sp.SP_RESIGN_LAST
lo = last["arrays"][0]
low = np.sort(lo.min(axis=1))
thr = float(-(low[5] + low[8]) / 2)
print("COLLECTING_RESIGNS_NOTHING", last["stats"]["games_resigned"] == 0 and last["stats"]["disabled_games"] == GAMES,
      [r[:2] for r in all_rows] == [r[:2] for r in slot_rows], low[5] < low[8] < 0)
on_rows, on_ring = generation(thr, 3)
last = sp.SP_RESIGN_LAST
kw = dict(resign_threshold=thr, resign_min_ply=2, resign_disable_fraction=0.25)
eng, want = engine_rows(3, **kw)
stats = eng.resign_stats()
print("RESIGNED_SOME", 0 < stats["games_resigned"] < GAMES, stats["plies"] == len(on_rows) < len(all_rows))
print("RING_IS_THE_ENGINE", np.array_equal(on_ring[0][:, :70], want[0][:, :70]),
      np.array_equal(on_ring[2], want[2].astype(np.float32)), len(on_rows) == len(want[0]))
pol = want[1].astype(np.float64)
pol = pol / pol.sum(1, keepdims=True)
print("FILE_IS_THE_ENGINE", [r[2] for r in on_rows] == want[2].tolist(), np.allclose(np.array([r[1] for r in on_rows]), pol, rtol=0, atol=1e-15))
print("STATISTICS_ARE_THE_ENGINES", last["stats"] == stats, last["threshold"] == thr,
      all(a.tobytes() == b.tobytes() for a, b in zip(last["arrays"], eng.resign_arrays())))
flag, plies = last["arrays"][3].astype(bool), last["arrays"][4]
ends = np.cumsum(plies) - 1
print("RESIGNING_ROWS_READ_MINUS_ONE", all(on_rows[e][2] == -1 for e, f in zip(ends, flag) if f), int(flag.sum()) == stats["games_resigned"])
'''


def test_self_play_with_the_options(dev, tmp_path):
    """One child process on the 5x5 board (the module's board size comes from the environment): self_play() with SP_SLOTS alone, then
    collecting (threshold 1.0, every game played out), then with a threshold taken from the collected minima, against engines built
    as self_play() builds its own: the ring, the file and the gathered statistics are the engine's."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("OFF_KEEPS_NO_STATISTICS True", "OFF_IS_THE_ENGINE True True", "SLOTS_IS_THE_REFILL_ENGINE True True True",
                 "COLLECTING_RESIGNS_NOTHING True True True", "RESIGNED_SOME True True", "RING_IS_THE_ENGINE True True True",
                 "FILE_IS_THE_ENGINE True True", "STATISTICS_ARE_THE_ENGINES True True True", "RESIGNING_ROWS_READ_MINUS_ONE True True"):
        assert line in r.stdout, (line, r.stdout[-3000:])
