"""Resignation on the host (include/aqgnn.h "resignation"): the enabled / disabled draw against a scalar restatement, the refusals of
the engine, the library and the evaluation paths, the false-positive count and the threshold suggestion on hand-made minima, the host
statement of tests/_resign.py against oracle.mcts.play, what the case lists of the GPU tests contain, and the exchange of the
statistics between two gloo ranks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _resign as R   # noqa: E402

INF = np.float32(np.inf)


# ------------------------------------------------------------------ the draw
def test_draw_resign_enabled_is_the_scalar_statement():
    from alphaquoridorgnn_amd.engine import draw_resign_enabled
    for seed in (0, 1, R.RESIGN_SEED, (1 << 64) - 1, 0x9E3779B97F4A7C15):
        ks = list(range(40)) + [255, 256, 65535, 2 ** 31 - 1]
        us = [R.uniform_scalar(seed, k) for k in ks]
        assert all(0.0 <= u < 1.0 for u in us) and len(set(us)) == len(us)
        for frac in (0.0, 0.1, 0.5, 1.0, us[3], np.nextafter(us[3], 1.0)):
            want = [u >= frac for u in us]
            assert draw_resign_enabled(seed, np.asarray(ks), frac).tolist() == want
            assert [draw_resign_enabled(seed, k, frac) for k in ks[:6]] == want[:6]
    assert draw_resign_enabled(7, np.arange(64), 0.0).all() and not draw_resign_enabled(7, np.arange(64), 1.0).any()
    share = draw_resign_enabled(7, np.arange(20000), 0.1).mean()           # a fair draw: 0.9 +- 5 sigma of 20,000 Bernoulli draws
    assert abs(share - 0.9) < 5 * np.sqrt(0.09 / 20000)


# ------------------------------------------------------------------ refusals
def test_check_resign():
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay, MultiSetSelfPlay, check_resign
    assert check_resign(None) is None and check_resign(None, 5, 0.3) is None
    assert check_resign(0.25, 3, 0.5) == (0.25, 3, 0.5) and check_resign(1.0)[0] == 1.0 and check_resign(1, 0, 0)[2] == 0.0
    assert check_resign(0.1)[0] == float(np.float32(0.1))                 # the struct's float32
    bad = (dict(resign_threshold=0.0), dict(resign_threshold=-0.1), dict(resign_threshold=1.0001), dict(resign_threshold=float("nan")),
           dict(resign_threshold=True), dict(resign_threshold="auto"), dict(resign_threshold=1e-50),
           dict(resign_threshold=0.5, resign_min_ply=-1), dict(resign_threshold=0.5, resign_min_ply=1.5),
           dict(resign_threshold=0.5, resign_disable_fraction=-0.01), dict(resign_threshold=0.5, resign_disable_fraction=1.01),
           dict(resign_threshold=0.5, resign_disable_fraction=float("nan")), dict(resign_threshold=0.5, record_history=False))
    for kw in bad:
        with pytest.raises(ValueError, match="resign"):
            check_resign(kw["resign_threshold"], kw.get("resign_min_ply", 0), kw.get("resign_disable_fraction", 0.1),
                         kw.get("record_history", True))
    for kw in bad:                                                         # ... and the engines refuse before they touch a device
        with pytest.raises(ValueError, match="resign"):
            BatchedSelfPlay(None, num_games=2, sims=8, board_size=5, evaluator="fake", **kw)
        with pytest.raises(ValueError, match="resign"):
            MultiSetSelfPlay(None, num_games=2, sims=8, board_size=5, evaluator="fake", **kw)


def test_moves_nobody_searched_and_searches_refuse():
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    eng = BatchedSelfPlay.__new__(BatchedSelfPlay)      # both refuse before they touch anything
    eng.tree_reuse, eng.resign = False, object()
    with pytest.raises(ValueError, match="resign_threshold"):
        eng.search(np.zeros((1, 72), np.uint8))
    with pytest.raises(ValueError, match="resign_threshold"):
        eng.apply_actions(np.zeros((1,), np.int32))
    off = type("E", (), {"resign": None, "resign_arrays": BatchedSelfPlay.resign_arrays})()
    for call in (BatchedSelfPlay.resign_stats, BatchedSelfPlay.resign_arrays, lambda e: BatchedSelfPlay.suggest_resign_threshold(e, 0.05),
                 lambda e: BatchedSelfPlay.set_resign_threshold(e, 0.5)):
        with pytest.raises(ValueError, match="resign_threshold"):
            call(off)


@pytest.mark.parametrize("opt", [dict(resign_threshold=0.5), dict(resign_min_ply=0), dict(resign_disable_fraction=0.1), dict(resign_seed=3)])
def test_matches_and_evaluation_paths_refuse(opt):
    from alphaquoridorgnn_amd import evaluate_agents, evaluate_network, pv_mcts
    word = "never resigns a game"
    with pytest.raises(ValueError, match=word):
        evaluate_network.BatchedMatch((0, 1), 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(ValueError, match=word):
        evaluate_agents.BatchedAgentMatch(0, "random", 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(ValueError, match=word):
        pv_mcts.pv_mcts_policy_batch(None, np.zeros((1, 72), np.uint8), 1.0, evaluator="fake", **opt)
    with pytest.raises(ValueError, match=word):
        pv_mcts.pv_mcts_action(None, **opt)
    with pytest.raises(ValueError, match=word):
        evaluate_network.evaluate_network(**opt)
    with pytest.raises(ValueError, match=word):
        evaluate_agents.evaluate_best_player(**opt)


def _structs(threshold=0.25, min_ply=0, fraction=0.1, max_plies=28):
    from alphaquoridorgnn_amd import _lib
    e = _lib.EngineStructGeneral()
    e.board_size, e.num_games, e.quota, e.sims, e.prior_mode, e.max_plies = 5, 4, 4, 8, 1, max_plies
    e.node_cap = 1 + 8 * 136
    for name in ("slot_game", "game_done", "game_slot", "game_first_move"):
        setattr(e, name, 0x1000)
    rs = _lib.ResignStruct()
    rs.threshold, rs.min_ply, rs.disable_fraction, rs.seed = threshold, min_ply, fraction, 5
    rs.resign_min = rs.game_resigned = 0x1000
    return e, rs


@pytest.mark.parametrize("kw,word", [(dict(threshold=0.0), "threshold"), (dict(threshold=-0.5), "threshold"), (dict(threshold=1.5), "threshold"),
                                     (dict(threshold=float("nan")), "threshold"), (dict(min_ply=-1), "min_ply"),
                                     (dict(fraction=-0.1), "disable_fraction"), (dict(fraction=1.1), "disable_fraction"),
                                     (dict(fraction=float("nan")), "disable_fraction"), (dict(max_plies=0), "max_plies")])
def test_library_refuses_before_any_launch(kw, word):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    u = ctypes.c_void_p(0x1000)
    e, rs = _structs(**kw)
    calls = (lambda: lib.aqg_engine_move_resign(ctypes.byref(e), u, 0, None, None, ctypes.byref(rs), None),
             lambda: lib.aqg_engine_finish_move_resign(ctypes.byref(e), u, 0, None, None, ctypes.byref(rs), None),
             lambda: lib.aqg_engine_reset_resign(ctypes.byref(e), ctypes.byref(rs), None))
    for call in calls:
        assert call() != 0 and word in lib.aqg_last_error().decode()
    for name in ("resign_min", "game_resigned"):
        e, rs = _structs()
        setattr(rs, name, None)
        for call in (lambda: lib.aqg_engine_move_resign(ctypes.byref(e), u, 0, None, None, ctypes.byref(rs), None),
                     lambda: lib.aqg_engine_finish_move_resign(ctypes.byref(e), u, 0, None, None, ctypes.byref(rs), None),
                     lambda: lib.aqg_engine_reset_resign(ctypes.byref(e), ctypes.byref(rs), None)):
            assert call() != 0 and "required" in lib.aqg_last_error().decode()
    e, rs = _structs()
    assert lib.aqg_engine_move_resign(ctypes.byref(e), u, 0, None, None, None, None) != 0
    assert lib.aqg_engine_reset_resign(ctypes.byref(e), None, None) != 0
    bad = _lib.TreeReuseStruct()                        # a tree-reuse struct beside it is checked as by the _reuse entry points
    bad.keep_visits = -1
    assert lib.aqg_engine_move_resign(ctypes.byref(e), u, 0, None, ctypes.byref(bad), ctypes.byref(rs), None) != 0
    assert "keep_visits" in lib.aqg_last_error().decode()


def test_abi_is_additive(tmp_path):
    from alphaquoridorgnn_amd import _lib
    assert _lib.ABI_VERSION == 15
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\n'
                   "int main() { std::printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %d\\n\", sizeof(aqg_engine), sizeof(aqg_resign),"
                   " offsetof(aqg_resign, threshold), offsetof(aqg_resign, min_ply), offsetof(aqg_resign, disable_fraction),"
                   " offsetof(aqg_resign, seed), offsetof(aqg_resign, resign_min), offsetof(aqg_resign, game_resigned),"
                   " AQG_ABI_VERSION); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E, S = _lib.EngineStructGeneral, _lib.ResignStruct
    assert got == [ctypes.sizeof(E), ctypes.sizeof(S), S.threshold.offset, S.min_ply.offset, S.disable_fraction.offset, S.seed.offset,
                   S.resign_min.offset, S.game_resigned.offset, 15]
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert "resignation (additive to ABI 15" in header
    for name in ("aqg_engine_move_resign", "aqg_engine_finish_move_resign", "aqg_engine_reset_resign"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header


# ------------------------------------------------------------------ the calibration
def test_false_positive_count_on_hand_made_games():
    from alphaquoridorgnn_amd.engine import resign_false_positives, resign_stats_of
    #            game: 0 first wins   1 second wins   2 draw          3 first wins (enabled)  4 second wins, never eligible
    lo = np.array([[-0.1, -0.6], [-0.5, -0.5], [-0.3, 0.2], [-0.9, -0.9], [INF, INF]], dtype=np.float32)
    res = np.array([1, -1, 0, 1, -1], dtype=np.int8)
    enabled = np.array([False, False, False, True, False])
    # T = 0.25: sides below -0.25 among the disabled games: (0, second: lost), (1, first: lost), (1, second: won -> false), (2, first: drew
    # -> false).  Non-losing sides: game 0 first, 1 second, 2 both, 4 second = 5.
    assert resign_false_positives(lo, res, enabled, 0.25) == (4, 2, 5)
    assert resign_false_positives(lo, res, enabled, 0.5) == (1, 0, 5)          # strict: a minimum of exactly -0.5 does not resign
    assert resign_false_positives(lo, res, enabled, np.nextafter(np.float32(0.5), np.float32(0))) == (3, 1, 5)
    assert resign_false_positives(lo, res, enabled, 1.0) == (0, 0, 5)
    assert resign_false_positives(lo, res, np.ones(5, bool), 0.25) == (0, 0, 0)
    plies, flag, done = np.array([10, 12, 28, 5, 9], np.int32), np.array([0, 0, 0, 1, 0], np.uint8), np.array([1, 1, 1, 1, 0], np.uint8)
    s = resign_stats_of([(lo, res, enabled, flag, plies, done)], 0.25)         # game 4 is not finished: it does not count
    assert s == dict(games=4, games_resigned=1, plies=55, disabled_games=3, would_resign=4, false_positives=2, false_positive_rate=0.5,
                     eligible_sides=4)
    two = resign_stats_of([(lo[:2], res[:2], enabled[:2], flag[:2], plies[:2], done[:2]), (lo[2:], res[2:], enabled[2:], flag[2:], plies[2:], done[2:])], 0.25)
    assert two == s
    assert resign_stats_of([(lo, res, enabled, flag, plies, done)], 1.0)["false_positive_rate"] == 0.0


def _sides(minima, losers=-1.0):
    """Played-out games the first player won: the winner's running minimum as given, the loser's `losers` (a value or one per game)."""
    n = len(minima)
    lo = np.stack([np.asarray(minima, dtype=np.float32), np.broadcast_to(np.asarray(losers, dtype=np.float32), (n,))], axis=1)
    return lo, np.ones(n, dtype=np.int8), np.zeros(n, dtype=bool)


def test_suggest_resign_threshold_on_hand_made_minima():
    from alphaquoridorgnn_amd.engine import resign_false_positives, suggest_resign_threshold as suggest
    # 40 played-out games: the losers' minima are -0.02, -0.04 .. -0.80; four winners looked lost once, at -0.70, -0.30, -0.28, -0.26
    losers = -np.arange(1, 41, dtype=np.float64) / 50.0
    winners = np.full(40, 0.1)
    winners[[3, 9, 20, 31]] = (-0.70, -0.30, -0.28, -0.26)
    lo, res, en = _sides(winners, losers)
    # bound 5 %: below -0.30 lie 25 losers and one winner (1 / 26); any higher cut lets in the winners at -0.30 .. -0.26 faster than
    # losers (2 / 28, 3 / 30, 4 / 32 .. 4 / 41 at the floor).  The loser and the winner AT -0.30 are tied with the cut: neither resigns.
    t = suggest(lo, res, en, 0.05)
    assert t == float(np.float32(0.3))
    assert resign_false_positives(lo, res, en, t) == (26, 1, 40)
    looser = np.nextafter(np.float32(t), np.float32(0))                        # the next smaller threshold takes both tied sides in
    assert resign_false_positives(lo, res, en, looser) == (28, 2, 40)
    for cut in np.unique(lo[lo < -np.float32(0.05)]):                         # every candidate above the answer breaks the bound
        would, wrong, _ = resign_false_positives(lo, res, en, -cut)
        assert cut <= np.float32(-0.3) or wrong > 0.05 * would, cut
    assert resign_false_positives(lo, res, en, 0.68)[:2] == (7, 1)            # (the rate does not fall steadily: 1 / 7 below -0.68)
    # a bound of 0: no winner may have resigned -- only cuts at or below -0.70 qualify, and five sides lie below that one
    assert suggest(lo, res, en, 0.0) is None                                   # ... too few to say by default
    t0 = suggest(lo, res, en, 0.0, min_sides=5)
    assert t0 == float(np.float32(0.7)) and resign_false_positives(lo, res, en, t0) == (5, 0, 40)
    assert suggest(lo, res, en, 0.0, min_sides=6) is None
    # enabled games never count: the same answer with a crowd of them added, whatever their minima and results
    lo3 = np.concatenate([lo, np.full((30, 2), -0.99, dtype=np.float32)])
    res3 = np.concatenate([res, np.zeros(30, dtype=np.int8)])
    en3 = np.concatenate([en, np.ones(30, dtype=bool)])
    assert suggest(lo3, res3, en3, 0.05) == t
    # too few sides to say: no played-out game at all, none recorded, fewer would-resign sides than min_sides, fewer than 1 / bound
    assert suggest(lo, res, np.ones(40, bool), 0.05) is None
    assert suggest(np.zeros((0, 2), np.float32), np.zeros(0, np.int8), np.zeros(0, bool), 0.05) is None
    assert suggest(lo[:19], res[:19], en[:19], 0.05) is None and suggest(lo, res, en, 0.05, min_sides=27) is None
    assert suggest(lo, res, en, 0.05, min_sides=26) == t
    assert suggest(lo, res, en, 0.01) is None                                  # 1 / bound = 100 sides, and at most 44 ever looked lost
    # winners that never looked lost: every cut qualifies, the floor wins; sides without an eligible ply (+inf) never resign
    lo4, res4, en4 = _sides(np.full(40, 0.3), losers)
    assert suggest(lo4, res4, en4, 0.05) == float(np.float32(0.05)) and resign_false_positives(lo4, res4, en4, 0.05) == (38, 0, 40)
    assert suggest(lo4, res4, en4, 0.05, min_threshold=0.2) == float(np.float32(0.2))
    lo5, res5, en5 = _sides([INF] * 40, losers)
    assert suggest(lo5, res5, en5, 0.0) == float(np.float32(0.05))
    # games that look lost and end in draws are all false positives: never resign
    draws = np.full((40, 2), -0.5, dtype=np.float32)
    assert suggest(draws, np.zeros(40, np.int8), np.zeros(40, bool), 0.05) is None
    assert resign_false_positives(draws, np.zeros(40, np.int8), np.zeros(40, bool), 0.25) == (80, 80, 80)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="max_false_positive"):
            suggest(lo, res, en, bad)
    with pytest.raises(ValueError, match="min_threshold"):
        suggest(lo, res, en, 0.05, min_threshold=0.0)


# ------------------------------------------------------------------ the statement
@pytest.mark.parametrize("N", [3, 5])
def test_statement_with_threshold_one_is_oracle_play(N):
    from oracle import mcts as om
    u = R.uniforms_of(N)
    for g in range(3):
        rows, z0, resigned, minima = R.play_game(N, R.SIMS, u[g], 1.0)
        ref = om.play(om.FakeModel(2), R.SIMS, N=N, uniforms=list(u[g]))
        assert not resigned and len(rows) == len(ref) and z0 == ref[0][2]
        assert all(r["action"] != 0xFF for r in rows)
        assert all(np.array_equal(r["rec"][:4], np.asarray(s[0] + s[1])) for r, (s, _, _) in zip(rows, ref))
        assert all(np.allclose(r["visits"] / r["visits"].sum(), pol, rtol=0, atol=1e-15) for r, (_, pol, _) in zip(rows, ref))
        assert (minima >= -1.0).all() and np.isfinite(minima).all()            # m >= -1: a threshold of 1 is never reached
        off = R.play_game(N, R.SIMS, u[g], None)
        assert off[1] == z0 and not off[2] and np.isinf(off[3]).all()
        assert all(a["visits"].tobytes() == b["visits"].tobytes() and a["action"] == b["action"] for a, b in zip(off[0], rows))


def test_resign_value_takes_the_first_maximum():
    from tests._tree_reuse import Node
    root = Node(None, 0)
    root.w, root.n = -3.0, 7
    kids = [Node(None, 0.3, a) for a in range(3)]
    for c, (w, n) in zip(kids, ((1.0, 2), (2.0, 4), (-3.0, 4))):
        c.w, c.n = w, n
    root.children = kids
    assert R.resign_value(root, [2, 4, 4]) == np.float32(max(np.float32(-3.0 / 7), np.float32(-2.0 / 4)))      # child 1, not child 2
    kids[0].n, kids[1].n, kids[2].n = 0, 0, 0
    assert R.resign_value(root, [0, 0, 0]) == np.float32(0.0)                                                  # no visit: q = 0


# ------------------------------------------------------------------ what the GPU tests' cases contain
@pytest.mark.parametrize("N", [3, 5])
def test_the_gpu_cases_hold_what_they_claim(N):
    on, off = R.generation(N), R.generation(N, threshold=None)
    early = [g for g in range(R.G) if on["resigned"][g] and on["plies"][g] < off["plies"][g]]
    ruled = [g for g in range(R.G) if not on["resigned"][g]]
    assert early and ruled                                   # a game that resigns before its rule end, and one that reaches it
    assert all(on["plies"][g] == off["plies"][g] and on["result"][g] == off["result"][g] for g in ruled)
    assert all(on["games"][g][-1]["action"] == 0xFF for g in early)
    assert on["enabled"].all() and not off["resigned"].any()
    # the resigning row's z is -1, and every earlier row of the game is the played-out game's
    row = 0
    for g in range(R.G):
        n = int(on["plies"][g])
        if on["resigned"][g]:
            assert on["z"][row + n - 1] == -1
            a, b = on["games"][g], off["games"][g]
            assert all(x["visits"].tobytes() == y["visits"].tobytes() for x, y in zip(a, b))
            assert all(x["action"] == y["action"] for x, y in zip(a[:-1], b))
        row += n
    # min_ply on either side of a first crossing: at the crossing ply the game resigns there, one later it plays on past it
    g = early[0]
    cross = int(on["plies"][g]) - 1
    at, past = R.generation(N, min_ply=cross), R.generation(N, min_ply=cross + 1)
    assert at["resigned"][g] and at["plies"][g] == cross + 1
    assert past["plies"][g] > cross + 1
    # in between: the enabled set is the draw's, holds both kinds, and a disabled game that would have resigned plays on
    from alphaquoridorgnn_amd.engine import draw_resign_enabled
    half = R.generation(N, disable_fraction=0.5)
    assert half["enabled"].tolist() == draw_resign_enabled(R.RESIGN_SEED, np.arange(R.G), 0.5).tolist()
    assert half["enabled"].any() and not half["enabled"].all()
    played_on = [k for k in early if not half["enabled"][k]]
    assert played_on and all(half["plies"][k] == off["plies"][k] and not half["resigned"][k] for k in played_on)
    assert any(half["resigned"][k] for k in early if half["enabled"][k])
    # an enabled / disabled pair that differs only in the flag: the same game under disable_fraction 0 and 1
    none = R.generation(N, disable_fraction=1.0)
    k = played_on[0]
    assert not none["enabled"].any() and not none["resigned"].any() and on["resigned"][k]
    assert none["minima"][k].tobytes() == half["minima"][k].tobytes()
    assert none["minima"][k][cross_side(on, k)] < -R.THRESHOLD


def cross_side(on, k):
    return (int(on["plies"][k]) - 1) & 1


# ------------------------------------------------------------------ the exchange
_GLOO_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch.distributed as dist
from alphaquoridorgnn_amd.engine import gather_resign_arrays, resign_stats_of, suggest_from_arrays
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + os.environ["AQG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()


def shard(rank):
    n = 30 if rank == 0 else 17                 # ragged
    rng = np.random.RandomState(rank)
    lo = (-rng.random_sample((n, 2))).astype(np.float32)
    lo[0] = np.inf
    lo[1, 1] = -0.0
    res = rng.randint(-1, 2, size=n).astype(np.int8)
    enabled = rng.random_sample(n) < 0.5
    flag = (rng.random_sample(n) < 0.3).astype(np.uint8)
    plies = rng.randint(1, 200000, size=n).astype(np.int32)
    done = np.ones(n, np.uint8)
    done[2] = 0
    return lo, res, enabled, flag, plies, done


want = tuple(np.concatenate([a, b]) for a, b in zip(shard(0), shard(1)))
got = gather_resign_arrays(shard(r))
assert len(got) == 6 and all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)), r
assert resign_stats_of([got], 0.25) == resign_stats_of([shard(0), shard(1)], 0.25)
assert suggest_from_arrays([got], 0.9, min_sides=5) == suggest_from_arrays([shard(0), shard(1)], 0.9, min_sides=5) is not None
got = gather_resign_arrays(None if r == 1 else shard(0))        # a rank without a game
assert all(g.tobytes() == w.tobytes() for g, w in zip(got, shard(0)))
dist.destroy_process_group()
print("ok", r)
'''


def test_resign_statistics_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    port = str(33500 + os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), AQG_REPO=REPO, AQG_PORT=port, MASTER_ADDR="127.0.0.1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=120)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o


def test_gather_without_a_group_returns_the_arrays():
    from alphaquoridorgnn_amd.engine import gather_resign_arrays
    a = (np.array([[-0.5, INF]], np.float32), np.array([-1], np.int8), np.array([True]), np.array([1], np.uint8), np.array([9], np.int32),
         np.array([1], np.uint8))
    got = gather_resign_arrays(a)
    assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, a))
    assert all(x.shape[0] == 0 for x in gather_resign_arrays(None))


# ------------------------------------------------------------------ the loop's options
def test_option_defaults_and_flags():
    from alphaquoridorgnn_amd import self_play as sp, train_cycle as tc
    assert sp.SP_RESIGN_THRESHOLD is None and sp.SP_RESIGN_MIN_PLY == 0 and sp.SP_RESIGN_DISABLE_FRACTION == 0.1 and sp.SP_SLOTS is None
    assert sp._resign_options() == ({}, None)
    saved = {k: getattr(sp, k) for k in ("SP_RESIGN_THRESHOLD", "SP_RESIGN_MIN_PLY", "SP_RESIGN_MAX_FALSE_POSITIVE", "SP_SLOTS", "SP_RESIGN_AUTO")}
    try:
        args = tc._parser().parse_args([])
        tc._set_resign_options(args)
        assert sp.SP_RESIGN_THRESHOLD is None and sp.SP_SLOTS is None
        tc._set_resign_options(tc._parser().parse_args(["--resign-threshold", "0.25", "--resign-min-ply", "6", "--slots", "8"]))
        assert (sp.SP_RESIGN_THRESHOLD, sp.SP_RESIGN_MIN_PLY, sp.SP_SLOTS) == (0.25, 6, 8)
        assert sp._resign_options() == (dict(resign_threshold=0.25, resign_min_ply=6, resign_disable_fraction=0.1), 0.25)
        tc._set_resign_options(tc._parser().parse_args(["--resign-threshold", "auto", "--resign-max-false-positive", "0.025"]))
        assert sp.SP_RESIGN_THRESHOLD == "auto" and sp.SP_RESIGN_MAX_FALSE_POSITIVE == 0.025
        # auto: generation 1 never resigns and plays every game out; afterwards the chosen threshold with the usual disabled share
        assert sp._resign_options() == (dict(resign_threshold=1.0, resign_min_ply=6, resign_disable_fraction=1.0), 1.0)
        x = -np.arange(1, 41, dtype=np.float64) / 50.0
        lo, res, en = _sides(x)
        arrays = (lo, res, en, np.zeros(40, np.uint8), np.full(40, 10, np.int32), np.ones(40, np.uint8))
        sp._after_resign_generation(arrays, 1.0, rank=1)
        assert sp.SP_RESIGN_LAST["next_threshold"] == sp.SP_RESIGN_AUTO["threshold"] == float(np.float32(0.78))      # one winner among 41 sides: 2.4 %
        assert sp._resign_options()[0] == dict(resign_threshold=float(np.float32(0.78)), resign_min_ply=6, resign_disable_fraction=0.1)
        few = tuple(a[:3] for a in arrays)
        sp.SP_RESIGN_AUTO = {"threshold": None, "parts": []}
        sp._after_resign_generation(few, 1.0, rank=1)
        assert sp.SP_RESIGN_LAST["next_threshold"] is None and sp._resign_options()[1] == 1.0                    # too few: collect again
        for argv in (["--resign-threshold", "0"], ["--resign-threshold", "1.5"], ["--resign-threshold", "x"], ["--resign-min-ply", "3"],
                     ["--resign-threshold", "0.5", "--resign-min-ply", "-1"], ["--resign-threshold", "0.5", "--resign-max-false-positive", "0.1"],
                     ["--resign-threshold", "auto", "--resign-max-false-positive", "1.0"], ["--slots", "0"]):
            with pytest.raises(ValueError):
                tc._set_resign_options(tc._parser().parse_args(argv))
    finally:
        for k, v in saved.items():
            setattr(sp, k, v)
        sp.SP_RESIGN_LAST = None
