"""Tree reuse on the GPU (include/aqgnn.h "tree reuse"; csrc/mcts_reuse.hip, csrc/mcts_move.hip): the keep launch alone, bit for bit
against engine.keep_subtree_reference, on pools of real searches and on synthetic ones; whole games bit for bit against the host
statement of tests/_tree_reuse.py; keep_visits 0 = the engine without the option; independence from slots, refill and sets; root
noise of kept and of fresh roots; the network evaluators with graph capture, the evaluation cache and the step options on and off."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _tree_reuse as T   # noqa: E402
from tests.test_root_noise_cpu import MAX_LEGAL, mix_statement   # noqa: E402

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


def _rows(eng):
    out = tuple(x.cpu() for x in eng.history_tensors()) + tuple(eng.t[k].cpu() for k in ("game_plies", "game_result", "hist_action"))
    return out + ((eng.history_values().cpu(),) if eng.record_search_value else ())


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _pools(eng):
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    return eng.t["node_rec"].cpu().numpy().view(NODE_DTYPE).reshape(eng.G, eng.node_cap).copy(), eng.t["node_count"].cpu().numpy().copy()


# ------------------------------------------------------------------ 1. the keep launch alone
def _run_keep(eng, pools, counts, child_index, keep, active):
    """Load the slots' pools, run the keep launch on child_index, and compare every slot with the reference: a kept slot's records
    [0, count) bit for bit, everything from its old count on untouched; any other slot byte for byte; the marker and the statistics."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import keep_subtree_reference
    G, cap = eng.G, eng.node_cap
    full = np.zeros((G, cap), dtype=pools[0].dtype)
    full[:] = np.frombuffer(b"\xA5" * 32, dtype=pools[0].dtype)[0]          # behind the used records: bytes nobody may touch
    for g in range(G):
        full[g, :counts[g]] = pools[g][:counts[g]]
    eng.t["node_rec"].copy_(torch.from_numpy(full.view(np.float64).reshape(G * cap, 4)))
    eng.t["node_count"].copy_(torch.from_numpy(np.asarray(counts, dtype=np.int32)))
    eng.t["game_active"].copy_(torch.from_numpy(np.asarray(active, dtype=np.uint8)))
    eng.t["kept"].fill_(1)
    eng.t["stat_moves_kept"].zero_()
    eng.t["stat_visits_kept"].zero_()
    eng.reuse.keep_visits = int(keep)
    idx = torch.from_numpy(np.asarray(child_index, dtype=np.int32)).to(eng.dev)
    _lib.check(eng.lib.aqg_engine_keep_subtrees(ctypes.byref(eng.e), ctypes.byref(eng.reuse), _lib.ptr(idx), eng._stream()), "keep")
    torch.cuda.synchronize()
    after, after_counts = _pools(eng)
    marker = eng.t["kept"].cpu().numpy()
    moves, visits = eng.t["stat_moves_kept"].cpu().numpy(), eng.t["stat_visits_kept"].cpu().numpy()
    kept_flags = []
    for g in range(G):
        want, cnt, kept = keep_subtree_reference(full[g], counts[g], child_index[g] if active[g] else -1, keep)
        kept_flags.append(kept)
        if kept:
            assert after_counts[g] == cnt and after[g, :cnt].tobytes() == want[:cnt].tobytes(), g
            assert after[g, counts[g]:].tobytes() == full[g, counts[g]:].tobytes(), g
            first = (int(full[g, 0]["kids"]) & 0xFFFFFF) + child_index[g]
            assert marker[g] == 1 and moves[g] == 1 and visits[g] == full[g, first]["n"], g
        else:
            assert after_counts[g] == counts[g] and after[g].tobytes() == full[g].tobytes(), g
            assert marker[g] == (0 if active[g] else 1) and moves[g] == 0 and visits[g] == 0, g
    return kept_flags


@pytest.mark.parametrize("N", [3, 5, 9])
def test_keep_launch_on_searched_pools(dev, N):
    from alphaquoridorgnn_amd import _lib
    from oracle import quoridor as oq
    G, sims = 8, 24
    eng = _engine(G, sims, N, tree_reuse=True, fake_bias=2, record_history=False)
    rng = np.random.RandomState(N)
    recs, s = [], oq.State(N=N)
    for g in range(G):                                   # roots along a short random walk: eight different trees
        recs.append(s.rec.copy())
        la = s.legal_actions()
        s = s.next(la[rng.randint(len(la))])
        if s.is_done() or not s.legal_actions():
            s = oq.State(N=N)                            # (a 3x3 game is over within a few plies: walk again from the opening)
    roots = torch.from_numpy(np.stack(recs).astype(np.uint8)).to(dev)
    _lib.check(eng.lib.aqg_engine_search(ctypes.byref(eng.e), _lib.ptr(roots), eng._stream()), "aqg_engine_search")
    torch.cuda.synchronize()
    pools, counts = _pools(eng)
    first = [int(pools[g, 0]["kids"]) & 0xFFFFFF for g in range(G)]
    kids = [pools[g, first[g]:first[g] + (int(pools[g, 0]["kids"]) >> 24)] for g in range(G)]
    assert all(f == 1 for f in first) and all(int(pools[g, 0]["n"]) == sims for g in range(G))
    # the most visited EXPANDED child (on 3x3 the most visited one may be a won position, which is never expanded)
    top = [int(np.argmax(np.where((k["kids"] >> 24) != 0, k["n"], -1))) for k in kids]
    bare = [int(np.flatnonzero((k["kids"] >> 24) == 0)[0]) if ((k["kids"] >> 24) == 0).any() else -1 for k in kids]
    assert N == 3 or bare[3] >= 0                        # (24 simulations may visit every child of a 3x3 root)
    n5 = int(kids[5][top[5]]["n"])
    assert n5 >= 1 and (int(kids[5][top[5]]["kids"]) >> 24) > 0
    # slot: 0 the first child, 1 the last, 2 the most visited, 3 an unexpanded one, 4 none, 5 / 6 the most visited with n == keep and
    # n == keep + 1 (two launches), 7 inactive
    index = [0, len(kids[1]) - 1, top[2], bare[3], -1, top[5], top[6], top[7]]
    active = [1] * 7 + [0]
    flags = _run_keep(eng, pools, counts, index, sims, active)
    assert flags[2] and not flags[3] and not flags[4] and not flags[7]
    flags = _run_keep(eng, pools, counts, index, n5, active)
    assert flags[5]                                      # n == keep is kept ...
    flags = _run_keep(eng, pools, counts, index, n5 - 1, active)
    assert not flags[5]                                  # ... n == keep + 1 is not
    assert not any(_run_keep(eng, pools, counts, index, 0, active))


SYNTH_KEEP = 300


@functools.lru_cache(maxsize=None)
def _synthetic_cases():
    """(pool, count, child index, active): a chain as deep as keep_visits allows (one-record blocks back to back: every record of a
    256-record window waits for the one before it), kept blocks interleaved with dropped ones, random trees whose kept blocks
    straddle the 64-record lane rounds and the 256-record windows, a slot that is told not to keep, and an inactive one."""
    chain = T.serialise(T.synthetic_tree(1, SYNTH_KEEP + 1, "chain"))
    inter = T.serialise(T.synthetic_tree(2, 90, "interleaved"))
    r1, r2, r3 = (T.serialise(T.synthetic_tree(s, 60, "random")) for s in (3, 4, 5))

    def biggest(pool):
        first, cnt = int(pool[0]["kids"]) & 0xFFFFFF, int(pool[0]["kids"]) >> 24
        return int(np.argmax(pool[first:first + cnt]["n"]))
    return [(chain[0], chain[1], 0, 1), (inter[0], inter[1], 1, 1), (r1[0], r1[1], biggest(r1[0]), 1), (r2[0], r2[1], biggest(r2[0]), 0),
            (r3[0], r3[1], -1, 1)]


def test_synthetic_cases_are_what_they_claim():
    from alphaquoridorgnn_amd.engine import keep_subtree_reference
    cases = _synthetic_cases()
    pool, count, idx, _ = cases[0]
    c = pool[1 + idx]
    n = int(c["n"])
    assert n == SYNTH_KEEP and count == 3 + SYNTH_KEEP                           # SYNTH_KEEP expanded nodes below the root, one leaf
    out, cnt, kept = keep_subtree_reference(pool, count, idx, n)
    assert kept and cnt == count - 2 and not keep_subtree_reference(pool, count, idx, n - 1)[2]
    assert all(int(out[i]["kids"]) == ((i + 1) | (1 << 24)) for i in range(cnt - 1))   # one-record blocks back to back
    for pool, count, idx, _ in cases[1:3]:
        out, cnt, kept = keep_subtree_reference(pool, count, idx, SYNTH_KEEP)
        assert kept and 1 < cnt < count and count > 1024
        cfirst = int(pool[(int(pool[0]["kids"]) & 0xFFFFFF) + idx]["kids"]) & 0xFFFFFF
        blocks = [b for b in T.block_starts(pool, count) if b[0] >= cfirst]
        sub = {b for b in T.block_starts(*_subpool(pool, idx))}
        flags = [b in sub for b in blocks]
        changes = sum(1 for a, b in zip(flags, flags[1:]) if a != b)
        assert changes >= 6                                                  # kept and dropped blocks alternate in the old pool
        kept_blocks = [b for b, f in zip(blocks, flags) if f]
        assert any(a // 64 != (a + c - 1) // 64 for a, c in kept_blocks) and \
            any((a - cfirst) // 256 != (a + c - 1 - cfirst) // 256 for a, c in kept_blocks)


def _subpool(pool, idx):
    """The old pool seen from the chosen child: block_starts of (pool with the child's record as root) are its subtree's blocks."""
    first = int(pool[0]["kids"]) & 0xFFFFFF
    view = pool.copy()
    view[0] = pool[first + idx]
    return view, len(pool)


@pytest.mark.parametrize("G", [1, 4, 5])
def test_keep_launch_on_synthetic_pools(dev, G):
    cases = _synthetic_cases()
    cases = (cases[G % 5:] + cases[:G % 5])[:G] if G > 1 else cases[:1]
    eng = _engine(G, 8, 3, tree_reuse=True, tree_reuse_visits=SYNTH_KEEP, record_history=False)
    pools, counts, index, active = ([c[i] for c in cases] for i in range(4))
    flags = _run_keep(eng, pools, counts, index, SYNTH_KEEP, active)
    assert flags == [bool(a) and i >= 0 for i, a in zip(index, active)]
    assert not any(_run_keep(eng, pools, counts, index, 1, active))          # every chosen child holds more than one visit


# ------------------------------------------------------------------ 2. whole games against the statement
@functools.lru_cache(maxsize=None)
def _statement_generation(N, sims, keep, K=0, G=8, noise_seed=None, eps=None):
    from alphaquoridorgnn_amd.constants import board_params
    plies = board_params(N)[1]
    u = np.random.RandomState(1000 * N + sims).random_sample(size=(G, plies))
    tables = None if noise_seed is None else np.random.RandomState(noise_seed).randint(1, 1025, size=(plies, G, MAX_LEGAL)).astype(np.float64)
    S, V, Z, ACT, Q, KEPT, KV = [], [], [], [], [], [], []
    for g in range(G):
        rows, z0 = T.play_game(N, sims, keep, u[g], temperature_plies=K, noise=None if tables is None else tables[:, g], eps=eps)
        for ply, r in enumerate(rows):
            S.append(r["rec"]); V.append(r["visits"]); ACT.append(r["action"]); Q.append(r["value"]); KEPT.append(r["kept"])
            KV.append(r["kept_visits"])
            Z.append(z0 if ply % 2 == 0 else -z0)
    return dict(u=u, tables=tables, states=np.stack(S), visits=np.stack(V), z=np.asarray(Z, dtype=np.int8),
                actions=np.asarray(ACT, dtype=np.uint8), values=np.asarray(Q, dtype=np.float32), kept=np.asarray(KEPT),
                kept_visits=np.asarray(KV))


def _play_table(eng, want):
    """A generation without refill: move m of every game is its ply m, drawn with u[:, m] (and mixed with tables[m])."""
    for m in range(eng.max_plies):
        eng.move(uniforms=torch.from_numpy(np.ascontiguousarray(want["u"][:, m])),
                 root_noise=None if want["tables"] is None else torch.from_numpy(want["tables"][m]))
    assert eng.counters()["active"] == 0


def _assert_generation(eng, want):
    st, vis, z = (x.cpu().numpy() for x in eng.history_tensors())
    act, val = eng.t["hist_action"][eng._history_valid()[0]].cpu().numpy(), eng.history_values().cpu().numpy()
    assert st.shape[0] == want["states"].shape[0]
    assert np.array_equal(st[:, :70], want["states"][:, :70])
    assert vis.tobytes() == want["visits"].tobytes() and z.tobytes() == want["z"].tobytes() and act.tobytes() == want["actions"].tobytes()
    assert val.dtype == np.float32 and val.tobytes() == want["values"].tobytes()
    stats = eng.tree_reuse_stats()
    assert stats["moves_kept"] == int(want["kept"].sum())
    assert abs(stats["mean_kept_visits"] - want["kept_visits"][want["kept"]].mean()) < 1e-9


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("N,sims,keep", [(3, 8, 3), (5, 16, 6)])
def test_whole_games_match_the_statement(dev, N, sims, keep, graph):
    from alphaquoridorgnn_amd import _lib
    want = _statement_generation(N, sims, keep)
    later = want["kept"][1:]
    assert want["kept"].any() and not later.all()                    # the statement keeps on some moves and starts fresh on others
    assert (want["visits"].sum(1) > sims).any() and want["kept_visits"].max() <= keep
    side = torch.cuda.Stream(device=dev)                             # a capturable stream: the move is replayed from a hipGraph
    _lib.set_option("use_graph", graph)
    try:
        with torch.cuda.stream(side):
            eng = _engine(8, sims, N, fake_bias=2, tree_reuse=True, tree_reuse_visits=keep, record_search_value=True)
            _play_table(eng, want)
            _assert_generation(eng, want)
    finally:
        _lib.set_option("use_graph", 1)
    off = _statement_generation(N, sims, None)
    assert off["visits"].tobytes() != want["visits"].tobytes()       # the option does change the games


def test_whole_games_with_the_temperature_schedule(dev):
    N, sims, keep, K = 5, 16, 8, 3
    want = _statement_generation(N, sims, keep, K)
    assert want["kept"].any() and not want["kept"][1:].all()
    eng = _engine(8, sims, N, fake_bias=2, tree_reuse=True, tree_reuse_visits=keep, record_search_value=True, temperature_plies=K)
    _play_table(eng, want)
    _assert_generation(eng, want)


def test_reuse_and_plain_moves_never_share_a_graph(dev):
    """One engine struct, reuse moves and plain moves in turn on a capturable stream: as with plain launches."""
    from alphaquoridorgnn_amd import _lib
    side = torch.cuda.Stream(device=dev)

    def run(graph):
        _lib.set_option("use_graph", graph)
        with torch.cuda.stream(side):
            eng = _engine(8, 8, 5, fake_bias=2, tree_reuse=True, seed=3)
            for m in range(9):
                if m % 3 != 2:                            # reuse, reuse (from kept subtrees), plain, ...
                    eng.move()
                else:                                     # the plain entry point on the same struct: fresh trees, then forget the marker
                    u = torch.rand((8,), dtype=torch.float64, device=dev, generator=eng.gen)
                    _lib.check(eng.lib.aqg_engine_move(ctypes.byref(eng.e), _lib.ptr(u), eng._stream()), "aqg_engine_move")
                    eng._forget_kept_trees()
            side.synchronize()
            return tuple(eng.t[k].cpu() for k in ("hist_visits", "hist_action", "root_state")), eng.tree_reuse_stats()
    try:
        a, b = run(1), run(0)
    finally:
        _lib.set_option("use_graph", 1)
    assert _same(a[0], b[0]) and a[1] == b[1] and a[1]["moves_kept"] > 0


# ------------------------------------------------------------------ 3. keep_visits 0 = the engine without the option
@pytest.mark.parametrize("kind", ["fake", "general"])
def test_keep_visits_zero_changes_nothing(dev, kind):
    N, G, sims = 5, 8, 12
    kw = dict(seed=6, record_search_value=True, temperature_plies=4)
    if kind == "general":
        from tests.test_gnn_any_shape import _make_net
        kw.update(model=_make_net((6, 16, 2), T.action_count(N), seed=11, N=N), evaluator="general")
    a = _engine(G, sims, N, **kw)
    a.play_generation()
    b = _engine(G, sims, N, tree_reuse=True, tree_reuse_visits=0, **kw)
    b.play_generation()
    assert _same(_rows(a), _rows(b))
    assert b.tree_reuse_stats() == dict(moves_kept=0, mean_kept_visits=0.0) and not bool(b.t["kept"].any())
    assert b.node_cap == a.node_cap and b.t["path"].shape == a.t["path"].shape


# ------------------------------------------------------------------ 4. independence from slots, refill and sets
def _play_quota(G, quota, U_game, N, sims, **kw):
    """Play `quota` games on G slots; game k's move at ply j is drawn with U_game[k, j] whatever slot it sits in."""
    eng = _engine(G, sims, N, quota=quota, **kw)
    for _ in range(eng.max_plies * quota + 1):
        active = eng.t["game_active"].cpu().numpy()
        if not active.any():
            break
        sg, gp = eng.t["slot_game"].cpu().numpy(), eng.t["game_plies"].cpu().numpy()
        u = np.zeros(G)
        for g in range(G):
            if active[g]:
                u[g] = U_game[sg[g], gp[sg[g]]]
        eng.move(torch.from_numpy(u))
    assert eng.counters()["finished"] == quota
    return _game_rows(eng), eng.tree_reuse_stats()


def _game_rows(eng):
    plies = eng.t["game_plies"].cpu().numpy()
    hs, hv, ha, hq = (eng.t[k].cpu().numpy() for k in ("hist_state72", "hist_visits", "hist_action", "hist_value"))
    res = eng.t["game_result"].cpu().numpy()
    return [(int(plies[k]), int(res[k]), hs[k, :plies[k]].tobytes(), hv[k, :plies[k]].tobytes(), ha[k, :plies[k]].tobytes(),
             hq[k, :plies[k]].tobytes()) for k in range(eng.quota)]


@pytest.mark.parametrize("noise", [False, True])
def test_a_games_rows_do_not_depend_on_its_slot(dev, noise):
    N, sims, G = 5, 8, 4
    quota = 3 * G
    U_game = np.random.RandomState(78).random_sample(size=(quota, 28))
    kw = dict(tree_reuse=True, tree_reuse_visits=4, record_search_value=True, seed=9, fake_bias=2)
    if noise:
        kw.update(root_noise_eps=0.25, root_noise_alpha=0.3)        # the generator: keyed by (seed, game, ply), kept root or fresh
    refill, rs = _play_quota(G, quota, U_game, N, sims, **kw)       # three games per slot
    wide, ws = _play_quota(quota, quota, U_game, N, sims, **kw)     # one slot per game
    assert refill == wide and rs == ws and rs["moves_kept"] > 0
    assert rs["moves_kept"] < sum(r[0] for r in wide) - quota        # ... and some later moves started fresh
    plain, _ = _play_quota(quota, quota, U_game, N, sims, **{**kw, "tree_reuse_visits": 0})
    assert plain != wide


def test_two_sets_play_the_single_sets_games(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    N, sims, G = 5, 8, 8
    kw = dict(board_size=N, evaluator="fake", fake_bias=2, tree_reuse=True, tree_reuse_visits=5, record_search_value=True)
    ms = MultiSetSelfPlay(None, num_games=G, sims=sims, num_sets=2, seed=3, quota=3 * G, **kw)
    ms.play_generation()
    ms.sync()
    total = ms.tree_reuse_stats()
    parts = []
    for i, s in enumerate(ms.sets):                       # set i is a stand-alone engine of seed 3 * 64 + i
        alone = _engine(s.G, sims, N, seed=3 * 64 + i, quota=s.quota, **{k: v for k, v in kw.items() if k not in ("board_size", "evaluator")})
        alone.play_generation()
        assert _game_rows(alone) == _game_rows(s)
        parts.append(alone.tree_reuse_stats())
    assert total["moves_kept"] == sum(p["moves_kept"] for p in parts) > 0


# ------------------------------------------------------------------ 5. root noise
def test_table_noise_games_match_the_statement(dev):
    N, sims, keep, eps = 5, 16, 6, 0.25
    want = _statement_generation(N, sims, keep, noise_seed=41, eps=eps)
    assert want["kept"].any() and not want["kept"][1:].all()
    assert want["visits"].tobytes() != _statement_generation(N, sims, keep)["visits"].tobytes()
    eng = _engine(8, sims, N, fake_bias=2, tree_reuse=True, tree_reuse_visits=keep, record_search_value=True, root_noise_eps=eps)
    _play_table(eng, want)
    _assert_generation(eng, want)


TOL = 4 * 2.0 ** -24      # eta, the two products and the sum: one f32 rounding each of a value <= 1 (the f64 library functions: 1e-15)


@pytest.mark.parametrize("mode", ["table", "generator"])
def test_kept_roots_priors_are_mixed_in_place(dev, mode):
    """Move 1 keeps; move 2 runs with keep_visits 0, so its roots' trees stay in the pools: the children of a root that was kept hold
    the mix of the priors they held after move 1, cp = f32(c_puct * p'); a fresh root's hold the mix of the evaluator's priors."""
    from alphaquoridorgnn_amd.engine import draw_root_noise
    from oracle import mcts as om, quoridor as oq
    N, G, sims, eps, alpha = 5, 16, 16, 0.25, 0.3
    eng = _engine(G, sims, N, fake_bias=2, tree_reuse=True, tree_reuse_visits=2, root_noise_eps=eps, root_noise_alpha=alpha, seed=12)
    tables = np.random.RandomState(5).randint(1, 1025, size=(2, G, MAX_LEGAL)).astype(np.float64)
    eng.move(torch.from_numpy(np.random.RandomState(6).random_sample(G)), None if mode == "generator" else torch.from_numpy(tables[0]))
    kept = eng.t["kept"].cpu().numpy().astype(bool)
    # (the table's games: 11 chosen children hold at most 2 visits, 5 hold 5 -- worked out on the host with tests/_tree_reuse.py)
    assert kept.any() and (mode == "generator" or int(kept.sum()) == 11)
    clean, count = (x.cpu().numpy() for x in eng.root_priors())
    recs = eng.root_states72().cpu().numpy()
    eng.reuse.keep_visits = 0
    eng.move(torch.full((G,), 0.5, dtype=torch.float64), None if mode == "generator" else torch.from_numpy(tables[1]))
    mixed, count2 = (x.cpu().numpy() for x in eng.root_priors())
    pools, _ = _pools(eng)
    worst = 0.0
    for g in range(G):
        st = oq.State(recs[g])
        cnt = len(st.legal_actions())
        assert count2[g] == cnt and st.plies_played == 1
        base = clean[g, :cnt] if kept[g] else om.FakeModel(2).predict(st)[0]
        assert not kept[g] or count[g] == cnt
        gam = tables[1, g] if mode == "table" else draw_root_noise(eng.root_noise_seed, g, 1, cnt, eng.root_noise_alpha)
        want = mix_statement(base, gam, eps)
        if mode == "table":
            assert mixed[g, :cnt].tobytes() == want.tobytes(), (g, kept[g])
        else:
            worst = max(worst, float(np.abs(mixed[g, :cnt].astype(np.float64) - want).max()))
        kids = pools[g, 1:1 + cnt]
        assert kids["cp"].tobytes() == (np.float32(1.25) * kids["p"]).astype(np.float32).tobytes() and kids["p"].tobytes() == mixed[g, :cnt].tobytes()
        assert not np.array_equal(mixed[g, :cnt], base) or cnt == 1
    print(f"{mode}: worst |device - mirror| = {worst:.3e} (bound {TOL:.3e})")
    assert worst <= TOL


# ------------------------------------------------------------------ 6. the network evaluators
def _net(kind, N, dev):
    if kind == "general":
        from tests.test_gnn_any_shape import _make_net
        return _make_net((6, 16, 2), T.action_count(N), seed=11, N=N)
    if kind == "cnn":
        from tests.test_cnn import _make_net
        return _make_net(8, 1, N, seed=12).to(dev)
    from tests.test_gpu_parity import _model
    return _model(2)[0]


def _play_checked(eng, limit=48):
    """`limit` moves, one by one: every kept root has n == 1 + its children's, and the host's count of kept moves is the engine's.
    Returns what the games recorded so far."""
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    moves = visits = 0
    for _ in range(min(limit, eng.max_plies)):
        eng.move()
        kept = eng.t["kept"].cpu().numpy().astype(bool) & eng.t["game_active"].cpu().numpy().astype(bool)
        if kept.any():
            pools = eng.t["node_rec"].view(eng.G, eng.node_cap, 4)[:, :1 + MAX_LEGAL].cpu().numpy().copy().view(NODE_DTYPE).reshape(eng.G, -1)
            for g in np.flatnonzero(kept):
                cnt, first = int(pools[g, 0]["kids"]) >> 24, int(pools[g, 0]["kids"]) & 0xFFFFFF
                assert first == 1 and cnt > 0 and int(pools[g, 0]["n"]) == 1 + int(pools[g, 1:1 + cnt]["n"].sum()) <= eng.keep_visits, g
                moves += 1
                visits += int(pools[g, 0]["n"])
    stats = eng.tree_reuse_stats()
    assert stats["moves_kept"] == moves > 0 and abs(stats["mean_kept_visits"] - visits / moves) < 1e-9
    return tuple(eng.t[k].cpu() for k in ("hist_state72", "hist_visits", "hist_action", "hist_value", "game_plies", "game_result", "root_state"))


@pytest.mark.parametrize("kind,N", [("gnn", 9), ("general", 5), ("cnn", 5)])
def test_network_evaluators(dev, kind, N):
    from alphaquoridorgnn_amd import _lib
    net = _net(kind, N, dev)
    G, sims = 8, 8
    kw = dict(model=net, evaluator=kind, seed=4, tree_reuse=True, record_search_value=True)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        base = _play_checked(_engine(G, sims, N, eval_cache_slots=0, **kw))           # graph capture on
        cached = _engine(G, sims, N, eval_cache_slots=64, **kw)
        assert _same(_play_checked(cached), base)
        print(f"{kind}: {cached.counters()['cache_hits']} evaluation-cache hits beside tree reuse")
        variants = [("use_graph", 0)] + ([("step_heads", 0), ("legal_beside_trunk", 0)] if kind == "gnn" else [])
        for name, value in variants:
            _lib.set_option(name, value)
            try:
                assert _same(_play_checked(_engine(G, sims, N, eval_cache_slots=0, **kw)), base), name
            finally:
                _lib.set_option(name, 1)
        plain = _engine(G, sims, N, model=net, evaluator=kind, seed=4, record_search_value=True, eval_cache_slots=0)
        for _ in range(min(48, plain.max_plies)):
            plain.move()
        assert not torch.equal(plain.t["hist_visits"].cpu(), base[1])                # the option does change the games
