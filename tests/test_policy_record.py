"""Recording completed-Q targets during self-play, on the GPU (include/aqgnn.h "recording completed-Q targets during self-play";
csrc/mcts_record.hip, the policy form of csrc/replay.hip, engine.py, self_play.py): the record launch alone against the read-out launch
bit for bit -- both run csrc/mcts_improve_row.hpp's one device function -- and against engine.improved_policy_reference at the derived
one-ulp bound of tests/_improved_policy.py; whole games with the option on against the same engine with it off (no game changes) and
against the host statement; the policy append against replay.append_reference(policy=) bit for bit; self_play() end to end; refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests._improved_policy import COUNTS, PATTERNS, pi_close, synthetic_pool   # noqa: E402
from tests._policy_record import policy_size, recorded_rows, statement_rows   # noqa: E402
from tests._reanalyse import MAX_LEGAL   # noqa: E402
from tests.test_replay_window_cpu import _bits, counts_rows   # noqa: E402
from tests.test_selfplay_targets_cpu import search_values   # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC12345          # the sentinel: a NaN no arithmetic produces, compared as bits
FILL_U8, FILL_F32 = 0xA5, np.float32(-7.25)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _engine(G, sims, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    return BatchedSelfPlay(kw.pop("model", None), num_games=G, sims=sims, board_size=N, **kw)


def _sentinel(eng):
    eng.t["hist_policy"].view(torch.int32).fill_(NAN_BITS)


def _record(eng, c_visit=50.0, c_scale=1.0):
    """aqg_engine_record_improved_policy on its own; returns (rc, hist_policy as int32 bits [Q, hp, A])."""
    from alphaquoridorgnn_amd import _lib
    pr = _lib.PolicyRecordStruct()
    pr.c_visit, pr.c_scale = c_visit, c_scale
    pr.hist_policy = eng.t["hist_policy"].data_ptr()
    rc = eng.lib.aqg_engine_record_improved_policy(ctypes.byref(eng.e), ctypes.byref(pr), eng._stream())
    torch.cuda.synchronize()
    return rc, eng.t["hist_policy"].cpu().numpy().view(np.int32)


def _scattered(policy, actions, count, A):
    """The read-out's row of one slot scattered by its action bytes over zeros; an action byte >= A is dropped."""
    row = np.zeros((A,), dtype=np.float32)
    for j in range(int(count)):
        if actions[j] < A:
            row[actions[j]] = policy[j]
    return row


# ------------------------------------------------------------------ 1. the launch alone
def _cases(cap, A):
    """Every (pattern, count) pool of the read-out's tests at the issue's counts, the two guard rows, and -- where the board's
    action ids fill a byte's range less than whole -- a pool with action bytes A and 255 planted."""
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    counts = [c for c in COUNTS if c in (0, 1, 63, 64, 65, 128, 136)]
    planted = synthetic_pool(NODE_DTYPE, cap, 100, "all_visited", seed=9, first=5)
    planted["action"][5:105] = np.random.RandomState(9).permutation(A)[:100] if A >= 100 else planted["action"][5:105]
    planted["action"][7], planted["action"][70] = A, 255
    cases = [planted]                                          # (in front: slot 0 records in every chunk shape)
    cases += [synthetic_pool(NODE_DTYPE, cap, cnt, pattern, seed=1000 * k + cnt) for k, pattern in enumerate(PATTERNS) for cnt in counts]
    cases.append(synthetic_pool(NODE_DTYPE, cap, 20, "mixed", seed=7, first=cap - 19))          # the child range leaves the pool
    cases.append(synthetic_pool(NODE_DTYPE, cap, 137, "mixed", seed=8, first=1))               # a count above MAX_LEGAL
    return cases


@pytest.mark.parametrize("N,G", [(3, 1), (3, 4), (3, 5), (9, 1), (9, 4), (9, 5)])
def test_record_launch_is_the_read_out_scattered(dev, N, G):
    """A self-play engine of G slots -- one wavefront, a full workgroup, a workgroup and a wavefront -- whose pools are overwritten
    with the synthetic ones, chunk by chunk.  Slot g plays game g; the plies are forced through game_plies: the last ply of the
    history for slot 0, past the history for the last slot of a chunk of 5, an inactive slot 1 in a chunk of 4 or 5.  Only the rows
    (g, ply_g) of the recording slots may change, and they are the read-out's rows scattered, bit for bit."""
    from alphaquoridorgnn_amd.engine import root_improved_policy_reference
    A = policy_size(N)
    eng = _engine(G, 2, N, policy_target="completed_q")
    cap, hp = eng.node_cap, eng.max_plies
    assert cap >= 1 + MAX_LEGAL and eng.t["hist_policy"].shape == (G, hp, A) and eng.t["hist_policy"].dtype == torch.float32
    cases = _cases(cap, A)
    plies = np.array([hp - 1, 3, 0, 1, hp][:G], dtype=np.int32)
    if G == 5:
        plies[4] = hp + 2 if N == 3 else hp                     # >= max_plies: never recorded
    active = np.ones(G, dtype=np.uint8)
    if G >= 4:
        active[1] = 0
    eng.t["game_plies"].copy_(torch.from_numpy(plies))
    eng.t["game_active"].copy_(torch.from_numpy(active))
    dropped = recorded = zero_rows = 0
    for first in range(0, len(cases), G):
        chunk = [cases[(first + g) % len(cases)] for g in range(G)]
        pools = np.stack(chunk)
        eng.t["node_rec"].copy_(torch.from_numpy(pools.view(np.float64).reshape(G * cap, 4)))
        for c_visit, c_scale in ((50.0, 1.0),) if first % 3 else ((50.0, 1.0), (0.0, 0.3), (7.5, 0.0)):
            policy, actions, count, _ = (x.cpu().numpy() for x in eng.root_improved_policy(c_visit, c_scale))
            _sentinel(eng)
            rc, got = _record(eng, c_visit, c_scale)
            assert rc == 0, eng.lib.aqg_last_error()
            want = np.full((G, hp, A), NAN_BITS, dtype=np.int32)
            for g in range(G):
                if active[g] and plies[g] < hp:
                    row = _scattered(policy[g], actions[g], count[g], A)
                    want[g, plies[g]] = row.view(np.int32)
                    dropped += int((actions[g, :count[g]] >= A).sum())
                    zero_rows += int(count[g] == 0 and (int(chunk[g][0]["kids"]) >> 24) > 0)
                    recorded += 1
                    # ... and against numpy, at the derived bound
                    ref_p, ref_a, ref_c, _ = root_improved_policy_reference(pools[g], c_visit, c_scale)
                    ref = _scattered(ref_p, ref_a, ref_c, A)
                    assert np.array_equal(row == 0, ref == 0) and pi_close(row, ref), (N, G, first, g)
            assert np.array_equal(got, want), (N, G, first, np.argwhere(got != want)[:4])
    assert recorded and dropped and zero_rows >= 1
    if G >= 4:
        assert (want[1] == NAN_BITS).all()                          # the inactive slot never wrote
    assert np.array_equal(eng.t["game_plies"].cpu().numpy(), plies)     # the launch only writes hist_policy


def test_record_launch_on_searched_roots(dev):
    """Real searches (5x5, 12 simulations, 6 slots) through move(): the finish-move launch reads the pool and leaves it as it is, so
    the read-out behind the move still sees the searched roots -- the recorded rows are its rows scattered, bit for bit, sum to one
    and are zero off the legal actions."""
    from oracle import quoridor as oq
    N, G, sims = 5, 6, 12
    A = policy_size(N)
    eng = _engine(G, sims, N, fake_bias=1, policy_target="completed_q", policy_c_visit=20.0, policy_c_scale=0.5)
    _sentinel(eng)
    eng.move(torch.from_numpy(np.random.RandomState(3).random_sample(G)))
    policy, actions, count, _ = (x.cpu().numpy() for x in eng.root_improved_policy(20.0, 0.5))
    got = eng.t["hist_policy"].cpu().numpy()
    legal = np.zeros(A, dtype=bool)
    legal[list(oq.State(N=N).legal_actions())] = True
    for g in range(G):
        row = _scattered(policy[g], actions[g], count[g], A)
        assert np.array_equal(got[g, 0].view(np.int32), row.view(np.int32)) and count[g] == legal.sum()
        assert abs(float(row.astype(np.float64).sum()) - 1.0) <= A * 2.0 ** -23
        assert (row[~legal] == 0).all() and (row[legal] > 0).all()
    assert (got[:, 1:].view(np.int32) == NAN_BITS).all()                # one row per slot, nothing else


# ------------------------------------------------------------------ 2. whole games
def _game_rows(eng):
    """Per game: (plies, result, states, visits, actions[, values]) as bytes, and the recorded policy rows where the option is on."""
    plies = eng.t["game_plies"].cpu().numpy()
    keys = ["hist_state72", "hist_visits", "hist_action"] + (["hist_value"] if "hist_value" in eng.t else [])
    h = [eng.t[k].cpu().numpy() for k in keys]
    res = eng.t["game_result"].cpu().numpy()
    games = [(int(plies[k]), int(res[k])) + tuple(x[k, :plies[k]].tobytes() for x in h) for k in range(eng.quota)]
    pol = eng.t["hist_policy"].cpu().numpy() if "hist_policy" in eng.t else None
    return games, None if pol is None else [pol[k, :plies[k]].copy() for k in range(eng.quota)]


def _assert_statement(eng, N, sims, bias, keep=None, c_visit=50.0, c_scale=1.0):
    """history_policies() row by row against the host statement, game by game."""
    plies = eng.t["game_plies"].cpu().numpy()
    recs, acts = eng.t["hist_state72"].cpu().numpy(), eng.t["hist_action"].cpu().numpy()
    got = eng.history_policies().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (int(plies.sum()), policy_size(N)) == tuple(eng.history_tensors()[1].shape)
    at = 0
    for k in range(eng.quota):
        want = statement_rows(N, sims, bias, recs[k, :plies[k]], acts[k, :plies[k]], keep, c_visit, c_scale)
        rows = got[at:at + plies[k]]
        at += plies[k]
        assert np.array_equal(rows == 0, want == 0) and pi_close(rows, want), (k, np.abs(rows.astype(np.float64) - want).max())
    hist = eng.history()
    assert len(hist) == got.shape[0] and all(type(x) is float for x in hist[0][1])
    assert np.array_equal(_bits(np.array([r[1] for r in hist]).astype(np.float32)), _bits(got))      # history(): the recorded row


CONFIGS = {
    "tree_reuse": dict(tree_reuse=True, tree_reuse_visits=5),
    "schedule": dict(temperature_plies=2, record_search_value=True),
    "resign": dict(resign_threshold=0.2, resign_min_ply=1, resign_disable_fraction=0.25, record_search_value=True),
    "external": dict(evaluator="external"),
}


# the external evaluator makes plain launches from the host whatever the option says: one pass per shape
WHOLE_GAMES = [(N, sims, config, graph) for N, sims in [(3, 2), (3, 8), (5, 2), (5, 8)] for config in sorted(CONFIGS)
               for graph in ((0,) if config == "external" else (0, 1))]


@pytest.mark.parametrize("N,sims,config,graph", WHOLE_GAMES)
def test_whole_games_record_the_statement_and_change_no_game(dev, N, sims, config, graph):
    from alphaquoridorgnn_amd import _lib
    kw = dict(CONFIGS[config], seed=11)
    if config == "external":
        from tests.test_gpu_parity import _OracleFakeAdapter
        kw.update(model=_OracleFakeAdapter(2))
    else:
        kw.update(fake_bias=2)
    G = 4 if config == "external" else 8
    side = torch.cuda.Stream(device=dev)                             # a capturable stream: with `graph` the search is replayed from a hipGraph
    _lib.set_option("use_graph", graph)
    try:
        with torch.cuda.stream(side):
            off = _engine(G, sims, N, **kw)
            off.play_generation()
            on = _engine(G, sims, N, policy_target="completed_q", **kw)
            on.play_generation()
            side.synchronize()
            games_off, none = _game_rows(off)
            games_on, _ = _game_rows(on)
            assert none is None and games_on == games_off                     # history, actions, values, results: byte-identical
            assert all(torch.equal(a, b) for a, b in zip(on.history_tensors(), off.history_tensors()))
            _assert_statement(on, N, sims, 2, keep=kw.get("tree_reuse_visits"))
            if config == "resign":
                assert on.resign_stats() == off.resign_stats()
            if config == "tree_reuse":
                assert on.tree_reuse_stats() == off.tree_reuse_stats() and (sims < 8 or on.tree_reuse_stats()["moves_kept"] > 0)
    finally:
        _lib.set_option("use_graph", 1)


def test_resigning_rows_are_recorded(dev):
    """A threshold every mover is below at once: the games end in their first eligible row, whose action is 0xFF -- and whose policy
    row is written like any other."""
    N, sims = 5, 8
    eng = _engine(8, sims, N, fake_bias=2, seed=4, policy_target="completed_q", resign_threshold=1e-6, resign_min_ply=0,
                  resign_disable_fraction=0.0, record_search_value=True)
    eng.play_generation()
    acts = eng.t["hist_action"][eng._history_valid()[0]].cpu().numpy()
    assert (acts == 0xFF).sum() >= 1 and eng.resign_stats()["games_resigned"] >= 1
    _assert_statement(eng, N, sims, 2)


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
    return eng


def test_refill_gives_the_same_rows_per_game(dev):
    N, sims, G = 3, 8, 3
    quota = 4 * G
    U_game = np.random.RandomState(78).random_sample(size=(quota, 64))
    kw = dict(fake_bias=2, seed=9, policy_target="completed_q", tree_reuse=True, tree_reuse_visits=4)
    refill, wide = _play_quota(G, quota, U_game, N, sims, **kw), _play_quota(quota, quota, U_game, N, sims, **kw)
    (ga, pa), (gb, pb) = _game_rows(refill), _game_rows(wide)
    assert ga == gb and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(pa, pb))
    assert all((a != 0).any(axis=1).all() for a in pa)                       # every played row was written
    _assert_statement(refill, N, sims, 2, keep=4)
    # nothing past a game's last ply was ever written: the buffer started as zeros
    plies, pol = refill.t["game_plies"].cpu().numpy(), refill.t["hist_policy"].cpu().numpy()
    assert all((pol[k, plies[k]:] == 0).all() for k in range(quota))


def test_two_sets_record_the_single_sets_rows(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    N, sims, G = 5, 8, 8
    kw = dict(board_size=N, evaluator="fake", fake_bias=2, policy_target="completed_q", policy_c_visit=30.0, record_search_value=True)
    ms = MultiSetSelfPlay(None, num_games=G, sims=sims, num_sets=2, seed=3, quota=2 * G, **kw)
    ms.play_generation()
    ms.sync()
    joined = ms.history_policies().cpu().numpy()
    parts = []
    for i, s in enumerate(ms.sets):                       # set i is a stand-alone engine of seed 3 * 64 + i
        alone = _engine(s.G, sims, N, seed=3 * 64 + i, quota=s.quota, **{k: v for k, v in kw.items() if k not in ("board_size", "evaluator")})
        alone.play_generation()
        (ga, pa), (gb, pb) = _game_rows(alone), _game_rows(s)
        assert ga == gb and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(pa, pb))
        parts.append(alone.history_policies().cpu().numpy())
    assert np.array_equal(_bits(joined), _bits(np.concatenate(parts))) and joined.shape[0] == ms.history_tensors()[0].shape[0]
    with pytest.raises(ValueError, match="completed_q"):
        MultiSetSelfPlay(None, num_games=2, sims=2, num_sets=1, board_size=3, evaluator="fake").history_policies()


def test_root_noise_targets_use_the_mixed_priors(dev):
    """With root noise on, the recorded row is softmax(log p_mixed + sigma): with c_scale = 0 it is the MIXED priors of the root,
    normalised -- root_priors() of a search of the same roots under the same noise table, scattered."""
    N, G, sims = 5, 4, 8
    kw = dict(fake_bias=2, seed=5, root_noise_eps=0.25, root_noise_alpha=0.3)
    table = torch.from_numpy(np.random.RandomState(2).randint(1, 1025, size=(G, MAX_LEGAL)).astype(np.float64))
    u = torch.from_numpy(np.random.RandomState(1).random_sample(G))
    on = _engine(G, sims, N, policy_target="completed_q", policy_c_scale=0.0, **kw)
    on.move(u, root_noise=table)
    quiet = _engine(G, sims, N, policy_target="completed_q", policy_c_scale=0.0, fake_bias=2, seed=5)
    quiet.move(u)
    probe = _engine(G, sims, N, record_history=False, **kw)
    _, actions, count = (x.cpu().numpy() for x in probe.search(on.t["hist_state72"][:, 0].contiguous(), root_noise=table))
    priors, pcount = (x.cpu().numpy() for x in probe.root_priors())
    rows, plain = on.t["hist_policy"][:, 0].cpu().numpy(), quiet.t["hist_policy"][:, 0].cpu().numpy()
    for g in range(G):
        p = priors[g, :count[g]].astype(np.float64)
        assert count[g] == pcount[g] and pi_close(rows[g][actions[g, :count[g]]], p / p.sum()), g
        assert not np.array_equal(rows[g], plain[g])                     # the unmixed priors give another row


# ------------------------------------------------------------------ 3. the append
def _filled(capacity, A):
    return (np.full((capacity, 72), FILL_U8, np.uint8), np.full((capacity, A), FILL_F32, np.float32),
            np.full((capacity,), FILL_F32, np.float32))


def _to(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _call_policy(dev, N, A, S, P, Z, q, blend, n, capacity, head, rings):
    from alphaquoridorgnn_amd import _lib
    d = [_to(dev, x) for x in (S, P, Z, q)]
    r = [_to(dev, x) for x in rings]
    rc = _lib.load().aqg_replay_append_policy(N, A, *(_lib.ptr(x) for x in d), blend, n, capacity, head, *(_lib.ptr(x) for x in r),
                                              _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in r]


@pytest.mark.parametrize("N", (3, 5, 7, 9))
def test_policy_append_equals_the_reference_bit_for_bit(dev, N):
    """One row, one below / at / one above a workgroup's 16 rows and four workgroups' 64; written at a head that makes the write
    wrap, into a pre-filled ring whose other slots must keep the pattern; without a blend and with one."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.replay import append_reference
    A = policy_size(N)
    for n in (1, 15, 16, 17, 64, 65):
        S, _, Z = counts_rows(N, n, seed=100 * N + n)
        P, q = recorded_rows(N, n, seed=200 * N + n), search_values(n, seed=300 * N + n)
        capacity = n + 7
        head = capacity - max(1, n // 2)                      # wraps for every n > 1
        written = (head + np.arange(n)) % capacity
        rest = np.setdiff1d(np.arange(capacity), written)
        assert n == 1 or written.min() == 0
        for values, blend in ((None, 0.0), (q, 0.0), (q, 0.25), (q, 1.0)):
            want = _filled(capacity, A)
            append_reference(N, S, None, Z, None, None, head, *want, search_value=values, value_blend=blend, policy=P)
            rc, got = _call_policy(dev, N, A, S, P, Z, values, blend, n, capacity, head, _filled(capacity, A))
            assert rc == 0, _lib.load().aqg_last_error()
            for g, w in zip(got, want):
                assert np.array_equal(_bits(g), _bits(w)), (N, n, blend)
            assert np.array_equal(_bits(got[1][written]), _bits(P)) and np.array_equal(got[0][written], S)
            assert (got[0][rest] == FILL_U8).all() and (got[1][rest] == FILL_F32).all() and (got[2][rest] == FILL_F32).all()


def test_policy_append_c_entry_refusals(dev):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, n, capacity = 5, 20, 32
    A = policy_size(N)
    S, V, Z = counts_rows(N, n, seed=1)
    P, q = recorded_rows(N, n, seed=2), search_values(n, seed=2)

    def refused(match, *, S_=S, P_=P, Z_=Z, q_=q, blend=0.5, A_=A, n_=n, capacity_=capacity, head=0, N_=N):
        rc, got = _call_policy(dev, N_, A_, S_, P_, Z_, q_, blend, n_, capacity_, head, _filled(capacity, A))
        assert rc != 0 and match in lib.aqg_last_error().decode(), (match, lib.aqg_last_error())
        assert (got[0] == FILL_U8).all() and (got[1] == FILL_F32).all() and (got[2] == FILL_F32).all()   # the rings are as they were

    refused("blend", blend=-0.25)
    refused("blend", blend=1.25)
    refused("blend", blend=float("nan"))
    refused("search_value", q_=None)                        # a blend without the values
    refused("board_size", N_=4)
    refused("policy_size", A_=policy_size(9))
    refused("n > capacity", capacity_=n - 1)
    refused("head", head=capacity)
    refused("head", head=-1)
    refused("capacity", capacity_=0)
    refused("negative", n_=-1)
    refused("pi and z_i8", P_=None)
    refused("pi and z_i8", Z_=None)
    refused("must be given", S_=None)
    rc, _ = _call_policy(dev, N, A, None, None, None, None, 0.5, 0, capacity, 0, _filled(capacity, A))
    assert rc == 0                                          # n == 0: no pointer is looked at
    st = _lib.stream_ptr(dev)
    dS, dP, dZ, dq = (_to(dev, x) for x in (S, P, Z, q))
    r72, rpi, rz = (_to(dev, x) for x in _filled(capacity, A))
    for value in (rz, rpi.view(-1)[5:]):                    # search_value overlapping a ring
        rc = lib.aqg_replay_append_policy(N, A, _lib.ptr(dS), _lib.ptr(dP), _lib.ptr(dZ), ctypes.c_void_p(value.data_ptr()), 0.5, n, capacity, 0,
                                          _lib.ptr(r72), _lib.ptr(rpi), _lib.ptr(rz), st)
        assert rc != 0 and "overlaps" in lib.aqg_last_error().decode()
    rc = lib.aqg_replay_append_policy(N, A, _lib.ptr(dS), ctypes.c_void_p(rpi.data_ptr()), _lib.ptr(dZ), None, 0.0, n, capacity, 0,
                                      _lib.ptr(r72), _lib.ptr(rpi), _lib.ptr(rz), st)
    assert rc != 0 and "overlaps" in lib.aqg_last_error().decode()      # the source rows ARE the ring
    # the old entry still refuses the mixed form
    rc = lib.aqg_replay_append(N, A, _lib.ptr(dS), None, _lib.ptr(dZ), _lib.ptr(dP), None, n, capacity, 0, _lib.ptr(r72), _lib.ptr(rpi), _lib.ptr(rz), st)
    assert rc != 0 and "form" in lib.aqg_last_error().decode()
    torch.cuda.synchronize()
    assert (r72 == FILL_U8).all() and (rz == float(FILL_F32)).all()


def test_the_window_on_the_device_is_the_window_on_the_host(dev):
    from alphaquoridorgnn_amd.replay import ReplayWindow
    N = 7
    g, h = ReplayWindow(N, max_generations=3, capacity_rows=40, device=dev), ReplayWindow(N, max_generations=3, capacity_rows=40)
    for k, m in enumerate((17, 9, 21, 45, 6)):              # a wrap, and a generation larger than the ring (its newest rows are kept)
        S, V, Z = counts_rows(N, m, seed=k)
        P, q = torch.from_numpy(recorded_rows(N, m, seed=30 + k)), torch.from_numpy(search_values(m, seed=20 + k))
        args = (torch.from_numpy(S), P, torch.from_numpy(Z))
        blend = dict(search_value=q, value_blend=0.25) if k % 2 else {}
        g.append_policy(*(x.to(dev) for x in args), **{a: (b.to(dev) if torch.is_tensor(b) else b) for a, b in blend.items()})
        h.append_policy(*args, **blend)
        assert g.generations == h.generations and torch.equal(g.index().cpu(), h.index())
    for a, b in zip(g.tensors(), h.tensors()):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.numpy()))


# ------------------------------------------------------------------ 4. self_play() end to end
_LOOP = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, pv_mcts, self_play as sp, train_network as tn
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, pack_states
from alphaquoridorgnn_amd.replay import ReplayWindow

assert constants.BOARD_SIZE == 3
torch.manual_seed(3)
dev = aqd.device()
net = GraphPolicyValueNetwork(6, 16, 2, 17, board_size=3)
os.makedirs(constants.PV_NETWORK_PATH)
torch.save(net.state_dict(), constants.PV_NETWORK_PATH + "best.pth")
model = net.to(dev).eval()
pv_mcts.PV_EVALUATE_COUNT = 8
bits = lambda x: x.view(np.int32)


def generation(target, blend=0.0):
    sp.SP_POLICY_TARGET, sp.SP_POLICY_C_VISIT, sp.SP_VALUE_BLEND = target, 20.0, blend
    sp.SP_REPLAY = ReplayWindow(3, max_generations=1, capacity_rows=4096, device=dev)
    path = sp.self_play(model, games=12, seed=17)
    with open(path, "rb") as f:
        rows = pickle.load(f)
    os.remove(path)
    return rows, [x.cpu().numpy() for x in sp.SP_REPLAY.rows()]


off_rows, off_ring = generation("visits")
on_rows, on_ring = generation("completed_q")
s, p, v = zip(*on_rows)
file_pi = torch.tensor(np.array(p), dtype=torch.float32).numpy()          # the conversion of the trainers
file_z = torch.tensor(np.array(v), dtype=torch.float32).numpy()
print("SAME_GAMES", len(on_rows) == len(off_rows) >= 12, [(r[0], r[2]) for r in on_rows] == [(r[0], r[2]) for r in off_rows])
print("RING_IS_THE_FILE", np.array_equal(bits(on_ring[1]), bits(file_pi)), np.array_equal(bits(on_ring[2]), bits(file_z)),
      np.array_equal(on_ring[0][:, :68], pack_states(s, 3)[:, :68]))
print("REST_OF_THE_RING", np.array_equal(on_ring[0], off_ring[0]), np.array_equal(bits(on_ring[2]), bits(off_ring[2])))
legal = off_ring[1] > 0
print("TARGET_CHANGED", not np.array_equal(on_ring[1], off_ring[1]), bool((on_ring[1][legal] > 0).all()),
      bool(np.abs(on_ring[1].astype(np.float64).sum(1) - 1.0).max() <= 17 * 2.0 ** -23), int((on_ring[1] > 0).sum()) > int(legal.sum()))
blend_rows, blend_ring = generation("completed_q", 0.5)
print("WITH_A_BLEND", np.array_equal(bits(blend_ring[1]), bits(on_ring[1])), all(type(r[2]) is float for r in blend_rows),
      np.array_equal(bits(blend_ring[2]), bits(np.array([r[2] for r in blend_rows]).astype(np.float32))))
# one parameter update from that window
tn.NUM_EPOCH, tn.TRAIN_WINDOW = 1, sp.SP_REPLAY
torch.manual_seed(11)
tn.train_network()
with open(constants.PV_NETWORK_PATH + "latest.pth", "rb") as f, open(constants.PV_NETWORK_PATH + "best.pth", "rb") as g:
    latest, best = f.read(), g.read()
state = torch.load(constants.PV_NETWORK_PATH + "latest.pth", map_location="cpu")
print("TRAINED", latest != best, all(bool(torch.isfinite(x).all()) for x in state.values() if x.is_floating_point()))
'''


def test_self_play_with_the_option(dev, tmp_path):
    """One child process on the 3x3 board (the module's board size comes from the environment): self_play() with a window and the
    option.  The ring equals the file the same call wrote, bit for bit; the games are those of the option off; one train_network()
    update from that window runs."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="3")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("SAME_GAMES True True", "RING_IS_THE_FILE True True True", "REST_OF_THE_RING True True", "TARGET_CHANGED True True True True",
                 "WITH_A_BLEND True True True", "TRAINED True True"):
        assert line in r.stdout, (line, r.stdout[-2000:])
    assert "policy target: completed_q" in r.stdout and "policy target: visits" in r.stdout          # the progress line names it


# ------------------------------------------------------------------ 5. refusals
def test_engine_refusals(dev):
    eng = _engine(2, 2, 3, policy_target="completed_q")
    with pytest.raises(ValueError, match="search\\(\\)"):
        eng.search(np.zeros((2, 72), np.uint8))
    with pytest.raises(ValueError, match="apply_actions\\(\\)"):
        eng.apply_actions(np.zeros((2,), np.int32))
    with pytest.raises(ValueError, match="record_history"):
        _engine(2, 2, 3, policy_target="completed_q", record_history=False)
    with pytest.raises(ValueError, match="completed_q"):
        _engine(2, 2, 3).history_policies()
    with pytest.raises(ValueError, match="c_visit"):
        _engine(2, 2, 3, policy_target="completed_q", policy_c_visit=-1.0)
    assert "hist_policy" not in _engine(2, 2, 3).t and _engine(2, 2, 3).policy_record is None       # off: nothing is allocated


def test_library_refusals(dev):
    """Before any launch: a NULL buffer, max_plies == 0, a coefficient that is negative or not finite -- on the launch alone and on
    both move forms; the buffer keeps its sentinel and no game advances."""
    from alphaquoridorgnn_amd import _lib
    eng = _engine(3, 2, 3, policy_target="completed_q")
    lib = eng.lib
    _sentinel(eng)
    u = torch.zeros((3,), dtype=torch.float64, device=eng.dev)

    def calls(pr, e=eng):
        yield lib.aqg_engine_record_improved_policy(ctypes.byref(e.e), ctypes.byref(pr), e._stream())
        for name in ("aqg_engine_move_policy", "aqg_engine_finish_move_policy"):
            yield getattr(lib, name)(ctypes.byref(e.e), _lib.ptr(u), 0, None, None, None, ctypes.byref(pr), e._stream())

    def struct(c_visit=50.0, c_scale=1.0, buf=eng.t["hist_policy"].data_ptr()):
        pr = _lib.PolicyRecordStruct()
        pr.c_visit, pr.c_scale, pr.hist_policy = c_visit, c_scale, buf
        return pr

    for pr, word in ((struct(buf=None), "hist_policy"), (struct(c_visit=-1.0), "c_visit"), (struct(c_visit=float("nan")), "c_visit"),
                     (struct(c_visit=float("inf")), "c_visit"), (struct(c_scale=-1e-9), "c_scale"), (struct(c_scale=float("nan")), "c_scale"),
                     (struct(c_scale=float("inf")), "c_scale")):
        for rc in calls(pr):
            assert rc != 0 and word in lib.aqg_last_error().decode(), (word, lib.aqg_last_error())
    flat = _engine(3, 2, 3, record_history=False)                   # max_plies == 0
    for rc in calls(struct(), flat):
        assert rc != 0 and "history" in lib.aqg_last_error().decode()
    assert lib.aqg_engine_record_improved_policy(ctypes.byref(eng.e), None, eng._stream()) != 0
    assert lib.aqg_engine_record_improved_policy(None, ctypes.byref(struct()), eng._stream()) != 0
    assert lib.aqg_engine_move_policy(ctypes.byref(eng.e), None, 0, None, None, None, ctypes.byref(struct()), eng._stream()) != 0
    torch.cuda.synchronize()
    assert (eng.t["hist_policy"].cpu().numpy().view(np.int32) == NAN_BITS).all()
    assert eng.counters()["moves"] == 0 and flat.counters()["moves"] == 0
    # a NULL option is the move without it: the _policy form with every option NULL plays the plain move
    a, b = _engine(3, 4, 3, fake_bias=1), _engine(3, 4, 3, fake_bias=1)
    uu = torch.from_numpy(np.asarray([0.1, 0.5, 0.9])).to(eng.dev)
    a.move(uu)
    assert lib.aqg_engine_move_policy(ctypes.byref(b.e), _lib.ptr(uu), 0, None, None, None, None, b._stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.t[k], b.t[k]) for k in ("hist_visits", "hist_action", "hist_state72", "root_state", "game_plies"))
