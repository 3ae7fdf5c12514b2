"""The kernels that end every self-play move, alone and at their edges (csrc/mcts_move.hip): engine_finish_move_kernel on tree pools
the test writes -- real roots after a real search, their visit counts overwritten and their child count narrowed to a prefix -- against
tests/_move_cycle.finish_move_reference, and engine_refill_kernel with idle slots in every wavefront and in both chunks, driven through
aqg_engine_apply_actions by scripts of end sets, against refill_reference; engine_reset_kernel behind them; one generation through
move() at 1,100 slots; and the refusal of a temperature the kernel cannot use.

Everything asserted is integers or bit patterns.  At T == 1 the uniforms sit ON the cdf values; at any other T they keep 1e-9 from
them (tests/_move_cycle.py says why)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _move_cycle as MC   # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
HISTORY = ("hist_state72", "hist_visits", "hist_action", "hist_value")


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _engine(G, sims, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    return BatchedSelfPlay(None, num_games=G, sims=sims, board_size=N, **kw)


def _host(eng):
    return {name: t.cpu().numpy().copy() for name, t in eng.t.items()}


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- A. the choice of a move
def _write_pools(eng, chunk):
    """Every slot's real root block after search(): the cases' visit counts and sums over it, the root's count narrowed to the case's."""
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    from oracle import quoridor as oq
    G, cap = eng.G, eng.node_cap
    pools = eng.t["node_rec"].cpu().numpy().view(NODE_DTYPE).reshape(G, cap).copy()
    legal = []
    for g, c in enumerate(chunk):
        kids = int(pools["kids"][g, 0])
        first, real = kids & 0xFFFFFF, kids >> 24
        acts = oq.legal_actions(c["root"])
        assert real == len(acts) and first >= 1 and first + real <= cap and pools["action"][g, first:first + real].tolist() == acts
        cnt = c["cnt"]
        assert 1 <= cnt <= real                                  # never a range the search did not make
        pools["n"][g, first:first + cnt], pools["w"][g, first:first + cnt], pools["q"][g, first:first + cnt] = c["n"], c["w"], c["q"]
        pools["kids"][g, 0] = first | (cnt << 24)
        pools["n"][g, 0], pools["w"][g, 0] = c["n_root"], c["w_root"]
        legal.append(acts[:cnt])
    eng.t["node_rec"].copy_(torch.from_numpy(pools.view(np.float64).reshape(G * cap, 4)))
    return legal


def _expected(eng, before, chunk, legal, us, K, inactive):
    """Every engine tensor after the launch, from the tensors before it and the statements (root_state of an active slot is taken
    from the device: it is compared as a record, through root_states72).  Returns (tensors, next records, ended slots)."""
    from oracle import quoridor as oq
    want = {name: x.copy() for name, x in before.items()}
    records, ended = {}, 0
    for g, c in enumerate(chunk):
        if g in inactive:
            continue
        plies = oq.State(c["root"]).plies_played
        idx, action, value = MC.finish_move_reference(c["n"], legal[g], c["w_root"], c["n_root"], eng.temperature, K, plies, us[g])
        assert action == legal[g][idx]
        want["hist_action"][g, 0] = action
        row = np.zeros((eng.A,), dtype=np.int16)
        row[legal[g]] = c["n"]
        want["hist_visits"][g, 0] = row
        want["hist_state72"][g, 0] = c["root"]
        want["hist_value"][g, 0] = value
        want["game_plies"][g] = 1
        records[g], done, z = MC.transition_reference(c["root"], action)
        if done:
            want["game_done"][g], want["game_result"][g], want["game_active"][g] = 1, z, 0
            want["counters"][0] -= 1
            want["counters"][1] += 1
            ended += 1
    return want, records, ended


def _run_cases(eng, cases, K=0, inactive=()):
    """The cases G at a time through the engine's slots, every case with each of its uniforms in turn.  Returns (launches, ended)."""
    from alphaquoridorgnn_amd import _lib
    G = eng.G
    launches = ended = 0
    for start in range(0, len(cases), G):
        chunk = [cases[(start + g) % len(cases)] for g in range(G)]
        eng.reset()
        eng.search(torch.from_numpy(np.stack([c["root"] for c in chunk])))
        legal = _write_pools(eng, chunk)
        for g in inactive:
            eng.t["game_active"][g] = 0
            for name in HISTORY:
                eng.t[name][g].view(torch.uint8).fill_(SENTINEL)
        saved = {name: t.clone() for name, t in eng.t.items()}
        before = _host(eng)
        assert not before["hist_visits"][[g for g in range(G) if g not in inactive], 0].any()        # the search cleared the row
        for j in range(max(len(c["us"]) for c in chunk)):
            if j:
                for name, t in eng.t.items():
                    t.copy_(saved[name])
            us = [c["us"][j % len(c["us"])] for c in chunk]
            u = torch.tensor(us, dtype=torch.float64).to(eng.dev)
            rc = eng.lib.aqg_engine_finish_move_targets(ctypes.byref(eng.e), _lib.ptr(u), K, _lib.ptr(eng.t["hist_value"]), eng._stream())
            assert rc == 0, eng.lib.aqg_last_error()
            after = _host(eng)
            states = eng.root_states72().cpu().numpy()
            want, records, n_ended = _expected(eng, before, chunk, legal, us, K, inactive)
            names = [c["name"] for c in chunk]
            for g, rec in records.items():
                assert np.array_equal(states[g], rec), (names[g], us[g])
                want["root_state"][g] = after["root_state"][g]
            for name in after:                                   # the pool, the inactive slots' rows and sentinels, every other tensor
                assert _same(after[name], want[name]), (name, names, us)
            launches += 1
            ended += n_ended
    return launches, ended


@pytest.mark.parametrize("G", (1, 4, 5, 9))
def test_sampled_choice_on_the_cdf_values(dev, G):
    """T == 1 on prefixes of the 9x9 opening root at every lane-round edge and on real 9x9 roots: one child with every visit, visited
    children between runs of unvisited ones with u ON every cdf value and one ulp below it, 32767 beside ones, random counts.  G = 9:
    slots 2 and 7 are inactive, their history rows a sentinel."""
    eng = _engine(G, 2, 9, temperature=1.0, record_search_value=True)
    launches, _ = _run_cases(eng, MC.sampling_cases() + MC.real_root_cases(9), inactive=(2, 7) if G == 9 else ())
    assert launches >= 100 // G


@pytest.mark.parametrize("N,G", [(3, 4), (3, 9), (5, 5), (5, 1)])
def test_sampled_choice_on_small_boards(dev, N, G):
    """Real 3x3 and 5x5 roots, one without a wall in hand, and one a step from the goal: the terminal branch of the transition."""
    eng = _engine(G, 2, N, temperature=1.0, record_search_value=True)
    _, ended = _run_cases(eng, MC.real_root_cases(N), inactive=(2, 7) if G == 9 else ())
    assert ended > 0 or N != 3


@pytest.mark.parametrize("G", (1, 4, 5, 9))
def test_first_maximum_tied_and_last(dev, G):
    """A maximum tied among three children and one in the last child: an engine at T = 0 takes the first maximum on both roots; one at
    T = 1 with temperature_plies = 1 samples the root at ply 0 and takes the first maximum of the root at ply 1."""
    cases = MC.first_maximum_cases()
    inactive = (2, 7) if G == 9 else ()
    _run_cases(_engine(G, 2, 9, temperature=0.0, record_search_value=True), cases, K=0, inactive=inactive)
    _run_cases(_engine(G, 2, 9, temperature=1.0, record_search_value=True), cases, K=1, inactive=inactive)


@pytest.mark.parametrize("G", (1, 4, 5, 9))
@pytest.mark.parametrize("T", MC.TEMPERATURES)
def test_other_temperatures(dev, T, G):
    """pow(n, 1 / T) at T = 0.5, 2 and 0.25 on the random and the 32767 patterns, u the midpoint of every visited child's interval."""
    eng = _engine(G, 2, 9, temperature=T, record_search_value=True)
    assert eng.temperature == T
    _run_cases(eng, MC.temperature_cases(T), inactive=(2, 7) if G == 9 else ())


def test_the_smallest_accepted_temperature(dev):
    """T = 0.02 is accepted at 200 simulations (log2(200) / 0.02 = 382): visit counts up to 200 go through pow(n, 50) and the move is
    the statement's.  The statement gets the float32 the engine holds, not 0.02."""
    eng = _engine(4, 200, 9, temperature=0.02, record_search_value=True)
    assert eng.temperature == float(np.float32(0.02)) != 0.02
    cases = MC.temperature_cases(eng.temperature, nmax=200, big=False)
    assert max(int(c["n"].max()) for c in cases) == 200
    _run_cases(eng, cases)


# ---------------------------------------------------------------------------------------------- C. refusals
def test_a_bad_temperature_in_the_struct_is_refused_untouched(dev):
    """The struct's field overwritten behind the constructor's check: aqg_engine_move and aqg_engine_finish_move return non-zero with
    a message that names the temperature, and no engine tensor changes."""
    from alphaquoridorgnn_amd import _lib
    eng = _engine(3, 200, 3, temperature=1.0, quota=5)
    eng.move()
    before = _host(eng)
    u = torch.full((3,), 0.5, dtype=torch.float64, device=eng.dev)
    for bad in (-1.0, float("nan"), float("inf"), 0.005):
        eng.e.temperature = bad
        for form in ("aqg_engine_move", "aqg_engine_finish_move"):
            rc = getattr(eng.lib, form)(ctypes.byref(eng.e), _lib.ptr(u), eng._stream())
            assert rc != 0 and "temperature" in eng.lib.aqg_last_error().decode(), (bad, form)
            torch.cuda.synchronize()
            after = _host(eng)
            assert all(_same(after[name], before[name]) for name in before), (bad, form)
    eng.e.temperature = 0.02                                     # accepted at 200 simulations
    eng.move(u)
    assert eng.counters()["moves"] == 2


# ---------------------------------------------------------------------------------------------- B. the slot refill
RESET_OWNED = ("counters", "game_plies", "game_result", "game_done", "game_slot", "game_first_move", "root_state", "game_active",
               "slot_game", "node_count", "leaf_flag", "stat_leaf_evals", "stat_terminal_sims")


def _play_script(eng, sets):
    """One pawn step in every slot (so that no running game stands at the opening), then the script's end sets move by move through
    apply_actions: -1 ends a slot's game as a dead end, an action past the board leaves the slot alone.  Every table and counter
    against the statement after every move."""
    from oracle import quoridor as oq
    G, Q, A = eng.G, eng.quota, eng.A
    opening = oq.init_record(eng.N)
    step = min(a for a in oq.legal_actions(opening) if a < eng.N ** 2)
    wants = MC.refill_reference(G, Q, [[]] + [list(s) for s in sets])
    plies = (np.arange(Q) < G).astype(np.int32)
    states = None
    for move, want in enumerate(wants):
        acts = np.full((G,), step if move == 0 else A, dtype=np.int32)
        if move:
            acts[sets[move - 1]] = -1
        eng.t["leaf_flag"].fill_(1)
        eng.apply_actions(torch.from_numpy(acts))
        got = {name: eng.t[name].cpu().numpy() for name in ("slot_game", "game_active", "game_slot", "game_first_move", "game_done",
                                                           "game_plies", "game_result", "leaf_flag", "counters")}
        for name in ("slot_game", "game_active", "game_slot", "game_first_move", "game_done"):
            assert np.array_equal(got[name], want[name]), (name, move)
        assert tuple(got["counters"][:5].tolist()) == want["counters"] and not got["counters"][5:].any(), (move, got["counters"], want["counters"])
        assert np.array_equal(got["game_plies"], plies) and not got["game_result"].any(), move
        refilled = want["refilled"]
        assert np.array_equal(got["leaf_flag"], np.where(refilled, 0, 1)), move
        now = eng.root_states72().cpu().numpy()
        assert (now[refilled] == opening).all(), move
        if states is None:
            assert (now == oq.next_record(opening, step)).all()
        else:
            assert np.array_equal(now[~refilled], states[~refilled]), move
        states = now
        # game_slot: a map of the started games onto slots in which no two live games share a slot
        started = want["counters"][3]
        slot = got["game_slot"]
        live = np.flatnonzero(got["game_done"][:started] == 0)
        assert (slot[:started] >= 0).all() and (slot[:started] < G).all() and (slot[started:] == -1).all()
        assert len(set(slot[live].tolist())) == len(live) == want["counters"][0]
        assert np.array_equal(got["slot_game"][slot[live]], live)
    return wants


def _check_reset(eng, **kw):
    fresh = _engine(eng.G, eng.sims, eng.N, quota=eng.quota, **kw)
    eng.reset()
    got, want = _host(eng), _host(fresh)
    for name in RESET_OWNED:
        assert _same(got[name], want[name]), name
    G, Q = eng.G, eng.quota
    assert got["game_slot"].tolist() == list(range(G)) + [-1] * (Q - G)
    assert got["counters"].tolist() == [G, 0, 0, G, 0, 0, 0, 0]


@pytest.mark.parametrize("G", MC.REFILL_SLOTS)
def test_refill_scripts(dev, G):
    """Idle slots in every wavefront and in both chunks of 1,024, never meeting the quota: every slot at once twice, lane 63 of every
    wavefront then lane 0, the last slot, slots 1023 and 1024, a random half then a random 1 %.  reset() behind them leaves what a
    fresh engine holds."""
    kw = dict(temperature=0.0)
    eng = _engine(G, 1, 3, quota=MC.plain_quota(G), **kw)
    for name, sets in MC.plain_scripts(G):
        eng.reset()
        _play_script(eng, sets)
    _check_reset(eng, **kw)


@pytest.mark.parametrize("G", MC.REFILL_SLOTS)
def test_refill_quota_cuts(dev, G):
    """The last refill has fewer games left than idle slots: the cut inside a wavefront, exactly between two, inside the second chunk,
    and with no game left; the move behind it hands nothing out and leaves the retired slots retired."""
    for name, Q, sets, retired in MC.cut_scripts(G):
        eng = _engine(G, 1, 3, quota=Q, temperature=0.0)
        wants = _play_script(eng, sets)
        assert wants[-1]["counters"][3] == Q and (wants[-1]["slot_game"] == -1).sum() > 0, name
        if retired is not None:
            assert int(eng.t["slot_game"][retired]) == -1 and int(eng.t["game_active"][retired]) == 0, name
        _check_reset(eng, temperature=0.0)


def test_refill_through_move_at_size(dev):
    """1,100 slots play 2,500 searched games from an explicit table of uniforms.  The recorded game lengths, fed to the statement,
    give every game's slot and first move; 24 games -- the quota's last, games of the second chunk's slots and of lane 63 -- are the
    games a one-slot engine plays from their slot's column of the table."""
    G, Q, sims, bias = 1100, 2500, 6, 2
    eng = _engine(G, sims, 3, temperature=1.0, quota=Q, fake_bias=bias)
    limit = eng.max_plies * 3
    U = torch.from_numpy(np.random.RandomState(17).random_sample((limit, G)))
    c = eng.play_generation(uniforms=U, check_every=1)
    assert c["finished"] == Q and c["started"] == Q and c["active"] == 0 and c["dead_ends"] == 0
    got = {name: eng.t[name].cpu().numpy() for name in ("game_plies", "game_slot", "game_first_move", "game_done", "game_result", "slot_game",
                                                       "hist_state72", "hist_visits", "hist_action")}
    plies, slot, first = got["game_plies"], got["game_slot"], got["game_first_move"]
    last = MC.refill_reference(G, Q, MC.end_sets_from_lengths(G, Q, plies))[-1]
    assert np.array_equal(slot, last["game_slot"]) and np.array_equal(first, last["game_first_move"])
    assert got["game_done"].all() and (got["slot_game"] == -1).all() and c["moves"] == last["counters"][4]
    later = np.arange(Q) >= G
    picks = [Q - 1] + np.flatnonzero(later & (slot >= 1024))[::8][:11].tolist() + np.flatnonzero(later & (slot % 64 == 63))[:8].tolist()
    picks += np.flatnonzero(later & (first == first.max()))[:2].tolist()
    picks = list(dict.fromkeys([int(k) for k in picks] + list(range(G - 2, G + 30))))[:24]
    assert len(set(picks)) == 24 and any(slot[k] >= 1024 and k >= G for k in picks) and any(slot[k] % 64 == 63 and k >= G for k in picks)
    one = _engine(1, sims, 3, temperature=1.0, fake_bias=bias)
    for k in picks:
        one.reset()
        one.play_generation(uniforms=U[first[k]:first[k] + eng.max_plies, slot[k]:slot[k] + 1], check_every=1)
        p = int(one.t["game_plies"][0])
        assert p == plies[k], k
        assert np.array_equal(one.t["hist_state72"][0, :p].cpu().numpy(), got["hist_state72"][k, :p]), k
        assert np.array_equal(one.t["hist_visits"][0, :p].cpu().numpy(), got["hist_visits"][k, :p]), k
        assert np.array_equal(one.t["hist_action"][0, :p].cpu().numpy(), got["hist_action"][k, :p]), k
        assert int(one.t["game_result"][0]) == got["game_result"][k], k
