"""Games that start from given positions (include/aqgnn.h, "start positions"), on the GPU: engine_reset_kernel / engine_refill_kernel with a
table against tests/_start_positions.refill_reference; whole games from a table against a host loop that restates oracle.mcts.play from
a given state; two game sets against one; tree reuse, resignation, the completed-Q record and the any-shape evaluator on a refilled
engine; paired matches against the host loop; random_book against random_book_reference; forked self_play() end to end.

Boards 3 and 5, 8 simulations.  Everything asserted is integers or bytes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _start_positions as SP   # noqa: E402

pytestmark = pytest.mark.gpu

SIMS, BIAS = 8, 2
_ROWS = {}


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _rows(N, plies, count=3):
    if (N, plies, count) not in _ROWS:
        rows = SP.start_rows(N, plies, count, seed=7 * N + plies)
        rows.setflags(write=False)
        _ROWS[N, plies, count] = rows
    return _ROWS[N, plies, count]


def _engine(G, N, sims=SIMS, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    kw.setdefault("fake_bias", BIAS)
    return BatchedSelfPlay(kw.pop("model", None), num_games=G, sims=sims, board_size=N, **kw)


def _index(Q, rows, seed):
    return np.random.RandomState(seed).randint(0, len(rows), Q).astype(np.int32)


# ---------------------------------------------------------------------------------------------- A. reset and refill
@pytest.mark.parametrize("explicit", (False, True), ids=("modulo", "index"))
@pytest.mark.parametrize("G", (1, 2, 3, 4, 5))
def test_reset_and_refill_start_from_the_table(dev, G, explicit):
    """1 to 5 slots, a quota above them: after reset() and after every refill a slot's position is the row of the game it was handed;
    every other slot, the slot tables and the counters are the statement's; the table itself is untouched."""
    N = 3 if G % 2 else 5
    rows = _rows(N, 2 if G < 4 else 4)
    Q = 2 * G + 3
    index = _index(Q, rows, seed=G) if explicit else None
    eng = _engine(G, N, sims=1, quota=Q, temperature=0.0, start_states=rows, start_index=index)
    sets = [list(range(G)), [0], [G - 1], list(range(G)), list(range(G))]
    wants = SP.refill_reference(G, Q, sets, rows, index)
    assert wants[-1]["counters"][3] == Q
    for round_ in range(2):
        states = eng.root_states72().cpu().numpy()
        assert np.array_equal(states, np.stack([rows[SP.row_of_game(g, rows, index)] for g in range(G)])), "reset"
        for move, (ended, want) in enumerate(zip(sets, wants)):
            acts = np.full((G,), eng.A, dtype=np.int32)            # an action past the board leaves a slot alone
            acts[ended] = -1                                       # ... -1 ends its game as a dead end
            eng.apply_actions(torch.from_numpy(acts))
            got = {name: eng.t[name].cpu().numpy() for name in ("slot_game", "game_active", "game_slot", "game_first_move", "game_done", "counters")}
            for name in ("slot_game", "game_active", "game_slot", "game_first_move", "game_done"):
                assert np.array_equal(got[name], want[name]), (name, move)
            assert tuple(got["counters"][:5].tolist()) == want["counters"], move
            now = eng.root_states72().cpu().numpy()
            for s in range(G):
                if want["refilled"][s]:
                    assert np.array_equal(now[s], want["start72"][s]), (move, s)
                else:
                    assert np.array_equal(now[s], states[s]), (move, s)
            states = now
        assert np.array_equal(eng.t["start_states72"].cpu().numpy(), rows)
        if explicit:
            assert np.array_equal(eng.t["start_index"].cpu().numpy(), index)
        eng.reset()
    assert eng.t["counters"].cpu().numpy().tolist() == [G, 0, 0, G, 0, 0, 0, 0]


def test_kernels_fall_back_to_the_opening_on_a_row_outside_the_table(dev):
    """The guard inside the kernels: the host refuses such an index, so the entry point is called with a struct of the test's own."""
    from alphaquoridorgnn_amd import _lib
    from oracle import quoridor as oq
    rows = _rows(3, 2)
    eng = _engine(3, 3, sims=1, quota=6, temperature=0.0, start_states=rows)
    index = torch.tensor([-1, 1, 3, 2, 2 ** 31 - 1, 0], dtype=torch.int32, device=dev)
    table = _lib.StartTableStruct()
    table.states72, table.index, table.count = eng.t["start_states72"].data_ptr(), index.data_ptr(), 3
    _lib.check(eng.lib.aqg_engine_reset_start(ctypes.byref(eng.e), ctypes.byref(table), eng._stream()), "aqg_engine_reset_start")
    opening = oq.init_record(3)
    assert np.array_equal(eng.root_states72().cpu().numpy(), np.stack([opening, rows[1], opening]))
    acts = torch.full((3,), -1, dtype=torch.int32, device=dev)
    _lib.check(eng.lib.aqg_engine_apply_actions_start(ctypes.byref(eng.e), _lib.ptr(acts), ctypes.byref(table), eng._stream()), "apply")
    assert np.array_equal(eng.root_states72().cpu().numpy(), np.stack([rows[2], opening, rows[0]]))
    for bad in ((None, 3), (eng.t["start_states72"].data_ptr(), 0)):          # refused before a launch
        table.states72, table.count = bad
        assert eng.lib.aqg_engine_reset_start(ctypes.byref(eng.e), ctypes.byref(table), eng._stream()) != 0
        assert eng.lib.aqg_engine_apply_actions_start(ctypes.byref(eng.e), _lib.ptr(acts), ctypes.byref(table), eng._stream()) != 0


def test_constructor_refuses_a_bad_table(dev):
    from oracle import quoridor as oq
    rows = _rows(3, 2)
    for index, word in (([0, 1, 3, 0, 0], "outside the 3 rows"), ([0, 1, -1, 0, 0], "outside the 3 rows"), ([0, 1, 2, 0], "4 entries for 5 games"),
                        ([0, 1, 2, 0, 1, 2], "6 entries for 5 games")):
        with pytest.raises(ValueError, match=word):
            _engine(2, 3, quota=5, start_states=rows, start_index=index)
    from alphaquoridorgnn_amd.game_logic import check_state_reference
    odd = rows.copy()
    odd[1] = next(r for r in (oq.next_record(rows[1], a) for a in oq.legal_actions(rows[1])) if check_state_reference(r, 3) == 32)
    with pytest.raises(ValueError, match=r"row 1 cannot start a game: checker flags 32 \(1 of 3"):
        _engine(2, 3, quota=5, start_states=odd)
    garbage = odd.copy()
    garbage[2, 0], garbage[2, 5] = 200, 7
    flags = check_state_reference(garbage[2], 3)
    assert flags & 3 == 3
    with pytest.raises(ValueError, match=rf"row 1 cannot start a game: checker flags 32 \(2 of 3"):
        _engine(2, 3, quota=5, start_states=garbage)
    with pytest.raises(ValueError, match=rf"row 2 cannot start a game: checker flags {flags} \(1 of 3"):
        _engine(2, 3, quota=5, start_states=np.stack([rows[0], rows[1], garbage[2]]))
    with pytest.raises(ValueError, match="needs start_states"):
        _engine(2, 3, quota=5, start_index=[0] * 5)
    with pytest.raises(ValueError, match="uint8"):
        _engine(2, 3, quota=5, start_states=rows[:0])
    eng = _engine(2, 3, start_states=rows)
    with pytest.raises(ValueError, match="without start_states"):
        eng.search(rows[:2])


# ---------------------------------------------------------------------------------------------- B. whole games against the host loop
def _play_and_hold(N, rows, index, slots, games, capture, **options):
    """A generation from a table of uniforms at T = 1; every game against play_from over its own column of the table."""
    from oracle import mcts as om
    stream = torch.cuda.Stream() if capture else torch.cuda.default_stream()
    with torch.cuda.stream(stream):
        eng = _engine(slots, N, quota=games, temperature=1.0, start_states=rows, start_index=index, **options)
        limit = eng.max_plies * (-(-games // slots))
        U = np.random.RandomState(100 * N + slots).random_sample((limit, slots))
        c = eng.play_generation(uniforms=torch.from_numpy(U), check_every=1)
        got = {name: eng.t[name].cpu().numpy() for name in ("game_plies", "game_slot", "game_first_move", "game_result", "hist_state72",
                                                           "hist_visits", "hist_action")}
        hist = [x.cpu().numpy() for x in eng.history_tensors()]
    assert c["finished"] == games and c["dead_ends"] == 0
    model, wants = om.FakeModel(BIAS), []
    for k in range(games):
        first, slot = int(got["game_first_move"][k]), int(got["game_slot"][k])
        want = SP.play_from(model, rows[SP.row_of_game(k, rows, index)], SIMS, U[first:first + eng.max_plies, slot],
                            temperature_plies=options.get("temperature_plies", 0))
        p = want["plies"]
        assert int(got["game_plies"][k]) == p and int(got["game_result"][k]) == want["result"], k
        assert np.array_equal(got["hist_state72"][k, :p], want["states"]), k
        assert np.array_equal(got["hist_visits"][k, :p], want["visits"]), k
        assert np.array_equal(got["hist_action"][k, :p], want["actions"]), k
        wants.append(want)
    for i, name in enumerate(("states", "visits", "z")):
        assert np.array_equal(hist[i], np.concatenate([w[name] for w in wants])), name
    return wants


@pytest.mark.parametrize("capture", (False, True), ids=("plain_launches", "captured_graph"))
@pytest.mark.parametrize("N, plies", ((3, 2), (3, 4), (5, 2), (5, 4)))
def test_whole_games_from_a_table(dev, N, plies, capture):
    """Five games on two slots and on five, starts 2 and 4 plies deep, the explicit index on two slots and the default one on five:
    history_tensors(), game_result and game_plies bit for bit the host loop's; a game is the same game on either engine when its
    uniforms are.  On a stream of its own the move's search is a captured graph, on the default stream plain launches."""
    rows = _rows(N, plies)
    index = _index(5, rows, seed=N + plies)
    _play_and_hold(N, rows, index, 2, 5, capture)
    _play_and_hold(N, rows, None, 5, 5, capture)


def test_temperature_plies_count_the_games_own_plies(dev):
    """Starts four plies deep with temperature_plies = 2: the first two plies of every GAME are sampled, the rest take the first
    maximum -- by the record's counter (4 and up) no ply would be sampled."""
    rows = _rows(5, 4)
    wants = _play_and_hold(5, rows, None, 2, 5, True, temperature_plies=2)
    assert all(w["plies"] > 2 for w in wants)


# ---------------------------------------------------------------------------------------------- C. a game is a function of its index
def _generation(eng):
    c = eng.play_generation()
    assert c["active"] == 0
    return [x.cpu().numpy() for x in eng.history_tensors()]


def _general_model(N):
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    torch.manual_seed(5)
    return GraphPolicyValueNetwork(6, 16, 2, N * N + 2 * (N - 1) ** 2, board_size=N).to("cuda").eval()


@pytest.mark.parametrize("option", ("plain", "tree_reuse", "resign", "completed_q", "general"))
def test_five_games_on_two_slots_are_the_games_on_five(dev, option):
    """T = 0, so a game is a function of its start alone: 5 games on 2 slots (reset + refills) leave the bytes of 5 games on 5 slots
    (reset only), with tree reuse, with resignation, with the completed-Q record and on the any-shape evaluator; every game's first
    row is its row of the table."""
    N = 3 if option in ("plain", "general") else 5
    rows = _rows(N, 2)
    index = _index(5, rows, seed=3)
    kw = dict(plain={}, tree_reuse=dict(tree_reuse=True), resign=dict(resign_threshold=0.05, resign_disable_fraction=0.2, resign_seed=4),
              completed_q=dict(policy_target="completed_q"), general=dict(evaluator="general", model=_general_model(N)))[option]
    out = []
    for slots in (2, 5):
        eng = _engine(slots, N, quota=5, temperature=0.0, start_states=rows, start_index=index, seed=slots, **kw)
        hist = _generation(eng)
        extra = [eng.t[name].cpu().numpy() for name in ("game_plies", "game_result")]
        if option == "completed_q":
            extra.append(eng.history_policies().cpu().numpy().view(np.int32))
        if option == "resign":
            extra.append(eng.t["game_resigned"].cpu().numpy())
        firsts = eng.t["hist_state72"][:, 0].cpu().numpy()
        assert np.array_equal(firsts, rows[index]), slots
        out.append(hist + extra)
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    if option == "resign":
        assert out[0][-1].any(), "no game resigned: the case shows nothing about resignation"


def test_two_sets_against_one(dev):
    """MultiSetSelfPlay hands each set its slice of the index: 7 games on two sets of two slots are the 7 games of one engine, in
    history_tensors()' order, with the caller's index and with the default one."""
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    rows = _rows(3, 2)
    for index in (_index(7, rows, seed=9), None):
        multi = MultiSetSelfPlay(None, num_games=4, sims=SIMS, num_sets=2, quota=7, board_size=3, evaluator="fake", fake_bias=BIAS,
                                 temperature=0.0, start_states=rows, start_index=index)
        assert [e.quota for e in multi.sets] == [4, 3]
        got = _generation(multi)
        one = _generation(_engine(7, 3, temperature=0.0, start_states=rows, start_index=index))
        for a, b in zip(got, one):
            assert np.array_equal(a, b)
        firsts = np.concatenate([e.t["hist_state72"][:, 0].cpu().numpy() for e in multi.sets])
        assert np.array_equal(firsts, np.stack([rows[SP.row_of_game(k, rows, index)] for k in range(7)]))


def test_a_table_of_the_opening_record_is_the_engine_without_one(dev):
    from oracle import quoridor as oq
    U = torch.from_numpy(np.random.RandomState(2).random_sample((14 * 3, 2)))
    engines = [_engine(2, 3, quota=5, temperature=1.0, **kw) for kw in ({}, dict(start_states=oq.init_record(3)[None, :]))]
    for eng in engines:
        eng.play_generation(uniforms=U, check_every=1)
    plain, table = ({k: v.cpu().numpy() for k, v in eng.t.items()} for eng in engines)
    assert set(table) - set(plain) == {"start_states72"}
    for name in plain:
        assert plain[name].tobytes() == table[name].tobytes(), name


# ---------------------------------------------------------------------------------------------- D. paired matches
@pytest.mark.parametrize("N", (3, 5))
def test_paired_match_is_the_host_loop(dev, N):
    """Two fake-evaluator biases at T = 0 from a book of three openings, eight games: game 2j and 2j + 1 both start from opening
    j % 3, player 0 moving first in game 2j and player 1 in game 2j + 1.  The points are the host loop's; a second play() gives the
    same points; with the players exchanged game 2j's points are 1 - game 2j + 1's and the reverse."""
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    from alphaquoridorgnn_amd.openings import pair_report
    from oracle import mcts as om
    book, biases = _rows(N, 2), (6, 0)
    match = BatchedMatch(biases, 8, sims=SIMS, board_size=N, temperature=0.0, evaluator="fake", openings=book)
    points = match.play()
    models = [om.FakeModel(b) for b in biases]
    want = [SP.match_points_from(models, book[(i // 2) % 3], i % 2, SIMS) for i in range(8)]
    assert points == want
    for first, eng in enumerate(match.engines):
        assert np.array_equal(eng.t["hist_state72"][:, 0].cpu().numpy(), book[np.arange(4) % 3]), first
    moves = []
    for eng in match.engines:                                      # (count the second play()'s moves: it must play, not read old results)
        eng.move = (lambda move: lambda *a, **kw: (moves.append(1), move(*a, **kw))[1])(eng.move)
    assert match.play() == points and len(moves) >= 4              # played again, from the book again
    assert match.report() == pair_report(points) and match.report()["pairs"] == 4
    swapped = BatchedMatch(biases[::-1], 8, sims=SIMS, board_size=N, temperature=0.0, evaluator="fake", openings=book).play()
    for j in range(4):
        assert swapped[2 * j] == 1.0 - points[2 * j + 1] and swapped[2 * j + 1] == 1.0 - points[2 * j], j


def test_a_match_without_openings_is_the_match_as_it_was(dev):
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    from oracle import mcts as om
    U = [np.random.RandomState(5 + f).random_sample((14, 3)) for f in range(2)]
    uni = [torch.from_numpy(u) for u in U]
    a = BatchedMatch((6, 0), 6, sims=SIMS, board_size=3, evaluator="fake", openings=None)
    b = BatchedMatch((6, 0), 6, sims=SIMS, board_size=3, evaluator="fake")
    assert all(eng.start is None for eng in a.engines)
    points = a.play(uni)
    assert points == b.play(uni)
    models = [om.FakeModel(6), om.FakeModel(0)]
    for i in range(6):            # ... and the reference's: evaluate_play from the opening
        first = i % 2
        p, _ = om.evaluate_play(models[first], models[1 - first], SIMS, N=3, uniforms=U[first][:, i // 2])
        assert points[i] == (p if first == 0 else 1.0 - p), i
    with pytest.raises(ValueError, match="report"):
        a.report()


# ---------------------------------------------------------------------------------------------- E. books
@pytest.mark.parametrize("N, plies, count, mirrors", ((3, 2, 16, False), (5, 2, 64, False), (3, 2, 12, True), (5, 4, 24, True), (3, 4, 40, True)))
def test_random_book_is_the_reference(dev, N, plies, count, mirrors):
    from alphaquoridorgnn_amd.game_logic import check_states_batch
    from alphaquoridorgnn_amd.openings import random_book, random_book_reference
    from alphaquoridorgnn_amd.replay import KEY_BYTES
    book = random_book(N, plies, count, seed=3, drop_mirrors=mirrors)
    assert book.is_cuda and book.dtype == torch.uint8 and tuple(book.shape) == (count, 72)
    assert not check_states_batch(book, N).any()
    rows = book.cpu().numpy()
    assert np.array_equal(rows, random_book_reference(N, plies, count, seed=3, drop_mirrors=mirrors))
    assert ((rows[:, 68].astype(int) | (rows[:, 69].astype(int) << 8)) == plies).all()
    assert len({r[KEY_BYTES].tobytes() for r in rows}) == count


def test_random_book_never_returns_a_short_book(dev):
    from alphaquoridorgnn_amd.openings import random_book
    with pytest.raises(ValueError, match="only 64 of 65"):
        random_book(3, 2, 65, seed=3, drop_mirrors=False)
    with pytest.raises(ValueError, match="even"):
        random_book(3, 3, 4, seed=3)


# ---------------------------------------------------------------------------------------------- F. forked self-play
_LOOP = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, engine, openings, pv_mcts, self_play as sp
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
from alphaquoridorgnn_amd.replay import ReplayWindow

assert constants.BOARD_SIZE == 3
torch.manual_seed(3)
dev = aqd.device()
model = GraphPolicyValueNetwork(6, 16, 2, 17, board_size=3).to(dev).eval()
pv_mcts.PV_EVALUATE_COUNT = 8
played = []


class Recording(engine.MultiSetSelfPlay):
    def __init__(self, *a, **kw):
        self.start_kw = {k: kw.get(k) for k in ("start_states", "start_index")}
        super().__init__(*a, **kw)
        played.append(self)


sp.MultiSetSelfPlay = Recording


def window(share):
    if share is not None:
        sp.SP_START_FROM_WINDOW_SHARE = share
    w = sp.SP_REPLAY = ReplayWindow(3, max_generations=3, capacity_rows=600, device=dev)
    for seed in (17, 18):
        os.remove(sp.self_play(model, games=12, seed=seed))
    return w


off = [x.cpu().numpy().copy() for x in window(None).tensors()]
zero = window(0.0)
print("SHARE_0_IS_THE_OPTION_OFF", all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(off, zero.tensors())),
      all(e.start_kw == dict(start_states=None, start_index=None) for e in played), zero.fork_updates)
# the third generation forks half of its games from the two the window holds
sp.SP_START_FROM_WINDOW_SHARE = 0.5
table, index = openings.fork_table(zero, 12, 0.5, 19, zero.fork_updates)
ring = zero.tensors()[0].cpu().numpy().copy()
os.remove(sp.self_play(model, games=12, seed=19))
eng = played[-1]
firsts = np.concatenate([e.t["hist_state72"][:, 0].cpu().numpy() for e in eng.sets])
forked = index > 0
print("TABLE_AND_INDEX", np.array_equal(eng.start_kw["start_states"], table), np.array_equal(eng.start_kw["start_index"], index),
      zero.fork_updates, sp.SP_FORKED_LAST == int(forked.sum()))
print("FORKED_GAMES", 2 <= int(forked.sum()) <= 10, np.array_equal(firsts[forked], table[index[forked]]),
      all(any(np.array_equal(r, x) for x in ring) for r in firsts[forked]))
print("OTHER_GAMES", bool((firsts[~forked] == openings.opening_record(3)).all()))
print("ROWS_APPENDED", zero.generations[-1] == int(sum(int(e.t["game_plies"].sum()) for e in eng.sets)))
'''


def test_self_play_forks_from_the_window(dev, tmp_path):
    """One child process on the 3x3 board: with SP_START_FROM_WINDOW_SHARE = 0 a two-generation window holds the bytes of the option
    off and no table is built; at 0.5 the third generation's engine is handed openings.fork_table's table and index, every forked
    game's first row is the window row its draw names, every other game starts from the opening, and the progress line counts them."""
    import subprocess
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="3", AQG_EVAL_CACHE_SLOTS="0")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("SHARE_0_IS_THE_OPTION_OFF True True 0", "TABLE_AND_INDEX True True 1 True", "FORKED_GAMES True True True", "OTHER_GAMES True",
                 "ROWS_APPENDED True"):
        assert line in r.stdout, (line, r.stdout[-3000:])
    assert "games forked from the window" in r.stdout
