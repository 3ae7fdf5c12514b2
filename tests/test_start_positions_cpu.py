"""Start positions, the parts that need no GPU: the checker's numpy statement against hand-stated flags, the host build of the
kernel's predicate (aqg_host_check_state) against the statement on crafted records, garbage and every position of seeded oracle
walks, the start index's checks and its split over game sets, and pair_report against hand-computed vectors."""
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _start_positions as SP   # noqa: E402

BOARDS = (3, 5, 9)


@pytest.mark.parametrize("N", BOARDS)
def test_reference_gives_the_hand_stated_flags(N):
    from alphaquoridorgnn_amd.game_logic import check_state_reference
    cases = SP.crafted_records(N)
    seen = set()
    for name, rec, flags in cases:
        assert check_state_reference(rec, N) == flags, (name, check_state_reference(rec, N), flags)
        seen.add(flags)
    assert {1, 2, 4, 8, 16, 32, 64} <= seen and sum(1 for f in seen if bin(f).count("1") == 2) >= 8


@pytest.mark.parametrize("N", BOARDS)
def test_host_checker_is_the_reference(N):
    from alphaquoridorgnn_amd.game_logic import check_state_host, check_state_reference
    recs = [rec for _, rec, _ in SP.crafted_records(N)] + list(SP.garbage_records(N, 300, seed=N))
    for i, rec in enumerate(recs):
        assert check_state_host(rec, N) == check_state_reference(rec, N), i
    # other constants than the board's own
    rec = recs[0]
    assert check_state_host(rec, N, num_walls=SP.params(N)[0] + 1) == check_state_reference(rec, N, num_walls=SP.params(N)[0] + 1) == 4
    assert check_state_host(rec, N, plies_for_draw=0) == check_state_reference(rec, N, plies_for_draw=0) == 16


@pytest.mark.parametrize("N", BOARDS)
def test_walk_positions_read_clean_or_odd(N):
    """Every even-ply position of seeded random walks reads 0 and every odd-ply position exactly 32, by the host checker and by the
    statement."""
    from alphaquoridorgnn_amd.game_logic import check_state_host, check_state_reference
    recs = SP.walk_positions(N, games={3: 40, 5: 12, 9: 3}[N], seed=11 + N)
    plies = recs[:, 68].astype(int) | (recs[:, 69].astype(int) << 8)
    assert (plies % 2 == 0).sum() > 20 and (plies % 2 == 1).sum() > 20
    for rec, p in zip(recs, plies):
        want = 32 if p % 2 else 0
        assert check_state_host(rec, N) == want, rec
        assert check_state_reference(rec, N) == want, rec


def test_host_checker_refusals():
    import ctypes
    from alphaquoridorgnn_amd import _lib
    from oracle import quoridor as oq
    lib = _lib.load()
    rec = oq.init_record(5)
    p = rec.ctypes.data_as(ctypes.c_void_p)
    assert lib.aqg_host_check_state(5, p, 2, 28) == 0
    assert lib.aqg_host_check_state(4, p, 2, 28) == -1 and lib.aqg_host_check_state(5, None, 2, 28) == -1
    assert lib.aqg_host_check_state(5, p, -1, 28) == -1 and lib.aqg_host_check_state(5, p, 2, 70000) == -1


def test_start_index_checks_and_set_slices():
    from alphaquoridorgnn_amd.selfplay_options import check_start_index, set_start_indices
    rows = np.zeros((3, 72), dtype=np.uint8)
    assert check_start_index(None, 3, 5) is None
    assert check_start_index([0, 2, 1, 1, 0], 3, 5).dtype == np.int32
    for bad, word in (([0, 1, 2, 3, 0], "outside"), ([0, -1, 0, 0, 0], "outside"), ([0, 1], "entries"), ([0] * 6, "entries"),
                      ([0.5] * 5, "integer"), ([[0] * 5], "one-dimensional")):
        with pytest.raises(ValueError, match=word):
            check_start_index(bad, 3, 5)
    # the default index, written out and cut at the sets' blocks: a game's row does not depend on the sets
    parts = set_start_indices(rows, None, [3, 2, 2])
    assert [p.tolist() for p in parts] == [[0, 1, 2], [0, 1], [2, 0]]
    parts = set_start_indices(rows, [2, 2, 1, 0, 0, 1, 2], [3, 2, 2])
    assert [p.tolist() for p in parts] == [[2, 2, 1], [0, 0], [1, 2]]
    assert set_start_indices(None, None, [3, 2]) == [None, None]
    with pytest.raises(ValueError, match="entries"):
        set_start_indices(rows, [0, 1, 2], [3, 2])
    with pytest.raises(ValueError, match="needs start_states"):
        set_start_indices(None, [0, 1, 2], [3])
    with pytest.raises(ValueError, match="uint8"):
        set_start_indices(np.zeros((3, 71), dtype=np.uint8), None, [3])


# ---------------------------------------------------------------------------------------------- pair_report
def _close(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == want or abs(got - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("points, want", [
    # all wins, all draws, all losses: no spread
    ([1, 1, 1, 1, 1, 1], dict(pairs=3, mean=1.0, se=0.0, elo=math.inf, elo_se=0.0, los=1.0)),
    ([0.5, 0.5, 0.5, 0.5], dict(pairs=2, mean=0.5, se=0.0, elo=0.0, elo_se=0.0, los=0.5)),
    ([0, 0, 0, 0], dict(pairs=2, mean=0.0, se=0.0, elo=-math.inf, elo_se=0.0, los=0.0)),
    # a single pair: a mean and no error estimate
    ([1, 0], dict(pairs=1, mean=0.5, se=math.nan, elo=0.0, elo_se=math.nan, los=math.nan)),
    ([1, 0.5], dict(pairs=1, mean=0.75, se=math.nan, elo=-400 * math.log10(1 / 3), elo_se=math.nan, los=math.nan)),
    # d = (0.5, 0.75): mean 0.625, std(ddof=1) = 0.25 / sqrt 2, se = 0.125, (mean - 0.5) / se = 1
    ([0.5, 0.5, 1, 0.5], dict(pairs=2, mean=0.625, se=0.125, elo=-400 * math.log10(0.6), elo_se=0.125 * 400 / (math.log(10) * 0.625 * 0.375),
                              los=0.5 * (1 + math.erf(1 / math.sqrt(2))))),
    # d = (0.75, 0.5, 1, 0.25): mean 0.625, sum of squares 0.3125, se = sqrt(5 / 192), (mean - 0.5) / se = sqrt 0.6
    ([1, 0.5, 0.5, 0.5, 1, 1, 0, 0.5], dict(pairs=4, mean=0.625, se=math.sqrt(5 / 192), elo=-400 * math.log10(0.6),
                                            elo_se=math.sqrt(5 / 192) * 400 / (math.log(10) * 0.625 * 0.375),
                                            los=0.5 * (1 + math.erf(math.sqrt(0.3))))),
    # every pair splits 1 : 0 the same way round: mean 0.5 with no spread
    ([1, 0, 1, 0, 1, 0], dict(pairs=3, mean=0.5, se=0.0, elo=0.0, elo_se=0.0, los=0.5)),
])
def test_pair_report_hand_computed(points, want):
    from alphaquoridorgnn_amd.openings import pair_report
    got = pair_report(points)
    assert set(got) == set(want)
    for k in want:
        assert type(got[k]) is type(want[k]) and _close(got[k], want[k]), (k, got[k], want[k])


def test_pair_report_refuses_odd_and_empty():
    from alphaquoridorgnn_amd.openings import pair_report
    for bad in ([], [1], [1, 0, 1]):
        with pytest.raises(ValueError, match="even number"):
            pair_report(bad)


# ---------------------------------------------------------------------------------------------- books on the host
def _distinct_after(N, plies):
    """The distinct non-terminal positions `plies` plies behind the opening, enumerated with the oracle."""
    from oracle import quoridor as oq
    level = {oq.init_record(N).tobytes(): oq.State(N=N)}
    for _ in range(plies):
        nxt = {}
        for s in level.values():
            for a in s.legal_actions():
                t = s.next(a)
                if not t.is_done():
                    nxt[t.rec.tobytes()] = t
        level = nxt
    return level


def test_reference_book_rows_and_counts():
    """Every row clean, even-ply and distinct; the position counts of the issue: 64 after two plies on 3x3 (count 65 raises), 653 on
    5x5 (count 64 is found)."""
    from alphaquoridorgnn_amd.game_logic import check_state_reference, mirror_record
    from alphaquoridorgnn_amd.openings import random_book_reference
    from alphaquoridorgnn_amd.replay import KEY_BYTES
    assert len(_distinct_after(3, 2)) == 64 and len(_distinct_after(5, 2)) == 653
    for N, plies, count, mirrors in ((3, 2, 16, False), (5, 2, 64, False), (3, 2, 12, True), (5, 4, 24, True)):
        book = random_book_reference(N, plies, count, seed=3, drop_mirrors=mirrors)
        assert book.shape == (count, 72) and book.dtype == np.uint8
        assert all(check_state_reference(r, N) == 0 for r in book)
        assert ((book[:, 68].astype(int) | (book[:, 69].astype(int) << 8)) == plies).all()
        keys = {r[KEY_BYTES].tobytes() for r in book}
        assert len(keys) == count
        if plies == 2:
            assert all(r.tobytes() in _distinct_after(N, 2) for r in book)
        if mirrors:      # no row is the mirror image of another row
            for i, r in enumerate(book):
                image = mirror_record(r)[KEY_BYTES].tobytes()
                assert all(image != o[KEY_BYTES].tobytes() for j, o in enumerate(book) if j != i)
    # a book does not depend on how many rows are asked for: the shorter one is a prefix
    assert np.array_equal(random_book_reference(3, 2, 16, seed=3, drop_mirrors=False)[:5], random_book_reference(3, 2, 5, seed=3, drop_mirrors=False))
    with pytest.raises(ValueError, match="only 64 of 65"):
        random_book_reference(3, 2, 65, seed=3, drop_mirrors=False)
    for plies in (0, 1, 3, 2.5):
        with pytest.raises(ValueError, match="even"):
            random_book_reference(3, plies, 4, seed=0)
    with pytest.raises(ValueError, match="count"):
        random_book_reference(3, 2, 0, seed=0)


def test_book_save_load(tmp_path):
    from alphaquoridorgnn_amd import openings
    book = openings.random_book_reference(5, 2, 9, seed=1)
    path = tmp_path / "book.npz"
    openings.save(path, book)
    rows, N = openings.load(path)
    assert N == 5 and rows.dtype == np.uint8 and np.array_equal(rows, book)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["board_size", "states72"]
    with pytest.raises(ValueError, match="uint8"):
        openings.save(path, book.astype(np.int32))


# ---------------------------------------------------------------------------------------------- rows of a window, forks
def _host_window(N, generations, seed):
    import torch
    from alphaquoridorgnn_amd.replay import ReplayWindow
    A = N * N + 2 * (N - 1) ** 2
    window = ReplayWindow(N, max_generations=generations, capacity_rows=400)
    for g in range(generations):
        recs = SP.walk_positions(N, 6, seed=seed + g)
        window.append_rows(torch.from_numpy(recs), torch.zeros((len(recs), A)), torch.zeros((len(recs),)))
    return window


def test_from_window_rows():
    from alphaquoridorgnn_amd.counter_rng import counter_uniform, stream_key
    from alphaquoridorgnn_amd.game_logic import check_state_reference
    from alphaquoridorgnn_amd.openings import from_window
    from alphaquoridorgnn_amd.replay import KEY_BYTES
    window = _host_window(3, 2, seed=5)
    ring = window.tensors()[0].numpy()
    rows, slots = from_window(window, 1000, seed=9, update=2, return_slots=True)
    assert 0 < len(rows) <= len(window) and np.array_equal(rows, ring[slots])
    assert all(check_state_reference(r, 3) == 0 for r in rows)
    assert len({r[KEY_BYTES].tobytes() for r in rows}) == len(rows)
    keys = np.asarray(counter_uniform(stream_key(9, 2), slots.astype(np.uint64)))
    assert (np.diff(keys) > 0).all()                                     # in key order
    # every usable position of the window is there once
    usable = {r[KEY_BYTES].tobytes() for r in ring[window.index().numpy()] if check_state_reference(r, 3) == 0}
    assert usable == {r[KEY_BYTES].tobytes() for r in rows}
    # fewer rows asked for: a prefix; another update: another order
    assert np.array_equal(from_window(window, 5, seed=9, update=2), rows[:5])
    assert not np.array_equal(from_window(window, 5, seed=9, update=3), rows[:5])
    assert from_window(window, 0, seed=9).shape == (0, 72)


def test_fork_table_and_draws():
    from alphaquoridorgnn_amd.openings import fork_draws, fork_table, from_window, opening_record
    window = _host_window(3, 2, seed=5)
    assert fork_table(window, 40, 0.0, seed=1, generation=0) is None and fork_table(None, 40, 0.5, seed=1, generation=0) is None
    table, index = fork_table(window, 40, 0.5, seed=1, generation=4)
    rows = from_window(window, 40, 1, 4)
    assert np.array_equal(table[0], opening_record(3)) and np.array_equal(table[1:], rows)
    assert index.dtype == np.int32 and index.shape == (40,) and index.min() == 0 and index.max() <= len(rows)
    assert 8 <= (index > 0).sum() <= 32                                   # about half of 40
    # a game's draw is a function of (seed, generation, game index): more games only add draws
    assert np.array_equal(fork_draws(1, 4, 25, 0.5, len(rows)), fork_draws(1, 4, 40, 0.5, len(rows))[:25])
    assert not np.array_equal(fork_draws(1, 5, 40, 0.5, len(rows)), index)
    assert (fork_draws(1, 4, 40, 1.0, len(rows)) > 0).all() and not fork_draws(1, 4, 40, 0.5, 0).any()
    for bad in (-0.1, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="share"):
            fork_table(window, 40, bad, seed=1, generation=0)


# ---------------------------------------------------------------------------------------------- parse-time refusals
def _args(*argv):
    from alphaquoridorgnn_amd import train_cycle as tc
    return tc._parser().parse_args(list(argv))


def test_train_cycle_refuses_at_parse_time():
    from alphaquoridorgnn_amd import train_cycle as tc
    for argv, word in ((("--eval-opening-plies", "3", "--eval-games", "8"), "even"),
                       (("--eval-opening-plies", "-2", "--eval-games", "8"), "even"),
                       (("--eval-opening-plies", "4", "--eval-games", "7"), "even number of games"),
                       (("--eval-opening-plies", "4"), "even number of games"),          # EN_GAME_COUNT is 15
                       (("--eval-opening-seed", "5"), "needs --eval-opening-plies"),
                       (("--start-from-window", "0.5"), "needs --replay-generations"),
                       (("--start-from-window", "1.5", "--replay-generations", "2"), "share"),
                       (("--start-from-window", "nan", "--replay-generations", "2"), "share")):
        with pytest.raises(ValueError, match=word):
            tc._check_start_args(_args(*argv))
    assert tc._check_start_args(_args()) == (None, None, None)
    assert tc._check_start_args(_args("--eval-opening-plies", "4", "--eval-games", "8", "--eval-opening-seed", "7",
                                      "--start-from-window", "0.25", "--replay-generations", "1")) == (4, 7, 0.25)
    assert tc._check_start_args(_args("--eval-opening-plies", "0")) == (0, None, None)


def test_match_and_engine_refuse_before_a_device_is_touched():
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch, check_opening_options
    from alphaquoridorgnn_amd.selfplay_options import check_start_table
    with pytest.raises(ValueError, match="num_games must be even"):
        BatchedMatch((0, 1), 5, sims=4, board_size=3, evaluator="fake", openings=np.zeros((2, 72), dtype=np.uint8))
    with pytest.raises(ValueError, match="needs start_states"):
        check_start_table(None, [0, 1], 3, 2, "cpu")
    with pytest.raises(ValueError, match="uint8"):
        check_start_table(np.zeros((2, 72), dtype=np.int64), None, 3, 2, "cpu")
    with pytest.raises(ValueError, match="outside the 2 rows"):
        check_start_table(np.zeros((2, 72), dtype=np.uint8), [0, 2], 3, 2, "cpu")
    assert check_opening_options(0, 15) == 0 and check_opening_options(2, 16) == 2
