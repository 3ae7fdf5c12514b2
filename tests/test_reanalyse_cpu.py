"""Reanalyse without a GPU: replay.refresh_reference (the refresh launch in numpy) against the arithmetic written out, its skips and
its blend; replay.draw_reanalyse_rows' properties; a host ReplayWindow.refresh_counts and its refusals; the ABI, the defaults and
train_cycle's flags."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from alphaquoridorgnn_amd.replay import ReplayWindow, blend_targets, draw_reanalyse_rows, refresh_reference   # noqa: E402
from tests._reanalyse import (MAX_LEGAL, SPECIAL, bits, expected_refresh, kinds_of, policy_size, random_rings, search_rows,   # noqa: E402
                              written_rows)
from tests.test_replay_window_cpu import counts_rows   # noqa: E402


# ------------------------------------------------------------------ the arithmetic and the skips
@pytest.mark.parametrize("N", (3, 5, 7, 9))
@pytest.mark.parametrize("blend", (0.0, 0.25, 1.0))
def test_refresh_reference_is_the_statement(N, blend):
    n, capacity = 40, 77
    visits, actions, count, q, slots, kinds = search_rows(N, n, seed=10 * N, capacity=capacity)
    assert set(SPECIAL) <= set(kinds)
    before = random_rings(N, capacity, seed=N)
    want = expected_refresh(N, visits, actions, count, q, blend, slots, before)
    r72, rpi, rz = (x.copy() for x in before)
    refresh_reference(N, visits, actions, count, q, blend, slots, rpi, rz)
    assert np.array_equal(bits(rpi), bits(want[1])) and np.array_equal(bits(rz), bits(want[2]))
    # which rows were written: exactly the ones the statement names, whole
    written = written_rows(N, visits, count, slots, capacity)
    for kind in ("count0", "zero_visits", "slot_above", "slot_below", "count_negative", "count137"):
        assert not written[kinds.index(kind)]
    for kind in ("plain", "count1", "count136", "big_action"):
        assert written[kinds.index(kind)]
    untouched = np.setdiff1d(np.arange(capacity), slots[written])
    assert np.array_equal(bits(rpi[untouched]), bits(before[1][untouched])) and np.array_equal(bits(rz[untouched]), bits(before[2][untouched]))
    assert len(untouched) == capacity - int(written.sum()) and set(slots[~written]) & set(range(capacity)) <= set(untouched)
    A = policy_size(N)
    for i in np.flatnonzero(written):
        row, c = rpi[slots[i]], int(count[i])
        tot = int(visits[i, :c].astype(np.int64).sum())
        dense = np.zeros(A, dtype=np.int64)
        inside = actions[i, :c] < A
        dense[actions[i, :c][inside]] = visits[i, :c][inside]
        assert np.array_equal(bits(row), bits(np.float32(np.float64(dense) / np.float64(tot))))
    i = kinds.index("count1")
    assert rpi[slots[i]].sum() == 1.0 and np.count_nonzero(rpi[slots[i]]) == 1
    if blend == 0.0:
        assert np.array_equal(bits(rz), bits(before[2]))                      # not even -0.0 for 0.0
    else:
        w = slots[written]
        assert np.array_equal(bits(rz[w]), bits(blend_targets(before[2][w], q[written], blend)))
        assert not np.array_equal(bits(rz[w]), bits(before[2][w]))


def test_refresh_reference_without_a_value_ring_and_its_refusals():
    N, n, capacity = 5, 12, 20
    visits, actions, count, q, slots, _ = search_rows(N, n, seed=3, capacity=capacity)
    _, rpi, rz = random_rings(N, capacity, seed=4)
    a, b = rpi.copy(), rpi.copy()
    refresh_reference(N, visits, actions, count, None, 0.0, slots, a, None)          # no blend: ring_z may be None
    refresh_reference(N, visits, actions, count, q, 0.0, slots, b, None)
    assert np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(a), bits(rpi))
    bad = [lambda: refresh_reference(4, visits, actions, count, None, 0.0, slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions, count, None, 0.5, slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions, count, q, 1.5, slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions, count, q, float("nan"), slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions, count, q, 0.5, slots, rpi, None),
           lambda: refresh_reference(N, visits.astype(np.int64), actions, count, q, 0.5, slots, rpi, rz),
           lambda: refresh_reference(N, visits[:, :100], actions, count, q, 0.5, slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions.astype(np.int8), count, q, 0.5, slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions, count[:5], q, 0.5, slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions, count, q.astype(np.float64), 0.5, slots, rpi, rz),
           lambda: refresh_reference(N, visits, actions, count, q, 0.5, slots.astype(np.int32), rpi, rz),
           lambda: refresh_reference(9, visits, actions, count, q, 0.5, slots, rpi, rz)]          # another board's policy rows
    keep = rpi.copy(), rz.copy()
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(bits(rpi), bits(keep[0])) and np.array_equal(bits(rz), bits(keep[1]))


# ------------------------------------------------------------------ the draw
def test_draw_reanalyse_rows():
    for seed, update, eligible in ((0, 0, 1), (5, 0, 37), (5, 1, 37), (2 ** 40 + 3, 7, 500)):
        last = np.zeros((0,), dtype=np.int64)
        for rows in range(0, min(eligible, 40) + 1):
            d = draw_reanalyse_rows(seed, update, eligible, rows)
            assert d.dtype == np.int64 and d.shape == (min(rows, eligible),)
            assert (np.diff(d) > 0).all() and (d >= 0).all() and (d < eligible).all()          # distinct, ascending, in range
            assert set(last) <= set(d)                                                          # R's draw inside (R + 1)'s
            assert np.array_equal(d, draw_reanalyse_rows(seed, update, eligible, rows))         # the same for any caller
            last = d
        for rows in (eligible, eligible + 1, 10 * eligible):
            assert np.array_equal(draw_reanalyse_rows(seed, update, eligible, rows), np.arange(eligible))
    assert draw_reanalyse_rows(1, 0, 0, 5).shape == (0,)
    # the keys are the counter generator's: the rows of the smallest u_i = counter_uniform(stream_key(seed, update), i)
    from alphaquoridorgnn_amd.counter_rng import counter_uniform, stream_key
    u = np.array([float(counter_uniform(stream_key(5, 1), i)) for i in range(37)])
    assert np.array_equal(draw_reanalyse_rows(5, 1, 37, 9), np.sort(np.argsort(u, kind="stable")[:9]))
    # another update or seed draws other rows
    assert not np.array_equal(draw_reanalyse_rows(5, 0, 37, 9), draw_reanalyse_rows(5, 1, 37, 9))
    assert not np.array_equal(draw_reanalyse_rows(5, 0, 500, 50), draw_reanalyse_rows(6, 0, 500, 50))
    for bad in ((0, 0, -1, 3), (0, 0, 3, -1)):
        with pytest.raises(ValueError):
            draw_reanalyse_rows(*bad)


# ------------------------------------------------------------------ the window on the host
def _window(N=5):
    w = ReplayWindow(N, max_generations=3, capacity_rows=40)
    for k, m in enumerate((17, 9, 21)):                         # the third drops the first and wraps
        S, V, Z = counts_rows(N, m, seed=k)
        w.append_counts(torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
    assert w.generations == [9, 21]
    return w


def _held(w):
    return [x.numpy().copy() for x in w.tensors()]


def test_host_window_refresh_counts():
    N = 5
    w = _window(N)
    index = w.index().numpy()
    stale = np.setdiff1d(np.arange(40), index)
    assert len(stale) == 10 and index[0] > index[-1]                          # the valid interval wraps
    visits, actions, count, q, _, kinds = search_rows(N, 12, seed=8, capacity=40)
    slots = index[[0, 3, 4, 8, 9, 12, 17, 20, 25, 26, 28, 29]].astype(np.int64)
    t = lambda x: torch.from_numpy(x)   # noqa: E731
    before = _held(w)
    book = (w.generations, len(w), w.index().clone())
    w.refresh_counts(t(slots), t(visits), t(actions), t(count), search_value=t(q), value_blend=0.25)
    want = expected_refresh(N, visits, actions, count, q, 0.25, slots, before)
    got = _held(w)
    assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(got, want)) and np.array_equal(got[0], before[0])
    assert not np.array_equal(bits(got[1]), bits(before[1])) and not np.array_equal(bits(got[2]), bits(before[2]))
    assert (w.generations, len(w)) == book[:2] and torch.equal(w.index(), book[2])
    # without a blend the value ring stays; an empty call writes nothing
    w.refresh_counts(t(slots), t(visits), t(actions), t(count))
    w.refresh_counts(t(slots), t(visits), t(actions), t(count), search_value=t(q))
    w.refresh_counts(t(slots[:0]), t(visits[:0]), t(actions[:0]), t(count[:0]))
    assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(_held(w), got))


def test_host_window_refusals_come_before_any_write():
    N = 5
    w = _window(N)
    index = w.index().numpy()
    stale = np.setdiff1d(np.arange(40), index)
    visits, actions, count, q, _, _ = search_rows(N, 4, seed=9, capacity=40)
    count[:] = np.maximum(count, 2)
    good = index[[1, 5, 7, 11]].astype(np.int64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))   # noqa: E731
    before = _held(w)
    bad = [lambda: w.refresh_counts(t(np.array([good[0], stale[0], good[2], good[3]])), t(visits), t(actions), t(count)),      # stale
           lambda: w.refresh_counts(t(np.array([good[0], good[1], good[0], good[3]])), t(visits), t(actions), t(count)),       # repeated
           lambda: w.refresh_counts(t(np.array([good[0], 40, good[2], good[3]])), t(visits), t(actions), t(count)),            # no slot
           lambda: w.refresh_counts(t(np.array([good[0], -1, good[2], good[3]])), t(visits), t(actions), t(count)),
           lambda: w.refresh_counts(t(good.astype(np.int32)), t(visits), t(actions), t(count)),                                # dtypes
           lambda: w.refresh_counts(t(good), t(visits.astype(np.int64)), t(actions), t(count)),
           lambda: w.refresh_counts(t(good), t(visits), t(actions.astype(np.int8)), t(count)),
           lambda: w.refresh_counts(t(good), t(visits), t(actions), t(count.astype(np.int64))),
           lambda: w.refresh_counts(t(good), t(visits), t(actions), t(count), search_value=t(q.astype(np.float64)), value_blend=0.5),
           lambda: w.refresh_counts(t(good), t(visits[:, :100]), t(actions), t(count)),                                        # shapes
           lambda: w.refresh_counts(t(good), t(visits), t(actions[:3]), t(count)),
           lambda: w.refresh_counts(t(good), t(visits), t(actions), t(count[:3])),
           lambda: w.refresh_counts(t(good.reshape(2, 2)), t(visits), t(actions), t(count)),
           lambda: w.refresh_counts(t(good), t(visits), t(actions), t(count), search_value=t(q[:3]), value_blend=0.5),
           lambda: w.refresh_counts(t(good), t(visits), t(actions), t(count), value_blend=0.5),                                # blend
           lambda: w.refresh_counts(t(good), t(visits), t(actions), t(count), search_value=t(q), value_blend=1.5)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(_held(w), before)), k
    with pytest.raises(ValueError):
        ReplayWindow(N, max_generations=2, capacity_rows=8).refresh_counts(t(good), t(visits), t(actions), t(count))          # holds no row
    w.refresh_counts(t(good), t(visits), t(actions), t(count))                                                               # accepted
    assert not np.array_equal(bits(_held(w)[1]), bits(before[1]))


def test_the_stage_on_a_window_without_older_rows():
    from alphaquoridorgnn_amd.reanalyse import check_reanalyse_options, eligible_rows, reanalyse
    N = 5
    w = ReplayWindow(N, max_generations=3, capacity_rows=40)
    assert eligible_rows(w) == 0 and reanalyse(w, None, 10, evaluator="fake") == 0
    S, V, Z = counts_rows(N, 17, seed=0)
    w.append_counts(torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
    assert eligible_rows(w) == 0 and reanalyse(w, None, 10, evaluator="fake") == 0      # the newest generation is never searched again
    assert eligible_rows(_window(N)) == 9 and reanalyse(_window(N), None, 0, evaluator="fake") == 0
    for bad in (dict(rows=-1), dict(rows=1.5), dict(rows=1, sims=0), dict(rows=1, value_blend=1.25), dict(rows=1, value_blend=float("nan")),
                dict(rows=1, slots=0), dict(rows=True)):
        with pytest.raises(ValueError):
            check_reanalyse_options(**bad)
        with pytest.raises(ValueError):
            reanalyse(_window(N), None, bad.pop("rows"), evaluator="fake", **bad)

    class OtherBoard:
        board_size, fused = 9, True
    with pytest.raises(ValueError, match="board"):
        reanalyse(_window(N), OtherBoard(), 4)


# ------------------------------------------------------------------ ABI, defaults, flags
def test_abi_and_binding():
    from alphaquoridorgnn_amd import _lib
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    assert re.search(r"\bint\s+aqg_replay_refresh\s*\(", header) and re.search(r"\bint\s+aqg_engine_root_values\s*\(", header)
    res, args = _lib.SIGNATURES["aqg_replay_refresh"]
    assert res is _lib._c.c_int and len(args) == 13 and args[6] is _lib._c.c_float
    res, args = _lib.SIGNATURES["aqg_engine_root_values"]
    assert res is _lib._c.c_int and len(args) == 3
    assert re.search(r"\breplay_refresh\b", open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "build.sh")).read())
    assert _lib.MAX_LEGAL == MAX_LEGAL and kinds_of(5) == ["plain"] * 5


def test_defaults_and_train_cycle_flags(monkeypatch):
    from alphaquoridorgnn_amd import distributed as aqd, self_play as sp, train_cycle as tc
    assert (sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_SIMS, sp.SP_REANALYSE_VALUE_BLEND, sp.SP_REANALYSE_SLOTS) == (0, None, 0.0, 2048)
    args = tc._parser().parse_args([])
    assert (args.reanalyse_rows, args.reanalyse_sims, args.reanalyse_value_blend) == (None, None, None)
    assert tc._check_reanalyse_args(args) is None
    tc._set_reanalyse_options(args)
    assert (sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_SIMS, sp.SP_REANALYSE_VALUE_BLEND) == (0, None, 0.0)
    ok = ["--replay-generations", "3", "--reanalyse-rows", "4000", "--reanalyse-sims", "25", "--reanalyse-value-blend", "0.5"]
    assert tc._check_reanalyse_args(tc._parser().parse_args(ok)) == (4000, 25, 0.5)
    assert tc._check_reanalyse_args(tc._parser().parse_args(ok[:4])) == (4000, None, 0.0)
    for name, value in (("SP_REANALYSE_ROWS", 0), ("SP_REANALYSE_SIMS", None), ("SP_REANALYSE_VALUE_BLEND", 0.0)):
        monkeypatch.setattr(sp, name, value)                                  # restored after the test
    tc._set_reanalyse_options(tc._parser().parse_args(ok))
    assert (sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_SIMS, sp.SP_REANALYSE_VALUE_BLEND) == (4000, 25, 0.5)

    # every refusal is raised at parse time: main() has touched neither a device nor the process group
    def reached(*a, **k):
        raise AssertionError("main() went past the flag checks")
    monkeypatch.setattr(aqd, "init_from_env", reached)
    for bad in (["--reanalyse-rows", "100"],                                                       # no window
                ["--replay-generations", "1", "--reanalyse-rows", "100"],                          # no older generation
                ["--replay-generations", "3", "--reanalyse-rows", "-1"],
                ["--replay-generations", "3", "--reanalyse-rows", "100", "--reanalyse-sims", "0"],
                ["--replay-generations", "3", "--reanalyse-rows", "100", "--reanalyse-value-blend", "1.5"],
                ["--replay-generations", "3", "--reanalyse-rows", "100", "--reanalyse-value-blend", "-0.1"],
                ["--replay-generations", "3", "--reanalyse-rows", "100", "--reanalyse-value-blend", "nan"],
                ["--replay-generations", "3", "--reanalyse-sims", "10"],                          # the dependent flags alone
                ["--replay-generations", "3", "--reanalyse-value-blend", "0.5"]):
        with pytest.raises(ValueError, match="reanalyse"):
            tc.main(bad)
    assert (sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_SIMS, sp.SP_REANALYSE_VALUE_BLEND) == (4000, 25, 0.5)      # a refused line sets nothing


def test_self_play_refuses_the_option_without_a_window(monkeypatch):
    from alphaquoridorgnn_amd import self_play as sp
    monkeypatch.setattr(sp, "SP_REANALYSE_ROWS", 10)
    monkeypatch.setattr(sp, "SP_REPLAY", None)
    with pytest.raises(ValueError, match="SP_REANALYSE_ROWS"):
        sp.self_play(model=object(), games=1, seed=1)
    monkeypatch.setattr(sp, "SP_REANALYSE_ROWS", -1)
    with pytest.raises(ValueError, match="rows"):
        sp.self_play(model=object(), games=1, seed=1)
