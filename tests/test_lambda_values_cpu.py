"""Lambda-return value targets without a GPU (include/aqgnn.h, "lambda-return value targets"): the numpy statement
engine.lambda_values_reference against the recurrence and its closed form in float64, its invariants and skip rules, the option
checks, and the host routes (the .history rows and a host ReplayWindow) that carry the lambda-returns in q's place."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _lambda_values as LV   # noqa: E402
from tests.test_replay_window_cpu import counts_rows   # noqa: E402

LAMBDAS = LV.LAMBDAS + (0.25, 0.7)


def _reference(plies, result, done, q, lam, fill=np.nan):
    from alphaquoridorgnn_amd.engine import lambda_values_reference
    out = np.full(q.shape, fill, dtype=np.float32)
    assert lambda_values_reference(plies, result, done, q, lam, out) is out
    return out


def _random_games(n, hp, seed):
    """n done games of 1 .. hp plies (1 and hp among them), results -1 / 0 / 1, q uniform in [-1, 1]."""
    rng = np.random.RandomState(seed)
    plies = rng.randint(1, hp + 1, n).astype(np.int32)
    plies[:2] = (1, hp)
    result = rng.randint(-1, 2, n).astype(np.int8)
    q = rng.uniform(-1.0, 1.0, (n, hp)).astype(np.float32)
    return plies, result, np.ones(n, dtype=np.uint8), q


# ------------------------------------------------------------------ 1. the statement against float64
@pytest.mark.parametrize("form", ["recurrence", "closed_form"])
@pytest.mark.parametrize("lam", LAMBDAS)
def test_reference_against_float64(lam, form):
    """Within 2 T 2^-24 of the float64 statement taken with the float32 lambda, for |q| <= 1.  The bar is derived: a ply adds four
    roundings of at most 2^-25 each -- a = 1 - lambda, two products and a sum of magnitudes at most 1 -- and inherits the error of
    the ply after it with weight lambda <= 1; T plies therefore stay below 4 T 2^-25 = 2 T 2^-24."""
    plies, result, done, q = _random_games(150, 129, seed=int(lam * 1000) + 5)
    got = _reference(plies, result, done, q, lam)
    f64 = LV.recurrence_f64 if form == "recurrence" else LV.closed_form_f64
    worst = 0.0
    for k in range(len(plies)):
        T = int(plies[k])
        err = np.abs(got[k, :T].astype(np.float64) - f64(q[k], T, int(result[k]), lam)).max()
        worst = max(worst, err / (2.0 ** -24))
        assert err <= 2 * T * 2.0 ** -24, (k, T, err)
        assert np.isnan(got[k, T:]).all()
    print(f"lambda {lam}: worst error {worst:.2f} units of 2^-24")


# ------------------------------------------------------------------ 2. invariants
def test_lambda_one_is_the_outcome():
    """lambda = 1: a = 0 and every ply is 0 * q + 1 * z_t.  Bit for bit z_t for a decided game; for a draw the sum of two zeros of
    either sign is a zero whose sign is not z_t's at every ply (0 * q is +0 for q > 0 and z_t is -0 at an odd ply), so a draw is
    compared as a number -- the reason the definition gives for lambda = 0."""
    plies, result, done, q = _random_games(60, 70, seed=1)
    got = _reference(plies, result, done, q, 1.0)
    for k in range(len(plies)):
        T = int(plies[k])
        z = np.array([LV.z_of(int(result[k]), t) for t in range(T)], dtype=np.float32)
        if result[k] != 0:
            assert np.array_equal(LV.bits(got[k, :T]), LV.bits(z)), k
        else:
            assert (got[k, :T] == z).all() and (got[k, :T] == 0).all(), k


def test_lambda_zero_is_the_search_value():
    plies, result, done, q = LV.games(40, 70, seed=2)
    q[0, :4] = (1.0, -1.0, 0.0, -0.0)
    got = _reference(plies, result, done, q, 0.0)
    live, written = LV.processed(plies, done, 70)
    assert live.any() and (got[written] == q[written]).all() and np.isnan(got[~written]).all()


def test_a_game_of_one_ply():
    for r in (-1, 0, 1):
        for lam in LAMBDAS:
            q = np.array([[0.375, 9.0]], dtype=np.float32)
            got = _reference(np.array([1], np.int32), np.array([r], np.int8), np.array([1], np.uint8), q, lam)
            lam32 = np.float32(lam)
            want = np.float32(np.float32((np.float32(1.0) - lam32) * q[0, 0]) + np.float32(lam32 * np.float32(r)))
            assert got[0, 0] == want and np.isnan(got[0, 1])


@pytest.mark.parametrize("lam", LAMBDAS)
def test_exchanging_the_sides_negates_every_entry(lam):
    plies, result, done, q = LV.games(50, 66, seed=3)
    a = _reference(plies, result, done, q, lam)
    b = _reference(plies, (-result).astype(np.int8), done, -q, lam)
    _, written = LV.processed(plies, done, 66)
    assert written.any() and (b[written] == -a[written]).all()               # rounding to nearest is symmetric; a zero's sign is not pinned
    assert np.isnan(a[~written]).all() and np.isnan(b[~written]).all()


def test_skipped_games_write_nothing():
    """NaN sentinels: a game that is not done, a game of 0 plies, of hp + 1 plies and of a negative count leave their row alone, and a
    processed game leaves the plies past its end alone."""
    hp = 6
    plies = np.array([3, 3, 0, hp + 1, -2, hp, 1], dtype=np.int32)
    done = np.array([1, 0, 1, 1, 1, 7, 1], dtype=np.uint8)
    result = np.array([1, 1, -1, 1, 0, -1, 0], dtype=np.int8)
    q = np.random.RandomState(4).uniform(-1, 1, (7, hp)).astype(np.float32)
    got = _reference(plies, result, done, q, 0.6)
    wrote = ~np.isnan(got)
    assert np.array_equal(wrote.sum(1), [3, 0, 0, 0, 0, hp, 1])
    assert wrote[0, :3].all() and wrote[5].all() and wrote[6, 0]
    for k in (0, 5, 6):
        T = int(plies[k])
        assert np.abs(got[k, :T] - LV.recurrence_f64(q[k], T, int(result[k]), 0.6)).max() <= 2 * T * 2.0 ** -24


def test_reference_refuses_wrong_arrays():
    from alphaquoridorgnn_amd.engine import lambda_values_reference
    plies, result, done, q = LV.games(4, 5, seed=0)
    out = np.zeros_like(q)
    for bad in (dict(hist_value=q.astype(np.float64)), dict(out=np.zeros((4, 6), np.float32)), dict(game_plies=plies[:3]), dict(lam=1.5),
                dict(lam=float("nan"))):
        kw = dict(game_plies=plies, game_result=result, game_done=done, hist_value=q, lam=0.5, out=out)
        kw.update(bad)
        with pytest.raises(ValueError):
            lambda_values_reference(**kw)
    assert not out.any()


# ------------------------------------------------------------------ 3. options
def test_check_value_lambda():
    from alphaquoridorgnn_amd import engine, selfplay_options
    check = selfplay_options.check_value_lambda
    assert engine.check_value_lambda is check
    assert check(0) == 0.0 and check(1) == 1.0 and check(np.float32(0.5)) == 0.5 and check(0.95) == float(np.float32(0.95))
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True, float("inf")):
        with pytest.raises(ValueError, match="value_lambda"):
            check(bad)


def test_train_cycle_refuses_a_lambda_without_a_blend(monkeypatch):
    from alphaquoridorgnn_amd import distributed as aqd, self_play as sp, train_cycle as tc
    assert sp.SP_VALUE_LAMBDA is None
    args = tc._parser().parse_args([])
    assert args.value_lambda is None and tc._check_value_lambda_args(args) is None
    tc._set_target_options(args)
    assert sp.SP_VALUE_LAMBDA is None and sp.SP_VALUE_BLEND == 0.0

    def reached(*a, **k):
        raise AssertionError("a refused command line reached the process group")

    monkeypatch.setattr(aqd, "init_from_env", reached)
    for argv in (["--value-lambda", "0.9"], ["--value-lambda", "0.9", "--value-blend", "0"], ["--value-blend", "0.5", "--value-lambda", "1.5"],
                 ["--value-blend", "0.5", "--value-lambda", "-0.1"], ["--value-blend", "0.5", "--value-lambda", "nan"]):
        with pytest.raises(ValueError, match="value-lambda"):
            tc.main(argv)
        with pytest.raises(ValueError, match="value-lambda"):
            tc._set_target_options(tc._parser().parse_args(argv))
        assert sp.SP_VALUE_LAMBDA is None and sp.SP_VALUE_BLEND == 0.0         # a refused option sets nothing
    try:
        tc._set_target_options(tc._parser().parse_args(["--value-blend", "0.5", "--value-lambda", "0.9"]))
        assert sp.SP_VALUE_BLEND == 0.5 and sp.SP_VALUE_LAMBDA == float(np.float32(0.9))
    finally:
        sp.SP_VALUE_BLEND, sp.SP_VALUE_LAMBDA = 0.0, None


def test_self_play_refuses_a_lambda_without_a_blend(monkeypatch):
    from alphaquoridorgnn_amd import self_play as sp
    monkeypatch.setattr(sp, "SP_VALUE_LAMBDA", 0.9)
    monkeypatch.setattr(sp, "SP_VALUE_BLEND", 0.0)
    with pytest.raises(ValueError, match="SP_VALUE_LAMBDA"):
        sp.self_play(model=object(), games=2, seed=1)
    with pytest.raises(ValueError, match="SP_VALUE_LAMBDA"):
        sp.play(object())
    monkeypatch.setattr(sp, "SP_VALUE_BLEND", 0.5)
    monkeypatch.setattr(sp, "SP_VALUE_LAMBDA", 1.5)
    with pytest.raises(ValueError, match="value_lambda"):
        sp.self_play(model=object(), games=2, seed=1)


# ------------------------------------------------------------------ 4. the host routes carry G in q's place
def test_history_rows_and_host_window_hold_the_blend_of_the_lambda_returns():
    from alphaquoridorgnn_amd.replay import ReplayWindow, blend_targets
    from alphaquoridorgnn_amd.self_play import _history_rows
    N, L = 3, 0.5
    plies = np.array([5, 1, 8], dtype=np.int32)
    result = np.array([1, 0, -1], dtype=np.int8)
    done = np.ones(3, dtype=np.uint8)
    q = np.random.RandomState(9).uniform(-1, 1, (3, 8)).astype(np.float32)
    _, written = LV.processed(plies, done, 8)
    G = _reference(plies, result, done, q, 0.9)[written]                      # game-major, as history_lambda_values() compacts it
    n = int(plies.sum())
    S, V, _ = counts_rows(N, n, seed=3)
    Z = np.concatenate([[int(LV.z_of(int(r), t)) for t in range(T)] for r, T in zip(result, plies)]).astype(np.int8)
    want = blend_targets(Z, G, L)
    assert not np.array_equal(want, blend_targets(Z, q[written], L))          # the lambda-returns are not the search values
    args = (torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
    rows = _history_rows(*args, N, values=torch.from_numpy(G), value_blend=L)
    assert all(type(r[2]) is float for r in rows)
    assert np.array_equal(LV.bits(np.array([r[2] for r in rows], dtype=np.float32)), LV.bits(want))
    w = ReplayWindow(N, max_generations=1, capacity_rows=n)
    w.append_counts(*args, search_value=torch.from_numpy(G), value_blend=L)
    assert np.array_equal(LV.bits(w.rows()[2].numpy()), LV.bits(want))
