"""CPU tests (no GPU): the six option-bearing move exports of libaqgnn_hip.so share one validation, and its order is behaviour --
the first failing check names the error: the engine, the two targets, tree reuse, resignation.  Every call here is refused on the
host before anything is launched."""
import ctypes

import numpy as np
import pytest

FORMS = ("aqg_engine_move_targets", "aqg_engine_finish_move_targets", "aqg_engine_move_reuse", "aqg_engine_finish_move_reuse",
         "aqg_engine_move_resign", "aqg_engine_finish_move_resign")


def _structs(bad_options=False):
    """The structs of tests/test_resign_cpu.py and tests/test_tree_reuse_cpu.py: 5x5, 4 games, 8 simulations, the fake evaluator.
    bad_options: a tree-reuse struct and a resignation struct that their own checks refuse."""
    from alphaquoridorgnn_amd import _lib
    e = _lib.EngineStructGeneral()
    e.board_size, e.num_games, e.quota, e.sims, e.prior_mode, e.max_plies = 5, 4, 4, 8, 1, 28
    e.node_cap = 1 + 16 * 136
    for name in ("slot_game", "game_done", "game_slot", "game_first_move"):
        setattr(e, name, 0x1000)
    ru = _lib.TreeReuseStruct()
    ru.keep_visits = -1 if bad_options else 8
    for name in ("kept", "child_index", "stat_moves_kept", "stat_visits_kept"):
        setattr(ru, name, 0x1000)
    rs = _lib.ResignStruct()
    rs.threshold, rs.min_ply, rs.disable_fraction, rs.seed = (0.0 if bad_options else 0.25), 0, 0.1, 5
    rs.resign_min = rs.game_resigned = 0x1000
    return e, ru, rs


def _call(form, e, ru, rs, temperature_plies=0, hist_value=None):
    """The export `form` on the NULL stream, with every option struct its signature has."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    args = [ctypes.byref(e), ctypes.c_void_p(0x1000), temperature_plies, hist_value]
    if form.endswith(("_reuse", "_resign")):
        args.append(ctypes.byref(ru))
    if form.endswith("_resign"):
        args.append(ctypes.byref(rs))
    rc = getattr(lib, form)(*args, None)
    return rc, lib.aqg_last_error().decode()


REFUSED_TEMPERATURES = [(-1.0, 50), (float("nan"), 50), (float("inf"), 50), (0.005, 200)]      # (temperature, simulations)
ACCEPTED_TEMPERATURES = [(0.0, 50), (1.0, 50), (0.25, 50), (2.0, 50), (0.02, 200)]


@pytest.mark.parametrize("temperature,sims", REFUSED_TEMPERATURES)
def test_a_temperature_the_kernel_cannot_use_is_refused(temperature, sims):
    """include/aqgnn.h, `temperature`: finite and >= 0, and log2(sims + keep_visits) / temperature <= 1016 -- by the host check, by
    the engine's constructor in front of any allocation (no GPU is asked for), and by every move form of the library.  The reference
    raises for the negative and for the too small one."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.selfplay_options import check_temperature
    from oracle import mcts as om
    with pytest.raises(ValueError, match="temperature"):
        check_temperature(temperature, sims)
    with pytest.raises(ValueError, match="temperature"):
        BatchedSelfPlay(None, num_games=4, sims=sims, board_size=5, evaluator="fake", temperature=temperature)
    if temperature == temperature and abs(temperature) != float("inf"):
        with pytest.raises((ZeroDivisionError, OverflowError)):
            om.boltzman([0, sims - 1], temperature)
    for form in FORMS + ("aqg_engine_move", "aqg_engine_finish_move"):
        e, ru, rs = _structs()
        e.temperature, e.sims, e.node_cap = temperature, sims, 1 + 2 * sims * 136
        rc, err = _call(form, e, ru, rs) if form in FORMS else _plain(form, e)
        assert rc != 0 and "temperature" in err and "temperature_plies" not in err, (form, err)


@pytest.mark.parametrize("temperature,sims", ACCEPTED_TEMPERATURES)
def test_a_usable_temperature_is_accepted(temperature, sims):
    from alphaquoridorgnn_amd.selfplay_options import check_temperature
    from oracle import mcts as om
    assert check_temperature(temperature, sims) == float(np.float32(temperature))
    if temperature:
        assert np.isfinite(om.boltzman([sims] * 136, float(np.float32(temperature)))).all()
    # the library's check passes it on to the next one: a negative temperature_plies is what these calls are refused for
    for form in FORMS:
        e, ru, rs = _structs()
        e.temperature, e.sims, e.node_cap = temperature, sims, 1 + 2 * sims * 136
        rc, err = _call(form, e, ru, rs, temperature_plies=-1)
        assert rc != 0 and "temperature_plies" in err, (form, err)


def test_the_temperature_rule_counts_the_kept_visits():
    """With tree reuse a child can hold keep_visits + sims visits: 0.01 passes at 200 simulations (log2(200) / 0.01 = 765) and is
    refused with 800 kept ones beside them (log2(1000) / 0.01 = 997 is fine, log2(1200) / 0.01 = 1023 is not)."""
    from alphaquoridorgnn_amd.selfplay_options import check_temperature
    assert check_temperature(0.01, 200) == check_temperature(0.01, 200, 800) == float(np.float32(0.01))
    with pytest.raises(ValueError, match="temperature"):
        check_temperature(0.01, 200, 1000)
    for bad in ("1.0", None, True):
        with pytest.raises(ValueError, match="temperature"):
            check_temperature(bad, 50)
    for keep, refused in ((800, False), (1000, True)):
        e, ru, rs = _structs()
        e.temperature, e.sims, ru.keep_visits, e.node_cap = 0.01, 200, keep, 1 + (200 + keep) * 136
        # (the accepted struct is stopped by the next check, a negative temperature_plies, which stands in front of tree reuse's own)
        rc, err = _call("aqg_engine_move_reuse", e, ru, rs, temperature_plies=0 if refused else -1)
        assert rc != 0 and ("temperature_plies" in err) == (not refused) and "temperature" in err, err


def _plain(form, e):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, form)(ctypes.byref(e), ctypes.c_void_p(0x1000), None)
    return rc, lib.aqg_last_error().decode()


@pytest.mark.parametrize("form", FORMS)
def test_one_validation_order_for_every_move_form(form):
    # the engine's own checks come first, whatever the option structs hold
    for N in (4, 11):
        e, ru, rs = _structs(bad_options=True)
        e.board_size = N
        rc, err = _call(form, e, ru, rs, temperature_plies=-1)
        assert rc != 0 and "unsupported board_size" in err, (N, err)
    # then the two targets, in front of the option structs' checks
    e, ru, rs = _structs(bad_options=True)
    rc, err = _call(form, e, ru, rs, temperature_plies=-1)
    assert rc != 0 and "temperature_plies" in err, err
    e, ru, rs = _structs()
    rc, err = _call(form, e, ru, rs, temperature_plies=-1)
    assert rc != 0 and "temperature_plies" in err, err
    # a search-value column without a history: the target's refusal, not resignation's own "needs a history"
    for bad in (False, True):
        e, ru, rs = _structs(bad_options=bad)
        e.max_plies = 0
        rc, err = _call(form, e, ru, rs, hist_value=ctypes.c_void_p(0x1000))
        assert rc != 0 and "hist_value" in err, err
    # tree reuse in front of resignation
    if form.endswith("_resign"):
        e, ru, rs = _structs(bad_options=True)
        rc, err = _call(form, e, ru, rs)
        assert rc != 0 and "keep_visits" in err and "threshold" not in err, err
