"""CPU tests (no GPU): the six option-bearing move exports of libaqgnn_hip.so share one validation, and its order is behaviour --
the first failing check names the error: the engine, the two targets, tree reuse, resignation.  Every call here is refused on the
host before anything is launched."""
import ctypes

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
