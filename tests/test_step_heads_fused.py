"""Heads inside the MCTS step kernel (csrc/mcts_step.hip engine_step_fast_kernel<N, CACHE, true>, option "step_heads"): the fused form --
step -> trunk per simulation, each step workgroup computing policy and value of its own eight leaves from the pooled rows -- against
the three-launch form (step -> trunk -> gcn_heads_mm_kernel) in one process, with the same seeds and weights.  Every comparison is
exact equality: both forms run the same heads arithmetic (csrc/gcn_heads_split.hpp) on the same pooled rows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _util as U

pytestmark = pytest.mark.gpu

SIMS, MOVES = 13, 6


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _model(dev, params):
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    model = GNNNetwork()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return model.to(dev).eval()


@pytest.fixture(scope="module")
def params():
    from oracle import gnn as og
    return og.init_params(3)


def _near_goal_roots(G):
    """Roots for G slots: the mover one pawn step from its goal row in every other slot (row 1: its children include terminal
    positions, and its game ends within a few moves), the opening in the rest -- so that terminal leaves, finished games and live
    games share step workgroups."""
    from oracle import quoridor as oq
    opening = oq.init_record(9)
    roots = np.stack([opening] * G)
    for g in range(0, G, 2):
        roots[g, 0] = 9 + (g % 9)                        # row 1, some column
        assert any(oq.State(roots[g]).next(a).is_done() for a in oq.State(roots[g]).legal_actions() if a < 81)
    return roots


def _play(dev, params, step_heads, G, roots=None, **kw):
    """MOVES moves of G games with SIMS simulations under one form; everything the two forms must agree on, as numpy arrays."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    _lib.set_option("step_heads", step_heads)
    try:
        eng = BatchedSelfPlay(_model(dev, params), num_games=G, sims=SIMS, seed=11, **kw)
        assert not (eng.e.gnn_flags & _lib.GNN_EXACT_F32)      # the split kernels: the fused form applies
        if roots is not None:
            d = torch.from_numpy(roots).to(dev)
            _lib.check(eng.lib.aqg_engine_set_roots(ctypes.byref(eng.e), _lib.ptr(d), eng._stream()), "aqg_engine_set_roots")
        for _ in range(MOVES):
            eng.move()
        out = dict(counters=eng.counters())
        for i, h in enumerate(eng.history_tensors()):
            out[f"history{i}"] = h.cpu().numpy()
        for name in ("hist_state72", "hist_visits", "hist_action", "game_plies", "game_result", "game_done", "stat_leaf_evals",
                     "stat_terminal_sims", "node_count") + (("stat_cache_hits",) if kw.get("eval_cache_slots") else ()):
            out[name] = eng.t[name].cpu().numpy()
        visits = torch.empty((G, U.MAX_LEGAL), dtype=torch.int32, device=dev)
        actions = torch.empty((G, U.MAX_LEGAL), dtype=torch.uint8, device=dev)
        count = torch.empty((G,), dtype=torch.int32, device=dev)
        _lib.check(eng.lib.aqg_engine_root_visits(ctypes.byref(eng.e), _lib.ptr(visits), _lib.ptr(actions), _lib.ptr(count), eng._stream()),
                   "aqg_engine_root_visits")
        priors, pcount = eng.root_priors()
        out.update(root_visits=visits.cpu().numpy(), root_actions=actions.cpu().numpy(), root_count=count.cpu().numpy(),
                   root_priors=priors.cpu().numpy(), root_prior_count=pcount.cpu().numpy())
        return out
    finally:
        _lib.set_option("step_heads", 1)


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "counters":
            assert a[k] == b[k], (a[k], b[k])
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k        # bit for bit (priors are floats)


# 21 games: two full step workgroups and one with five games; 1 and 8: a lone wave and exactly one workgroup
@pytest.mark.parametrize("G", [21, 1, 8])
@pytest.mark.parametrize("kw", [dict(), dict(eval_cache_slots=64), dict(root_noise_eps=0.25)], ids=["plain", "cache64", "noise"])
def test_fused_equals_three_launches(dev, params, G, kw):
    """history_tensors(), the raw history, counters() incl. leaf_evals (and cache_hits), the per-game statistics, the root visit
    counts and the root priors of the last search: identical between step_heads 0 and 1."""
    three = _play(dev, params, 0, G, **kw)
    fused = _play(dev, params, 1, G, **kw)
    assert three["counters"]["leaf_evals"] > 0 and three["root_visits"].sum() > 0
    if kw.get("eval_cache_slots"):
        assert three["counters"]["cache_hits"] > 0
    _assert_same(three, fused)


def test_fused_with_the_compact_leaf_list(dev, params):
    """More than 512 games with the evaluation cache on: the trunk takes the leaves that miss the table as a compact list and writes
    pooled rows for the listed boards only, so a fused step workgroup's tile mixes fresh rows (leaf_flag 1), cache hits (leaf_flag 2:
    stale pooled rows, priors from memory) and idle slots.  520 games: 65 step workgroups, and more slots than the trunk's grid of
    512 workgroups."""
    G = 520
    three = _play(dev, params, 0, G, eval_cache_slots=64)
    fused = _play(dev, params, 1, G, eval_cache_slots=64)
    assert three["counters"]["cache_hits"] > 0 and three["counters"]["leaf_evals"] > 0
    _assert_same(three, fused)


@pytest.mark.parametrize("kw", [dict(), dict(eval_cache_slots=64)], ids=["plain", "cache64"])
def test_fused_with_terminal_leaves_and_finished_games(dev, params, kw):
    """Roots one pawn step from the goal beside openings: simulations that end on terminal nodes (no leaf: leaf_flag 0) and slots
    whose game is over share their workgroup's heads tile with live leaves."""
    G = 21
    roots = _near_goal_roots(G)
    three = _play(dev, params, 0, G, roots=roots, **kw)
    fused = _play(dev, params, 1, G, roots=roots, **kw)
    assert three["counters"]["terminal_sims"] > 0
    assert 0 < three["counters"]["finished"] < G, three["counters"]        # some games ended, some go on
    _assert_same(three, fused)


def test_fused_drops_the_global_policy_rows_and_rekeys_the_graph(dev, params):
    """On a capturable stream a move is one captured graph keyed by the options: toggling step_heads on ONE engine must re-capture.
    Seen through the one thing the forms differ in -- the fused form writes no leaf's policy / value to global memory but the root's
    (simulation 0 keeps its heads launch), the three-launch form leaves the last simulation's leaf there."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    s = torch.cuda.Stream(device=dev)
    try:
        with torch.cuda.stream(s):
            model = _model(dev, params)
            eng = BatchedSelfPlay(model, num_games=9, sims=SIMS, seed=5)
            for form, root_rows in ((1, True), (0, False), (1, True)):
                _lib.set_option("step_heads", form)
                policy, value = model.forward_states(eng.root_states72())
                eng.move()
                s.synchronize()
                assert torch.equal(eng.t["policy"], policy) == root_rows, form
                assert torch.equal(eng.t["value"], value[:, 0]) == root_rows, form
            assert eng.counters()["leaf_evals"] > 0
    finally:
        _lib.set_option("step_heads", 1)


def _pooled_overflow_params():
    """A weight set that stays inside fp16 range in the trunk everywhere, and whose POOLED row leaves it (6.8e4) only on a record with
    255 walls in hand (4.5e4 on ordinary ones: it passes the calibration) -- uniform layer-2 / layer-3 weights, a layer-3 bias of
    4.4e4 (tests/test_gpu_parity.py::test_gnn_runtime_saturation_signal builds its sets the same way).  Largest |U| of the linear
    maps on the crafted records: 5.1e3, 4.3e3, 2.8e4 -- the last one 5.9e4 on the trunk's activation image (scale 15/16 sqrt(deg)),
    below its threshold of 65504 -- so only the heads' check of the pooled row can see it (the heads' hidden units stay below 2.4e4)."""
    from oracle import gnn as og
    p = {k: v.copy() for k, v in og.init_params(6).items()}
    p["gcn_layers.0.lin.weight"][:, 1] = 20.0
    p["gcn_layers.1.lin.weight"][:] = 0.006
    p["gcn_layers.2.lin.weight"][:] = 0.049
    p["gcn_layers.2.bias"][:] = 4.4e4
    p["policy_head.0.weight"] *= 0.25
    return p


def test_fused_range_guard_reports_and_host_falls_back(dev):
    """The pooled row's fp16-range check runs inside the step kernel too: the engine's saturation word is set in both forms, and the
    guarded search falls back to the exact kernels with identical results."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from oracle import gnn as og
    g = U.golden("walk_9x9.npz")
    crafted = g["states"][[10, 400, 3000, 9000, 10, 400, 3000, 9000, 10, 400, 3000]].copy()      # 11 roots: a full workgroup and a ragged one
    crafted[:, 1] = 255
    p = _pooled_overflow_params()
    pooled = og.forward_states(p, crafted[:4])["pooled"]
    assert pooled.max() > 65504.0
    # the trunk alone does not report on these records, trunk + heads does: it is the pooled row
    model = _model(dev, p)
    assert model.gnn_flags(dev) == 0
    lib = _lib.load()
    word = torch.zeros((1,), dtype=torch.int32, device=dev)
    d = torch.from_numpy(crafted[:4]).to(dev)
    buf = dict(pooled=torch.empty((4, 128), device=dev), policy=torch.empty((4, 209), device=dev), value=torch.empty((4,), device=dev))
    for heads, want in ((False, 0), (True, 1)):
        word.zero_()
        _lib.check(lib.aqg_gcn_forward_boards_guarded(9, _lib.ptr(d), 0, 4, _lib.ptr(model.packed_weights(dev)), _lib.ptr(buf["pooled"]), None,
                                                      _lib.ptr(buf["policy"]) if heads else None, None, _lib.ptr(buf["value"]) if heads else None,
                                                      0, _lib.ptr(word), _lib.stream_ptr(dev)), "guarded")
        assert int(word.item()) == want, heads
    results = {}
    try:
        for form in (0, 1):
            _lib.set_option("step_heads", form)
            eng = BatchedSelfPlay(_model(dev, p), num_games=crafted.shape[0], sims=SIMS, seed=2)
            assert eng.e.gnn_flags == 0 and eng.counters()["gnn_saturated"] == 0
            eng.search(crafted, check_saturation=False)
            assert eng.counters()["gnn_saturated"] == 1, form                   # the word: set by the form's own heads
            visits, actions, count = eng.search(crafted)                         # guarded: notices, switches, searches again
            assert eng.e.gnn_flags == _lib.GNN_EXACT_F32, form
            for _ in range(2):
                eng.move()                                                       # ... and plays on with the exact kernels
            results[form] = dict(counters=eng.counters(), visits=visits.cpu().numpy(), actions=actions.cpu().numpy(), count=count.cpu().numpy(),
                                 hist_state72=eng.t["hist_state72"].cpu().numpy(), hist_visits=eng.t["hist_visits"].cpu().numpy(),
                                 hist_action=eng.t["hist_action"].cpu().numpy())
    finally:
        _lib.set_option("step_heads", 1)
    assert results[0]["visits"].sum() > 0
    _assert_same(results[0], results[1])
