"""Network-driven searches of the engine held to the oracle over the whole tree, at depth (tests/_tree_parity.py: part E exact, part N
numeric; tests/test_tree_parity_cpu.py proves that the checker refuses planted faults and that the inputs are what is said here).

The networks are initialisation-scale with only the last policy layer scaled, so that the search goes 7 to 29 plies deep instead of
the 2 to 3 of flat priors; the roots come from the reference walks and include an opening, mid-game positions, positions whose trees
hold lost terminals and positions within 6 plies of the draw limit.  Every case reads the finished trees out of the engine's pool:
part E on every listed game -- no tolerance -- and part N on a sample of them against the fp64 oracle of the same network, at the
root tests' bar (priors atol 1e-6 / rtol 1e-5, value 1e-5) or, for a peaked network, at the larger of it and 4 x the worst error of
plain fp32 on the same states.  Each part-N call prints one line (profiles/tree_parity.log is the MI355X run's)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _tree_parity as P   # noqa: E402

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = dict(step_heads=1, legal_beside_trunk=1, step_fast_depth=61)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _pools(eng):
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    return eng.t["node_rec"].cpu().numpy().view(NODE_DTYPE).reshape(eng.G, eng.node_cap).copy(), eng.t["node_count"].cpu().numpy().copy()


def _device_model(name, dev):
    """(the case's network on the GPU, its reference, the engine's evaluator name)."""
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork
    c = P.CASES[name]
    net, ref = P.case_network(name)
    if c["kind"] == "gnn":
        m = GNNNetwork() if c["N"] == 9 else GraphPolicyValueNetwork(6, 128, 3, P.action_count(c["N"]), board_size=c["N"])
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in net.items()})
        return m.to(dev).eval(), ref, "gnn"
    return net.to(dev), ref, c["kind"]           # (the reference reads the same parameters back: it keeps no copy)


def _search(name, dev, recs=None, exact_kernels=False, **kw):
    """One engine, one search of the case's roots at the case's simulations -> (engine, roots, kinds, reference)."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    c = P.CASES[name]
    kinds = None
    if recs is None:
        recs, kinds = P.case_roots(name)
    model, ref, evaluator = _device_model(name, dev)
    eng = BatchedSelfPlay(model, num_games=recs.shape[0], sims=kw.pop("sims", c["sims"]), board_size=c["N"], evaluator=evaluator,
                          record_history=False, **kw)
    if exact_kernels:
        eng._gnn_flags = eng.e.gnn_flags = _lib.GNN_EXACT_F32
    eng.search(recs)
    torch.cuda.synchronize()
    return eng, recs, kinds, ref


def _sample(kinds, G, k):
    """k games for part N: one of every designated kind first, then the others in order."""
    first = [kinds[key][0] for key in ("opening", "mid", "near_goal", "near_draw")] if kinds else []
    rest = [g for g in range(G) if g not in first]
    return (first + rest)[:k]


def _check(eng, recs, ref, label, games, numeric, peaked=True):
    """Part E on `games`, part N on the games `numeric` among them.  -> the part-N figures."""
    pools, counts = _pools(eng)
    nodes, deepest = [], 0
    for g in games:
        try:
            fed = P.check_exact(pools[g], counts[g], recs[g], eng.sims)
        except AssertionError as err:
            raise AssertionError(f"{label}: game {g}: {err}") from err
        deepest = max(deepest, max(x.depth for x in fed.expanded) + 1)
        if g in numeric:
            nodes += fed.expanded
    got = P.check_numeric(nodes, ref, peaked, label)
    got["deepest"] = deepest
    return got


def _split_kernels_served(eng):
    from alphaquoridorgnn_amd import _lib
    return not (eng.e.gnn_flags & _lib.GNN_EXACT_F32) and eng.counters()["gnn_saturated"] == 0


# ------------------------------------------------------------------ 1. gnn 9x9, default options, three step workgroups
def test_gnn_9x9_peaked_x48_default_options(dev):
    """24 roots in one engine (three step workgroups whose games reach different depths), 128 simulations: the split kernels, the
    heads inside the step launch, the legal-move search beside the trunk."""
    eng, recs, kinds, ref = _search("gnn9_x48", dev)
    assert _split_kernels_served(eng)
    assert eng.deferred_legal_searches() > 0
    got = _check(eng, recs, ref, "gnn 9x9 x48 default", range(24), _sample(kinds, 24, 8))
    assert got["deepest"] >= P.CASES["gnn9_x48"]["deepest"]
    assert eng.counters()["terminal_sims"] > 0


# ------------------------------------------------------------------ 2. the same, one option at a time
VARIANTS = {
    "step_heads0": (dict(step_heads=0), dict(), False),
    "legal_beside_trunk0": (dict(legal_beside_trunk=0), dict(), False),
    "step_fast_depth0": (dict(step_fast_depth=0), dict(), False),
    "step_fast_depth2": (dict(step_fast_depth=2), dict(), False),
    "eval_cache": (dict(), dict(eval_cache_slots=256), False),
    "exact_f32": (dict(), dict(), True),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gnn_9x9_peaked_x48_one_option_varied(dev, variant):
    from alphaquoridorgnn_amd import _lib
    options, kw, exact = VARIANTS[variant]
    try:
        for k, v in options.items():
            _lib.set_option(k, v)
        eng, recs, kinds, ref = _search("gnn9_x48", dev, exact_kernels=exact, **kw)
        if exact:
            assert eng.e.gnn_flags == _lib.GNN_EXACT_F32
        else:
            assert _split_kernels_served(eng)
        if variant == "eval_cache":
            assert eng.counters()["cache_hits"] > 0 and int(eng.t["stat_cache_hits"].sum().item()) > 0
        if variant == "legal_beside_trunk0":
            assert eng.deferred_legal_searches() == 0
        _check(eng, recs, ref, f"gnn 9x9 x48 {variant}", range(24), _sample(kinds, 24, 4))
    finally:
        for k, v in OPTION_DEFAULTS.items():
            _lib.set_option(k, v)


# ------------------------------------------------------------------ 3. / 4. sharper and flat priors
def test_gnn_9x9_peaked_x128(dev):
    eng, recs, kinds, ref = _search("gnn9_x128", dev)
    got = _check(eng, recs, ref, "gnn 9x9 x128", range(8), range(8))
    assert got["deepest"] >= P.CASES["gnn9_x128"]["deepest"]


def test_gnn_9x9_initialisation_scale(dev):
    """The flat regime at 128 simulations: the root tests' bar as it stands, at every node."""
    eng, recs, kinds, ref = _search("gnn9_flat", dev)
    assert _split_kernels_served(eng)
    _check(eng, recs, ref, "gnn 9x9 flat", range(8), range(8), peaked=False)


# ------------------------------------------------------------------ 5. the any-size forward (prior_mode 0 below 9x9)
@pytest.mark.parametrize("name", ["gnn3_x32", "gnn7_x48"])
def test_gnn_small_boards(dev, name):
    eng, recs, kinds, ref = _search(name, dev)
    got = _check(eng, recs, ref, name.replace("_", " "), range(8), range(8))
    assert got["deepest"] >= P.CASES[name]["deepest"]
    if name == "gnn3_x32":                                  # most simulations end on terminal nodes inside the tree
        assert eng.counters()["terminal_sims"] >= 4 * 150


# ------------------------------------------------------------------ 6. / 7. the other evaluators
@pytest.mark.parametrize("name", ["general5_x48", "general9_x48", "general3_x32"])
def test_general(dev, name):
    eng, recs, kinds, ref = _search(name, dev)
    got = _check(eng, recs, ref, name.replace("_", " "), range(8), range(8))
    assert got["deepest"] >= P.CASES[name]["deepest"]
    assert eng.counters()["terminal_sims"] > 0


@pytest.mark.parametrize("cache", [0, 256], ids=["cache_off", "cache_on"])
def test_cnn_5x5(dev, cache):
    eng, recs, kinds, ref = _search("cnn5_x48", dev, eval_cache_slots=cache)
    if cache:
        assert eng.counters()["cache_hits"] > 0
    got = _check(eng, recs, ref, f"cnn 5x5 x48 cache {cache}", range(8), range(8))
    assert got["deepest"] >= P.CASES["cnn5_x48"]["deepest"]


# ------------------------------------------------------------------ 8. one large set: the compact list of cache misses
def test_gnn_9x9_large_set_compact_list(dev):
    """640 games in one set with the evaluation cache on (more than 512: the trunk takes the misses as a compact list), 32
    simulations; part E on every 16th game, part N on four of them."""
    recs, kinds = P.pick_roots(9, 640)
    eng, recs, _, ref = _search("gnn9_x48", dev, recs=recs, sims=32, eval_cache_slots=64)
    assert _split_kernels_served(eng) and eng.counters()["cache_hits"] > 0
    games = list(range(0, 640, 16))
    _check(eng, recs, ref, "gnn 9x9 x48 640 games", games, games[:4])


# ------------------------------------------------------------------ 9. after real moves
def test_general_5x5_trees_after_moves_with_refill(dev):
    """quota > num_games, three move() calls with explicit uniforms from the case's roots (two of them end within the three moves
    and their slots are refilled): the pool outlives the transition, so after each move every slot that was active holds the
    finished tree of the position it moved FROM."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    name = "general5_x48"
    c = P.CASES[name]
    recs, kinds = P.case_roots(name)
    model, ref, evaluator = _device_model(name, dev)
    G = recs.shape[0]
    eng = BatchedSelfPlay(model, num_games=G, quota=G + 4, sims=c["sims"], board_size=c["N"], evaluator=evaluator, seed=3)
    d = torch.from_numpy(recs).to(dev)
    _lib.check(eng.lib.aqg_engine_set_roots(ctypes.byref(eng.e), _lib.ptr(d), eng._stream()), "aqg_engine_set_roots")
    rng = np.random.RandomState(9)
    checked = 0
    for move in range(3):
        before = eng.root_states72().cpu().numpy()
        active = eng.t["game_active"].cpu().numpy()
        eng.move(uniforms=torch.from_numpy(rng.random_sample(G)))
        torch.cuda.synchronize()
        pools, counts = _pools(eng)
        for g in np.flatnonzero(active):
            try:
                P.check_exact(pools[g], counts[g], before[g], eng.sims)
            except AssertionError as err:
                raise AssertionError(f"move {move}, slot {g}: {err}") from err
            checked += 1
    counters = eng.counters()
    assert counters["finished"] > 0 and counters["started"] > G, counters       # games ended and slots were refilled
    assert checked >= 3 * G - 4
