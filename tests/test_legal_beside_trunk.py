"""Legal moves beside the trunk (csrc/mcts_eval.hip engine_eval_kernel, option "legal_beside_trunk"): an expanding step launch of the
default self-play chain ends on its new leaf, and the evaluation launch behind it carries the leaves' legal-move searches in front of the
trunk's board workgroups.  The same wave_legal_prepare + wave_legal_finish on the same state, so every comparison with the form in
which the step searches itself (option 0) is exact equality; the search workgroups are also checked alone against the stand-alone
kernel behind aqg_legal_actions."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _util as U

pytestmark = pytest.mark.gpu

SIMS = 16


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def params():
    from oracle import gnn as og
    return og.init_params(3)


def _model(dev, params):
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    model = GNNNetwork()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return model.to(dev).eval()


def _sets(eng):
    return eng.sets if hasattr(eng, "sets") else [eng]


def _run(dev, params, option, make, play):
    """Build an engine with `make(model)`, drive it with `play(eng)` under one value of the option; everything the two forms must agree
    on as numpy arrays, and the number of leaves the search workgroups took."""
    from alphaquoridorgnn_amd import _lib
    _lib.set_option("legal_beside_trunk", option)
    try:
        eng = make(_model(dev, params))
        for e in _sets(eng):
            assert not (e.e.gnn_flags & _lib.GNN_EXACT_F32)          # the split kernels: the deferring form applies
        play(eng)
        out = dict(counters=eng.counters())
        for i, h in enumerate(eng.history_tensors()):
            out[f"history{i}"] = h.cpu().numpy()
        for k, e in enumerate(_sets(eng)):
            for name in ("hist_state72", "hist_visits", "hist_action", "game_plies", "game_result", "game_done", "stat_leaf_evals",
                         "stat_terminal_sims", "node_count", "root_state"):
                out[f"{name}{k}"] = e.t[name].cpu().numpy()
            assert int((e.t["legal_count"] < 0).sum().item()) == 0   # no marker is left behind
        return out, eng.deferred_legal_searches()
    finally:
        _lib.set_option("legal_beside_trunk", 1)


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "counters":
            assert a[k] == b[k], (a[k], b[k])
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _generation(eng):
    eng.play_generation()


def _two_moves(eng):
    eng.move()
    eng.move()


def _single(G, sims=SIMS, **kw):
    def make(model):
        from alphaquoridorgnn_amd.engine import BatchedSelfPlay
        return BatchedSelfPlay(model, num_games=G, sims=sims, seed=7, **kw)
    return make


def _multi(model):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    return MultiSetSelfPlay(model, num_games=12, sims=SIMS, num_sets=4, seed=7)


# Whole generations at 16 simulations -- every game passes through walls in hand, walls spent and a finished slot beside live ones:
# 1 game (a lone wave), 8 (exactly one search workgroup), 9 (the second search workgroup holds one game), 20, four sets on four streams
# (captured graphs), a refilled quota, root noise.  513 games for two moves at 4 simulations: more boards than the trunk's 512 board
# workgroups, so the block offset and the persistent walk are both exercised.
CASES = {
    "g1": (_single(1), _generation),
    "g8": (_single(8), _generation),
    "g9": (_single(9), _generation),
    "g20": (_single(20), _generation),
    "sets4x3": (_multi, _generation),
    "g513_two_moves": (_single(513, sims=4), _two_moves),
    "refill": (_single(8, quota=13), _generation),
    "noise": (_single(9, root_noise_eps=0.25), _generation),
}


@pytest.mark.parametrize("case", list(CASES))
def test_option_on_equals_option_off(dev, params, case):
    """history_tensors(), counters(), the raw history and the per-game statistics: identical with the option off and on; the search
    workgroups took leaves with it on and none with it off."""
    make, play = CASES[case]
    off, n_off = _run(dev, params, 0, make, play)
    on, n_on = _run(dev, params, 1, make, play)
    assert off["counters"]["leaf_evals"] > 0
    if play is _generation:
        assert off["counters"]["finished"] > 0 and off["history0"].shape[0] > 0
    assert n_off == 0 and n_on > 0, (n_off, n_on)
    _assert_same(off, on)


def _rec72_of_leaf(raw24):
    """state72 records of packed 24-byte leaf states (csrc/quoridor_core.hpp pack72)."""
    q = np.ascontiguousarray(raw24).view(np.uint64).reshape(-1, 3)
    out = np.zeros((q.shape[0], 72), dtype=np.uint8)
    bits = np.arange(64, dtype=np.uint64)
    for i, (hw, vw, m) in enumerate(q):
        out[i, 4:68] = ((hw >> bits) & np.uint64(1)).astype(np.uint8) | (((vw >> bits) & np.uint64(1)).astype(np.uint8) << 1)
        m = int(m)
        out[i, 0], out[i, 1], out[i, 2], out[i, 3] = m & 0xFF, (m >> 8) & 0xFF, (m >> 16) & 0xFF, (m >> 24) & 0xFF
        out[i, 68], out[i, 69], out[i, 70] = (m >> 32) & 0xFF, (m >> 40) & 0xFF, 9
    return out


def _role_roots():
    """21 roots (two full search workgroups and one of five games) from the golden files: the fullest wall layouts of jumps_9x9.npz
    (18 walls; the child of the sixth is a finished game: no leaf), states whose first child leaves more than 32 candidates to the
    path searches with walls in both hands, states with no wall in either hand, the opening, and ordinary middle-game states."""
    from oracle import quoridor as oq
    j, w = U.golden("jumps_9x9.npz")["states"], U.golden("walk_9x9.npz")["states"]
    roots = [j[i] for i in (4524, 4525, 4526, 4527, 4528, 4529, 5703, 5704)]
    roots += [w[i] for i in (726, 2924, 3848, 86, 87, 88, 10, 400, 3000, 9000, 12000, 13000)]
    roots.append(oq.init_record(9))
    return np.stack(roots)


def test_search_workgroups_equal_the_standalone_kernel(dev, params):
    """A two-simulation search: simulation 0's step does not expand and searches the root itself, simulation 1's step ends on the
    root's first child and leaves its search to the evaluation launch.  For every game with a leaf, legal_order[:legal_count] and
    legal_count are what aqg_legal_actions gives on the engine's leaf_state; no marker is left; and the search workgroups took exactly
    those leaves.  Not vacuous: among the leaves (counted with the host build of the rule header, tests/witness_cases.py) is one with
    walls in both hands and more than 32 candidates for the path searches -- the one-task-per-lane form -- and one with no wall in
    either hand."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from oracle import quoridor as oq
    from tests import witness_cases as W
    roots = _role_roots()
    G = roots.shape[0]
    assert (oq.status_batch(roots, 116) == 0).all()
    searched = {}
    try:
        for option in (0, 1):
            _lib.set_option("legal_beside_trunk", option)
            eng = BatchedSelfPlay(_model(dev, params), num_games=G, sims=2, seed=3)
            eng.search(roots)
            searched[option] = eng.deferred_legal_searches()
            flag = eng.t["leaf_flag"].cpu().numpy()
            count = eng.t["legal_count"].cpu().numpy()
            order = eng.t["legal_order"].cpu().numpy()
            leaves = _rec72_of_leaf(eng.t["leaf_state"].cpu().numpy())
            live = np.nonzero(flag == 1)[0]
            assert 0 < live.size < G                                   # (one root's first child is a finished game)
            assert (count >= 0).all()
            # the leaves are the roots' first children (all children unvisited: np.argmax takes the first)
            acts, cnt, _ = oq.legal_actions_batch(roots)
            want_leaves = oq.next_batch(roots[live], acts[live, 0].astype(np.int32))
            assert np.array_equal(leaves[live][:, :68], want_leaves[:, :68])
            d = torch.from_numpy(leaves[live]).to(dev)
            ref_order = torch.empty((live.size, U.MAX_LEGAL), dtype=torch.uint8, device=dev)
            ref_count = torch.empty((live.size,), dtype=torch.int32, device=dev)
            _lib.check(eng.lib.aqg_legal_actions(9, _lib.ptr(d), live.size, None, _lib.ptr(ref_order), _lib.ptr(ref_count),
                                                 _lib.stream_ptr(dev)), "aqg_legal_actions")
            ref_order, ref_count = ref_order.cpu().numpy(), ref_count.cpu().numpy()
            assert np.array_equal(count[live], ref_count), option
            for k, g in enumerate(live):
                assert np.array_equal(order[g, :count[g]], ref_order[k, :ref_count[k]]), (option, g)
            if option == 1:
                assert searched[1] == live.size, (searched, live.size)
                pre = np.array([W.survivors(9, r)[0] if r[1] > 0 else 0 for r in leaves[live]])
                both = (leaves[live][:, 1] > 0) & (leaves[live][:, 3] > 0)
                assert ((pre > 32) & both).any(), pre
                assert ((leaves[live][:, 1] == 0) & (leaves[live][:, 3] == 0)).any()
                assert ((pre > 0) & (pre <= 32)).any()                 # ... and the one-fill-per-lane form
    finally:
        _lib.set_option("legal_beside_trunk", 1)
    assert searched[0] == 0


def test_flipping_the_option_rekeys_the_graph(dev, params):
    """On a capturable stream a move is one captured graph keyed by the options: flipping legal_beside_trunk between the moves of ONE
    engine must re-capture -- the search workgroups' counter moves in the moves with the option on and stands still in the others --
    and gives the rows of an engine that never flipped."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    s = torch.cuda.Stream(device=dev)
    rows = {}
    try:
        with torch.cuda.stream(s):
            for name, forms in (("flipped", (1, 0, 1, 0)), ("steady", (1, 1, 1, 1))):
                eng = BatchedSelfPlay(_model(dev, params), num_games=9, sims=SIMS, seed=5)
                for form in forms:
                    _lib.set_option("legal_beside_trunk", form)
                    before = eng.deferred_legal_searches()
                    eng.move()
                    s.synchronize()
                    took = eng.deferred_legal_searches() - before
                    assert (took > 0) == bool(form), (name, form, took)
                rows[name] = {k: eng.t[k].cpu().numpy() for k in ("hist_state72", "hist_visits", "hist_action", "root_state", "node_count")}
                rows[name]["counters"] = eng.counters()
    finally:
        _lib.set_option("legal_beside_trunk", 1)
    assert rows["steady"]["hist_visits"].sum() > 0
    _assert_same(rows["flipped"], rows["steady"])
