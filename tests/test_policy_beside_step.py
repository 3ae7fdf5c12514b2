"""The policy head beside the step (csrc/mcts_step.hip engine_step_fast_kernel<.., PB>, option "policy_beside_step"): a step launch behind an
evaluation launch computes only the value head in its step workgroups and leaves the policy layer, the softmax, the gather at the legal
actions and the new child records to policy workgroups of the same launch, fed by the job records the evaluation launch's searches
left.  The same MFMA sequence per output and the same order of every sum, so every comparison with the one-workgroup form (option 0) is
exact equality: history, counters, and every byte of the games' node pools."""
import numpy as np
import pytest
import torch

from tests import _util as U

pytestmark = pytest.mark.gpu

NODE_DTYPE = np.dtype([("w", "<f8"), ("p", "<f4"), ("action", "<u4"), ("n", "<i4"), ("kids", "<u4"), ("q", "<f4"), ("cp", "<f4")])


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


def _snapshot(eng, extra=None):
    """Everything the two forms must agree on, as numpy arrays: the history, the counters, the statistics and the whole node pools."""
    out = dict(counters=eng.counters())
    for i, h in enumerate(eng.history_tensors()):
        out[f"history{i}"] = h.cpu().numpy()
    for name in ("hist_state72", "hist_visits", "hist_action", "game_plies", "game_result", "game_done", "stat_leaf_evals",
                 "stat_terminal_sims", "node_count", "root_state", "node_rec", "path", "path_len", "leaf_flag", "leaf_state",
                 "legal_count"):
        out[name] = eng.t[name].cpu().numpy()
    out.update(extra or {})
    assert int((eng.t["legal_count"] < 0).sum().item()) == 0         # no marker is left behind
    assert int(eng.t["gnn_workspace"].view(torch.int32).ne(0).sum().item()) == 0      # ... and no job
    return out


def _run(dev, params, option, play, graph, node_cap=None, **kw):
    """One engine under one value of the option.  graph: on a side stream a move of >= 4 simulations is one captured graph; on the
    default stream it is plain launches."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    _lib.set_option("policy_beside_step", option)
    try:
        s = torch.cuda.Stream(device=dev) if graph else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            eng = BatchedSelfPlay(_model(dev, params), seed=7, **kw)
            assert not (eng.e.gnn_flags & _lib.GNN_EXACT_F32)             # the split kernels: the form applies
            if node_cap is not None:
                eng.e.node_cap = eng.node_cap = node_cap                     # (a smaller stride inside the same pool)
            extra = play(eng)
            s.synchronize()
            return _snapshot(eng, extra), eng.policy_beside_expansions(), eng
    finally:
        _lib.set_option("policy_beside_step", 1)


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "counters":
            assert a[k] == b[k], (a[k], b[k])
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _both(dev, params, play, graph=True, **kw):
    off, n_off, _ = _run(dev, params, 0, play, graph, **kw)
    on, n_on, eng = _run(dev, params, 1, play, graph, **kw)
    assert off["counters"]["leaf_evals"] > 0
    assert n_off == 0 and n_on > 0, (n_off, n_on)            # the policy workgroups took leaves with the option on, none with it off
    _assert_same(off, on)
    return on, eng


def _generation(eng):
    eng.play_generation()


def _moves(n):
    def play(eng):
        for _ in range(n):
            eng.move()
    return play


def test_ragged_last_workgroup(dev, params):
    """13 games x 12 simulations: num_games is no multiple of 8, the last step workgroup and the last policy workgroup are half empty."""
    _both(dev, params, _moves(3), num_games=13, sims=12)


def test_pool_too_small_for_the_expansion(dev, params):
    """8 games x 6 simulations with room for the root's children and 60 more records: from the second expansion on first_new + cnt exceeds
    node_cap, neither kind of workgroup writes a child, and `kids` and node_count agree between the forms."""
    cap = 1 + U.MAX_LEGAL + 60
    on, eng = _both(dev, params, _moves(1), num_games=8, sims=6, node_cap=cap)
    pools = on["node_rec"].view(np.uint8).reshape(-1)[:8 * cap * 32].view(NODE_DTYPE).reshape(8, cap)
    assert (on["node_count"] <= cap).all()
    expanded = np.array([int(((pools[g, :on["node_count"][g]]["kids"] >> 24) > 0).sum()) for g in range(8)])
    assert (expanded < on["stat_leaf_evals"]).any(), (expanded, on["stat_leaf_evals"])      # evaluated leaves that could not be expanded


def test_plain_launches(dev, params):
    """16 games x 3 simulations on the default stream: no graph, one policy step launch (simulation 2) and the last expansion."""
    _both(dev, params, _moves(2), graph=False, num_games=16, sims=3)


def test_generation_played_to_the_end(dev, params):
    """24 games x 16 simulations, played out: finished slots beside live ones, terminal leaves -- the first child of a leaf expanded a
    launch ago among them, whose record both kinds of workgroup write -- and leaves whose player has no wall in hand."""
    on, _ = _both(dev, params, _generation, num_games=24, sims=16)
    assert on["counters"]["finished"] > 0 and on["counters"]["terminal_sims"] > 0 and on["history0"].shape[0] > 0
    assert (on["hist_state72"].reshape(-1, 72)[:, 1] == 0).any()             # a recorded position whose mover has no wall left


def test_generation_with_root_noise(dev, params):
    on, _ = _both(dev, params, _generation, num_games=24, sims=16, root_noise_eps=0.25)
    assert on["counters"]["finished"] > 0


def test_generation_with_tree_reuse(dev, params):
    on, _ = _both(dev, params, _generation, num_games=24, sims=16, tree_reuse=True)
    assert on["counters"]["finished"] > 0


def _pooled_overflow_params():
    """tests/test_step_heads_fused.py's weight set: inside fp16 range in the trunk everywhere, with a POOLED row that leaves it (6.8e4)
    only on a record whose mover has 255 walls in hand (4.5e4 on every other one)."""
    from oracle import gnn as og
    p = {k: v.copy() for k, v in og.init_params(6).items()}
    p["gcn_layers.0.lin.weight"][:, 1] = 20.0
    p["gcn_layers.1.lin.weight"][:] = 0.006
    p["gcn_layers.2.lin.weight"][:] = 0.049
    p["gcn_layers.2.bias"][:] = 4.4e4
    p["policy_head.0.weight"] *= 0.25
    return p


def test_range_guard_word_of_a_tracked_weight_set(dev):
    """A weight set that is not range-proven (the evaluation launch's tracking build).  The roots give the OTHER player 255 walls: their
    own pooled rows stay in range, their children's -- the mover's walls there -- leave it, their grandchildren's are in range again
    (checked against the oracle below).  So the word is raised by the heads of a simulation's leaf and by nothing else: by the step
    workgroup with the option off, by the policy workgroup with it on.  Word, visits and pools are equal."""
    from alphaquoridorgnn_amd import _lib
    from oracle import gnn as og
    from oracle import quoridor as oq
    g = U.golden("walk_9x9.npz")
    roots = g["states"][[10, 400, 3000, 9000, 10, 400, 3000, 9000, 10, 400, 3000]].copy()          # 11 roots: a full workgroup and a ragged one
    roots[:, 3] = 255
    p = _pooled_overflow_params()
    acts, _, _ = oq.legal_actions_batch(roots[:4])
    kids = oq.next_batch(roots[:4], acts[:, 0].astype(np.int32))
    assert og.forward_states(p, roots[:4])["pooled"].max() < 65504.0 < og.forward_states(p, kids)["pooled"].max(axis=1).min()

    def play(eng):
        assert eng.e.gnn_flags == 0 and eng.counters()["gnn_saturated"] == 0
        visits, actions, count = eng.search(roots, check_saturation=False)
        return dict(visits=visits.cpu().numpy(), actions=actions.cpu().numpy(), count=count.cpu().numpy())

    results = {}
    for option in (0, 1):
        results[option], n, _ = _run(dev, p, option, play, True, num_games=roots.shape[0], sims=8)
        assert (n > 0) == bool(option)
        assert results[option]["counters"]["gnn_saturated"] == 1, option
    assert results[0]["visits"].sum() > 0
    _assert_same(results[0], results[1])
