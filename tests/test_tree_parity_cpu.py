"""CPU tests (no GPU) of the whole-tree checker tests/_tree_parity.py and of the inputs tests/test_tree_parity.py gives it.

The checker must fail on a wrong kernel: oracle.mcts' own search is written into the engine's pool layout (a child block per
expansion, in expansion order) and passes both parts on 3x3, 5x5 and 9x9; then one fault at a time is planted below depth 3 -- a visit
moved between siblings, two siblings' priors swapped, a search that ran with a wrong-signed value at one state, a search whose backup
drops the sign flip, a child block in another order -- and the part named for it must refuse the tree.

The inputs must be what the GPU file says they are, with the fp64 oracle alone: the peaked networks' mean root entropy is at most
1.5 nats, the oracle's search reaches the depth stated in _tree_parity.CASES, the designated roots' trees really hold lost terminals
and draws, and every root is a live position with a legal move."""
import numpy as np
import pytest

from oracle import mcts as om, quoridor as oq
from tests import _tree_parity as P
from tests import _tree_reuse as T


def _model(name):
    return P.RefModel(P.case_network(name)[1])


def _searched(name, root_index, sims=None):
    """(pool, count, root record, simulations, reference) of the oracle's search from one of the case's roots."""
    c = P.CASES[name]
    rec = P.case_roots(name)[0][root_index]
    sims = sims or c["sims"]
    pool, count = P.oracle_pool(_model(name), rec, sims)
    return pool, count, rec, sims, P.case_network(name)[1]


# ------------------------------------------------------------------ the checker passes on the reference search
@pytest.mark.parametrize("name,roots", [("gnn3_x32", (0, 2, 7)), ("general5_x48", (0, 1, 7)), ("gnn9_x48", (1, 7, 11))])
def test_oracle_tree_in_pool_layout_passes_both_parts(name, roots):
    """3x3, 5x5 and 9x9; an opening or mid-game root, one whose tree holds lost terminals, one near the end of the game."""
    nodes = []
    for r in roots:
        pool, count, rec, sims, ref = _searched(name, r)
        fed = P.check_exact(pool, count, rec, sims)
        assert fed.expanded[0].idx == 0
        nodes += fed.expanded
    assert len(nodes) >= 50 and max(x.depth for x in nodes) >= 5
    # the tree was searched with the fp64 network rounded to f32 -- the value once, the priors at the gather, in their sum and at
    # the division -- so the stored evaluations sit within a few f32 roundings of it
    got = P.check_numeric(nodes, ref, peaked=False, label=f"cpu {name}")
    assert got["priors_error"] <= 8 * 2.0 ** -24 and got["value_error"] <= 2.0 ** -24


def test_pool_order_is_not_relied_on():
    """The same tree with its child blocks laid out in REVERSE expansion order passes: the checker follows `kids` only."""
    pool, count, rec, sims, _ = _searched("general5_x48", 1)
    blocks = T.block_starts(pool, count)
    out = pool.copy()
    new_first, at = {}, 1
    for first, cnt in reversed(blocks):
        new_first[first] = at
        out[at:at + cnt] = pool[first:first + cnt]
        at += cnt
    assert at == count
    for i in range(count):
        first, cnt = P.kids_of(out[i])
        if cnt:
            out[i]["kids"] = new_first[first] | (cnt << 24)
    assert out.tobytes() != pool.tobytes()
    P.check_exact(out, count, rec, sims)


# ------------------------------------------------------------------ planted faults
FAULT_CASE, FAULT_ROOT = "gnn9_x48", 1          # a mid-game 9x9 root whose search goes 10 deep


@pytest.fixture(scope="module")
def clean():
    pool, count, rec, sims, ref = _searched(FAULT_CASE, FAULT_ROOT)
    fed = P.check_exact(pool, count, rec, sims)
    assert max(x.depth for x in fed.expanded) >= 5
    return pool, count, rec, sims, ref, fed


def _deep_node(fed, pool, want):
    """The most visited expanded node at depth >= 3 for which want(node, its child block) holds."""
    best = None
    for x in fed.expanded:
        first, cnt = P.kids_of(pool[x.idx])
        if x.depth >= 3 and want(x, pool[first:first + cnt]) and (best is None or pool[x.idx]["n"] > pool[best.idx]["n"]):
            best = x
    assert best is not None
    return best, P.kids_of(pool[best.idx])[0]


def test_fault_visit_moved_between_siblings(clean):
    pool, count, rec, sims, ref, fed = clean
    x, first = _deep_node(fed, pool, lambda x, kids: (kids["n"] > 0).sum() >= 1 and len(kids) >= 2)
    kids = pool[first:first + len(x.legal)]
    a = int(np.argmax(kids["n"]))
    b = (a + 1) % len(kids)
    bad = pool.copy()
    bad[first + a]["n"] -= 1
    bad[first + b]["n"] += 1
    with pytest.raises(AssertionError, match="the reference search"):
        P.check_exact(bad, count, rec, sims)


def test_fault_siblings_priors_swapped(clean):
    pool, count, rec, sims, ref, fed = clean
    x, first = _deep_node(fed, pool, lambda x, kids: (kids["n"] > 0).sum() >= 1 and len(kids) >= 2)
    kids = pool[first:first + len(x.legal)]
    a, b = int(np.argmax(kids["n"])), int(np.argmin(kids["p"]))
    assert a != b and kids[a]["p"] != kids[b]["p"]
    bad = pool.copy()
    for f in ("p", "cp"):
        bad[first + a][f], bad[first + b][f] = pool[first + b][f], pool[first + a][f]
    with pytest.raises(AssertionError, match="the reference search|never expanded"):       # part E: the search goes elsewhere
        P.check_exact(bad, count, rec, sims)
    nodes = [P.Expanded(y.idx, y.depth, y.rec, y.legal, bad[first:first + len(y.legal)]["p"].copy() if y is x else y.priors, y.value, y.path)
             for y in fed.expanded]
    with pytest.raises(AssertionError, match=f"priors of node {x.idx} at depth {x.depth}"):     # part N: not the network's priors
        P.check_numeric(nodes, ref, peaked=True, label="fault")


class _WrongSign:
    """The model with the sign of its value flipped at ONE position."""

    def __init__(self, model, rec):
        self.model, self.key = model, bytes(rec[:70])

    def predict(self, state, device=None):
        p, v = self.model.predict(state, device)
        return p, (-v if bytes(state.rec[:70]) == self.key else v)


def test_fault_wrong_signed_value_at_one_deep_state(clean):
    pool, count, rec, sims, ref, fed = clean
    x, _ = _deep_node(fed, pool, lambda x, kids: abs(float(x.value)) > 1e-3 and pool[x.idx]["n"] >= 3)
    bad, bad_count = P.oracle_pool(_WrongSign(_model(FAULT_CASE), x.rec), rec, sims)
    got = P.check_exact(bad, bad_count, rec, sims)           # part E cannot see it: the tree is a consistent search
    with pytest.raises(AssertionError, match="value of node"):
        P.check_numeric(got.expanded, ref, peaked=True, label="fault")


def _search_without_flip_below_3(model, root, sims, clock=None, first_priors=None):
    """tests/_tree_reuse.py search_from with a backup that stops alternating the sign below depth 3."""
    clock = clock or T.Clock()
    for _ in range(sims):
        path, node = [root], root
        while True:
            if node.state.is_done():
                value = -1 if node.state.is_lose() else 0
                break
            if not node.children:
                prior, value = model.predict(node.state)
                legal = node.state.legal_actions()
                node.children = [T.Node(node.state.next(a), p, int(a)) for a, p in zip(legal, prior)]
                node.seq = clock.tick()
                break
            node = om._select(node)
            path.append(node)
        v = value
        for depth in range(len(path) - 1, -1, -1):
            path[depth].w += v
            path[depth].n += 1
            if depth <= 3:
                v = -v
    return root


def test_fault_backup_drops_the_sign_flip_below_depth_3(clean):
    pool, count, rec, sims, ref, fed = clean
    bad, bad_count = P.oracle_pool(_model(FAULT_CASE), rec, sims, search=_search_without_flip_below_3)
    with pytest.raises(AssertionError, match="is no f32 number|the reference search|never expanded"):
        got = P.check_exact(bad, bad_count, rec, sims)
        P.check_numeric(got.expanded, ref, peaked=True, label="fault")      # (if every sum happened to be an f32 number)


def test_fault_child_block_permuted(clean):
    pool, count, rec, sims, ref, fed = clean
    x, first = _deep_node(fed, pool, lambda x, kids: len(kids) >= 2)
    bad = pool.copy()
    bad[first], bad[first + 1] = pool[first + 1], pool[first]          # whole records: statistics, priors and actions travel together
    with pytest.raises(AssertionError, match="not legal_actions\\(\\) in order"):
        P.check_exact(bad, count, rec, sims)


def test_fault_shared_child_block_and_block_out_of_bounds(clean):
    pool, count, rec, sims, ref, fed = clean
    x, first = _deep_node(fed, pool, lambda x, kids: True)
    bad = pool.copy()
    bad[x.idx]["kids"] = (count - 1) | (len(x.legal) << 24)
    with pytest.raises(AssertionError, match="outside the used pool"):
        P.check_exact(bad, count, rec, sims)


# ------------------------------------------------------------------ the forward the bars are measured with
@pytest.mark.parametrize("N", [3, 9])
def test_dense_forward_fp64_is_the_oracle_forward(N):
    params = P.peaked_gnn_params(11, N, 48.0)
    recs = P.pick_roots(N, 12)[0]
    pol, val = P.dense_forward(params, recs, np.float64)
    ref = P.GnnRef(params).fp64(recs)
    np.testing.assert_allclose(pol, ref[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(val, ref[1], rtol=0, atol=1e-12)
    pol32, val32 = P.dense_forward(params, recs, np.float32)
    assert 0 < np.abs(pol32 - pol).max() < 1e-3 and np.abs(val32 - val).max() < 1e-5


# ------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("name", list(P.CASES))
def test_roots_are_live_and_of_the_designated_kinds(name):
    c = P.CASES[name]
    recs, kinds = P.case_roots(name)
    N, draw = c["N"], oq.BOARDS[c["N"]][1]
    assert recs.shape == (c["roots"], 72) and len({bytes(r) for r in recs}) == c["roots"]
    assert (oq.status_batch(recs, draw) == 0).all() and (oq.legal_actions_batch(recs)[1] > 0).all()
    for r in recs:
        s = oq.State(r)
        assert not s.is_done() and s.legal_actions()
    assert all(len(kinds[k]) >= 1 for k in ("opening", "mid", "near_goal", "near_draw"))
    ply = P.plies(recs)
    assert ply[kinds["opening"][0]] == 0
    assert all(draw // 4 <= ply[i] <= draw // 2 for i in kinds["mid"])
    assert all(draw - 6 <= ply[i] < draw for i in kinds["near_draw"])


@pytest.mark.parametrize("name", [n for n, c in P.CASES.items() if c["factor"] > 1])
def test_peaked_networks_mean_root_entropy(name):
    _, ref = P.case_network(name)
    recs, _ = P.case_roots(name)
    pol, _ = ref.fp64(recs)
    h = [P.entropy(P._priors_at(pol[b], oq.State(r).legal_actions(), np.float64)) for b, r in enumerate(recs)]
    assert np.mean(h) <= 1.5, h


def test_flat_network_is_flat():
    _, ref = P.case_network("gnn9_flat")
    recs, kinds = P.case_roots("gnn9_flat")
    pol, _ = ref.fp64(recs[kinds["opening"] + kinds["mid"]])
    assert all(P.entropy(p) > 4.0 for p in pol)


def _facts(name, indices, sims):
    out = []
    model = _model(name)
    recs = P.case_roots(name)[0]
    for i in indices:
        pool, count = P.oracle_pool(model, recs[i], sims)
        out.append(P.tree_facts(P.check_exact(pool, count, recs[i], sims)))
    return out


@pytest.mark.parametrize("name", [n for n, c in P.CASES.items() if c["deepest"]])
def test_oracle_search_reaches_the_stated_depth(name):
    """Over the opening and mid-game roots (the others' trees end on terminals early).  9x9 x48 / x128: at 128 simulations."""
    c = P.CASES[name]
    kinds = P.case_roots(name)[1]
    sims = 128 if name in ("gnn9_x48", "gnn9_x128") else c["sims"]
    deepest = [f["deepest"] for f in _facts(name, kinds["opening"] + kinds["mid"][:2], sims)]
    assert max(deepest) >= c["deepest"], deepest


@pytest.mark.parametrize("name", [n for n, c in P.CASES.items() if c["factor"] > 1])
def test_designated_roots_hold_lost_terminals_and_draws(name):
    c = P.CASES[name]
    kinds = P.case_roots(name)[1]
    lost = _facts(name, kinds["near_goal"][:2], c["sims"])
    assert all(f["lost"] > 0 for f in lost), lost
    drawn = _facts(name, kinds["near_draw"][:2], c["sims"])
    assert all(f["drawn"] > 0 for f in drawn), drawn


def test_3x3_simulations_mostly_end_on_terminals():
    f = _facts("gnn3_x32", range(8), 200)
    assert sum(1 for x in f if x["lost"] + x["drawn"] >= 150) >= 4, f
