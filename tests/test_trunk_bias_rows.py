"""The aggregation's bias rows of the default 9x9 trunk (csrc/gcn_trunk_body.hpp): every workgroup stages the three layers' rows of
PackedLayout::TB in LDS once (TrunkSmemM::BR, regrouped per wave) and each lane reads the row of its node's degree from there, for
every node tile and layer.  PyG initialises GCN biases to zero, which would make all of this invisible, so both weight sets here carry
biases that differ per layer and per feature; the boards are crafted so that every closed degree 1..5 occurs, all five inside one
16-node tile, with node 80 -- the sixth tile's only live node -- at both degrees it can have, and a board without walls.

Bar: pooled against oracle/gnn.py (fp64) at the tolerance tests/test_gpu_parity.py uses for it, and the rows of one board equal bit
for bit across launch shapes and paths -- one board, one workgroup walking three boards (it re-reads its staged image), the default
grid, the tracking and the proven-range build, the compact-list build, and the engine's evaluation launch (engine_eval_kernel: packed
24-byte leaf states behind the leaf_flag mask)."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

POOLED_BAR = dict(atol=2e-6, rtol=1e-4)       # tests/test_gpu_parity.py, pooled rows against the fp64 oracle
SENTINEL = -7.25
LIST_GAMES = 640                              # > 512 games in one set with the cache on: the trunk's compact-list build (csrc/mcts.hip)
S = 8                                         # wall slots per side


def _record(h=(), v=(), ppos=None, pwl=10, epos=None, ewl=10):
    """A 72-byte record: horizontal walls at the slots `h`, vertical ones at `v` ((x, y) pairs), pawn tiles, walls in hand."""
    from oracle import quoridor as oq
    rec = oq.init_record(9).copy()
    for x, y in h:
        rec[4 + x * S + y] = 1
    for x, y in v:
        rec[4 + x * S + y] = 2
    if ppos is not None:
        rec[0] = ppos
    if epos is not None:
        rec[2] = epos
    rec[1], rec[3] = pwl, ewl
    return rec


def _pinwheel(x, y):
    """Four walls around tile (x, y), 1 <= x, y <= 7, that close all four of its edges: closed degree 1."""
    return dict(h=[(x, y), (x - 1, y - 1)], v=[(x - 1, y), (x, y - 1)])


def _boards():
    """17 crafted records (not all of them reachable positions: only the network sees the first batch; the engine's roots are chosen
    among them by their status).  0: a pinwheel around tile (1, 3) -- node 12 has degree 1, node 3 degree 2, and tile 0 (nodes 0..15)
    holds all five degrees; 1: no walls; 2, 3: node 80 at degree 2 through a horizontal / a vertical wall at slot (7, 7), the latter
    beside a pinwheel in the fifth tile; 4..16: 1..20 random walls, pawns anywhere below row 1, 0..10 walls in hand."""
    rng = np.random.RandomState(5)
    pin = _pinwheel(7, 4)
    recs = [_record(**_pinwheel(1, 3)), _record(), _record(h=[(7, 7)], pwl=3, ewl=0),
            _record(h=pin["h"], v=pin["v"] + [(7, 7)], pwl=0, ewl=7)]
    for _ in range(13):
        slots = rng.permutation(S * S)[:rng.randint(1, 21)]
        kinds = rng.randint(1, 3, size=slots.size)
        ppos = int(rng.randint(18, 81))
        epos = int(rng.randint(18, 81))
        if ppos == 80 - epos:
            epos = 18 + (epos - 17) % 63
        rec = _record(ppos=ppos, epos=epos, pwl=int(rng.randint(0, 11)), ewl=int(rng.randint(0, 11)))
        rec[4 + slots] = kinds
        recs.append(rec)
    return np.stack(recs)


def _degrees(rec):
    """Closed degree (the node itself + open edges) of the 81 nodes, from the oracle's edge list."""
    from oracle import gnn as og
    return 1 + np.bincount(og.board_edges(rec)[1], minlength=81)


def _mixes_all_degrees(recs):
    """(every degree 1..5 occurs, some 16-node tile of some board holds all five, node 80 occurs at degrees 2 and 3)"""
    degs = np.stack([_degrees(r) for r in recs])
    tiles = any(set(d[16 * t:16 * t + 16]) == {1, 2, 3, 4, 5} for d in degs for t in range(5))
    return set(degs.ravel()) == {1, 2, 3, 4, 5}, tiles, {2, 3} <= set(degs[:, 80])


def _weights(which):
    """'proven': initialisation-scale weights with biases linspace(-0.3, 0.5) x (layer + 1) -- inside the static fp16 bound, served by
    the build without range tracking (TRACK 0).  'tracking': the same, but hidden unit 5 of layer 2 has bias -100 (its ReLU output
    is 0 on every board) and its column of layer 3's weights is 300: the static bound over ALL inputs fails (300 x 100 x 2.3 > 65504), so
    the tracking build (TRACK 2) serves the set, while every value that occurs stays at initialisation scale and the bar is unchanged."""
    from oracle import gnn as og
    params = dict(og.init_params(41))
    for l in range(3):
        params[f"gcn_layers.{l}.bias"] = (np.linspace(-0.3, 0.5, 128) * (1 + l)).astype(np.float32)
    if which == "tracking":
        params["gcn_layers.1.bias"] = params["gcn_layers.1.bias"].copy()
        params["gcn_layers.1.bias"][5] = -100.0
        params["gcn_layers.2.lin.weight"] = params["gcn_layers.2.lin.weight"].copy()
        params["gcn_layers.2.lin.weight"][:, 5] = 300.0
    return params


class _Set:
    """One weight set: the module, its flags, the fp64 pooled rows of the 17 boards (computed once) and the default-grid launch's rows."""
    def __init__(self, which, dev):
        from alphaquoridorgnn_amd import _lib
        from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
        from oracle import gnn as og
        self.params = _weights(which)
        m = GNNNetwork()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in self.params.items()})
        self.model = m.to(dev).eval()
        self.flags = self.model.gnn_flags(dev)
        assert self.flags == (_lib.GNN_RANGE_PROVEN if which == "proven" else 0), (which, self.flags)
        self.recs = _boards()
        self.oracle = og.forward_states_dense(self.params, self.recs)["pooled"]
        self.rows = trunk(self, self.recs, dev)                 # B = 17, default grid: the rows every other shape must reproduce


def trunk(ws, recs, dev, fmt=0, flags=None, grid=0):
    """pooled [B, 128] of the trunk alone (LDS poisoned first, the output pre-filled with NaN); the range guard's word must stay 0."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    d = recs if torch.is_tensor(recs) else torch.from_numpy(np.ascontiguousarray(recs)).to(dev)
    B = d.shape[0]
    pooled = torch.full((B, 128), float("nan"), device=dev)
    word = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.set_option("trunk_grid", grid)
    try:
        _lib.poison_lds(dev)
        _lib.check(lib.aqg_gcn_forward_boards_guarded(9, _lib.ptr(d), fmt, B, _lib.ptr(ws.model.packed_weights(dev)), _lib.ptr(pooled), None, None,
                                                      None, None, ws.flags if flags is None else flags, _lib.ptr(word), _lib.stream_ptr(dev)),
                   "aqg_gcn_forward_boards_guarded")
        torch.cuda.synchronize()
    finally:
        _lib.set_option("trunk_grid", 0)
    assert int(word.item()) == 0
    return pooled


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


_SETS = {}


@pytest.fixture(params=["proven", "tracking"])
def ws(request, dev):
    if request.param not in _SETS:
        _SETS[request.param] = _Set(request.param, dev)
    return _SETS[request.param]


def test_boards_hold_every_degree():
    """The CPU oracle's word on the crafted records: all five degrees, all five inside one node tile, node 80 at both of its degrees,
    and a board with no walls (every node at its grid degree: corners 3, edges 4, inside 5)."""
    recs = _boards()
    assert recs.shape == (17, 72)
    assert _mixes_all_degrees(recs) == (True, True, True)
    assert set(_degrees(recs[0])[:16]) == {1, 2, 3, 4, 5} and _degrees(recs[0])[12] == 1
    assert not recs[1, 4:68].any() and sorted(np.bincount(_degrees(recs[1]))[3:]) == [4, 28, 49]


def test_default_grid_vs_oracle(ws, dev):
    """B = 17, one board per workgroup: every row against the fp64 oracle."""
    np.testing.assert_allclose(ws.rows.cpu().numpy(), ws.oracle, **POOLED_BAR)


def test_one_board(ws, dev):
    """B = 1: a launch of a single workgroup."""
    for i in (0, 2):
        got = trunk(ws, ws.recs[i:i + 1], dev)
        assert torch.equal(got, ws.rows[i:i + 1]), i
        np.testing.assert_allclose(got.cpu().numpy(), ws.oracle[i:i + 1], **POOLED_BAR)


def test_one_workgroup_walks_three_boards(ws, dev):
    """B = 3 with trunk_grid capped at 1: the second and third board read the image the workgroup staged in front of the first."""
    got = trunk(ws, ws.recs[:3], dev, grid=1)
    assert torch.equal(got, ws.rows[:3])
    np.testing.assert_allclose(got.cpu().numpy(), ws.oracle[:3], **POOLED_BAR)
    got = trunk(ws, ws.recs, dev, grid=2)                       # 17 boards over two workgroups: nine and eight boards each
    assert torch.equal(got, ws.rows)


def test_both_guard_builds_agree(ws, dev):
    """The build without range tracking and the tracking build on the same weights and boards: the same bits (the tracking build serves
    any set; the proven-range build is only asked where the bound holds)."""
    from alphaquoridorgnn_amd import _lib
    assert torch.equal(trunk(ws, ws.recs, dev, flags=0), ws.rows)
    if ws.flags == _lib.GNN_RANGE_PROVEN:
        assert torch.equal(trunk(ws, ws.recs, dev, flags=_lib.GNN_RANGE_PROVEN), ws.rows)


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


def _engine_roots(recs):
    """16 roots for the engine: the first 16 boards, games 1, 6 and 11 made terminal (enemy pawn on row 0 of its own frame)."""
    roots = recs[:16].copy()
    dead = np.zeros(16, dtype=bool)
    dead[[1, 6, 11]] = True
    roots[dead, 2] = roots[dead, 2] % 9
    return roots, dead


def test_engine_roots_are_positions():
    """The engine's roots, on the CPU: the live ones are games in progress, and their first children -- the leaves the evaluation launch
    will see, in the other player's frame -- still hold every degree."""
    from oracle import quoridor as oq
    roots, dead = _engine_roots(_boards())
    status = oq.status_batch(roots, 116)
    assert (status[~dead] == 0).all() and (status[dead] != 0).all()
    acts, cnt, _ = oq.legal_actions_batch(roots[~dead])
    assert (cnt > 0).all()
    leaves = oq.next_batch(roots[~dead], acts[:, 0].astype(np.int32))
    assert _mixes_all_degrees(leaves)[0]


def test_engine_masked_evaluation_launch(ws, dev):
    """16 games, three of them terminal at the root, two simulations: simulation 0 evaluates the roots through the plain trunk behind the
    leaf_flag mask (fmt 1), simulation 1's leaves -- the roots' first children -- go through engine_eval_kernel.  Rows of terminal
    games keep their sentinel; every other row is the row of its leaf (or of its root where the first child ended the game): the fp64
    oracle's within the bar, and the plain launch's on the same packed states bit for bit."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from oracle import gnn as og
    roots, dead = _engine_roots(ws.recs)
    eng = BatchedSelfPlay(ws.model, num_games=16, sims=2, seed=3, record_history=False)
    eng.t["pooled"].fill_(SENTINEL)
    _lib.poison_lds(dev)
    eng.search(roots)
    torch.cuda.synchronize()
    assert eng.e.gnn_flags == ws.flags                              # no range-guard replay
    pooled = eng.t["pooled"]
    flag = eng.t["leaf_flag"].cpu().numpy()
    live = np.nonzero(flag == 1)[0]
    assert live.size >= 8 and not dead[live].any()
    assert eng.deferred_legal_searches() == live.size              # the evaluation launch ran, for exactly these leaves
    assert bool((pooled[torch.from_numpy(dead).to(dev)] == SENTINEL).all())
    leaves = _rec72_of_leaf(eng.t["leaf_state"].cpu().numpy())[live]
    assert _mixes_all_degrees(leaves)[0]
    got = pooled[torch.from_numpy(live).to(dev)]
    np.testing.assert_allclose(got.cpu().numpy(), og.forward_states_dense(ws.params, leaves)["pooled"], **POOLED_BAR)
    assert torch.equal(got, trunk(ws, eng.t["leaf_state"][torch.from_numpy(live).to(dev)].contiguous(), dev, fmt=1))
    assert torch.equal(got, trunk(ws, leaves, dev))
    # the roots' own rows through the masked plain launch (a one-simulation search): the rows of the same boards as above
    eng = BatchedSelfPlay(ws.model, num_games=16, sims=1, seed=3, record_history=False)
    eng.t["pooled"].fill_(SENTINEL)
    _lib.poison_lds(dev)
    eng.search(roots)
    torch.cuda.synchronize()
    keep = torch.from_numpy(~dead).to(dev)
    assert bool((eng.t["pooled"][~keep] == SENTINEL).all())
    assert torch.equal(eng.t["pooled"][keep], ws.rows[:16][keep])


def test_compact_list_of_three(ws, dev):
    """640 games with the evaluation cache on, all but three terminal at the root, one simulation: the three misses reach the trunk's
    list build as a compact list of three entries.  Their rows are the rows of the same boards above; every other row keeps its sentinel."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    where = {5: 0, 300: 2, 639: 3}                                  # game -> board
    roots = np.repeat(ws.recs[1:2], LIST_GAMES, axis=0)
    roots[:, 2] = roots[:, 2] % 9                                   # terminal
    for g, i in where.items():
        roots[g] = ws.recs[i]
    eng = BatchedSelfPlay(ws.model, num_games=LIST_GAMES, sims=1, seed=3, record_history=False, eval_cache_slots=64)
    eng.t["pooled"].fill_(SENTINEL)
    _lib.poison_lds(dev)
    eng.search(roots)
    torch.cuda.synchronize()
    assert eng.e.gnn_flags == ws.flags
    assert int(eng.t["eval_count"][0].item()) == 3 and sorted(eng.t["eval_list"][:3].cpu().tolist()) == sorted(where)
    games = torch.tensor(sorted(where), device=dev)
    rest = torch.ones(LIST_GAMES, dtype=torch.bool, device=dev)
    rest[games] = False
    assert bool((eng.t["pooled"][rest] == SENTINEL).all())
    want = ws.rows[torch.tensor([where[g] for g in sorted(where)], device=dev)]
    assert torch.equal(eng.t["pooled"][games], want)
    np.testing.assert_allclose(eng.t["pooled"][games].cpu().numpy(), ws.oracle[[where[g] for g in sorted(where)]], **POOLED_BAR)
