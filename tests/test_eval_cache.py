"""The evaluation cache (include/aqgnn.h `eval_cache_keys`, csrc/mcts_step.hip game_step_fast<N, true>) where the end-to-end cache tests of
test_gpu_parity.py do not reach: the compact miss list of sets larger than 512 games (the trunk's <0, true> / <2, true> builds), the
table's entries read back and restated on the host (key, hash window, legal list, the fp64 network's priors and value), the table
after a weight change without a reset (the long-lived pv_mcts engines), and the launch options that change geometry only."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _util as U   # noqa: E402
from tests.test_gnn_any_shape import _make_net, _params64, _ref_forward   # noqa: E402
from tests.test_gpu_parity import _board_graphs, _generation, _model   # noqa: E402

pytestmark = pytest.mark.gpu

LIST_GAMES = 640          # > 512 games in one set: enqueue_sims (csrc/mcts.hip) hands the trunk a compact list of the misses
KEY_BYTES, ROW_BYTES = 32, 704
WINDOW = 64               # one probe round: entries home .. home + 63 of the slot's table
AUDIT_SAMPLE = 1500       # entries per audit checked against the fp64 network
PRIOR_BAR = dict(atol=1e-6, rtol=1e-5)       # test_gpu_parity.test_eval_cache_search_served_from_table_vs_oracle
VALUE_BAR = dict(atol=1e-5, rtol=1e-4)
COUNTERS = ("finished", "leaf_evals", "terminal_sims", "dead_ends")


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _x3(params):
    """The trunk weights x3: outside the static fp16 bound, so the tracking trunk build (<2, *>) serves the set
    (test_gpu_parity.test_gnn_range_proven_path)."""
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    big = {k: (v * (3.0 if "gcn" in k and "weight" in k else 1.0)).astype(np.float32) for k, v in params.items()}
    m = GNNNetwork()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in big.items()})
    return m.to("cuda").eval(), big


def _weight_set(which):
    return _model(9) if which == "proven" else _x3(_model(9)[1])


def _dense_reference(params):
    """fp64 (policy [B, A], value [B]) of the default network (oracle/gnn.py forward_states_dense)."""
    from oracle import gnn as og

    def ref(recs):
        out = og.forward_states_dense(params, recs)
        return out["policy"], out["value"]
    return ref


def _general_reference(net):
    """fp64 (policy [B, A], value [B]) of a GraphPolicyValueNetwork of any shape over the oracle's board graphs."""
    p, L = _params64(net), net.num_gcn_layers

    def ref(recs):
        x, ei, batch = _board_graphs(recs)
        pol, val = _ref_forward(p, L, torch.from_numpy(np.asarray(x, np.float64)), ei, batch, recs.shape[0])[:2]
        return pol.numpy(), val[:, 0].numpy()
    return ref


def _assert_same(a, b):
    """Two _generation results: counters and every tensor bit for bit."""
    (_, ca, ta), (_, cb, tb) = a, b
    for k in COUNTERS:
        assert ca[k] == cb[k], (k, ca, cb)
    assert len(ta) == len(tb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), i


def _move_evals(eng):
    """One move -> (network evaluations, entries of the compact lists, eval_count[sims]).  A leaf is counted in stat_leaf_evals when
    it is expanded, whether its evaluation came from the network or from the table (stat_cache_hits), so the move's network
    evaluations are d(leaf_evals) - d(cache_hits); every one of them was appended to the list of the simulation that selected it
    (eval_count[0 .. sims)), and the last element -- there is no trunk launch behind the final expansion -- stays 0."""
    c0 = eng.counters()
    eng.move()
    c1 = eng.counters()
    evals = (c1["leaf_evals"] - c0["leaf_evals"]) - (c1["cache_hits"] - c0["cache_hits"])
    cnt = eng.t["eval_count"].cpu().numpy()
    return evals, int(cnt[:eng.sims].sum()), int(cnt[eng.sims])


# ------------------------------------------------------------------ the table itself
def _key_states72(hw, vw, misc, N):
    """state72 records of key records (plies 0) -- the unpacking of engine._leaf_states, vectorised."""
    nw = (N - 1) ** 2
    r = np.zeros((hw.shape[0], 72), np.uint8)
    for i in range(4):
        r[:, i] = (misc >> np.uint32(8 * i)) & np.uint32(0xFF)
    bit = np.arange(nw, dtype=np.uint64)[None, :]
    one = np.uint64(1)
    r[:, 4:4 + nw] = ((hw[:, None] >> bit) & one) | (((vw[:, None] >> bit) & one) << one)
    r[:, 70] = N
    return r


def _home(hw, vw, misc, mask):
    """The probe window's first entry (csrc/mcts_step.hip, the select step's cache probe), in numpy uint64 arithmetic."""
    u = np.uint64
    with np.errstate(over="ignore"):
        h = hw * u(0x9E3779B97F4A7C15) ^ vw * u(0xC2B2AE3D27D4EB4F) ^ misc.astype(np.uint64) * u(0x165667B19E3779F9)
        h ^= h >> u(29)
        h *= u(0xBF58476D1CE4E5B9)
        h ^= h >> u(32)
    return (h & u(mask)).astype(np.int64)


def _audit_table(eng, reference, evaluations=None, sample=AUDIT_SAMPLE):
    """Read the evaluation cache back and restate it.  Key record (32 B): u64 hw, u64 vw, u32 ppos | pwl << 8 | epos << 16 | ewl << 24,
    u32 state (0 empty, 2 filled), i32 legal count, f32 value; row (704 B): f32 priors[136], u8 actions[136] (include/aqgnn.h).
    Every entry: the state word is 0 or 2; a live entry lies in its key's probe window, no key is held twice by one slot, and its
    legal count and action list are legal_actions() of the key's position (host build of the rules), the priors beyond the count 0.
    A fixed sample of live entries: priors and value against `reference(recs72) -> (policy [B, A], value [B])` in fp64.
    evaluations (a table that never had to replace an entry): the network evaluations since the table was last emptied -- each one
    reserved an empty entry of its own, so exactly that many entries are live.  Returns the number of live entries."""
    from alphaquoridorgnn_amd.game_logic import State
    N, S = eng.N, eng.eval_cache_slots
    keys = eng.t["eval_cache_keys"].cpu().numpy()
    assert keys.shape == (eng.G * S, KEY_BYTES)
    w32 = keys.view(np.uint32)
    state = w32[:, 5]
    assert np.isin(state, (0, 2)).all(), np.unique(state)
    live = np.nonzero(state == 2)[0]
    assert live.size > 0
    if evaluations is not None:
        assert live.size == evaluations, (live.size, evaluations)
    k = keys[live]
    hw, vw = k[:, 0:8].copy().view(np.uint64)[:, 0], k[:, 8:16].copy().view(np.uint64)[:, 0]
    misc = k[:, 16:20].copy().view(np.uint32)[:, 0]
    cnt = k[:, 24:28].copy().view(np.int32)[:, 0]
    value = k[:, 28:32].copy().view(np.float32)[:, 0]
    slot, pos = live // S, live % S
    # findable: the entry lies in the window its key's hash opens
    home = _home(hw, vw, misc, S - 1)
    off = (pos - home) & (S - 1)
    assert (off < WINDOW).all(), f"{int((off >= WINDOW).sum())} of {live.size} entries outside their probe window"
    # unique per slot
    ident = np.concatenate([slot.astype(np.int64).view(np.uint8).reshape(-1, 8), k[:, :20]], 1)
    assert np.unique(ident, axis=0).shape[0] == live.size, "a key is held twice by one slot's table"
    # legal list of the key's position (the host build of the rule header), once per distinct position
    recs = _key_states72(hw, vw, misc, N)
    uniq, inv = np.unique(recs, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order, count = U.hc_legal(N, uniq)
    order, count = order[inv], count[inv]
    assert np.array_equal(cnt, count), f"{int((cnt != count).sum())} of {live.size} legal counts differ"
    rows = eng.t["eval_cache_rows"].view(-1, ROW_BYTES)[torch.from_numpy(live).to(eng.dev)].cpu().numpy()
    pri = rows[:, :4 * U.MAX_LEGAL].copy().view(np.float32)
    act = rows[:, 4 * U.MAX_LEGAL:5 * U.MAX_LEGAL]
    inside = np.arange(U.MAX_LEGAL)[None, :] < cnt[:, None]
    assert np.array_equal(act[inside], order[inside].astype(np.uint8)), "stored action lists differ from legal_actions()"
    assert (act[~inside] == 0xFF).all() and (pri[~inside] == 0.0).all()
    # the network's evaluation of the key, on a fixed sample
    pick = np.sort(np.random.RandomState(0).choice(live.size, min(sample, live.size), replace=False))
    for i in pick[:8]:          # the vectorised unpacking is engine._leaf_states': game_logic.State of the 24-byte record
        m = int(misc[i])
        h, v = int(hw[i]), int(vw[i])
        walls = [((h >> j) & 1) + 2 * ((v >> j) & 1) for j in range((N - 1) ** 2)]
        st = State(board_size=N, player=[m & 0xFF, (m >> 8) & 0xFF], enemy=[(m >> 16) & 0xFF, (m >> 24) & 0xFF], walls=walls)
        assert np.array_equal(st.record(), recs[i])
    policy, val = reference(recs[pick])
    for j, i in enumerate(pick):
        n = int(cnt[i])
        p = np.asarray(policy[j], np.float64)[order[i, :n].astype(np.int64)]
        s = p.sum()
        np.testing.assert_allclose(pri[i, :n], p / (s if s else 1.0), err_msg=f"priors of entry {live[i]}", **PRIOR_BAR)
    np.testing.assert_allclose(value[pick], val, err_msg="values", **VALUE_BAR)
    return live.size


# ------------------------------------------------------------------ A + B: the compact list, both trunk builds
@pytest.mark.parametrize("weights", ["proven", "x3"])
def test_compact_list_generation_bit_identical(dev, weights):
    """640 games in one set, quota 704 (slots refill inside the list path), 8 simulations: with the cache on, the misses reach the
    trunk as a compact list -- the <0, true> build for a weight set inside the static fp16 bound, <2, true> for the x3 set -- and the
    generation must equal the cache-less one bit for bit, with a roomy table and with a 64-entry one (one probe window: entries are
    replaced all the time).  Both tables are then audited against the fp64 network."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    model, params = _weight_set(weights)
    flags = _lib.GNN_RANGE_PROVEN if weights == "proven" else 0
    assert model.gnn_flags(dev) == flags
    kw = dict(num_games=LIST_GAMES, quota=704, sims=8, seed=3)
    ref = _generation(model, 0, **kw)
    assert ref[1]["finished"] == 704
    ref_fn = _dense_reference(params)
    for slots in (256, 64):
        got = _generation(model, slots, **kw)
        eng, c = got[0], got[1]
        assert eng.e.gnn_flags == flags            # no range-guard replay: the list builds served the whole generation
        assert c["cache_hits"] > 0.1 * c["leaf_evals"], c
        _assert_same(ref, got)
        _audit_table(eng, ref_fn)
    # the path ran: every network evaluation of a move went through the compact lists
    eng = BatchedSelfPlay(model, num_games=LIST_GAMES, sims=8, seed=3, record_history=False, eval_cache_slots=256)
    for _ in range(4):
        evals, listed, tail = _move_evals(eng)
        assert evals == listed > 0 and tail == 0, (evals, listed, tail)


def test_compact_list_only_above_512_games_on_9x9(dev):
    """The list is the path of large 9x9 sets only: at 512 games per set (the headline's set size) and on 5x5 the trunk walks the
    mask, and no list entry is written."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from oracle import gnn as og
    model, _ = _model(2)
    m5 = GraphPolicyValueNetwork(6, 128, 3, _A(5), board_size=5)
    m5.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in og.init_params(1, N=5).items()})
    m5 = m5.to(dev).eval()
    for m, G, N in ((model, 512, 9), (m5, LIST_GAMES, 5)):
        eng = BatchedSelfPlay(m, num_games=G, sims=8, board_size=N, seed=3, record_history=False, eval_cache_slots=256)
        for _ in range(2):
            evals, listed, tail = _move_evals(eng)
            assert evals > 0 and listed == 0 and tail == 0, (G, N, evals, listed)


def test_compact_list_multiset_bit_identical(dev):
    """Two sets of 640 games on two streams, each with its own list."""
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    model, _ = _model(7)
    runs = []
    for slots in (0, 256):
        m = MultiSetSelfPlay(model, num_games=2 * LIST_GAMES, sims=8, num_sets=2, seed=4, eval_cache_slots=slots)
        assert [e.G for e in m.sets] == [LIST_GAMES, LIST_GAMES]
        c = m.play_generation()
        rows = tuple(x.cpu() for x in m.history_tensors())
        per_game = tuple(e.t[k].cpu() for e in m.sets for k in ("game_plies", "game_result", "game_slot", "game_first_move", "hist_action"))
        runs.append((c, rows + per_game))
    (c0, t0), (c1, t1) = runs
    assert c0["finished"] == 2 * LIST_GAMES and c0["cache_hits"] == 0 and c1["cache_hits"] > 0
    for k in COUNTERS:
        assert c0[k] == c1[k], k
    for x, y in zip(t0, t1):
        assert torch.equal(x, y)


def test_compact_list_range_guard_replay(dev):
    """The fp16-range guard at 640 games: the replay on the exact f32 kernels walks the mask (no list under EXACT_F32), starts from an
    empty table and equals the cache-less replay."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    runs = []
    for slots in (256, 0):
        model, _ = _model(5)                 # a copy per run: the first replay marks its model
        a = BatchedSelfPlay(model, num_games=LIST_GAMES, sims=6, seed=3, eval_cache_slots=slots)
        if slots:
            evals, listed, _ = _move_evals(a)
            assert evals == listed > 0
        else:
            a.move()
        for _ in range(2):
            a.move()
        a.t["counters"][5] = 1
        c = a.play_generation()
        assert a.e.gnn_flags == _lib.GNN_EXACT_F32 and c["finished"] == LIST_GAMES and (c["cache_hits"] > 0) == (slots > 0)
        rows = tuple(x.cpu() for x in a.history_tensors())
        per_game = tuple(a.t[k].cpu() for k in ("game_plies", "game_result", "game_slot", "game_first_move", "hist_action"))
        runs.append((a, c, rows + per_game))
        if slots:
            a.reset()
            evals, listed, tail = _move_evals(a)
            assert evals > 0 and listed == 0 and tail == 0
    _assert_same(runs[0], runs[1])


# ------------------------------------------------------------------ B: one entry per evaluation
def test_table_audit_roomy_table_holds_every_evaluation(dev):
    """A table no window of which fills up (at most 116 plies x 16 simulations per slot in 4,096 entries) never replaces an entry:
    after a generation it holds exactly one live entry per network evaluation of its slot -- an evaluation written anywhere but the
    entry its miss reserved (an entry another key's miss will then reserve and overwrite, or one outside the key's window) shows
    as a lost entry here, whatever the search made of it."""
    model, params = _model(3)
    kw = dict(num_games=64, sims=16, seed=5)
    ref = _generation(model, 0, **kw)
    got = _generation(model, 4096, **kw)
    c = got[1]
    assert c["cache_hits"] > 0
    _assert_same(ref, got)
    _audit_table(got[0], _dense_reference(params), evaluations=c["leaf_evals"] - c["cache_hits"])


# ------------------------------------------------------------------ B: the table on the other evaluators
def test_table_audit_small_board(dev):
    """5x5: the any-size forward fills the table over the same mask."""
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from oracle import gnn as og
    params = og.init_params(1, N=5)
    model = GraphPolicyValueNetwork(6, 128, 3, _A(5), board_size=5)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    model = model.to(dev).eval()
    kw = dict(num_games=48, sims=24, board_size=5, seed=9)
    ref = _generation(model, 0, **kw)
    got = _generation(model, 256, **kw)
    assert got[1]["cache_hits"] > 0
    _assert_same(ref, got)
    _audit_table(got[0], _dense_reference(params))


def test_table_audit_general_evaluator(dev):
    """prior_mode 3 (a network of another shape on the engine's own kernels): the same table, restated in fp64."""
    N = 5
    net = _make_net((6, 80, 2), _A(N), seed=31, N=N)
    kw = dict(num_games=48, sims=24, board_size=N, seed=9, evaluator="general")
    ref = _generation(net, 0, **kw)
    got = _generation(net, 256, **kw)
    assert got[1]["cache_hits"] > 0
    _assert_same(ref, got)
    _audit_table(got[0], _general_reference(net))


# ------------------------------------------------------------------ C: new weights, no reset
def _state_words(eng):
    return eng.t["eval_cache_keys"].view(-1, KEY_BYTES)[:, 20:24].contiguous().view(torch.int32)


def _train_inputs(recs, dev):
    rng = np.random.RandomState(1)
    pi = rng.rand(recs.shape[0], _A(9)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    z = rng.choice([-1.0, 0.0, 1.0], recs.shape[0]).astype(np.float32)
    return tuple(torch.from_numpy(x).to(dev) for x in (recs, pi, z))


@pytest.mark.parametrize("update", ["mul", "trainer"])
def test_refresh_weights_clears_table_without_reset(dev, update):
    """The fused 9x9 evaluator: after an in-place weight update refresh_weights() alone (no reset: what the long-lived pv_mcts engines
    do) must empty the table, and the next search must be a fresh engine's; with unchanged weights it must leave the table alone."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.train_network import GNNTrainer
    from oracle import quoridor as oq
    model, _ = _model(4)
    g = U.golden("walk_9x9.npz")
    recs = np.stack([g["states"][i] for i in [0, 5, 40, 333, 1200, 2600, 5000, 9000]])
    recs = recs[[not oq.State(r).is_done() for r in recs]]
    kw = dict(num_games=recs.shape[0], sims=16, record_history=False, eval_cache_slots=256)
    eng = BatchedSelfPlay(model, **kw)
    before = eng.search(recs)
    keys = eng.t["eval_cache_keys"].clone()
    assert int((_state_words(eng) != 0).sum()) > 0
    eng.refresh_weights()                                   # nothing changed: the entries are still the network's
    assert torch.equal(eng.t["eval_cache_keys"], keys)
    if update == "mul":
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1.25)
    else:
        tr = GNNTrainer(model, max_batch=recs.shape[0])
        tr.step(*_train_inputs(recs, dev), lr=0.05, update=True)
    eng.refresh_weights()
    assert int((_state_words(eng) != 0).sum()) == 0         # the old weights' rows are gone
    hits0 = eng.counters()["cache_hits"]
    got = eng.search(recs)
    fresh = BatchedSelfPlay(model, **kw)
    want = fresh.search(recs)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], before[0])               # the update does change the searches
    assert eng.counters()["cache_hits"] - hits0 == fresh.counters()["cache_hits"]
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    c = fresh.counters()                                    # ... and the table holds the NEW network's evaluations, all of them
    _audit_table(eng, _dense_reference(params), evaluations=c["leaf_evals"] - c["cache_hits"])


def test_pv_mcts_engine_refresh_after_in_place_update(dev, monkeypatch):
    """pv_mcts_policy keeps its engine (and with AQG_EVAL_CACHE_SLOTS its table) between calls: a walk whose model is updated in place
    halfway must return the policies of the same walk without a table."""
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.game_logic import State
    monkeypatch.setattr(pv_mcts, "PV_EVALUATE_COUNT", 16)

    def walk(slots, update=True):
        monkeypatch.setenv("AQG_EVAL_CACHE_SLOTS", str(slots))
        model, _ = _model(1)                 # a copy per walk: the update is in place
        pv_mcts._engines.clear()
        try:
            st, out = State(), []
            for ply in range(8):
                if ply == 4 and update:
                    with torch.no_grad():
                        for p in model.parameters():
                            p.mul_(1.25)
                pol = pv_mcts.pv_mcts_policy(model, st, 1.0)
                out.append(list(pol))
                st = st.next(st.legal_actions()[int(np.argmax(pol))])
            eng = next(iter(pv_mcts._engines.values()))
            return out, eng.eval_cache_slots, eng.counters()["cache_hits"]
        finally:
            pv_mcts._engines.clear()

    got, slots, hits = walk(256)
    assert slots == 256 and hits > 0
    want, slots, _ = walk(0)
    assert slots == 0
    assert got == want
    still, _, _ = walk(0, update=False)
    assert still[4:] != want[4:]             # the update changes the walk's later policies


# ------------------------------------------------------------------ D: launch options that change geometry only
OPTION_DEFAULTS = dict(step_waves=8, trunk_grid=0, trunk_delay_min_boards=2048, trunk_phase_delay=100, trunk_prio=-1, step_prio=1,
                       heads_prio=3, use_graph=1)     # csrc/mcts.hip, csrc/mcts_step.hip, csrc/gcn_trunk_split.hip: the g_* initialisers
OPTION_SETTINGS = [dict(step_waves=1), dict(step_waves=2), dict(step_waves=4),
                   dict(trunk_grid=1), dict(trunk_grid=7), dict(trunk_grid=100),
                   dict(trunk_delay_min_boards=1, trunk_phase_delay=0), dict(trunk_delay_min_boards=1),
                   dict(trunk_prio=0), dict(step_prio=0), dict(step_prio=3), dict(heads_prio=0), dict(use_graph=0)]
_OPTION_RUNS = {}


def _option_runs(model, dev):
    """(40 games without and with the table, 640 games with the table: the list) under the options in force, on a side stream: there
    a move is captured into a hipGraph that bakes the options in (csrc/mcts.hip run_sims), as in MultiSetSelfPlay's sets."""
    if "side" not in _OPTION_RUNS:
        _OPTION_RUNS["side"] = torch.cuda.Stream(device=dev)
    small = dict(num_games=40, sims=12, seed=11)
    large = dict(num_games=LIST_GAMES, sims=8, seed=12)
    out = []
    with torch.cuda.stream(_OPTION_RUNS["side"]):
        for slots, kw in ((0, small), (256, small), (256, large)):
            eng, c, t = _generation(model, slots, **kw)
            out.append((c, t))
    return out


@pytest.mark.parametrize("setting", OPTION_SETTINGS, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_launch_options_leave_results_bit_identical(dev, setting):
    """Options that only lay the same work out differently (games per step workgroup, the trunk's grid and start offsets, wave
    priorities, graph capture) must leave every generation bit-identical: without the table, with it, and on the compact list, where a
    trunk grid shorter than the list makes each workgroup walk several entries."""
    from alphaquoridorgnn_amd import _lib
    model, _ = _model(2)
    if "defaults" not in _OPTION_RUNS:
        for k, v in OPTION_DEFAULTS.items():
            _lib.set_option(k, v)
        _OPTION_RUNS["defaults"] = _option_runs(model, dev)
    try:
        for k, v in setting.items():
            _lib.set_option(k, v)
        got = _option_runs(model, dev)
    finally:
        for k, v in OPTION_DEFAULTS.items():
            _lib.set_option(k, v)
    for (c0, t0), (c1, t1) in zip(_OPTION_RUNS["defaults"], got):
        assert c0 == c1
        for i, (x, y) in enumerate(zip(t0, t1)):
            assert torch.equal(x, y), i
