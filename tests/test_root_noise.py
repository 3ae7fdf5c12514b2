"""Root exploration noise on the device (csrc/mcts_move.hip engine_root_noise_kernel; include/aqgnn.h "root exploration noise"): the mix
bit for bit against its numpy statement, searches and whole games bit for bit against the oracle's PV-MCTS with a model that mixes
at the root, the generator against its numpy mirror, independence from slots and launch geometry, the evaluation cache kept clean,
and noise off = the engine as it was."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _util as U
from tests.test_root_noise_cpu import MAX_LEGAL, mix_statement

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _no_walls_in_hand():
    """A 9x9 position with no walls in hand on either side: only pawn moves are legal (between 1 and 5 actions)."""
    from oracle import quoridor as oq
    rec = oq.init_record(9)
    rec[1] = rec[3] = 0
    assert 1 <= len(oq.State(rec).legal_actions()) <= 5
    return rec


@functools.lru_cache(maxsize=None)
def _roots(N, count):
    """`count` roots of board N that are not over: the opening (35 / 131 actions: one lane round / three with a ragged last one),
    on 9x9 the position without walls in hand, then positions spread over the recorded walk."""
    from oracle import quoridor as oq
    recs = [oq.init_record(N)] + ([_no_walls_in_hand()] if N == 9 else [])
    pool = U.golden(f"walk_{N}x{N}.npz")["states"]
    for i in np.linspace(1, pool.shape[0] - 1, 4 * count).astype(int):
        if len(recs) == count:
            break
        st = oq.State(pool[i])
        if not st.is_done() and len(st.legal_actions()) > 0:
            recs.append(pool[i].copy())
    assert len(recs) == count
    return np.stack(recs).astype(np.uint8)


def _table(seed, *shape):
    """Integer-valued doubles in 1 .. 1024: every partial sum is exact, so S does not depend on the reduction tree."""
    return np.random.RandomState(seed).randint(1, 1025, size=shape + (MAX_LEGAL,)).astype(np.float64)


def _engine(G, sims, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    kw.setdefault("record_history", False)
    return BatchedSelfPlay(kw.pop("model", None), num_games=G, sims=sims, board_size=N, **kw)


def _clean_priors(recs, bias=0):
    from oracle import mcts as om, quoridor as oq
    return [om.FakeModel(bias).predict(oq.State(r))[0] for r in recs]


class _RootMix:
    """oracle.mcts.FakeModel whose predict returns the mixed priors for the root of the search that start() announced and the clean
    ones elsewhere.  Only the FIRST predict of a search is mixed -- the root, while the tree is empty: a transposition back to the
    root's position further down (a different plies_played, but guard anyway) is never mixed a second time."""

    def __init__(self, bias=0):
        from oracle import mcts as om
        self.base = om.FakeModel(bias)
        self.fresh, self.root, self.mixer = False, None, None

    def start(self, root_state, mixer):
        self.fresh, self.root, self.mixer = True, root_state.rec.tobytes(), mixer

    def predict(self, state, device=None):
        p, v = self.base.predict(state, device)
        if self.fresh:
            assert state.rec.tobytes() == self.root
            self.fresh = False
            p = np.asarray(self.mixer(p), dtype=np.float32)
            assert p.shape[0] == len(state.legal_actions())
        return p, v


def _oracle_visits(rec, sims, mixer, bias=0):
    from oracle import mcts as om, quoridor as oq
    model, st = _RootMix(bias), oq.State(rec)
    model.start(st, mixer)
    return [c.n for c in om.search(model, st, sims).children]


def _assert_visits(got, recs, want):
    visits, actions, count = (x.cpu().numpy() for x in got)
    from oracle import quoridor as oq
    for g, rec in enumerate(recs):
        legal = oq.State(rec).legal_actions()
        assert count[g] == len(legal) and list(actions[g, :count[g]]) == list(legal), g
        assert list(visits[g, :count[g]]) == want[g], g


# ------------------------------------------------------------------ 1. table mode: the mix, bit for bit
@pytest.mark.parametrize("eps", [0.25, 0.5])
@pytest.mark.parametrize("N", [3, 5, 9])
def test_table_mix_bit_exact(dev, N, eps):
    recs = _roots(N, 8)
    table = _table(100 + N, 8)
    eng = _engine(8, 2, N, root_noise_eps=eps)
    eng.search(recs, root_noise=table)
    priors, count = (x.cpu().numpy() for x in eng.root_priors())
    clean = _clean_priors(recs)
    changed = 0
    for g in range(8):
        assert count[g] == len(clean[g])
        want = mix_statement(clean[g], table[g], eps)
        assert priors[g, :count[g]].tobytes() == want.tobytes(), (g, count[g])
        assert not priors[g, count[g]:].any()
        changed += int(not np.array_equal(want, clean[g]))
    assert changed == int((count > 1).sum()) >= 4       # (cnt = 1 mixes 1 with 1)
    if N == 9:
        assert count[0] == 131 and 1 <= count[1] <= 5   # three lane rounds, ragged; and a handful of pawn moves
    if N == 5:
        assert count[0] == 35


# ------------------------------------------------------------------ 2. table mode: searches and games against the oracle
@functools.lru_cache(maxsize=None)
def _oracle_searches(N, eps, sims):
    recs, table = _roots(N, 16), _table(200 + N, 16)
    clean = _clean_priors(recs, bias=3)
    return [_oracle_visits(recs[g], sims, lambda p, g=g: mix_statement(p, table[g], eps), bias=3) for g in range(16)], clean


@pytest.mark.parametrize("fast_depth", [0, 61])
@pytest.mark.parametrize("N", [5, 9])
def test_table_search_matches_oracle(dev, N, fast_depth):
    from alphaquoridorgnn_amd import _lib
    eps, sims = 0.25, 50
    want, _ = _oracle_searches(N, eps, sims)
    recs, table = _roots(N, 16), _table(200 + N, 16)
    _lib.set_option("step_fast_depth", fast_depth)
    try:
        eng = _engine(16, sims, N, root_noise_eps=eps, fake_bias=3)
        got = eng.search(recs, root_noise=table)
        _assert_visits(got, recs, want)
        plain = _engine(16, sims, N, fake_bias=3).search(recs)
        assert not torch.equal(plain[0], got[0])        # ... and the noise did steer the search
    finally:
        _lib.set_option("step_fast_depth", 61)


def _oracle_game(N, sims, uniforms, tables, eps, bias=0):
    """oracle.mcts.play's loop -- search, Boltzmann at T = 1, np.random.choice's draw, next(), z -- with the root of every move mixed
    with that ply's table row (eps None: no mix; then it IS oracle.mcts.play, which the test checks)."""
    from oracle import mcts as om, quoridor as oq
    model, state, hist, ply = _RootMix(bias), oq.State(N=N), [], 0
    while not state.is_done():
        model.start(state, (lambda p: p) if eps is None else (lambda p: mix_statement(p, tables[ply], eps)))
        visits = [c.n for c in om.search(model, state, sims).children]
        scores = om.boltzman(visits, 1.0)
        legal = state.legal_actions()
        row = np.zeros(_A(N), dtype=np.int64)
        row[list(legal)] = visits
        hist.append((state.rec.copy(), row))
        state = state.next(legal[om.choice_index(scores, uniforms[ply])])
        ply += 1
    return hist, om.first_player_value(state)


@pytest.mark.parametrize("N", [3, 5])
def test_table_games_match_oracle(dev, N):
    from oracle import mcts as om
    eps, sims, G = 0.25, 16, 4
    eng = _engine(G, sims, N, root_noise_eps=eps, record_history=True, fake_bias=2)
    u = np.random.RandomState(300 + N).random_sample(size=(eng.max_plies, G))
    tables = _table(400 + N, eng.max_plies, G)
    eng.play_generation(uniforms=torch.from_numpy(u), check_every=1, root_noise=torch.from_numpy(tables))
    plies = eng.t["game_plies"].cpu().numpy()
    hs, hv = eng.t["hist_state72"].cpu().numpy(), eng.t["hist_visits"].cpu().numpy()
    res, done = eng.t["game_result"].cpu().numpy(), eng.t["game_done"].cpu().numpy()
    for k in range(G):                                   # no refill: game k sits in slot k, and move m is its ply m
        hist, z = _oracle_game(N, sims, u[:, k], tables[:, k], eps, bias=2)
        assert done[k] and plies[k] == len(hist) and res[k] == z, k
        for j, (rec, row) in enumerate(hist):
            assert np.array_equal(hs[k, j, :70], rec[:70]) and np.array_equal(hv[k, j].astype(np.int64), row), (k, j)
    # the loop above with no mix is oracle.mcts.play
    ref = om.play(om.FakeModel(2), sims, N=N, uniforms=list(u[:, 0]))
    hist, z = _oracle_game(N, sims, u[:, 0], None, None, bias=2)
    assert len(ref) == len(hist) and ref[0][2] == z
    for (sa, pol, _), (rec, row) in zip(ref, hist):
        assert sa[0] == [int(rec[0]), int(rec[1])] and np.allclose(pol, row / row.sum(), rtol=0, atol=1e-15)


# ------------------------------------------------------------------ 3. generator mode against the numpy mirror
TOL = 4 * 2.0 ** -24      # eta, the two products and the sum: one f32 rounding each of a value <= 1 (the f64 library functions: 1e-15)


def _mirror_rows(eng, recs, ks, eps, bias=0):
    from alphaquoridorgnn_amd.engine import draw_root_noise
    from oracle import quoridor as oq
    out = []
    for rec, k in zip(recs, ks):
        st = oq.State(rec)
        clean = _clean_priors([rec], bias)[0]
        g = draw_root_noise(eng.root_noise_seed, int(k), st.plies_played, len(clean), eng.root_noise_alpha)
        out.append(mix_statement(clean, g, eps))
    return out


@pytest.mark.parametrize("alpha", [0.03, 0.3, 3.0])
def test_generator_matches_mirror(dev, alpha):
    N, G, eps, sims = 9, 64, 0.25, 8
    mid = _roots(N, G + 1)[1:]                            # the position without walls in hand and 63 of the walk
    runs = []
    for _ in range(2):
        eng = _engine(G, sims, N, root_noise_eps=eps, root_noise_alpha=alpha, seed=5, record_history=True)
        out = []
        for ply in range(2):                              # two moves from the opening: game k = slot k at plies 0 and 1
            recs = eng.root_states72().cpu().numpy()
            eng.move(torch.full((G,), 0.37 + 0.2 * ply, dtype=torch.float64))
            out.append((recs, [x.cpu().numpy() for x in eng.root_priors()], eng.t["hist_visits"][:, ply].cpu().numpy()))
        vis = eng.search(mid)                             # ... and a search of mid-game roots: k = slot, ply = the root's own
        out.append((mid, [x.cpu().numpy() for x in eng.root_priors()], vis[0].cpu().numpy()))
        runs.append(out)
    for a, b in zip(*runs):                               # two runs: identical bytes
        assert a[1][0].tobytes() == b[1][0].tobytes() and a[2].tobytes() == b[2].tobytes()
    worst = 0.0
    for step, (recs, (priors, count), _) in enumerate(runs[0]):
        want = _mirror_rows(eng, recs, range(G), eps)
        for g in range(G):
            assert count[g] == len(want[g])
            worst = max(worst, float(np.abs(priors[g, :count[g]].astype(np.float64) - want[g]).max()))
            assert abs(float(priors[g, :count[g]].astype(np.float64).sum()) - 1.0) < 1e-5
    print(f"alpha {alpha}: worst |device - mirror| = {worst:.3e} (bound {TOL:.3e})")
    assert worst <= TOL
    # noise differs between slots (the 64 openings share their clean priors) ...
    first = runs[0][0][1][0]
    assert len({first[g, :131].tobytes() for g in range(G)}) == G
    # ... and between plies, on the device's own output: eta as the device mixed it in, (p' - (1 - eps) p) / eps, of the same game at
    # ply 0 and at ply 1 (each entry is off by a few f32 roundings / eps at most; two Dirichlet draws differ by far more somewhere)
    etas = []
    for recs, (priors, count), _ in runs[0][:2]:
        clean = _clean_priors(recs)
        etas.append([(priors[g, :count[g]].astype(np.float64) - 0.75 * clean[g].astype(np.float64)) / eps for g in range(G)])
    for g in range(G):
        n = min(len(etas[0][g]), len(etas[1][g]))
        assert n > 5 and np.abs(etas[0][g][:n] - etas[1][g][:n]).max() > 1e-4, g
    # the search is exact GIVEN the priors: the oracle fed the device's own mixed priors visits the same children as often -- every
    # slot, the two moves and the search
    from oracle import quoridor as oq
    for step, (recs, (priors, count), visits) in enumerate(runs[0]):
        for g in range(G):
            want = _oracle_visits(recs[g], sims, lambda p, g=g: priors[g, :count[g]])
            got = visits[g, :count[g]] if step == 2 else visits[g][list(oq.State(recs[g]).legal_actions())]
            assert list(got) == want, (step, g)


# ------------------------------------------------------------------ 4. independence from geometry
def _play_quota(G, quota, U_game, N, sims, **kw):
    """Play `quota` games on G slots; game k's move at ply j is drawn with U_game[k, j] whatever slot it sits in."""
    eng = _engine(G, sims, N, quota=quota, record_history=True, **kw)
    for _ in range(eng.max_plies * quota + 1):
        active = eng.t["game_active"].cpu().numpy()
        if not active.any():
            break
        sg, gp = eng.t["slot_game"].cpu().numpy(), eng.t["game_plies"].cpu().numpy()
        u = np.zeros(G)
        for g in range(G):
            if active[g]:
                u[g] = U_game[sg[g], gp[sg[g]]]
        eng.move(torch.from_numpy(u))
    assert eng.counters()["finished"] == quota
    plies = eng.t["game_plies"].cpu().numpy()
    hs, hv, ha = (eng.t[k].cpu().numpy() for k in ("hist_state72", "hist_visits", "hist_action"))
    return [(int(plies[k]), int(eng.t["game_result"][k]), hs[k, :plies[k]].tobytes(), hv[k, :plies[k]].tobytes(),
             ha[k, :plies[k]].tobytes()) for k in range(quota)]


def test_noise_is_keyed_by_game_not_by_slot(dev):
    N, sims, quota = 5, 8, 12
    U_game = np.random.RandomState(77).random_sample(size=(quota, 28))
    kw = dict(root_noise_eps=0.25, root_noise_alpha=0.3, seed=9)
    refill = _play_quota(4, quota, U_game, N, sims, **kw)          # three games per slot
    wide = _play_quota(12, quota, U_game, N, sims, **kw)           # one slot per game
    assert refill == wide
    assert _play_quota(12, quota, U_game, N, sims, seed=9) != wide     # (the noise does change the games)


def test_multiset_games_have_distinct_streams(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay, draw_root_noise
    N, eps, alpha = 5, 0.25, 0.3
    ms = MultiSetSelfPlay(None, num_games=8, sims=4, num_sets=2, seed=3, board_size=N, evaluator="fake", quota=20,
                          root_noise_eps=eps, root_noise_alpha=alpha, root_noise_seed=1234)
    assert len({s.root_noise_seed for s in ms.sets}) == 2
    ms.move()
    ms.sync()
    rows = []
    first = 0
    clean = _clean_priors(_roots(N, 1))[0]
    for s in ms.sets:
        priors = s.root_priors()[0].cpu().numpy()
        for k in range(s.G):                               # set i's game k is game first_i + k of the whole engine
            want = mix_statement(clean, draw_root_noise(1234, first + k, 0, 35, alpha), eps)
            assert np.abs(priors[k, :35].astype(np.float64) - want).max() <= TOL
            rows.append(priors[k, :35].tobytes())
        first += s.quota
    assert len(set(rows)) == 8                             # eight openings, eight different noises
    assert first == 20


# ------------------------------------------------------------------ 5. the evaluation cache never holds a noisy row
def _net(kind, N, dev):
    if kind == "general":
        from tests.test_gnn_any_shape import _make_net
        return _make_net((6, 16, 2), _A(N), seed=11, N=N)
    if kind == "cnn":
        from tests.test_cnn import _make_net
        return _make_net(8, 1, N, seed=12).to(dev)
    from tests.test_gpu_parity import _model
    return _model(2)[0]


def _rows(eng):
    return tuple(x.cpu() for x in eng.history_tensors()) + tuple(eng.t[k].cpu() for k in ("game_plies", "game_result", "hist_action"))


@pytest.mark.parametrize("kind,N", [("general", 5), ("gnn", 9), ("cnn", 5)])
def test_eval_cache_stays_clean(dev, kind, N):
    net = _net(kind, N, dev)
    G, sims = 8, 12
    kw = dict(model=net, evaluator=kind, seed=4, record_history=True, root_noise_eps=0.25)
    off = _engine(G, sims, N, eval_cache_slots=0, **kw)
    off.play_generation()
    on = _engine(G, sims, N, eval_cache_slots=64, **kw)
    c = on.play_generation()
    assert c["finished"] == G and c["cache_hits"] > 0
    assert all(torch.equal(a, b) for a, b in zip(_rows(off), _rows(on)))
    plain = _engine(G, sims, N, model=net, evaluator=kind, seed=4, record_history=True, eval_cache_slots=0)
    plain.play_generation()
    assert not all(torch.equal(a, b) for a, b in zip(_rows(plain), _rows(on)))     # the noise was on
    # Positions the noisy games had as roots, slot by slot (a slot's table outlives its games), searched WITHOUT noise on the same
    # engine must come out as on a fresh one: a noisy row in the table would be served here.  Noise-free on the same engine = a
    # table of zeros, which leaves every root untouched.  Every slot probes its ply-2 root, and then the opening, the latter on an
    # engine that has played three moves into a roomy table (nothing evicted): the opening is the one root that always misses the
    # table when it is evaluated -- had its mixed row been stored then, simulation 0's probe would find it now.
    zeros = torch.zeros((G, MAX_LEGAL), dtype=torch.float64)
    fresh = _engine(G, sims, N, model=net, evaluator=kind, eval_cache_slots=0)
    plies = on.t["game_plies"].cpu().numpy()
    roots = torch.stack([on.t["hist_state72"][g, min(2, plies[g] - 1)] for g in range(G)])
    got = on.search(roots, root_noise=zeros)
    assert all(torch.equal(a, b) for a, b in zip(got, fresh.search(roots)))
    young = _engine(G, sims, N, eval_cache_slots=4096, **kw)
    for _ in range(3):
        young.move()
    opening = young.t["hist_state72"][:, 0].clone()
    assert bool((opening == opening[0]).all()) and int(opening[0, 68]) == 0 and int(opening[0, 69]) == 0
    got = young.search(opening, root_noise=zeros)
    assert all(torch.equal(a, b) for a, b in zip(got, fresh.search(opening)))


# ------------------------------------------------------------------ 6. off is off
@pytest.mark.parametrize("kind", ["fake", "general"])
def test_noise_off_changes_nothing(dev, kind):
    from alphaquoridorgnn_amd import _lib
    N, G, sims = 5, 8, 12
    kw = dict(seed=6, record_history=True)
    if kind == "general":
        kw.update(model=_net("general", N, dev), evaluator="general")
    a = _engine(G, sims, N, **kw)
    a.play_generation()
    b = _engine(G, sims, N, root_noise_eps=0.0, root_noise_alpha=0.3, root_noise_seed=99, **kw)
    b.play_generation()
    assert all(torch.equal(x, y) for x, y in zip(_rows(a), _rows(b)))
    assert (b.e.root_noise_eps, b.e.root_noise_alpha, b.e.root_noise_seed, b.e.root_noise) == (0.0, 0.0, 0, None)
    # the launch on its own, on an engine with eps == 0: returns 0 and writes nothing
    b.search(_roots(N, G))
    names = ("policy", "leaf_flag", "legal_count", "path_len", "value", "node_rec")
    before = {k: b.t[k].clone() for k in names}
    assert _lib.load().aqg_engine_root_noise(ctypes.byref(b.e), b._stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], b.t[k]) for k in names)


# ------------------------------------------------------------------ 7. external evaluator
def test_external_evaluator_takes_the_same_noise(dev):
    from tests.test_gpu_parity import _OracleFakeAdapter
    N, G, sims, eps = 5, 8, 12, 0.25
    recs, table = _roots(N, G), _table(700, G)
    fake = _engine(G, sims, N, root_noise_eps=eps, fake_bias=1)
    want = fake.search(recs, root_noise=table)
    ext = _engine(G, sims, N, model=_OracleFakeAdapter(1), evaluator="external", root_noise_eps=eps)
    got = ext.search(recs, root_noise=table)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(ext.root_priors()[0], fake.root_priors()[0])
    assert not torch.equal(_engine(G, sims, N, fake_bias=1).search(recs)[0], want[0])


# ------------------------------------------------------------------ 8. guards
def test_guards(dev):
    N, G, eps = 9, 8, 0.25
    recs = _roots(N, G)
    table = _table(800, G)
    table[0] = 0.0                                          # no usable noise: the root keeps its priors
    table[2, :5] = [np.nan, -1.0, np.inf, 0.0, 7.0]         # entries that are not > 0 and finite count as 0
    one = [g for g in range(G) if len(_clean_priors([recs[g]])[0]) == 1]
    eng = _engine(G, 4, N, root_noise_eps=eps)
    eng.search(recs, root_noise=table)
    priors, count = (x.cpu().numpy() for x in eng.root_priors())
    clean = _clean_priors(recs)
    assert priors[0, :count[0]].tobytes() == clean[0].tobytes()
    for g in range(1, G):
        assert priors[g, :count[g]].tobytes() == mix_statement(clean[g], table[g], eps).tobytes(), g
    for g in one:                                            # cnt = 1: (1 - eps) 1 + eps 1, as the formula gives it
        assert priors[g, 0] == np.float32(np.float32(0.75) + np.float32(0.25))


def test_single_legal_action(dev):
    """cnt = 1 on the device: a 3x3 root with one pawn move and no wall left gives p' = (1 - eps) 1 + eps 1."""
    from oracle import quoridor as oq
    N = 3
    pool = U.golden("walk_3x3.npz")
    idx = [i for i in np.flatnonzero(pool["counts"] == 1) if not oq.State(pool["states"][i]).is_done()]
    if not idx:
        pytest.fail("the recorded 3x3 walk holds no live position with a single legal action")
    recs = np.stack([pool["states"][idx[0]]] * 4)
    eng = _engine(4, 4, N, root_noise_eps=0.5)
    eng.search(recs, root_noise=_table(900, 4))
    priors, count = (x.cpu().numpy() for x in eng.root_priors())
    assert list(count) == [1] * 4
    assert (priors[:, 0] == np.float32(np.float32(0.5) * np.float32(1) + np.float32(0.5) * np.float32(1))).all()


@pytest.mark.parametrize("mode", ["table", "generator"])
def test_graph_capture_on_and_off(dev, mode):
    from alphaquoridorgnn_amd import _lib
    N, G, sims = 5, 8, 12
    rows = []
    try:
        for use_graph in (1, 0):
            _lib.set_option("use_graph", use_graph)
            eng = _engine(G, sims, N, root_noise_eps=0.25, root_noise_alpha=0.3, seed=8, record_history=True)
            u = np.random.RandomState(1).random_sample(size=(eng.max_plies, G))
            tables = torch.from_numpy(_table(1000, eng.max_plies, G)) if mode == "table" else None
            eng.play_generation(uniforms=torch.from_numpy(u), root_noise=tables)
            rows.append(_rows(eng))
    finally:
        _lib.set_option("use_graph", 1)
    assert all(torch.equal(a, b) for a, b in zip(*rows))
