"""Completed-Q policy targets on the GPU (include/aqgnn.h "completed-Q policy targets"; csrc/mcts_improve.hip, the POLICY form of
csrc/replay_refresh.hip, reanalyse.py, pv_mcts.py): the read-out launch against engine.improved_policy_reference on synthetic pools at
every lane-round and workgroup edge and on real searches, with sentinel margins around its outputs; the refresh form bit for bit
against replay.refresh_policy_reference; the whole reanalyse stage against a host statement; and the user function.

The tolerances are the derived ones of tests/_improved_policy.py: one f32 ulp for pi', one f32 ulp plus (cnt + 1)(Nsum + 1) 2^-53 for
vmix -- the device and numpy evaluate log, exp and the sums with different libraries and in different orders."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests._improved_policy import (COUNTS, PATTERNS, POLICY_SPECIAL, expected_refresh_policy, oracle_children, paper_policy,   # noqa: E402
                                    pi_close, policy_rows, policy_written_rows, synthetic_pool, vmix_bound, vmix_close, walked_records)
from tests._reanalyse import MAX_LEGAL, bits, policy_size, random_rings   # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _engine(G, sims, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    return BatchedSelfPlay(kw.pop("model", None), num_games=G, sims=sims, board_size=N, **kw)


def _pools(eng):
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    return eng.t["node_rec"].cpu().numpy().view(NODE_DTYPE).reshape(eng.G, eng.node_cap).copy()


def _read_out(eng, c_visit=50.0, c_scale=1.0, null=None):
    """The C entry with a sentinel margin of one row in front of and behind every output; (rc, policy, actions, count, vmix) with the
    margins checked and cut off."""
    from alphaquoridorgnn_amd import _lib
    G = eng.G
    shapes = (("policy", torch.float32, MAX_LEGAL), ("actions", torch.uint8, MAX_LEGAL), ("count", torch.int32, 1), ("vmix", torch.float32, 1))
    bufs = [torch.full(((G + 2) * w * torch.empty((), dtype=dt).element_size(),), SENTINEL, dtype=torch.uint8, device=eng.dev) for _, dt, w in shapes]
    ptrs = [None if name == null else ctypes.c_void_p(b.data_ptr() + w * torch.empty((), dtype=dt).element_size())
            for b, (name, dt, w) in zip(bufs, shapes)]
    rc = eng.lib.aqg_engine_root_improved_policy(ctypes.byref(eng.e), c_visit, c_scale, *ptrs, eng._stream())
    torch.cuda.synchronize()
    out = []
    for b, (name, dt, w) in zip(bufs, shapes):
        raw = b.cpu().numpy()
        row = w * np.dtype(str(dt).split(".")[1]).itemsize
        assert (raw[:row] == SENTINEL).all() and (raw[-row:] == SENTINEL).all(), name
        if rc != 0:
            assert (raw == SENTINEL).all(), name                 # a refusal comes before any launch
        body = raw[row:-row].view(str(dt).split(".")[1])
        out.append(body.reshape(G, w) if w > 1 else body.reshape(G))
    return (rc, *out)


def _check_rows(pools, got, c_visit=50.0, c_scale=1.0):
    """Every slot's row against the pool-level reference, at the derived tolerances; the bytes past the count exactly."""
    from alphaquoridorgnn_amd.engine import root_improved_policy_reference
    policy, actions, count, vmix = got
    for g in range(pools.shape[0]):
        want_p, want_a, want_c, want_v = root_improved_policy_reference(pools[g], c_visit, c_scale)
        assert count[g] == want_c and np.array_equal(actions[g], want_a), g
        assert (bits(policy[g, want_c:]) == 0).all() and (actions[g, want_c:] == 0xFF).all(), g
        assert np.array_equal(policy[g] == 0, want_p == 0), g                        # excluded and underflowed entries are exactly 0
        assert pi_close(policy[g], want_p), (g, np.abs(policy[g].astype(np.float64) - want_p).max())
        first = int(pools[g, 0]["kids"]) & 0xFFFFFF
        nsum = int(pools[g, first:first + want_c]["n"].astype(np.int64).sum()) if want_c else 0
        assert vmix_close(vmix[g], want_v, want_c, nsum), (g, float(vmix[g]), float(want_v), vmix_bound(want_v, want_c, nsum))


# ------------------------------------------------------------------ 1a. the read-out on synthetic pools
@pytest.mark.parametrize("G", (1, 4, 5))
def test_read_out_on_synthetic_pools(dev, G):
    """Every (pattern, count) pool in turn through an engine of G slots -- one workgroup with idle wavefronts, a full one, and one
    wavefront into a second -- plus the two guard rows: a child range past node_cap and a count above MAX_LEGAL."""
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    eng = _engine(G, 2, 5, record_history=False)
    cap = eng.node_cap
    assert cap >= 1 + MAX_LEGAL
    cases = [synthetic_pool(NODE_DTYPE, cap, cnt, pattern, seed=1000 * k + cnt) for k, pattern in enumerate(PATTERNS) for cnt in COUNTS]
    cases.append(synthetic_pool(NODE_DTYPE, cap, 20, "mixed", seed=7, first=cap - 19))          # first + cnt == node_cap + 1
    cases.append(synthetic_pool(NODE_DTYPE, cap, 137, "mixed", seed=8, first=1))
    cases.append(synthetic_pool(NODE_DTYPE, cap, 136, "mixed", seed=9, first=cap - 136))        # ... and the last range that fits
    seen_zero_rows = 0
    for first in range(0, len(cases), G):
        chunk = [cases[(first + g) % len(cases)] for g in range(G)]
        pools = np.stack(chunk)
        eng.t["node_rec"].copy_(torch.from_numpy(pools.view(np.float64).reshape(G * cap, 4)))
        settings = ((50.0, 1.0),) if first % 3 else ((50.0, 1.0), (0.0, 0.3), (7.5, 0.0))
        for c_visit, c_scale in settings:
            rc, *got = _read_out(eng, c_visit, c_scale)
            assert rc == 0, eng.lib.aqg_last_error()
            _check_rows(pools, got, c_visit, c_scale)
        seen_zero_rows += sum(int(c) == 0 and (int(p[0]["kids"]) >> 24) > 0 for c, p in zip(got[2], chunk))
        assert np.array_equal(_pools(eng).view(np.uint8), pools.view(np.uint8))     # the launch only reads the pool
    assert seen_zero_rows >= 2


def test_read_out_patterns_do_what_they_claim(dev):
    """The named patterns, on the device's own rows: underflow to exact zeros beside n = 32767, exact zeros at zero priors beside
    1e-38 priors (which may underflow beside a dominant entry, as the reference's do), PV == 0 completing with vhat."""
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    eng = _engine(4, 2, 5, record_history=False)
    cap = eng.node_cap
    chunk = [synthetic_pool(NODE_DTYPE, cap, 136, p, seed=3) for p in ("big_n", "tiny_priors", "zero_prior_visited", "q_extremes")]
    pools = np.stack(chunk)
    eng.t["node_rec"].copy_(torch.from_numpy(pools.view(np.float64).reshape(4 * cap, 4)))
    rc, policy, actions, count, vmix = _read_out(eng)
    assert rc == 0 and (count == 136).all()
    kids = [p[(int(p[0]["kids"]) & 0xFFFFFF):][:136] for p in chunk]
    assert kids[0]["n"].max() == 32767 and (policy[0] == 0).sum() >= 100 and policy[0].max() > 0.99
    assert (policy[1][kids[1]["p"] == 0] == 0).all() and (kids[1]["p"] == 0).any() and (kids[1]["p"] == np.float32(1e-38)).any()
    assert (policy[2][kids[2]["p"] == 0] == 0).all() and not kids[2]["p"][kids[2]["n"] > 0].any()
    assert vmix_close(vmix[2], np.float32(chunk[2]["w"][0] + kids[2]["w"].sum()), 136, int(kids[2]["n"].sum()))
    assert set(np.abs(kids[3]["q"][kids[3]["n"] > 0]).tolist()) == {1.0}
    for g in range(4):
        assert abs(float(policy[g].astype(np.float64).sum()) - 1.0) <= 136 * 2.0 ** -24


def test_read_out_refusals(dev):
    eng = _engine(3, 2, 5, record_history=False)
    eng.search(torch.from_numpy(walked_records(5, 3, seed=1)))
    lib = eng.lib
    for kw, match in ((dict(null="policy"), "null"), (dict(null="actions"), "null"), (dict(null="count"), "null"), (dict(null="vmix"), "null"),
                      (dict(c_visit=-1.0), "c_visit"), (dict(c_visit=float("nan")), "c_visit"), (dict(c_visit=float("inf")), "c_visit"),
                      (dict(c_scale=-1e-9), "c_scale"), (dict(c_scale=float("nan")), "c_scale"), (dict(c_scale=float("inf")), "c_scale")):
        rc = _read_out(eng, **kw)[0]
        assert rc != 0 and match in lib.aqg_last_error().decode(), (kw, lib.aqg_last_error())
    rc = lib.aqg_engine_root_improved_policy(None, 50.0, 1.0, None, None, None, None, eng._stream())
    assert rc != 0 and "null" in lib.aqg_last_error().decode()
    for bad in (dict(c_visit=-1.0), dict(c_scale=float("nan")), dict(c_visit="x")):
        with pytest.raises(ValueError):
            eng.root_improved_policy(**bad)
    assert _read_out(eng, 0.0, 0.0)[0] == 0


# ------------------------------------------------------------------ 1b. the read-out on real searches
@pytest.fixture(scope="module")
def roots5():
    """Five real positions per board: the opening and a short walk from it."""
    return {N: walked_records(N, 5, seed=N) for N in (3, 5, 9)}


@pytest.mark.parametrize("N", (3, 5, 9))
@pytest.mark.parametrize("sims", (1, 2, 8, 50))
def test_read_out_after_a_fake_search(dev, roots5, N, sims):
    eng = _engine(5, sims, N, fake_bias=1, record_history=False)
    visits, actions, count = eng.search(torch.from_numpy(roots5[N]))
    policy, acts, cnt, vmix = eng.root_improved_policy()
    assert policy.dtype == torch.float32 and tuple(policy.shape) == (5, MAX_LEGAL) and policy.device == eng.dev
    assert tuple(vmix.shape) == (5,) and vmix.dtype == torch.float32
    assert torch.equal(acts, actions) and torch.equal(cnt, count)                    # the layout of search()'s rows
    pools = _pools(eng)
    rc, *got = _read_out(eng)
    assert rc == 0
    assert all(np.array_equal(bits(a.cpu().numpy()), bits(b)) for a, b in zip((policy, acts, cnt, vmix), got))     # the same launch
    _check_rows(pools, got)
    p, c = got[0], got[2]
    for g in range(5):
        assert (p[g, :c[g]] > 0).all() and abs(float(p[g].astype(np.float64).sum()) - 1.0) <= c[g] * 2.0 ** -24
        assert int(visits[g].sum()) == sims - 1
    if sims == 1:                                               # no visit: the priors, within one ulp
        priors = eng.root_priors()[0].cpu().numpy()
        assert pi_close(p, priors)
    if sims == 50 and N == 9:                                   # what the option is for: most children of such a root are unvisited
        assert (np.count_nonzero(visits.cpu().numpy(), axis=1) < c // 2).all() and (np.count_nonzero(p, axis=1) == c).all()
    if N == 5 and sims == 8:                                    # ... and against the paper's formulas on the oracle's own trees
        from oracle import mcts as om, quoridor as oq
        for g, rec in enumerate(roots5[N]):
            state = oq.State(rec)
            root = om.search(om.FakeModel(1), state, sims)
            want, want_v = paper_policy(*oracle_children(root))
            assert pi_close(p[g, :c[g]], np.asarray(want, dtype=np.float32))
            assert vmix_close(got[3][g], np.float32(want_v), c[g], sims - 1)
            vhat = float(pools[g, 0]["w"]) + float(pools[g, 1:1 + c[g]]["w"].sum())
            assert abs(vhat - om.FakeModel(1).predict(state)[1]) <= (c[g] + 1) * sims * 2.0 ** -53


def _gnn(N, dev):
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from oracle import gnn as og
    model = GraphPolicyValueNetwork(6, 128, 3, policy_size(N), board_size=N)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in og.init_params(1, N=N).items()})
    return model.to(dev).eval()


def test_read_out_after_a_gnn_search(dev, roots5):
    N, sims = 9, 8
    eng = _engine(5, sims, N, model=_gnn(N, dev), evaluator="gnn", record_history=False)
    eng.search(torch.from_numpy(roots5[N]))
    pools = _pools(eng)
    rc, *got = _read_out(eng)
    assert rc == 0
    _check_rows(pools, got)
    assert (got[2] > 100).all() and (np.count_nonzero(got[0], axis=1) == got[2]).all() and (np.abs(got[3]) <= 1).all()


def test_read_out_on_kept_roots(dev):
    """With tree reuse a kept root is an inner node of the last search: the same identity gives its own network value."""
    from oracle import mcts as om, quoridor as oq
    N, G, sims = 5, 5, 24
    eng = _engine(G, sims, N, fake_bias=2, tree_reuse=True, seed=4)
    eng.move()
    assert eng.counters()["active"] == G
    kept = eng.t["kept"].cpu().numpy()[:G] != 0
    assert kept.any()
    pools = _pools(eng)
    rc, *got = _read_out(eng)
    assert rc == 0
    _check_rows(pools, got)
    states = eng.root_states72().cpu().numpy()
    for g in np.flatnonzero(kept):
        first, cnt = int(pools[g, 0]["kids"]) & 0xFFFFFF, int(pools[g, 0]["kids"]) >> 24
        assert cnt == got[2][g] > 0
        vhat = float(pools[g, 0]["w"]) + float(pools[g, first:first + cnt]["w"].sum())
        nsum = int(pools[g, first:first + cnt]["n"].sum())
        assert abs(vhat - om.FakeModel(2).predict(oq.State(states[g]))[1]) <= (cnt + 1) * (nsum + 1) * 2.0 ** -53


# ------------------------------------------------------------------ 2. the refresh form, bit for bit
def _to(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _refresh(dev, N, A, policy, actions, count, q, blend, slots, n, capacity, rings, with_z=True):
    from alphaquoridorgnn_amd import _lib
    d = [_to(dev, x) for x in (policy, actions, count, q, slots)]
    r = [_to(dev, x) for x in rings]
    rc = _lib.load().aqg_replay_refresh_policy(N, A, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), blend, _lib.ptr(d[4]), n,
                                               capacity, _lib.ptr(r[1]), _lib.ptr(r[2]) if with_z else None, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in r]


SIZES = (1, 3, 4, 5, 15, 16, 17, 33)            # csrc/replay_refresh.hip: groups of 4 rows per wavefront, 16 rows per workgroup


@pytest.mark.parametrize("N", (3, 5, 7, 9))
def test_refresh_form_equals_the_reference_bit_for_bit(dev, N):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.replay import refresh_policy_reference
    A = policy_size(N)
    for n in SIZES:
        capacity = n + 37
        policy, actions, count, q, slots, kinds = policy_rows(N, n, seed=100 * N + n, capacity=capacity)
        if n > len(POLICY_SPECIAL):
            assert set(POLICY_SPECIAL) <= set(kinds)
        written = policy_written_rows(policy, count, slots, capacity)
        named = slots[written]
        rest = np.setdiff1d(np.arange(capacity), named)
        assert written.any() and len(rest) >= 37
        before = random_rings(N, capacity, seed=7 * N + n)
        for blend in (0.0, 0.25, 1.0):
            want = [x.copy() for x in before]
            refresh_policy_reference(N, policy, actions, count, q, blend, slots, want[1], want[2])
            rc, got = _refresh(dev, N, A, policy, actions, count, q, blend, slots, n, capacity, before)
            assert rc == 0, _lib.load().aqg_last_error()
            for g, w in zip(got, want):
                assert np.array_equal(bits(g), bits(w)), (N, n, blend)
            for g, w in zip(got, expected_refresh_policy(N, policy, actions, count, q, blend, slots, before)):
                assert np.array_equal(bits(g), bits(w)), (N, n, blend)
            assert np.array_equal(got[0], before[0])
            assert np.array_equal(bits(got[1][rest]), bits(before[1][rest])) and np.array_equal(bits(got[2][rest]), bits(before[2][rest]))
            if blend == 0.0:
                assert np.array_equal(bits(got[2]), bits(before[2]))                 # the whole value ring
                for q_, with_z in ((None, True), (None, False), (q, False)):
                    rc, alt = _refresh(dev, N, A, policy, actions, count, q_, 0.0, slots, n, capacity, before, with_z=with_z)
                    assert rc == 0 and all(np.array_equal(bits(a), bits(g)) for a, g in zip(alt, got))
            else:
                assert not np.array_equal(bits(got[2][named]), bits(before[2][named]))


def test_refresh_form_refusals(dev):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, n, capacity = 5, 20, 32
    A = policy_size(N)
    policy, actions, count, q, slots, _ = policy_rows(N, n, seed=1, capacity=capacity)
    before = random_rings(N, capacity, seed=2)

    def refused(match, *, P=policy, Ac=actions, C=count, q_=q, blend=0.5, S=slots, A_=A, n_=n, capacity_=capacity, N_=N, with_z=True):
        rc, got = _refresh(dev, N_, A_, P, Ac, C, q_, blend, S, n_, capacity_, before, with_z=with_z)
        assert rc != 0 and match in lib.aqg_last_error().decode() and "aqg_replay_refresh_policy" in lib.aqg_last_error().decode()
        assert all(np.array_equal(bits(g), bits(b)) for g, b in zip(got, before))

    refused("board_size", N_=4)
    refused("policy_size", A_=policy_size(9))
    refused("negative", n_=-1)
    refused("capacity", capacity_=0)
    refused("blend", blend=-0.25)
    refused("blend", blend=float("nan"))
    refused("search_value", q_=None)
    refused("must be given", P=None)
    refused("must be given", Ac=None)
    refused("must be given", C=None)
    refused("must be given", S=None)
    refused("ring_z", with_z=False)
    rc, got = _refresh(dev, N, A, None, None, None, None, 0.0, None, 0, capacity, before)
    assert rc == 0 and all(np.array_equal(bits(g), bits(b)) for g, b in zip(got, before))
    dP, dA, dC, dq, dS = (_to(dev, x) for x in (policy, actions, count, q, slots))
    _, rpi, rz = (_to(dev, x) for x in before)
    rc = lib.aqg_replay_refresh_policy(N, A, _lib.ptr(dP), _lib.ptr(dA), _lib.ptr(dC), _lib.ptr(dq), 0.5, _lib.ptr(dS), n, 4,
                                       ctypes.c_void_p(dP.view(-1)[5:].data_ptr()), _lib.ptr(rz), _lib.stream_ptr(dev))
    assert rc != 0 and "overlaps" in lib.aqg_last_error().decode()


# ------------------------------------------------------------------ 3. the whole stage
def _played_window(dev, N, sims, games=6, generations=2, capacity=1200):
    from alphaquoridorgnn_amd.replay import ReplayWindow
    w = ReplayWindow(N, max_generations=generations, capacity_rows=capacity, device=dev)
    for k in range(generations):
        eng = _engine(games, sims, N, fake_bias=0, seed=30 + k)
        eng.play_generation()
        w.append_counts(*eng.history_tensors())
    return w


def _rings(w):
    return [x.cpu().numpy().copy() for x in w.tensors()]


@pytest.mark.parametrize("N,sims,blend", [(3, 8, 0.25), (5, 10, 0.0)])
def test_the_stage_equals_the_host_statement(dev, N, sims, blend):
    """Two chunks with a padded last one.  The refreshed rows are the host statement's -- the draw, the oracle's search of every drawn
    record, improved_policy_reference, refresh_policy_reference -- within the tolerance of pi'; every other byte is as it was."""
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.engine import improved_policy_reference
    from alphaquoridorgnn_amd.reanalyse import eligible_rows, reanalyse
    from alphaquoridorgnn_amd.replay import draw_reanalyse_rows, refresh_policy_reference
    from oracle import mcts as om, quoridor as oq
    w = _played_window(dev, N, sims)
    E = eligible_rows(w)
    R, chunk, seed, update, c_visit, c_scale = 7, 4, 5, 1, 50.0, 1.0
    assert E > R and R % chunk and R > chunk
    cached = set(pv_mcts._engines)
    before = _rings(w)
    index = w.index().cpu().numpy()
    done = reanalyse(w, None, R, sims=sims + 2, value_blend=blend, seed=seed, update=update, slots=chunk, evaluator="fake", fake_bias=2,
                     policy_target="completed_q", c_visit=c_visit, c_scale=c_scale)
    assert done == R and set(pv_mcts._engines) <= cached
    got = _rings(w)
    slots = index[draw_reanalyse_rows(seed, update, E, R)].astype(np.int64)
    policy = np.zeros((R, MAX_LEGAL), dtype=np.float32)
    actions = np.full((R, MAX_LEGAL), 0xFF, dtype=np.uint8)
    count, q = np.zeros((R,), dtype=np.int32), np.zeros((R,), dtype=np.float32)
    for i, slot in enumerate(slots):
        state = oq.State(before[0][slot])
        root = om.search(om.FakeModel(2), state, sims + 2)
        legal = list(state.legal_actions())
        count[i], q[i] = len(legal), np.float32(root.w / root.n)
        actions[i, :len(legal)] = legal
        policy[i, :len(legal)] = improved_policy_reference(*oracle_children(root), c_visit, c_scale)[0]
    want = [x.copy() for x in before]
    refresh_policy_reference(N, policy, actions, count, q, blend, slots, want[1], want[2])
    rest = np.setdiff1d(np.arange(before[1].shape[0]), slots)
    assert np.array_equal(got[0], before[0]) and np.array_equal(bits(got[2]), bits(want[2]))         # the blend has no tolerance
    assert all(np.array_equal(bits(g[rest]), bits(b[rest])) for g, b in zip(got, before))
    for i, s in enumerate(slots):
        assert np.array_equal(got[1][s] == 0, want[1][s] == 0) and pi_close(got[1][s], want[1][s]), i
        assert np.count_nonzero(got[1][s]) == count[i]
    # the option did act (a root with a single legal action keeps its target: 1.0 either way)
    assert 2 * sum(not np.array_equal(bits(got[1][s]), bits(before[1][s])) for s in slots) >= R
    # 'visits' on a copy of the same window is the parent's path: normalised counts, with zeros at the unvisited actions
    v = _played_window(dev, N, sims)
    assert reanalyse(v, None, R, sims=sims + 2, value_blend=blend, seed=seed, update=update, slots=chunk, evaluator="fake", fake_bias=2) == R
    vis = _rings(v)
    assert np.array_equal(bits(vis[2]), bits(got[2]))
    if N == 5:                                                  # (every child of a 3x3 root may have a visit)
        assert any(np.count_nonzero(vis[1][s]) < count[i] for i, s in enumerate(slots))


# ------------------------------------------------------------------ 4. the user function
@pytest.mark.parametrize("N", (3, 9))
def test_pv_mcts_improved_policy_batch(dev, roots5, N):
    from alphaquoridorgnn_amd import pv_mcts
    sims, A = 8, policy_size(N)
    dense, vmix = pv_mcts.pv_mcts_improved_policy_batch(None, roots5[N], sims=sims, evaluator="fake", fake_bias=1, c_visit=20.0, c_scale=0.5)
    assert dense.dtype == torch.float32 and tuple(dense.shape) == (5, A) and tuple(vmix.shape) == (5,)
    eng = _engine(5, sims, N, fake_bias=1, record_history=False)
    eng.search(torch.from_numpy(roots5[N]))
    policy, actions, count, want_v = (x.cpu().numpy() for x in eng.root_improved_policy(20.0, 0.5))
    want = np.zeros((5, A), dtype=np.float32)
    for g in range(5):
        want[g, actions[g, :count[g]]] = policy[g, :count[g]]
    assert np.array_equal(bits(dense.cpu().numpy()), bits(want)) and np.array_equal(bits(vmix.cpu().numpy()), bits(want_v))
    assert (np.count_nonzero(want, axis=1) == count).all()


# ------------------------------------------------------------------ 5. self_play() with the module options
_LOOP = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, pv_mcts, self_play as sp
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
from alphaquoridorgnn_amd.reanalyse import reanalyse
from alphaquoridorgnn_amd.replay import ReplayWindow

assert constants.BOARD_SIZE == 3
torch.manual_seed(3)
dev = aqd.device()
model = GraphPolicyValueNetwork(6, 16, 2, 17, board_size=3).to(dev).eval()
pv_mcts.PV_EVALUATE_COUNT = 8
ROWS, SIMS, SLOTS, SEEDS, CV, CS = 11, 12, 4, (17, 18), 20.0, 0.5
bits = lambda x: x.view(np.int32) if x.dtype == np.float32 else x
sp.SP_REANALYSE_SIMS, sp.SP_REANALYSE_SLOTS, sp.SP_REANALYSE_C_VISIT, sp.SP_REANALYSE_C_SCALE = SIMS, SLOTS, CV, CS


def run(rows, target, after=None):
    sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_POLICY_TARGET = rows, target
    w = sp.SP_REPLAY = ReplayWindow(3, max_generations=3, capacity_rows=400, device=dev)
    for update, seed in enumerate(SEEDS):
        os.remove(sp.self_play(model, games=5, seed=seed))
        if after is not None:
            after(w, seed, update)
    return [x.cpu().numpy().copy() for x in w.tensors()]


on = run(ROWS, "completed_q")
alone = run(0, "visits", after=lambda w, seed, update: reanalyse(w, model, ROWS, sims=SIMS, seed=seed, update=update, slots=SLOTS,
                                                                 evaluator="general", policy_target="completed_q", c_visit=CV, c_scale=CS))
visits = run(ROWS, "visits")
print("ON_IS_OFF_THEN_REANALYSE", all(np.array_equal(bits(a), bits(b)) for a, b in zip(on, alone)))
print("ANOTHER_TARGET_THAN_VISITS", np.array_equal(on[0], visits[0]), not np.array_equal(bits(on[1]), bits(visits[1])),
      np.array_equal(bits(on[2]), bits(visits[2])))
print("MORE_NON_ZERO_ENTRIES", np.count_nonzero(on[1]) > np.count_nonzero(visits[1]), bool(np.isfinite(on[1]).all()))
'''


def test_self_play_with_the_completed_q_target(dev, tmp_path):
    """One child process on the 3x3 board: self_play() with SP_REANALYSE_POLICY_TARGET = 'completed_q' is self_play() without the
    option followed by reanalyse(policy_target='completed_q') with the same constants, ring for ring; the progress line names the
    target; with 'visits' the records and the value ring are the same and the policy ring is not."""
    import subprocess
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="3", AQG_EVAL_CACHE_SLOTS="0")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("ON_IS_OFF_THEN_REANALYSE True", "ANOTHER_TARGET_THAN_VISITS True True True", "MORE_NON_ZERO_ENTRIES True True"):
        assert line in r.stdout, (line, r.stdout[-3000:])
    assert "rows at 12 simulations, policy target: completed_q" in r.stdout and "policy target: visits" in r.stdout
