"""Completed-Q policy targets without a GPU (include/aqgnn.h "completed-Q policy targets"): engine.improved_policy_reference against
an independent transcription of the paper's formulas on the oracle's trees, the identity vhat = root.w + sum w_i, the invariants of
the improved policy, replay.refresh_policy_reference's verbatim rows and skips, a host window through the whole stage, the ABI and
every refusal of the options and of train_cycle's parser."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from alphaquoridorgnn_amd.engine import improved_policy_reference, root_improved_policy_reference   # noqa: E402
from alphaquoridorgnn_amd.replay import ReplayWindow, blend_targets, draw_reanalyse_rows, refresh_policy_reference, refresh_reference   # noqa: E402
from tests._improved_policy import (COUNTS, PATTERNS, POLICY_SPECIAL, ULP, OracleEngine, expected_refresh_policy, oracle_children,   # noqa: E402
                                    paper_policy, pi_close, policy_rows, policy_written_rows, synthetic_pool, vmix_bound, vmix_close,
                                    walked_records)
from tests._reanalyse import MAX_LEGAL, bits, policy_size, random_rings   # noqa: E402

SIMS = (1, 2, 8, 50)


@pytest.fixture(scope="module")
def trees():
    """The oracle's search trees the tests share: (N, sims) -> list of (state, root); computed once, never changed."""
    from oracle import mcts as om, quoridor as oq
    out = {}
    for N in (3, 5):
        states = [oq.State(rec) for rec in walked_records(N, 4, seed=N)]
        assert states[0].plies_played == 0
        for sims in SIMS:
            out[N, sims] = [(s, om.search(om.FakeModel(1), s, sims)) for s in states]
    return out


# ------------------------------------------------------------------ the reference against the paper's formulas
@pytest.mark.parametrize("N", (3, 5))
@pytest.mark.parametrize("sims", SIMS)
def test_reference_equals_an_independent_transcription(trees, N, sims):
    for state, root in trees[N, sims]:
        p, n, q, w, root_w = oracle_children(root)
        assert len(p) == len(state.legal_actions()) > 0 and int(n.sum()) == sims - 1
        for c_visit, c_scale in ((50.0, 1.0), (0.0, 1.0), (50.0, 0.1), (10.0, 2.5)):
            got, vmix = improved_policy_reference(p, n, q, w, root_w, c_visit, c_scale)
            want, want_vmix = paper_policy(p, n, q, w, root_w, c_visit, c_scale)
            assert got.dtype == np.float32 and got.shape == p.shape and isinstance(vmix, np.float32)
            assert pi_close(got, np.asarray(want, dtype=np.float32)), (N, sims, c_visit, c_scale)
            assert vmix_close(vmix, np.float32(want_vmix), len(p), int(n.sum()))
            assert abs(float(got.astype(np.float64).sum()) - 1.0) <= len(p) * 2.0 ** -24


@pytest.mark.parametrize("N", (3, 5))
@pytest.mark.parametrize("sims", SIMS)
def test_the_root_network_value_is_recovered_from_the_tree(trees, N, sims):
    from oracle import mcts as om
    for state, root in trees[N, sims]:
        p, n, q, w, root_w = oracle_children(root)
        vhat = root_w + float(w.sum())
        want = om.FakeModel(1).predict(state)[1]
        assert abs(vhat - want) <= (len(p) + 1) * (int(n.sum()) + 1) * 2.0 ** -53, (N, sims, vhat, want)
        assert root.n == sims and want != 0


# ------------------------------------------------------------------ the invariants
@pytest.mark.parametrize("N", (3, 5))
def test_one_simulation_and_zero_scale_give_the_priors(trees, N):
    for sims in SIMS:
        for _, root in trees[N, sims]:
            p, n, q, w, root_w = oracle_children(root)
            if sims == 1:                                       # every completed value is vmix: the transform is a constant shift
                assert not n.any()
                got, vmix = improved_policy_reference(p, n, q, w, root_w)
                assert pi_close(got, p) and vmix == np.float32(root_w)
            got, _ = improved_policy_reference(p, n, q, w, root_w, c_scale=0.0)
            assert pi_close(got, p), (N, sims)


def test_raising_a_visited_childs_value():
    """With every child visited, raising one q raises that entry and lowers every other one.  With unvisited children the mixed value
    rises with it -- by less than the raise, being an average -- so their entries need not fall; what holds for EVERY other entry is
    that it falls relative to the raised one, and every other visited entry falls outright."""
    rng = np.random.RandomState(3)
    for cnt, all_visited in ((5, True), (40, True), (7, False), (136, False)):
        p = rng.dirichlet(np.ones(cnt)).astype(np.float32)
        n = rng.randint(1, 9, cnt).astype(np.int32)
        if not all_visited:
            n[rng.rand(cnt) < 0.5] = 0
            n[0] = 3
        q = np.where(n > 0, rng.uniform(-0.6, 0.6, cnt), 0).astype(np.float32)
        w = -q.astype(np.float64) * n
        j = int(np.flatnonzero(n > 0)[rng.randint(int((n > 0).sum()))])
        before, _ = improved_policy_reference(p, n, q, w, 0.25, c_visit=10.0, c_scale=0.5)
        q2 = q.copy()
        q2[j] += np.float32(0.2)
        after, _ = improved_policy_reference(p, n, q2, w, 0.25, c_visit=10.0, c_scale=0.5)
        others = np.arange(cnt) != j
        assert after[j] > before[j] and (before > 0).all()
        falls = (n > 0) & others if not all_visited else others
        assert (after[falls] < before[falls]).all()
        assert (after[others].astype(np.float64) / after[j] < before[others].astype(np.float64) / before[j]).all()


def test_zero_priors_zero_rows_and_refusals():
    rng = np.random.RandomState(5)
    p = rng.dirichlet(np.ones(20)).astype(np.float32)
    p[[0, 7, 19]] = 0
    p[3] = np.float32("nan")
    n = rng.randint(0, 4, 20).astype(np.int32)
    n[0] = 5                                                    # a visited child without a prior still reads 0
    q = np.where(n > 0, rng.uniform(-1, 1, 20), 0).astype(np.float32)
    got, vmix = improved_policy_reference(p, n, q, -q.astype(np.float64) * n, 0.1)
    assert (bits(got[[0, 3, 7, 19]]) == 0).all() and (got[np.setdiff1d(np.arange(20), [0, 3, 7, 19])] > 0).all()
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= 20 * 2.0 ** -24 and np.isfinite(vmix)
    # no prior above 0, and no child at all: zeros, vmix still the mix / vhat
    got, vmix = improved_policy_reference(np.zeros(4, np.float32), [1, 0, 2, 0], [0.5, 0, -0.5, 0], [-0.5, 0, 1.0, 0], 0.0)
    assert (bits(got) == 0).all() and vmix == np.float32(0.5)                 # PV == 0: vhat
    got, vmix = improved_policy_reference(np.zeros(0, np.float32), [], [], [], -0.375)
    assert got.shape == (0,) and vmix == np.float32(-0.375)
    # PV == 0 with unvisited priors: the unvisited children are completed by vhat
    got, _ = improved_policy_reference(np.array([0, 0.5, 0.5], np.float32), [2, 0, 0], [1.0, 0, 0], [-2.0, 0, 0], 2.25)
    assert got[0] == 0 and got[1] == got[2] == np.float32(0.5)
    for bad in (dict(c_visit=-1.0), dict(c_scale=-0.5), dict(c_visit=float("nan")), dict(c_scale=float("inf")), dict(c_visit=None),
                dict(c_scale="1"), dict(c_visit=True)):
        with pytest.raises(ValueError):
            improved_policy_reference(p, n, q, -q.astype(np.float64) * n, 0.1, **bad)
    with pytest.raises(ValueError):
        improved_policy_reference(p, n[:5], q, -q.astype(np.float64) * n, 0.1)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_synthetic_pools_reference_and_transcription(pattern):
    """The pools the GPU test writes into the engine: the pool-level reference is the transcription on the child block, in the layout
    of the read-out -- and the patterns are what they claim."""
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    cap = 300
    for cnt in COUNTS:
        pool = synthetic_pool(NODE_DTYPE, cap, cnt, pattern, seed=cnt)
        policy, actions, count, vmix = root_improved_policy_reference(pool)
        first = int(pool["kids"][0]) & 0xFFFFFF
        kids = pool[first:first + cnt]
        want, want_vmix = paper_policy(kids["p"], kids["n"], kids["q"], kids["w"], pool["w"][0])
        assert count == cnt and policy.dtype == np.float32 and actions.dtype == np.uint8
        assert pi_close(policy[:cnt], np.asarray(want, dtype=np.float32)) and vmix_close(vmix, np.float32(want_vmix), cnt, int(kids["n"].sum()))
        assert (bits(policy[cnt:]) == 0).all() and (actions[cnt:] == 0xFF).all() and np.array_equal(actions[:cnt], kids["action"])
        if pattern == "zero_prior_visited" and cnt:
            assert not kids["p"][kids["n"] > 0].any() and vmix == np.float32(pool["w"][0] + kids["w"].sum())
        if pattern == "big_n" and cnt > 1:
            assert kids["n"].max() == 32767 and (policy[:cnt] == 0).sum() >= cnt // 2 and policy[:cnt].max() > 0.99
        if pattern == "none_visited" and cnt:
            assert pi_close(policy[:cnt], (kids["p"].astype(np.float64) / kids["p"].astype(np.float64).sum()).astype(np.float32))
    # the guards: a range that leaves the pool, and a count above MAX_LEGAL
    pool = synthetic_pool(NODE_DTYPE, cap, 20, pattern, seed=1, first=cap - 19)
    for bad in (pool, synthetic_pool(NODE_DTYPE, cap, 137, pattern, seed=2, first=5)):
        policy, actions, count, vmix = root_improved_policy_reference(bad)
        assert count == 0 and vmix == 0 and (bits(policy) == 0).all() and (actions == 0xFF).all()
    assert root_improved_policy_reference(synthetic_pool(NODE_DTYPE, cap, 20, pattern, seed=1, first=cap - 20))[2] == 20


# ------------------------------------------------------------------ the refresh form's statement
@pytest.mark.parametrize("N", (3, 5, 7, 9))
@pytest.mark.parametrize("blend", (0.0, 0.25, 1.0))
def test_refresh_policy_reference_is_the_statement(N, blend):
    n, capacity = 40, 77
    policy, actions, count, q, slots, kinds = policy_rows(N, n, seed=10 * N, capacity=capacity)
    assert set(POLICY_SPECIAL) <= set(kinds)
    before = random_rings(N, capacity, seed=N)
    want = expected_refresh_policy(N, policy, actions, count, q, blend, slots, before)
    r72, rpi, rz = (x.copy() for x in before)
    refresh_policy_reference(N, policy, actions, count, q, blend, slots, rpi, rz)
    assert np.array_equal(bits(rpi), bits(want[1])) and np.array_equal(bits(rz), bits(want[2]))
    written = policy_written_rows(policy, count, slots, capacity)
    for kind in ("count0", "zero_row", "slot_above", "slot_below", "count_negative", "count137", "nan_entry", "inf_entry", "negative_entry"):
        assert not written[kinds.index(kind)], kind
    for kind in ("plain", "count1", "count136", "big_action"):
        assert written[kinds.index(kind)], kind
    untouched = np.setdiff1d(np.arange(capacity), slots[written])
    assert np.array_equal(bits(rpi[untouched]), bits(before[1][untouched])) and np.array_equal(bits(rz[untouched]), bits(before[2][untouched]))
    A = policy_size(N)
    for i in np.flatnonzero(written):                           # verbatim: the entry's own bits at its action id, +0.0 elsewhere
        c = int(count[i])
        dense = np.zeros(A, dtype=np.float32)
        inside = actions[i, :c] < A
        dense[actions[i, :c][inside]] = policy[i, :c][inside]
        assert np.array_equal(bits(rpi[slots[i]]), bits(dense))
    assert (bits(rpi[slots[written]]) == np.int32(-2 ** 31)).any()              # a -0.0 went through as it was
    if blend == 0.0:
        assert np.array_equal(bits(rz), bits(before[2]))
    else:
        w = slots[written]
        assert np.array_equal(bits(rz[w]), bits(blend_targets(before[2][w], q[written], blend)))


def test_refresh_policy_reference_refusals():
    N, n, capacity = 5, 12, 20
    policy, actions, count, q, slots, _ = policy_rows(N, n, seed=3, capacity=capacity)
    _, rpi, rz = random_rings(N, capacity, seed=4)
    a, b = rpi.copy(), rpi.copy()
    refresh_policy_reference(N, policy, actions, count, None, 0.0, slots, a, None)
    refresh_policy_reference(N, policy, actions, count, q, 0.0, slots, b, None)
    assert np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(a), bits(rpi))
    bad = [lambda: refresh_policy_reference(4, policy, actions, count, None, 0.0, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy, actions, count, None, 0.5, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy, actions, count, q, 1.5, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy, actions, count, q, float("nan"), slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy, actions, count, q, 0.5, slots, rpi, None),
           lambda: refresh_policy_reference(N, np.zeros(policy.shape, np.float64), actions, count, q, 0.5, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy.view(np.int32), actions, count, q, 0.5, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy[:, :100], actions, count, q, 0.5, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy, actions.astype(np.int8), count, q, 0.5, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy, actions, count[:5], q, 0.5, slots, rpi, rz),
           lambda: refresh_policy_reference(N, policy, actions, count, q, 0.5, slots.astype(np.int32), rpi, rz),
           lambda: refresh_policy_reference(9, policy, actions, count, q, 0.5, slots, rpi, rz)]
    keep = rpi.copy(), rz.copy()
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(bits(rpi), bits(keep[0])) and np.array_equal(bits(rz), bits(keep[1]))


# ------------------------------------------------------------------ the window on the host
def _host_window(N, sizes=(9, 8, 6)):
    """A host window of real positions: three generations of walked records with one-hot targets."""
    w = ReplayWindow(N, max_generations=3, capacity_rows=40)
    A = policy_size(N)
    for k, m in enumerate(sizes):
        S = walked_records(N, m, seed=50 + k)
        V = np.zeros((m, A), dtype=np.int16)
        V[np.arange(m), np.arange(m) % A] = 1
        w.append_counts(torch.from_numpy(S), torch.from_numpy(V), torch.from_numpy(np.ones(m, dtype=np.int8)))
    return w


def _held(w):
    return [x.numpy().copy() for x in w.tensors()]


def test_host_window_refresh_policy_and_its_refusals():
    N = 5
    w = _host_window(N)
    index = w.index().numpy()
    policy, actions, count, q, _, kinds = policy_rows(N, 14, seed=8, capacity=40)
    slots = index[[0, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 20, 22]].astype(np.int64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))   # noqa: E731
    before = _held(w)
    w.refresh_policy(t(slots), t(policy), t(actions), t(count), search_value=t(q), value_blend=0.25)
    want = expected_refresh_policy(N, policy, actions, count, q, 0.25, slots, before)
    got = _held(w)
    assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(got, want)) and np.array_equal(got[0], before[0])
    assert not np.array_equal(bits(got[1]), bits(before[1])) and not np.array_equal(bits(got[2]), bits(before[2]))
    w.refresh_policy(t(slots), t(policy), t(actions), t(count))
    w.refresh_policy(t(slots[:0]), t(policy[:0]), t(actions[:0]), t(count[:0]))
    assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(_held(w), got))
    stale = np.setdiff1d(np.arange(40), index)
    bad = [lambda: w.refresh_policy(t(np.r_[stale[:1], slots[1:]]), t(policy), t(actions), t(count)),
           lambda: w.refresh_policy(t(np.r_[slots[1:2], slots[1:]]), t(policy), t(actions), t(count)),
           lambda: w.refresh_policy(t(np.r_[[40], slots[1:]]), t(policy), t(actions), t(count)),
           lambda: w.refresh_policy(t(slots), t(policy.view(np.int32)), t(actions), t(count)),             # visit rows are not policy rows
           lambda: w.refresh_policy(t(slots), t(np.zeros(policy.shape, np.float64)), t(actions), t(count)),
           lambda: w.refresh_policy(t(slots), t(policy[:, :100]), t(actions), t(count)),
           lambda: w.refresh_policy(t(slots), t(policy), t(actions[:3]), t(count)),
           lambda: w.refresh_policy(t(slots), t(policy), t(actions), t(count.astype(np.int64))),
           lambda: w.refresh_policy(t(slots), t(policy), t(actions), t(count), value_blend=0.5),
           lambda: w.refresh_policy(t(slots), t(policy), t(actions), t(count), search_value=t(q), value_blend=1.5),
           lambda: w.refresh_counts(t(slots), t(policy), t(actions), t(count))]                            # ... and the other way round
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(_held(w), got)), k
    with pytest.raises(ValueError):
        ReplayWindow(N, max_generations=2, capacity_rows=8).refresh_policy(t(slots), t(policy), t(actions), t(count))


@pytest.mark.parametrize("N,blend", [(3, 0.0), (5, 0.25)])
def test_the_stage_on_a_host_window(monkeypatch, N, blend):
    """reanalyse() on a host window with the oracle for the engine: policy_target='completed_q' is the draw, the oracle's search of
    every drawn record, improved_policy_reference and refresh_policy_reference on a copy; 'visits' is what it was."""
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.reanalyse import eligible_rows, reanalyse
    from oracle import mcts as om, quoridor as oq
    sims, R, chunk, seed, update, bias = 8, 11, 4, 5, 2, 2
    built = []
    monkeypatch.setattr(pv_mcts, "_engine_for", lambda model, G, s, n, ev, fb: built.append(OracleEngine(n, G, s, fb)) or built[-1])
    base = _host_window(N)
    E = eligible_rows(base)
    assert E == 17 > R and R % chunk
    before = _held(base)
    index = base.index().numpy()
    slots = index[draw_reanalyse_rows(seed, update, E, R)].astype(np.int64)
    roots = [om.search(om.FakeModel(bias), oq.State(before[0][s]), sims) for s in slots]
    actions = np.full((R, MAX_LEGAL), 0xFF, dtype=np.uint8)
    visits, policy = np.zeros((R, MAX_LEGAL), dtype=np.int32), np.zeros((R, MAX_LEGAL), dtype=np.float32)
    count, q = np.zeros((R,), dtype=np.int32), np.zeros((R,), dtype=np.float32)
    for i, root in enumerate(roots):
        legal = list(root.state.legal_actions())
        count[i], q[i] = len(legal), np.float32(root.w / root.n)
        visits[i, :len(legal)], actions[i, :len(legal)] = [c.n for c in root.children], legal
        policy[i, :len(legal)] = improved_policy_reference(*oracle_children(root), 25.0, 0.5)[0]
    kw = dict(sims=sims, value_blend=blend, seed=seed, update=update, slots=chunk, evaluator="fake", fake_bias=bias)
    for target, name in (("completed_q", "completed_q"), ("completed-q", "completed_q"), ("visits", "visits")):
        w = _host_window(N)
        del built[:]
        extra = dict(policy_target=target, c_visit=25.0, c_scale=0.5) if name == "completed_q" else dict(policy_target=target)
        assert reanalyse(w, None, R, **kw, **extra) == R
        assert len(built) == 1 and (built[0].G, built[0].sims, built[0].searches) == (chunk, sims, 3)       # two chunks and a padded one
        want = [x.copy() for x in before]
        if name == "completed_q":
            refresh_policy_reference(N, policy, actions, count, q, blend, slots, want[1], want[2])
        else:
            refresh_reference(N, visits, actions, count, q, blend, slots, want[1], want[2])
        got = _held(w)
        assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(got, want)), target
        assert not np.array_equal(bits(got[1]), bits(before[1])) and np.array_equal(got[0], before[0])
        if name == "completed_q":                               # non-zero on every legal action, unlike the visit rows
            filled = [np.count_nonzero(got[1][s]) for s in slots]
            assert filled == count.tolist() and (count > np.count_nonzero(visits, axis=1)).any()
    # the default is 'visits'
    w = _host_window(N)
    assert reanalyse(w, None, R, **kw) == R
    want = [x.copy() for x in before]
    refresh_reference(N, visits, actions, count, q, blend, slots, want[1], want[2])
    assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(_held(w), want))


# ------------------------------------------------------------------ options, ABI, flags
def test_option_refusals():
    from alphaquoridorgnn_amd.reanalyse import check_reanalyse_options, reanalyse
    from alphaquoridorgnn_amd.selfplay_options import check_completed_q, check_policy_target
    assert check_policy_target() == ("visits", 50.0, 1.0) and check_policy_target("completed-q", 0, 0) == ("completed_q", 0.0, 0.0)
    assert check_completed_q(np.float32(2.5), 3) == (2.5, 3.0)
    assert check_reanalyse_options(5, 3, 0.5, 7, "completed_q", 10.0, 0.25) == (5, 3, 0.5, 7) == check_reanalyse_options(5, 3, 0.5, 7)
    for bad in (dict(policy_target="q"), dict(policy_target=None), dict(policy_target=1), dict(c_visit=-1e-9), dict(c_scale=-1.0),
                dict(c_visit=float("nan")), dict(c_scale=float("nan")), dict(c_visit=float("inf")), dict(c_scale=float("-inf")),
                dict(c_visit="50"), dict(c_scale=None)):
        with pytest.raises(ValueError):
            check_policy_target(**bad)
        with pytest.raises(ValueError):
            check_reanalyse_options(1, **bad)
        with pytest.raises(ValueError):                         # refused even where a pass would have nothing to do
            reanalyse(ReplayWindow(5, max_generations=3, capacity_rows=40), None, 4, evaluator="fake", **bad)
    from alphaquoridorgnn_amd import pv_mcts
    for bad in (dict(c_visit=-1.0), dict(c_scale=float("nan"))):
        with pytest.raises(ValueError):                         # before an engine is looked for
            pv_mcts.pv_mcts_improved_policy_batch(None, np.zeros((1, 72), np.uint8), evaluator="fake", **bad)


def test_abi_binding_and_build_list():
    from alphaquoridorgnn_amd import _lib
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    assert re.search(r"\bint\s+aqg_engine_root_improved_policy\s*\(", header) and re.search(r"\bint\s+aqg_replay_refresh_policy\s*\(", header)
    assert "completed-Q policy targets" in header
    res, args = _lib.SIGNATURES["aqg_engine_root_improved_policy"]
    assert res is _lib._c.c_int and len(args) == 8 and args[1] is args[2] is _lib._c.c_double
    res, args = _lib.SIGNATURES["aqg_replay_refresh_policy"]
    assert res is _lib._c.c_int and args == _lib.SIGNATURES["aqg_replay_refresh"][1]
    build = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "build.sh")).read()
    assert re.search(r"\bmcts_improve\b", build)
    src = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "mcts_improve.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in code and "__FAST_MATH__" in code
    assert "__shared__" not in code and "atomic" not in code and "__syncthreads" not in code


def test_defaults_and_train_cycle_flags(monkeypatch):
    from alphaquoridorgnn_amd import distributed as aqd, self_play as sp, train_cycle as tc
    assert (sp.SP_REANALYSE_POLICY_TARGET, sp.SP_REANALYSE_C_VISIT, sp.SP_REANALYSE_C_SCALE) == ("visits", 50.0, 1.0)
    args = tc._parser().parse_args([])
    assert (args.reanalyse_policy_target, args.reanalyse_c_visit, args.reanalyse_c_scale) == (None, None, None)
    assert tc._check_reanalyse_policy_args(args) is None
    for name in ("SP_REANALYSE_ROWS", "SP_REANALYSE_SIMS", "SP_REANALYSE_VALUE_BLEND", "SP_REANALYSE_POLICY_TARGET", "SP_REANALYSE_C_VISIT",
                 "SP_REANALYSE_C_SCALE"):
        monkeypatch.setattr(sp, name, getattr(sp, name))        # restored after the test
    tc._set_reanalyse_options(args)
    assert (sp.SP_REANALYSE_POLICY_TARGET, sp.SP_REANALYSE_C_VISIT, sp.SP_REANALYSE_C_SCALE) == ("visits", 50.0, 1.0)
    ok = ["--replay-generations", "3", "--reanalyse-rows", "4000", "--reanalyse-policy-target", "completed-q"]
    assert tc._check_reanalyse_policy_args(tc._parser().parse_args(ok)) == ("completed_q", 50.0, 1.0)
    more = ok + ["--reanalyse-c-visit", "25", "--reanalyse-c-scale", "0.1"]
    assert tc._check_reanalyse_policy_args(tc._parser().parse_args(more)) == ("completed_q", 25.0, 0.1)
    assert tc._check_reanalyse_policy_args(tc._parser().parse_args(ok[:4] + ["--reanalyse-c-visit", "0"])) == ("visits", 0.0, 1.0)
    tc._set_reanalyse_options(tc._parser().parse_args(more))
    assert (sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_POLICY_TARGET, sp.SP_REANALYSE_C_VISIT, sp.SP_REANALYSE_C_SCALE) == (4000, "completed_q", 25.0, 0.1)

    def reached(*a, **k):
        raise AssertionError("main() went past the flag checks")
    monkeypatch.setattr(aqd, "init_from_env", reached)
    window = ["--replay-generations", "3"]
    for bad in (window + ["--reanalyse-policy-target", "completed-q"],                             # the dependent flags alone
                window + ["--reanalyse-c-visit", "10"],
                window + ["--reanalyse-c-scale", "0.5"],
                window + ["--reanalyse-rows", "100", "--reanalyse-c-visit", "-1"],
                window + ["--reanalyse-rows", "100", "--reanalyse-c-scale", "-0.5"],
                window + ["--reanalyse-rows", "100", "--reanalyse-c-visit", "nan"],
                window + ["--reanalyse-rows", "100", "--reanalyse-c-scale", "inf"]):
        with pytest.raises(ValueError, match="reanalyse"):
            tc.main(bad)
    with pytest.raises(SystemExit):                             # not one of the two spellings: the parser's own refusal
        tc._parser().parse_args(window + ["--reanalyse-rows", "100", "--reanalyse-policy-target", "gumbel"])
    assert (sp.SP_REANALYSE_POLICY_TARGET, sp.SP_REANALYSE_C_VISIT, sp.SP_REANALYSE_C_SCALE) == ("completed_q", 25.0, 0.1)


def test_self_play_refuses_bad_policy_target_options(monkeypatch):
    from alphaquoridorgnn_amd import self_play as sp
    monkeypatch.setattr(sp, "SP_REANALYSE_POLICY_TARGET", "gumbel")
    with pytest.raises(ValueError, match="policy_target"):
        sp.self_play(model=object(), games=1, seed=1)
    monkeypatch.setattr(sp, "SP_REANALYSE_POLICY_TARGET", "completed_q")
    monkeypatch.setattr(sp, "SP_REANALYSE_C_SCALE", -1.0)
    with pytest.raises(ValueError, match="c_scale"):
        sp.self_play(model=object(), games=1, seed=1)
