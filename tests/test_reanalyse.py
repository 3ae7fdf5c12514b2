"""Reanalyse on the GPU (include/aqgnn.h "reanalyse"; csrc/replay_refresh.hip, csrc/mcts_move.hip engine_root_values_kernel,
reanalyse.py): the refresh launch bit for bit against replay.refresh_reference at every edge, with everything it does not name
untouched; the C entry's refusals; the root value read-out against a played move's recorded value and the oracle's PV-MCTS; the whole
stage against a host statement (the draw, the oracle's search per row, refresh_reference); a fresh search of a recorded position is
the search that recorded it; the network evaluators; and self_play() with the option on and off."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests._reanalyse import (MAX_LEGAL, SPECIAL, bits, expected_refresh, policy_size, random_rings, search_rows,   # noqa: E402
                              written_rows)

pytestmark = pytest.mark.gpu

# csrc/replay_refresh.hip: RFR_ROWS = 16 source rows per workgroup; one row, one below / at / one above one and four workgroups
SIZES = (1, 15, 16, 17, 63, 64, 65)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def test_the_sizes_are_the_kernels():
    src = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "replay_refresh.hip")).read()
    assert "RFR_GROUP = 4" in src and "RFR_WAVES = 4" in src and "RFR_ROWS = RFR_WAVES * RFR_GROUP" in src


def _to(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _call(dev, N, A, visits, actions, count, q, blend, slots, n, capacity, rings, with_z=True):
    """The C entry on device copies; (rc, the three rings back on the host -- the record ring is no argument, it rides along)."""
    from alphaquoridorgnn_amd import _lib
    d = [_to(dev, x) for x in (visits, actions, count, q, slots)]
    r = [_to(dev, x) for x in rings]
    rc = _lib.load().aqg_replay_refresh(N, A, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), blend, _lib.ptr(d[4]), n,
                                        capacity, _lib.ptr(r[1]), _lib.ptr(r[2]) if with_z else None, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in r]


# ------------------------------------------------------------------ 1. the launch against its statement
@pytest.mark.parametrize("N", (3, 5, 7, 9))
def test_kernel_equals_the_reference_bit_for_bit(dev, N):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.replay import refresh_reference
    A = policy_size(N)
    for n in SIZES:
        capacity = n + 37
        visits, actions, count, q, slots, kinds = search_rows(N, n, seed=100 * N + n, capacity=capacity)
        if n > 1:
            assert set(SPECIAL) <= set(kinds) and 0 in slots and capacity - 1 in slots
        written = written_rows(N, visits, count, slots, capacity)
        named = slots[written]
        rest = np.setdiff1d(np.arange(capacity), named)
        assert written.any() and len(rest) >= 37
        before = random_rings(N, capacity, seed=7 * N + n)
        for blend in (0.0, 0.25, 1.0):
            want = [x.copy() for x in before]
            refresh_reference(N, visits, actions, count, q, blend, slots, want[1], want[2])
            rc, got = _call(dev, N, A, visits, actions, count, q, blend, slots, n, capacity, before)
            assert rc == 0, _lib.load().aqg_last_error()
            for g, w in zip(got, want):
                assert np.array_equal(bits(g), bits(w)), (N, n, blend)
            for g, w in zip(got, expected_refresh(N, visits, actions, count, q, blend, slots, before)):
                assert np.array_equal(bits(g), bits(w)), (N, n, blend)
            assert np.array_equal(got[0], before[0])                                     # the records
            assert np.array_equal(bits(got[1][rest]), bits(before[1][rest])) and np.array_equal(bits(got[2][rest]), bits(before[2][rest]))
            assert not np.array_equal(bits(got[1][named]), bits(before[1][named]))
            if blend == 0.0:
                assert np.array_equal(bits(got[2]), bits(before[2]))
                # without search_value, and without a value ring at all: the same policy ring
                for q_, with_z in ((None, True), (None, False), (q, False)):
                    rc, alt = _call(dev, N, A, visits, actions, count, q_, 0.0, slots, n, capacity, before, with_z=with_z)
                    assert rc == 0 and all(np.array_equal(bits(a), bits(g)) for a, g in zip(alt, got))
            else:
                assert not np.array_equal(bits(got[2][named]), bits(before[2][named]))


def test_c_entry_refusals(dev):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, n, capacity = 5, 20, 32
    A = policy_size(N)
    visits, actions, count, q, slots, _ = search_rows(N, n, seed=1, capacity=capacity)
    before = random_rings(N, capacity, seed=2)

    def refused(match, *, V=visits, Ac=actions, C=count, q_=q, blend=0.5, S=slots, A_=A, n_=n, capacity_=capacity, N_=N, with_z=True):
        rc, got = _call(dev, N_, A_, V, Ac, C, q_, blend, S, n_, capacity_, before, with_z=with_z)
        assert rc != 0 and match in lib.aqg_last_error().decode(), (match, lib.aqg_last_error())
        assert all(np.array_equal(bits(g), bits(b)) for g, b in zip(got, before))          # the rings are as they were

    refused("board_size", N_=4)
    refused("policy_size", A_=policy_size(9))
    refused("negative", n_=-1)
    refused("capacity", capacity_=0)
    refused("blend", blend=-0.25)
    refused("blend", blend=1.25)
    refused("blend", blend=float("nan"))
    refused("search_value", q_=None)
    refused("must be given", V=None)
    refused("must be given", Ac=None)
    refused("must be given", C=None)
    refused("must be given", S=None)
    refused("ring_z", with_z=False)
    rc, got = _call(dev, N, A, None, None, None, None, 0.0, None, 0, capacity, before)
    assert rc == 0 and all(np.array_equal(bits(g), bits(b)) for g, b in zip(got, before))      # n == 0: no pointer is looked at
    # ring_pi NULL, and a ring that overlaps a source: the value ring IS search_value; the policy ring begins inside the visit rows
    st = _lib.stream_ptr(dev)
    dV, dA, dC, dq, dS = (_to(dev, x) for x in (visits, actions, count, q, slots))
    _, rpi, rz = (_to(dev, x) for x in before)
    tail = dV.view(-1)[5:].view(torch.float32)
    calls = (("must be given", (dq, None, rz)), ("overlaps", (rz[:n], rpi, rz)), ("overlaps", (dq, tail, rz)),
             ("overlaps", (dq, rpi, rpi.view(-1)[3:])))
    for match, (value, ring_pi, ring_z) in calls:
        rc = lib.aqg_replay_refresh(N, A, _lib.ptr(dV), _lib.ptr(dA), _lib.ptr(dC), ctypes.c_void_p(value.data_ptr()), 0.5, _lib.ptr(dS), n,
                                    capacity if ring_pi is not tail else 4, None if ring_pi is None else ctypes.c_void_p(ring_pi.data_ptr()),
                                    ctypes.c_void_p(ring_z.data_ptr()), st)
        assert rc != 0 and match in lib.aqg_last_error().decode(), (match, lib.aqg_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(dV.cpu().numpy(), visits) and np.array_equal(bits(rpi.cpu().numpy()), bits(before[1]))
    assert np.array_equal(bits(rz.cpu().numpy()), bits(before[2]))


# ------------------------------------------------------------------ 2. the root value read-out
def _engine(G, sims, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("evaluator", "fake")
    return BatchedSelfPlay(kw.pop("model", None), num_games=G, sims=sims, board_size=N, **kw)


@pytest.mark.parametrize("N,sims,moves", [(3, 8, 1), (5, 16, 2)])          # a 3x3 game can end with its second ply
@pytest.mark.parametrize("G", (1, 4, 5))
def test_root_values(dev, N, sims, moves, G):
    from alphaquoridorgnn_amd import _lib
    from oracle import mcts as om, quoridor as oq
    played = _engine(G, sims, N, fake_bias=2, seed=3 + G, record_search_value=True)
    for _ in range(moves):
        played.move()
    assert played.counters()["active"] == G
    roots = played.root_states72().clone()
    plies = played.t["game_plies"].cpu().numpy()
    played.move()                                                 # the move from `roots`: its hist_value row is the root's w / n
    recorded = np.array([played.t["hist_value"][g, plies[g]].item() for g in range(G)], dtype=np.float32)
    eng = _engine(G, sims, N, fake_bias=2, record_history=False)
    visits, actions, count = eng.search(roots)
    got = eng.root_values()
    assert got.dtype == torch.float32 and tuple(got.shape) == (G,) and got.device == eng.dev
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(recorded))
    want = []
    for g, rec in enumerate(roots.cpu().numpy()):
        root = om.search(om.FakeModel(2), oq.State(rec), sims)
        assert [c.n for c in root.children] == visits[g, :int(count[g])].tolist()
        want.append(np.float32(root.w / root.n))
    assert np.array_equal(bits(got), bits(np.asarray(want, dtype=np.float32)))
    assert (got != 0).any() and (np.abs(got) <= 1).all()
    for e_, v_ in ((None, got), (eng.e, None)):                   # a NULL argument is refused before any launch
        rc = _lib.load().aqg_engine_root_values(None if e_ is None else ctypes.byref(e_), None if v_ is None else _lib.ptr(eng.root_values()),
                                                eng._stream())
        assert rc != 0 and "null" in _lib.load().aqg_last_error().decode()
    fresh = _engine(G, sims, N, record_history=False)             # a root without a visit reads 0
    fresh.reset()
    _lib.check(fresh.lib.aqg_engine_begin_move(ctypes.byref(fresh.e), fresh._stream()), "aqg_engine_begin_move")
    assert (fresh.root_values().cpu().numpy() == 0).all()


# ------------------------------------------------------------------ 3. the whole stage
def _played_window(dev, N, sims, bias, games=4, generations=3, capacity=1500, host=False):
    """A window of `generations` small generations played with the fake evaluator, appended as the engine leaves them."""
    from alphaquoridorgnn_amd.replay import ReplayWindow
    w = ReplayWindow(N, max_generations=generations, capacity_rows=capacity, device=None if host else dev)
    for k in range(generations):
        eng = _engine(games, sims, N, fake_bias=bias, seed=20 + k)
        eng.play_generation()
        w.append_counts(*eng.history_tensors())
    assert len(w.generations) == generations
    return w


def _rings(w):
    return [x.cpu().numpy().copy() for x in w.tensors()]


@pytest.mark.parametrize("N,sims,blend", [(3, 8, 0.25), (5, 12, 0.0), (5, 12, 1.0)])
def test_the_stage_equals_the_host_statement(dev, N, sims, blend):
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.reanalyse import eligible_rows, reanalyse
    from alphaquoridorgnn_amd.replay import draw_reanalyse_rows, refresh_reference
    from oracle import mcts as om, quoridor as oq
    w = _played_window(dev, N, sims, bias=0)
    E = eligible_rows(w)
    R, chunk, seed, update = 17, 7, 5, 2
    assert E == len(w) - w.generations[-1] and E > R and R % chunk
    cached = set(pv_mcts._engines)
    before = _rings(w)
    index = w.index().cpu().numpy()
    done = reanalyse(w, None, R, sims=sims + 4, value_blend=blend, seed=seed, update=update, slots=chunk, evaluator="fake", fake_bias=2)
    assert done == R and set(pv_mcts._engines) <= cached           # ... and the search engine is gone
    got = _rings(w)
    # the host statement: the draw, the oracle's search of every chosen record, refresh_reference on a host copy
    positions = draw_reanalyse_rows(seed, update, E, R)
    slots = index[positions].astype(np.int64)
    visits = np.zeros((R, MAX_LEGAL), dtype=np.int32)
    actions = np.full((R, MAX_LEGAL), 0xFF, dtype=np.uint8)
    count, q = np.zeros((R,), dtype=np.int32), np.zeros((R,), dtype=np.float32)
    for i, slot in enumerate(slots):
        state = oq.State(before[0][slot])
        root = om.search(om.FakeModel(2), state, sims + 4)
        legal = list(state.legal_actions())
        count[i] = len(legal)
        visits[i, :len(legal)], actions[i, :len(legal)] = [c.n for c in root.children], legal
        q[i] = np.float32(root.w / root.n)
    want = [x.copy() for x in before]
    refresh_reference(N, visits, actions, count, q, blend, slots, want[1], want[2])
    for g, x in zip(got, want):
        assert np.array_equal(bits(g), bits(x))
    newest = index[E:]
    assert len(newest) == w.generations[-1] and all(np.array_equal(bits(g[newest]), bits(b[newest])) for g, b in zip(got, before))
    rest = np.setdiff1d(np.arange(before[1].shape[0]), slots)
    assert all(np.array_equal(bits(g[rest]), bits(b[rest])) for g, b in zip(got, before)) and np.array_equal(got[0], before[0])
    # the option did act: at least half of the refreshed rows hold other targets than before
    changed = sum(not np.array_equal(bits(got[1][s]), bits(before[1][s])) for s in slots)
    assert 2 * changed >= R, changed
    if blend:
        assert 2 * sum(bits(got[2])[s] != bits(before[2])[s] for s in slots) >= R
    else:
        assert np.array_equal(bits(got[2]), bits(before[2]))
    # the bookkeeping did not move; a second pass with another update draws other rows
    assert np.array_equal(w.index().cpu().numpy(), index)
    assert not np.array_equal(draw_reanalyse_rows(seed, update + 1, E, R), positions)


@pytest.mark.parametrize("N,sims", [(3, 8), (5, 12)])
def test_a_fresh_search_of_a_recorded_position_is_the_search_that_recorded_it(dev, N, sims):
    from alphaquoridorgnn_amd.reanalyse import eligible_rows, reanalyse
    w = _played_window(dev, N, sims, bias=1)
    before = _rings(w)
    E = eligible_rows(w)
    assert reanalyse(w, None, 10 ** 6, sims=sims, value_blend=0.0, evaluator="fake", fake_bias=1, slots=16) == E > 16
    for g, b in zip(_rings(w), before):
        assert np.array_equal(bits(g), bits(b))
    # ... and it was a search: another simulation count leaves other targets
    assert reanalyse(w, None, 10 ** 6, sims=sims + 3, value_blend=0.0, evaluator="fake", fake_bias=1, slots=16) == E
    assert not np.array_equal(bits(_rings(w)[1]), bits(before[1]))


def test_a_host_window_is_refreshed_like_a_device_window(dev):
    from alphaquoridorgnn_amd.reanalyse import reanalyse
    N, sims = 3, 8
    g, h = _played_window(dev, N, sims, bias=0), _played_window(dev, N, sims, bias=0, host=True)
    kw = dict(sims=sims, value_blend=0.5, seed=9, update=1, slots=5, evaluator="fake", fake_bias=2)
    assert reanalyse(g, None, 13, **kw) == reanalyse(h, None, 13, **kw) == 13
    for a, b in zip(_rings(g), _rings(h)):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ 4. the network evaluators
def _copy_of(w, dev):
    from alphaquoridorgnn_amd.replay import ReplayWindow
    c = ReplayWindow(w.board_size, max_generations=w.max_generations, capacity_rows=w.capacity, device=dev)
    c._rings = tuple(x.clone() for x in w.tensors())
    c._generations, c._start, c._valid, c._index = list(w._generations), w._start, w._valid, w._index.clone()
    return c


def test_gnn_with_and_without_the_evaluation_cache(dev, monkeypatch):
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.reanalyse import reanalyse
    from oracle import gnn as og
    N, sims = 5, 16
    model = GraphPolicyValueNetwork(6, 128, 3, policy_size(N), board_size=N)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in og.init_params(1, N=N).items()})
    model = model.to(dev).eval()
    base = _played_window(dev, N, 8, bias=0, games=3)
    before = _rings(base)
    seen = []
    plain = pv_mcts._engine_for
    monkeypatch.setattr(pv_mcts, "_engine_for", lambda *a, **k: seen.append(plain(*a, **k)) or seen[-1])
    rings = []
    for cache in ("0", "64"):
        monkeypatch.setenv("AQG_EVAL_CACHE_SLOTS", cache)
        w = _copy_of(base, dev)
        assert reanalyse(w, model, 20, sims=sims, value_blend=0.25, seed=1, slots=16) == 20
        rings.append(_rings(w))
    assert [e.eval_cache_slots for e in seen] == [0, 64] and all(e.evaluator == "gnn" for e in seen)
    for a, b in zip(*rings):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(bits(rings[0][1]), bits(before[1])) and not np.array_equal(bits(rings[0][2]), bits(before[2]))
    assert np.array_equal(rings[0][0], before[0]) and np.isfinite(rings[0][1]).all()


@pytest.mark.parametrize("kind", ["general", "cnn"])
def test_the_other_network_evaluators(dev, kind, monkeypatch):
    from alphaquoridorgnn_amd import pv_mcts
    from alphaquoridorgnn_amd.reanalyse import eligible_rows, reanalyse
    from tests.test_root_noise import _net
    N, sims = 5, 8
    model = _net(kind, N, dev)
    w = _played_window(dev, N, 8, bias=0, games=3)
    before = _rings(w)
    index, E = w.index().cpu().numpy(), eligible_rows(w)
    seen = []
    plain = pv_mcts._engine_for
    monkeypatch.setattr(pv_mcts, "_engine_for", lambda *a, **k: seen.append(plain(*a, **k)) or seen[-1])
    assert reanalyse(w, model, 12, sims=sims, seed=2, slots=8) == 12                       # the evaluator follows the model
    assert [e.evaluator for e in seen] == [kind]
    got = _rings(w)
    # what the engine's own search of those records gives, through the reference
    from alphaquoridorgnn_amd.replay import draw_reanalyse_rows, refresh_reference
    slots = index[draw_reanalyse_rows(2, 0, E, 12)].astype(np.int64)
    eng = _engine(12, sims, N, model=model, evaluator=kind, record_history=False)
    visits, actions, count = (x.cpu().numpy() for x in eng.search(torch.from_numpy(before[0][slots])))
    want = [x.copy() for x in before]
    refresh_reference(N, visits, actions, count, None, 0.0, slots, want[1], None)
    for g, x in zip(got, want):
        assert np.array_equal(bits(g), bits(x))
    assert not np.array_equal(bits(got[1]), bits(before[1]))


# ------------------------------------------------------------------ 5. self_play() end to end
_LOOP = r'''
import os, pickle, sys
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
ROWS, SIMS, BLEND, SLOTS, SEEDS = 11, 12, 0.25, 4, (17, 18)
bits = lambda x: x.view(np.int32) if x.dtype == np.float32 else x

built = []
plain = pv_mcts._engine_for
pv_mcts._engine_for = lambda *a, **k: built.append(plain(*a, **k)) or built[-1]


def run(on, after=None):
    """Two self_play() calls into a fresh window; (the rings, each call's file, what each call printed about the pass)."""
    sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_SIMS, sp.SP_REANALYSE_VALUE_BLEND, sp.SP_REANALYSE_SLOTS = (ROWS, SIMS, BLEND, SLOTS) if on else (0, None, 0.0, 2048)
    w = sp.SP_REPLAY = ReplayWindow(3, max_generations=3, capacity_rows=400, device=dev)
    files = []
    for update, seed in enumerate(SEEDS):
        path = sp.self_play(model, games=5, seed=seed)
        with open(path, "rb") as f:
            files.append(pickle.load(f))
        os.remove(path)
        if after is not None:
            after(w, seed, update)
    return [x.cpu().numpy().copy() for x in w.tensors()], files, w


off_rings, off_files, off_w = run(False)
print("OFF_BUILDS_NO_SEARCH_ENGINE", not built, off_w.reanalyse_updates == 0)
on_rings, on_files, on_w = run(True)
print("ON_BUILT_ONE_ENGINE", len(built) == 1, built[0].G == SLOTS and built[0].sims == SIMS and built[0].evaluator == "general",
      not pv_mcts._engines, on_w.reanalyse_updates == 2)
passes = []
alone_rings, alone_files, _ = run(False, after=lambda w, seed, update: passes.append(
    reanalyse(w, model, ROWS, sims=SIMS, value_blend=BLEND, seed=seed, update=update, slots=SLOTS, evaluator="general")))
print("PASSES", passes[0] == 0 and passes[1] == min(ROWS, len(off_files[0])), len(off_files[0]) > ROWS)
print("ON_IS_OFF_THEN_REANALYSE", all(np.array_equal(bits(a), bits(b)) for a, b in zip(on_rings, alone_rings)))
print("THE_OPTION_ACTED", np.array_equal(on_rings[0], off_rings[0]), not np.array_equal(bits(on_rings[1]), bits(off_rings[1])),
      not np.array_equal(bits(on_rings[2]), bits(off_rings[2])))
print("FILES_ARE_THE_OPTION_OFFS", on_files == off_files, alone_files == off_files)
# off: the ring holds the rows of the files, as it always did
p = torch.tensor(np.array([r[1] for h in off_files for r in h]), dtype=torch.float32).numpy()
v = torch.tensor(np.array([r[2] for h in off_files for r in h]), dtype=torch.float32).numpy()
wp, wv = (x.cpu().numpy() for x in off_w.rows()[1:])
print("OFF_RING_IS_THE_FILES", wp.shape == p.shape and np.array_equal(bits(wp), bits(p)), wv.shape == v.shape and np.array_equal(bits(wv), bits(v)))
n0 = len(off_files[0])
print("NEWEST_GENERATION_UNTOUCHED", np.array_equal(bits(on_rings[1][n0:]), bits(off_rings[1][n0:])),
      np.array_equal(bits(on_rings[2][n0:]), bits(off_rings[2][n0:])))
'''


def test_self_play_with_reanalyse(dev, tmp_path):
    """One child process on the 3x3 board: two self_play() calls with a fixed seed into a window, with the option on, off, and off
    followed by a stand-alone reanalyse with the same arguments.  On equals off-then-reanalyse ring for ring; the .history files are
    the option off's; with the option off no search engine is built and the ring holds the rows of the files."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="3", AQG_EVAL_CACHE_SLOTS="0")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("OFF_BUILDS_NO_SEARCH_ENGINE True True", "ON_BUILT_ONE_ENGINE True True True True", "PASSES True True",
                 "ON_IS_OFF_THEN_REANALYSE True", "THE_OPTION_ACTED True True True", "FILES_ARE_THE_OPTION_OFFS True True",
                 "OFF_RING_IS_THE_FILES True True", "NEWEST_GENERATION_UNTOUCHED True True"):
        assert line in r.stdout, (line, r.stdout[-3000:])
    assert "reanalysed 0 of 0 rows at 12 simulations" in r.stdout and "reanalysed 11 of " in r.stdout
