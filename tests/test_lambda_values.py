"""Lambda-return value targets on the GPU (include/aqgnn.h, "lambda-return value targets"; csrc/value_targets.hip): the launch on
synthetic arrays inside a NaN-filled output, its refusals, the engine's history_lambda_values() after whole generations, and
self_play() into a window and a file.  Everything is held to engine.lambda_values_reference bit for bit: the kernel and the statement
make the same three f32 operations per ply and no transcendental, so there is no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _lambda_values as LV   # noqa: E402
from tests import _start_positions as SP   # noqa: E402

pytestmark = pytest.mark.gpu

QUOTAS = (1, 3, 4, 5, 8, 9, 257)                 # the edges of a workgroup of four wavefronts


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _launch(dev, plies, result, done, q, lam, out, quota=None, hp=None, null=None):
    """aqg_lambda_values on host arrays: (return code, out as it is afterwards).  null: the name of a pointer passed as NULL."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    t = dict(plies=torch.from_numpy(plies).to(dev), result=torch.from_numpy(result).to(dev), done=torch.from_numpy(done).to(dev),
             q=torch.from_numpy(q).to(dev), out=torch.from_numpy(out).to(dev))
    p = {k: None if k == null else _lib.ptr(v) for k, v in t.items()}
    rc = lib.aqg_lambda_values(q.shape[0] if quota is None else quota, q.shape[1] if hp is None else hp, p["plies"], p["result"],
                               p["done"], p["q"], lam, p["out"], _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, t["out"].cpu().numpy()


def _reference(plies, result, done, q, lam):
    from alphaquoridorgnn_amd.engine import lambda_values_reference
    return lambda_values_reference(plies, result, done, q, lam, np.full(q.shape, np.nan, dtype=np.float32))


def _same(a, b):
    """Bit for bit, the NaN sentinels included (np.full's NaN travels through the device unchanged)."""
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 1. the kernel on synthetic arrays
@pytest.mark.parametrize("hp", [1, 2, 63, 64, 65, 116, 127, 128, 129, 200, 256, 257, 321, 600])
def test_kernel_matches_the_statement(dev, hp):
    """Every quota at the workgroup edges and every lambda, rows of `hp` floats: 1 to 4 rounds of 64 held in registers at once, and
    above 256 plies the chunked path with its carried value (257 = one ply in the chunk above, 321 = a round and a ply, 600 = three
    chunks).  Games of 1, 63, 64, 65 and hp plies, skipped ones (0, hp + 1, negative, not done) between them, results -1, 0, 1, all
    in one launch.  Every float outside t < plies of a processed game stays NaN."""
    for quota in QUOTAS:
        plies, result, done, q = LV.games(quota, hp, seed=quota + hp)
        _, written = LV.processed(plies, done, hp)
        for lam in LV.LAMBDAS:
            want = _reference(plies, result, done, q, lam)
            assert np.array_equal(~np.isnan(want), written)
            rc, got = _launch(dev, plies, result, done, q, lam, np.full(q.shape, np.nan, dtype=np.float32))
            assert rc == 0 and _same(got, want), (quota, hp, lam)


@pytest.mark.parametrize("hp", [1, 65, 200, 300])
def test_kernel_on_ones_and_zeros(dev, hp):
    """q from +-1 and +-0 only: every product is exact and the signs of the zeros must come out as the statement's."""
    for quota in (5, 9):
        plies, result, done, q = LV.games(quota, hp, seed=7 * quota + hp, special_q=True)
        for lam in LV.LAMBDAS:
            rc, got = _launch(dev, plies, result, done, q, lam, np.full(q.shape, np.nan, dtype=np.float32))
            assert rc == 0 and _same(got, _reference(plies, result, done, q, lam)), (quota, hp, lam)


def test_kernel_ends(dev):
    """lambda = 1 is z_t (bit for bit for a decided game, as a number for a draw, whose zero has no pinned sign) and lambda = 0 is q
    as a number."""
    hp = 130
    plies, result, done, q = LV.games(40, hp, seed=11)
    _, written = LV.processed(plies, done, hp)
    fill = np.full(q.shape, np.nan, dtype=np.float32)
    rc, one = _launch(dev, plies, result, done, q, 1.0, fill)
    z = np.where(np.arange(hp)[None, :] % 2 == 0, result[:, None].astype(np.float32), -result[:, None].astype(np.float32)).astype(np.float32)
    decided = written & (result != 0)[:, None]
    assert rc == 0 and decided.any() and np.array_equal(LV.bits(one[decided]), LV.bits(z[decided])) and (one[written] == z[written]).all()
    rc, zero = _launch(dev, plies, result, done, q, 0.0, fill)
    assert rc == 0 and (zero[written] == q[written]).all() and np.isnan(zero[~written]).all()


def test_refusals_leave_out_untouched(dev):
    from alphaquoridorgnn_amd import _lib
    plies, result, done, q = LV.games(9, 70, seed=5)
    fill = np.full(q.shape, np.nan, dtype=np.float32)
    cases = [dict(null=name) for name in ("plies", "result", "done", "q", "out")]
    cases += [dict(hp=0), dict(hp=-1), dict(quota=-1), dict(lam=1.5), dict(lam=-0.25), dict(lam=float("nan"))]
    for kw in cases:
        lam = kw.pop("lam", 0.5)
        rc, got = _launch(dev, plies, result, done, q, lam, fill, **kw)
        assert rc == -1 and _lib.load().aqg_last_error().decode().startswith("aqg_lambda_values"), kw
        assert _same(got, fill), kw
    rc, got = _launch(dev, plies, result, done, q, 0.5, fill, quota=0)              # nothing to do is not an error
    assert rc == 0 and _same(got, fill)
    lib = _lib.load()
    t = torch.zeros((9, 70), dtype=torch.float32, device=dev)                       # out may not be hist_value
    args = [_lib.ptr(torch.from_numpy(x).to(dev)) for x in (plies, result, done)]
    assert lib.aqg_lambda_values(9, 70, *args, _lib.ptr(t), 0.5, _lib.ptr(t), _lib.stream_ptr(dev)) == -1


# ------------------------------------------------------------------ 2. the engine
def _engine(G, N, **kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    kw.setdefault("record_search_value", True)
    return BatchedSelfPlay(None, num_games=G, sims=8, board_size=N, evaluator="fake", fake_bias=2, **kw)


def _engine_reference(eng, lam):
    """The statement on the engine's own four tensors, compacted by the mask of the recorded rows."""
    plies, result, done, q = (eng.t[k].cpu().numpy() for k in ("game_plies", "game_result", "game_done", "hist_value"))
    return _reference(plies, result, done, q, lam)[eng._history_valid()[0].cpu().numpy()]


def _assert_engine(eng, games):
    assert eng.play_generation()["finished"] == games
    q = eng.history_values().cpu().numpy()
    z = eng.history_tensors()[2].cpu().numpy()
    assert q.shape[0] >= games and (q != 0).any()
    for lam in (0.0, 0.5, 0.95, 1.0):
        got = eng.history_lambda_values(lam)
        assert got.dtype == torch.float32 and got.shape == (q.shape[0],)
        want = _engine_reference(eng, lam)
        assert not np.isnan(want).any() and _same(got.cpu().numpy(), want), lam
    assert (eng.history_lambda_values(0.0).cpu().numpy() == q).all()
    assert (eng.history_lambda_values(1.0).cpu().numpy() == z.astype(np.float32)).all()
    assert not _same(eng.history_lambda_values(0.5).cpu().numpy(), q)
    assert _same(eng.history_values().cpu().numpy(), q)                             # the recorded values themselves are not touched


@pytest.mark.parametrize("N,slots", [(3, 1), (3, 4), (5, 5)])
def test_engine_with_refill(dev, N, slots):
    _assert_engine(_engine(slots, N, quota=2 * slots + 3, seed=slots), 2 * slots + 3)


@pytest.mark.parametrize("N,kw", [(5, dict(resign_threshold=0.1, resign_disable_fraction=0.0)), (3, dict(tree_reuse=True)),
                                  (5, dict(tree_reuse=True, temperature_plies=2))], ids=["resign", "reuse3", "reuse5"])
def test_engine_with_resignation_and_tree_reuse(dev, N, kw):
    eng = _engine(4, N, quota=9, seed=3, **kw)
    _assert_engine(eng, 9)
    if "resign_threshold" in kw:
        assert eng.resign_stats()["games_resigned"] > 0                            # a resigned game's last row is bootstrapped like any other


def test_engine_with_a_start_table(dev):
    rows = SP.start_rows(3, 2, 3, seed=13)
    _assert_engine(_engine(4, 3, quota=7, seed=5, start_states=rows), 7)


def test_two_sets_are_their_concatenation(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    ms = MultiSetSelfPlay(None, num_games=6, sims=8, num_sets=2, seed=4, board_size=3, evaluator="fake", fake_bias=2, quota=11,
                          record_search_value=True)
    assert ms.play_generation()["finished"] == 11 and len(ms.sets) == 2
    for lam in (0.5, 0.95):
        got = ms.history_lambda_values(lam).cpu().numpy()
        want = np.concatenate([_engine_reference(eng, lam) for eng in ms.sets])
        assert got.shape == ms.history_values().shape and _same(got, want)
    with pytest.raises(ValueError, match="value_lambda"):
        ms.history_lambda_values(1.5)


def test_engine_refusals(dev):
    eng = _engine(2, 3)
    for bad in (-0.1, 1.5, float("nan"), "0.5"):
        with pytest.raises(ValueError, match="value_lambda"):
            eng.history_lambda_values(bad)
    eng.move()
    eng.apply_actions(torch.full((2,), -1, dtype=torch.int32))                     # both games end as draws, by moves nobody searched
    assert eng.counters()["finished"] == 2
    with pytest.raises(ValueError, match="apply_actions"):
        eng.history_lambda_values(0.5)
    eng.reset()
    assert eng.history_lambda_values(0.5).shape == (0,)                             # nothing finished yet, and the flag is cleared
    _assert_engine(eng, 2)
    with pytest.raises(ValueError, match="record_search_value"):
        _engine(2, 3, record_search_value=False).history_lambda_values(0.5)


# ------------------------------------------------------------------ 3. self_play() end to end
_LOOP = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, engine, pv_mcts, self_play as sp
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
from alphaquoridorgnn_amd.replay import ReplayWindow, blend_targets

assert constants.BOARD_SIZE == 3 and sp.SP_VALUE_LAMBDA is None
torch.manual_seed(3)
dev = aqd.device()
model = GraphPolicyValueNetwork(6, 16, 2, 17, board_size=3).to(dev).eval()
pv_mcts.PV_EVALUATE_COUNT = 8
sp.SP_VALUE_BLEND = 0.5
bits = lambda x: np.ascontiguousarray(x).view(np.int32)

# what the generation's engine held when self_play() asked it for the lambda-returns: the statement on every set's four tensors
calls = []
plain = engine.MultiSetSelfPlay.history_lambda_values


def watched(self, lam):
    want = []
    for eng in self.sets:
        plies, result, done, q = (eng.t[k].cpu().numpy() for k in ("game_plies", "game_result", "game_done", "hist_value"))
        out = engine.lambda_values_reference(plies, result, done, q, lam, np.full(q.shape, np.nan, dtype=np.float32))
        want.append(out[eng._history_valid()[0].cpu().numpy()])
    calls.append(dict(lam=lam, G=np.concatenate(want), z=self.history_tensors()[2].cpu().numpy(), q=self.history_values().cpu().numpy()))
    return plain(self, lam)


engine.MultiSetSelfPlay.history_lambda_values = watched


def generation():
    sp.SP_REPLAY = ReplayWindow(3, max_generations=1, capacity_rows=4096, device=dev)
    path = sp.self_play(model, games=6, seed=17)
    with open(path, "rb") as f:
        rows = pickle.load(f)
    os.remove(path)
    return rows, [x.cpu().numpy() for x in sp.SP_REPLAY.rows()]


never_rows, never_ring = generation()                   # SP_VALUE_LAMBDA has never been assigned in this process
print("NEVER_SET_MAKES_NO_LAUNCH", not calls)
sp.SP_VALUE_LAMBDA = 0.9
on_rows, on_ring = generation()
c = calls[0]
print("ONE_CALL", len(calls) == 1, c["lam"] == float(np.float32(0.9)))
print("SAME_GAMES", len(on_rows) == len(never_rows) >= 6, [r[:2] for r in on_rows] == [r[:2] for r in never_rows],
      np.array_equal(on_ring[0], never_ring[0]), np.array_equal(bits(on_ring[1]), bits(never_ring[1])))
print("RING_Z_IS_THE_BLEND_OF_G", np.array_equal(bits(on_ring[2]), bits(blend_targets(c["z"], c["G"], 0.5))),
      not np.isnan(c["G"]).any() and not np.array_equal(c["G"], c["q"]) and not np.array_equal(on_ring[2], never_ring[2]))
print("NEVER_SET_IS_THE_BLEND_OF_Q", np.array_equal(bits(never_ring[2]), bits(blend_targets(c["z"], c["q"], 0.5))))
z_file = np.array([r[2] for r in on_rows], dtype=np.float64)
print("FILE_GIVES_THE_FLOAT32_BACK", all(type(r[2]) is float for r in on_rows),
      np.array_equal(bits(z_file.astype(np.float32)), bits(on_ring[2])), np.array_equal(z_file.astype(np.float32).astype(np.float64), z_file))
sp.SP_VALUE_LAMBDA = None
off_rows, off_ring = generation()
print("NONE_IS_NEVER_SET", len(calls) == 1, all(a.tobytes() == b.tobytes() for a, b in zip(off_ring, never_ring)), off_rows == never_rows)
sp.SP_VALUE_BLEND, sp.SP_VALUE_LAMBDA = 0.0, 0.9
try:
    generation()
    print("REFUSED_WITHOUT_A_BLEND False")
except ValueError as e:
    print("REFUSED_WITHOUT_A_BLEND", "SP_VALUE_LAMBDA" in str(e))
'''


def test_self_play_with_a_lambda(dev, tmp_path):
    """One child process on the 3x3 board (the module's board size comes from the environment): self_play() with a window, a blend of
    0.5 and lambda 0.9.  The ring's z is blend_targets of the engine's z and the statement's G, and float32 of the file's z; with
    SP_VALUE_LAMBDA None the ring and the file are, byte for byte, those of a run in which the option was never assigned -- the
    blend of the plain search values, without a lambda launch."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="3")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("NEVER_SET_MAKES_NO_LAUNCH True", "ONE_CALL True True", "SAME_GAMES True True True True", "RING_Z_IS_THE_BLEND_OF_G True True",
                 "NEVER_SET_IS_THE_BLEND_OF_Q True", "FILE_GIVES_THE_FLOAT32_BACK True True True", "NONE_IS_NEVER_SET True True True",
                 "REFUSED_WITHOUT_A_BLEND True"):
        assert line in r.stdout, (line, r.stdout[-3000:])
    assert "value lambda: 0.9" in r.stdout
