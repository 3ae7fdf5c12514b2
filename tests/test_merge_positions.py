"""The position merge on the GPU (csrc/replay_merge.hip), everything bit for bit against the numpy statements of replay.py: the keys,
the run heads, the merge launch over hand-built runs at every edge of its geometry and of its summation order, merge_positions end to
end, a GPU window against a host window, the C entries' refusals, and train_network() with TRAIN_MERGE_POSITIONS on the 5x5 board."""
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

from tests.test_merge_positions_cpu import (OTHER_BYTES, _A, check_against_float64, mixed, repeated_rows, same)   # noqa: E402
from tests.test_replay_window_cpu import counts_rows   # noqa: E402

pytestmark = pytest.mark.gpu

FILL_U8, FILL_F32, FILL_I32 = 0xA5, np.float32(-7.25), np.int32(-77)
# csrc/replay_merge.hip: MRG_GROUP = 4 rows per wavefront, MRG_ROWS = 16 rows per workgroup, MRG_CHUNK = 64 rows per chunk of the
# summation order (and per window of the chunk launch), MRG_ADD = 8 rows (or partial rows) in flight when a run's further rows are added
GROUP, ROWS, CHUNK, ADD = 4, 16, 64, 8
SIZES = (0, 1, GROUP - 1, GROUP, GROUP + 1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 5)
BOARDS = (3, 5, 7, 9)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def test_the_sizes_are_the_kernels():
    src = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "replay_merge.hip")).read()
    for text in (f"MRG_GROUP = {GROUP};", f"MRG_WAVES = {ROWS // GROUP};", "MRG_ROWS = MRG_WAVES * MRG_GROUP;", f"MRG_CHUNK = {CHUNK};",
                 f"MRG_ADD = {ADD};"):
        assert text in src
    from alphaquoridorgnn_amd import replay
    assert replay.MERGE_CHUNK == CHUNK


def _t(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ------------------------------------------------------------------ the keys
@pytest.mark.parametrize("N", BOARDS)
def test_keys_equal_the_numpy_hash(dev, N):
    """n = 0, 1, and one below, at and one above a wavefront's four rows and a workgroup's sixteen, and two workgroups plus five; all
    rows in order, and a gathered index in an order of its own with rows left out.  keys has three spare entries that keep a pattern."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.replay import position_keys
    lib = _lib.load()
    for n in SIZES:
        S = counts_rows(N, n + 9, seed=300 * N + n)[0]
        S[:, 71] = np.arange(n + 9)
        for index in (None, np.random.RandomState(n).permutation(n + 9)[:n].astype(np.int64)):
            d_s, d_i = _t(dev, S[:n] if index is None else S), _t(dev, index)
            keys = torch.full((n + 3,), -5, dtype=torch.int64, device=dev)
            rc = lib.aqg_replay_position_keys(_lib.ptr(d_s) if n else None, _lib.ptr(d_i) if n else None, n, _lib.ptr(keys),
                                              _lib.stream_ptr(dev))
            torch.cuda.synchronize()
            assert rc == 0
            got = keys.cpu().numpy()
            assert np.array_equal(got[:n], position_keys(S[:n] if index is None else S, index)) and np.all(got[n:] == -5)
            assert np.array_equal(d_s.cpu().numpy(), S[:n] if index is None else S)


# ------------------------------------------------------------------ the run heads
def _heads(dev, S, perm):
    from alphaquoridorgnn_amd import _lib
    n = len(perm)
    d_s, d_p = _t(dev, S), _t(dev, np.asarray(perm, dtype=np.int64))
    heads = torch.full((n + 3,), FILL_U8, dtype=torch.uint8, device=dev)
    rc = _lib.load().aqg_replay_run_heads(_lib.ptr(d_s), _lib.ptr(d_p) if n else None, n, _lib.ptr(heads), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(d_s.cpu().numpy(), S) and np.all(heads.cpu().numpy()[n:] == FILL_U8)
    return heads.cpu().numpy()[:n]


def _want_heads(S, perm):
    from alphaquoridorgnn_amd.replay import KEY_BYTES
    kb = S[np.asarray(perm, dtype=np.int64)][:, KEY_BYTES]
    want = np.ones(len(perm), np.uint8)
    want[1:] = (kb[1:] != kb[:-1]).any(axis=1)
    return want


def test_run_heads_compare_the_bytes_not_the_keys(dev):
    """Rows A B A under the identity perm -- what a forged key that is equal for A and B would sort them to -- are three runs; A A B are
    two: a collision splits a run and never merges one.  Bytes 68, 69 and 71 differing inside a run do not split it; any single key
    byte does, the eight behind the wavefront's first 64 included."""
    rng = np.random.RandomState(12)
    A, B = rng.randint(0, 256, (2, 72)).astype(np.uint8)
    A2 = A.copy()
    A2[list(OTHER_BYTES)] ^= 0xFF
    assert _heads(dev, np.stack([A, B, A2]), [0, 1, 2]).tolist() == [1, 1, 1]
    assert _heads(dev, np.stack([A, B, A2]), [0, 2, 1]).tolist() == [1, 0, 1]
    assert _heads(dev, np.stack([A, A2, B]), [0, 1, 2]).tolist() == [1, 0, 1]
    pairs = np.repeat(rng.randint(0, 256, (72, 72)).astype(np.uint8), 2, axis=0)         # pair k differs in byte k alone
    pairs[2 * np.arange(72) + 1, np.arange(72)] ^= 0x01
    got = _heads(dev, pairs, np.arange(144))
    assert np.all(got[0::2] == 1) and got[1::2].tolist() == [0 if k in OTHER_BYTES else 1 for k in range(72)]


@pytest.mark.parametrize("N", BOARDS)
def test_run_heads_equal_the_numpy_statement(dev, N):
    for n in SIZES:
        S, _, _ = repeated_rows(N, n + 6, 5, seed=400 * N + n)
        perm = np.random.RandomState(n + 1).permutation(n + 6)[:n]
        perm = perm[np.argsort(S[perm][:, 0], kind="stable")]                   # some neighbours equal, some not
        assert np.array_equal(_heads(dev, S, perm), _want_heads(S, perm))


# ------------------------------------------------------------------ the merge launch
def _merge_runs(dev, N, S, P, Z, perm, starts):
    """aqg_replay_merge_runs on device copies, outputs of u + 3 rows pre-filled with a pattern; the four outputs back on the host (all
    u + 3 rows).  The sources must come back unchanged."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    A, n, u = _A(N), len(perm), len(starts)
    d = [_t(dev, x) for x in (S, P, Z, np.asarray(perm, np.int64), np.asarray(starts, np.int64))]
    outs = [torch.full((u + 3, 72), FILL_U8, dtype=torch.uint8, device=dev), torch.full((u + 3, A), float(FILL_F32), device=dev),
            torch.full((u + 3,), float(FILL_F32), device=dev), torch.full((u + 3,), int(FILL_I32), dtype=torch.int32, device=dev)]
    floats = int(lib.aqg_replay_merge_workspace_floats(N, n, u))
    assert floats == (0 if n - u < CHUNK else 2 * -(-n // CHUNK) * (A + 1))
    work = torch.full((floats + 5,), float("nan"), device=dev) if floats else None
    rc = lib.aqg_replay_merge_runs(N, A, *(_lib.ptr(x) for x in d), n, u, *(_lib.ptr(x) for x in outs), _lib.ptr(work), floats,
                                   _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0, lib.aqg_last_error()
    for x, h in zip(d[:3], (S, P, Z)):
        assert same(x.cpu().numpy(), h)
    if work is not None:
        assert torch.isnan(work[floats:]).all()                 # nothing behind the floats asked for
    return [x.cpu().numpy() for x in outs]


def _check_merge_runs(dev, N, lengths, seed):
    from alphaquoridorgnn_amd.replay import merge_runs_reference
    rng = np.random.RandomState(seed)
    n, A = int(sum(lengths)), _A(N)
    rows = n + 11
    S = rng.randint(0, 256, (rows, 72)).astype(np.uint8)
    P, Z = mixed(rng, rows, A), mixed(rng, rows)
    perm = rng.permutation(rows)[:n]                             # within a run the rows are in no order of their slots
    starts = np.cumsum(lengths) - np.asarray(lengths)
    for s, L in zip(starts, lengths):
        if L >= 16:
            assert np.any(np.diff(perm[s:s + L]) < 0) and np.any(np.diff(perm[s:s + L]) > 0)
    want = merge_runs_reference(S, P, Z, perm, starts)
    got = _merge_runs(dev, N, S, P, Z, perm, starts)
    u = len(lengths)
    for g, w, fill in zip(got, want, (FILL_U8, FILL_F32, FILL_F32, FILL_I32)):
        assert same(g[:u], w)
        assert np.all(g[u:] == fill)                             # the three spare rows keep the pattern
    assert np.array_equal(want[3], np.asarray(lengths, np.int32))
    return starts


# run lengths: 1, 2, 3; a wavefront's four rows (4, 5, 6); one below / at / one above the rows in flight when a run's other rows are
# added (the first row apart: 8, 9, 10, and twice that, 16, 17, 18);
# the chunk (63, 64, 65 -- 65 is the first length the chunk launch sums) and two chunks (127, 128, 129); long runs first (at place 0, a
# multiple of the window), last, and between runs of length 1; a long run that begins in the window in which its neighbour's last chunk
# begins (127 then 128: places 64 and 127), so both workspace rows of a window are in use; more output rows than two workgroups' 32
LAYOUT = (127, 128, 129, 1, 1, 1, 2, 3, 4, 5, 6, 1, 8, 9, 10, 16, 17, 18, 63, 64, 1, 65, 1, 1) + (1,) * ROWS + (2, 1, 129)


@pytest.mark.parametrize("N", BOARDS)
def test_merge_runs_equal_the_reference_bit_for_bit(dev, N):
    starts = _check_merge_runs(dev, N, LAYOUT, seed=500 + N)
    assert len(LAYOUT) > 2 * ROWS and starts[1] // CHUNK == (starts[0] + CHUNK) // CHUNK == 1 and LAYOUT[0] > CHUNK < LAYOUT[1]
    # no run longer than a chunk, and fewer than 64 repeats: no chunk launch and no workspace
    _check_merge_runs(dev, N, (3, 1, 2, 1, 1, 5, 1), seed=600 + N)
    for u in (1, GROUP - 1, GROUP, GROUP + 1, ROWS - 1, ROWS, ROWS + 1):          # output rows at the edges of the geometry
        _check_merge_runs(dev, N, (2,) + (1,) * (u - 1), seed=700 + N + u)
    _check_merge_runs(dev, N, (1,) * 37, seed=800 + N)                            # a plain gather
    # more runs than one round of the chunk launch's 64-way search of starts covers, long runs behind and between them
    _check_merge_runs(dev, N, (1,) * 70 + (65,) + (1,) * 70 + (130, 1), seed=850 + N)


def test_merge_runs_at_the_partial_rows_in_flight(dev):
    """A long run's chunk sums are added eight at a time behind the first: 8, 9 and 10 chunks (one below / at / one above), whole and
    with a last chunk of one row.  On the smallest board: the lengths are what the constant asks for."""
    lengths = (1, CHUNK * ADD, 1, CHUNK * (ADD + 1), CHUNK * (ADD + 1) + 1, CHUNK * (ADD + 2) - 7, 1)
    _check_merge_runs(dev, 3, lengths, seed=900)


def test_merge_runs_behind_thousands_of_runs(dev):
    """More than 64 x 64 runs in front of the long ones: the chunk launch's 64-way search of starts takes a third round.  The smallest
    board: 17 actions a row."""
    _check_merge_runs(dev, 3, (1,) * (CHUNK * CHUNK + 104) + (65,) + (1,) * 30 + (129, 2), seed=950)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("N", BOARDS)
def test_merge_positions_end_to_end(dev, N):
    """Repeats scattered over the input, all rows and a gathered index: merge_positions equals merge_reference fed the stable sort of the
    numpy keys, and lies within the bound of the float64 statement."""
    from alphaquoridorgnn_amd.replay import merge_positions, merge_reference, position_keys
    S, P, Z = repeated_rows(N, 0, 0, seed=1000 + N, lengths=(70, 1, 1, 33, 2, 1, 150, 1, 5, 1, 1, 1, 64, 3))
    n = S.shape[0]
    for index in (None, np.random.RandomState(N).permutation(n)[:n - 40].astype(np.int64)):
        perm = np.argsort(position_keys(S, index), kind="stable")
        want = merge_reference(S, P, Z, index=index, perm=perm)
        d = [_t(dev, x) for x in (S, P, Z)]
        got = [x.cpu().numpy() for x in merge_positions(*d, index=_t(dev, index), board_size=N)]
        assert len(got) == 4 and all(same(g, w) for g, w in zip(got, want))
        check_against_float64(got, S, P, Z, index)
        assert all(same(x.cpu().numpy(), h) for x, h in zip(d, (S, P, Z)))
    empty = merge_positions(*[_t(dev, x[:0]) for x in (S, P, Z)], board_size=N)
    assert [tuple(x.shape) for x in empty] == [(0, 72), (0, _A(N)), (0,), (0,)]
    with pytest.raises(ValueError):
        merge_positions(*[_t(dev, x) for x in (S, P, Z)], index=_t(dev, np.array([0, n], np.int64)), board_size=N)
    with pytest.raises(ValueError):
        merge_positions(*[_t(dev, x) for x in (S, P, Z)], index=_t(dev, np.array([-1, 0], np.int64)), board_size=N)


def _appended(device, N, gens, **kw):
    from alphaquoridorgnn_amd.replay import ReplayWindow
    w = ReplayWindow(N, device=device, **kw)
    for S, P, Z in gens:
        w.append_rows(torch.from_numpy(S), torch.from_numpy(P), torch.from_numpy(Z))
    return w


@pytest.mark.parametrize("N", BOARDS)
def test_gpu_window_against_host_window(dev, N):
    """After the same appends -- three generations, the third wraps the ring and evicts the first -- merged() of the GPU window and of
    the host window are the same four arrays, the ring and rows() are as they were, and a window without repeats merges to rows()."""
    from alphaquoridorgnn_amd.replay import KEY_BYTES
    six = np.random.RandomState(N).randint(0, 256, (6, 72)).astype(np.uint8)
    gens = [repeated_rows(N, m, 6, seed=40 * N + m) for m in (14, 16, 15)]
    for S, _, _ in gens:
        S[:, KEY_BYTES] = six[np.arange(S.shape[0]) % 6][:, KEY_BYTES]
    g, h = (_appended(d, N, gens, max_generations=2, capacity_rows=40) for d in (dev, None))
    ring = [x.cpu().numpy().copy() for x in g.tensors()]
    rows = [x.cpu().numpy() for x in g.rows()]
    got, want = [x.cpu().numpy() for x in g.merged()], [x.numpy() for x in h.merged()]
    assert all(x.is_cuda for x in g.merged()) and got[0].shape[0] == 6 and int(got[3].sum()) == 31
    assert all(same(a, b) for a, b in zip(got, want))
    assert all(same(a, b.cpu().numpy()) for a, b in zip(ring, g.tensors())) and all(same(a, b.cpu().numpy()) for a, b in zip(rows, g.rows()))
    rng = np.random.RandomState(50 + N)
    distinct = [(rng.randint(0, 256, (m, 72)).astype(np.uint8), mixed(rng, m, _A(N)), mixed(rng, m)) for m in (21, 30, 25)]
    w = _appended(dev, N, distinct, max_generations=2, capacity_rows=60)
    merged, plain = [x.cpu().numpy() for x in w.merged()], [x.cpu().numpy() for x in w.rows()]
    assert all(same(a, b) for a, b in zip(merged[:3], plain)) and np.array_equal(merged[3], np.ones(55, np.int32))


# ------------------------------------------------------------------ refusals
def test_the_c_entries_refuse_on_the_host(dev):
    """Every refusal of the three entries, made before any launch: -1 with a message, outputs and sources as they were.  perm, index
    and starts are valid in every call."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, A, n, u = 5, _A(5), 70, 3
    rng = np.random.RandomState(0)
    host = [rng.randint(0, 256, (n, 72)).astype(np.uint8), mixed(rng, n, A), mixed(rng, n), rng.permutation(n).astype(np.int64),
            np.array([0, 66, 68], np.int64)]
    S, P, Z, perm, starts = [_t(dev, x) for x in host]
    outs = [torch.full((n, 72), FILL_U8, dtype=torch.uint8, device=dev), torch.full((n, A), float(FILL_F32), device=dev),
            torch.full((n,), float(FILL_F32), device=dev), torch.full((n,), int(FILL_I32), dtype=torch.int32, device=dev)]
    keys, heads = torch.full((n,), -5, dtype=torch.int64, device=dev), torch.full((n,), FILL_U8, dtype=torch.uint8, device=dev)
    floats = int(lib.aqg_replay_merge_workspace_floats(N, n, u))
    assert floats == 2 * 2 * (A + 1)
    work = torch.full((floats,), float(FILL_F32), device=dev)
    st, p = _lib.stream_ptr(dev), _lib.ptr
    at = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731

    def refused(rc, word):
        assert rc == -1 and word in lib.aqg_last_error().decode(), (rc, lib.aqg_last_error())

    refused(lib.aqg_replay_position_keys(p(S), None, -1, p(keys), st), "negative")
    refused(lib.aqg_replay_position_keys(None, None, n, p(keys), st), "must be given")
    refused(lib.aqg_replay_position_keys(p(S), None, n, None, st), "must be given")
    refused(lib.aqg_replay_position_keys(p(S), None, n, at(S, 72 * (n - 1)), st), "overlaps")          # the last of n rows
    refused(lib.aqg_replay_position_keys(p(S), p(perm), n, at(S, 8), st), "overlaps")                    # the one row that is certain
    refused(lib.aqg_replay_position_keys(p(S), p(perm), n, at(perm, 8 * (n - 1)), st), "overlaps")
    assert lib.aqg_replay_position_keys(None, None, 0, None, st) == 0

    refused(lib.aqg_replay_run_heads(p(S), p(perm), -1, p(heads), st), "negative")
    for args in ((None, p(perm), n, p(heads)), (p(S), None, n, p(heads)), (p(S), p(perm), n, None)):
        refused(lib.aqg_replay_run_heads(*args, st), "must be given")
    refused(lib.aqg_replay_run_heads(p(S), p(perm), n, at(S, 71), st), "overlaps")
    refused(lib.aqg_replay_run_heads(p(S), p(perm), n, at(perm, 8 * n - 1), st), "overlaps")
    assert lib.aqg_replay_run_heads(None, None, 0, None, st) == 0

    def merge(board=N, policy=A, src=(S, P, Z, perm, starts), rows=n, runs=u, out=outs, ws=work, ws_floats=floats):
        ptr = lambda x: x if isinstance(x, ctypes.c_void_p) or x is None else p(x)      # noqa: E731
        return lib.aqg_replay_merge_runs(board, policy, *(ptr(x) for x in src), rows, runs, *(ptr(x) for x in out), ptr(ws), ws_floats, st)

    for board in (4, 11, 0):
        refused(merge(board=board), "board_size")
    refused(merge(policy=A + 1), "policy_size")
    refused(merge(rows=-1), "negative")
    refused(merge(runs=-1), "negative")
    refused(merge(runs=n + 1), "u > n")
    refused(merge(runs=0), "u == 0")
    for i in range(5):
        refused(merge(src=[None if j == i else x for j, x in enumerate((S, P, Z, perm, starts))]), "must be given")
    for i in range(4):
        refused(merge(out=[None if j == i else x for j, x in enumerate(outs)]), "must be given")
    refused(merge(ws=None), "workspace")
    refused(merge(ws_floats=floats - 1), "workspace")
    refused(merge(out=[outs[0], at(P, 4 * (A - 1)), outs[2], outs[3]]), "overlaps a source")            # inside the one certain row
    refused(merge(out=[at(S, 71), outs[1], outs[2], outs[3]]), "overlaps a source")
    refused(merge(out=[outs[0], outs[1], at(Z), outs[3]]), "overlaps a source")
    refused(merge(out=[outs[0], outs[1], outs[2], at(perm, 8 * n - 4)]), "overlaps a source")
    refused(merge(out=[outs[0], outs[1], at(starts, 8 * u - 4), outs[3]]), "overlaps a source")
    refused(merge(ws=at(P)), "overlaps a source")
    refused(merge(out=[outs[0], outs[1], outs[2], at(outs[2], 4 * (u - 1))]), "outputs overlap")
    refused(merge(ws=at(outs[1], 4 * (u * A - 1))), "outputs overlap")
    assert merge(rows=0, runs=0, src=(None,) * 5, out=(None,) * 4, ws=None, ws_floats=0) == 0
    torch.cuda.synchronize()
    for x, hx in zip((S, P, Z, perm, starts), host):
        assert same(x.cpu().numpy(), hx)
    for x, fill in zip(outs + [keys, heads, work], (FILL_U8, FILL_F32, FILL_F32, FILL_I32, -5, FILL_U8, FILL_F32)):
        assert bool((x == (float(fill) if x.is_floating_point() else int(fill))).all())
    assert merge() == 0                                             # and the call they were variations of is a good one
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the loop end to end
_LOOP = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, train_network as tn
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, pack_states
from alphaquoridorgnn_amd.replay import KEY_BYTES, ReplayWindow, merge_reference

g = np.load(os.path.join(os.environ["AQG_REPO"], "tests", "golden", "cnn_train_5x5.npz"))
rows = [[[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:20]]], p.tolist(), int(z)]
        for s, p, z in zip(g["states"], g["pi"], g["z"])]
_, first = np.unique(pack_states([r[0] for r in rows], 5)[:, KEY_BYTES], axis=0, return_index=True)
rows = [rows[i] for i in sorted(first)]                       # the golden rows repeat positions: each one once
assert len(rows) == 25 and constants.BOARD_SIZE == 5
older = [[s, [0.25 * x + 0.75 / 57 for x in p], -z] for s, p, z in rows[:15]]      # the first 15 positions again, other targets
os.makedirs("data")
FILES = ["data/20260101000000.history", "data/20260101000001.history"]
for path, h in zip(FILES, (older, rows)):
    with open(path, "wb") as f:
        pickle.dump(h, f)
os.makedirs(constants.PV_NETWORK_PATH)
torch.manual_seed(3)
torch.save(GraphPolicyValueNetwork(6, 16, 2, 57, board_size=5).state_dict(), constants.PV_NETWORK_PATH + "best.pth")
tn.NUM_EPOCH = 2
dev = aqd.device()


def run():
    torch.manual_seed(11)               # the epochs' shuffles
    tn.train_network()
    with open(constants.PV_NETWORK_PATH + "latest.pth", "rb") as f:
        return f.read()


def window(generations, histories):
    w = ReplayWindow(5, max_generations=generations, device=dev)
    for h in histories:
        w.append_history(h)
    return w


two = window(2, [older, rows])
s, p, z = (x.cpu().numpy() for x in two.rows())
distinct = len(np.unique(s[:, KEY_BYTES], axis=0))
merged = merge_reference(s, p, z)
print("REPEATS", len(s) == 40, distinct == merged[0].shape[0] == 25, int(merged[3].max()) == 2)
tn.TRAIN_WINDOW = two
unmerged = run()
tn.TRAIN_MERGE_POSITIONS = True
on = run()
tn.TRAIN_MERGE_POSITIONS = False
host = ReplayWindow(5, max_generations=1, device=dev)
host.append_rows(*(torch.from_numpy(x) for x in merged[:3]))
tn.TRAIN_WINDOW = host
print("MERGED_IS_THE_HOST_MERGED_WINDOW", run() == on, on != unmerged)
tn.TRAIN_WINDOW, tn.TRAIN_GENERATIONS, tn.TRAIN_MERGE_POSITIONS = None, 2, True
print("TRAIN_GENERATIONS", run() == on)
tn.TRAIN_GENERATIONS, tn.TRAIN_EPOCH_ROWS, tn.TRAIN_MIRROR = 1, 16, True
tn.TRAIN_WINDOW = two
short = run()
tn.TRAIN_WINDOW, tn.TRAIN_MERGE_POSITIONS = host, False
print("EPOCH_ROWS_AND_MIRROR", run() == short, short != on)
tn.TRAIN_EPOCH_ROWS, tn.TRAIN_MIRROR = None, False
one = window(1, [rows])                  # a window without repeats: the option changes nothing
s1 = one.rows()[0].cpu().numpy()
tn.TRAIN_WINDOW = one
off = run()
tn.TRAIN_MERGE_POSITIONS = True
print("NO_REPEATS", len(np.unique(s1[:, KEY_BYTES], axis=0)) == 25, run() == off)
tn.TRAIN_WINDOW = None                   # the newest file alone
newest_on = run()
tn.TRAIN_MERGE_POSITIONS = False
print("NEWEST_FILE", run() == newest_on, newest_on == off)
'''


def test_the_loop_with_merged_positions(dev, tmp_path):
    """One child process on the 5x5 board with a 6/16/2 best.pth, NUM_EPOCH = 2: two generations that share 15 positions, trained with
    TRAIN_MERGE_POSITIONS, give the latest.pth -- byte for byte, same torch seed -- of the option off on a one-generation window that
    holds the rows merged on the host (merge_reference); so do TRAIN_GENERATIONS = 2 over the two files, and TRAIN_EPOCH_ROWS with the
    mirror on top.  A window without repeats, and the newest file alone, train to the option-off bytes."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("REPEATS True True True", "MERGED_IS_THE_HOST_MERGED_WINDOW True True", "TRAIN_GENERATIONS True",
                 "EPOCH_ROWS_AND_MIRROR True True", "NO_REPEATS True True", "NEWEST_FILE True True"):
        assert line in r.stdout, (line, [x for x in r.stdout.splitlines() if x[:1].isupper() and "Epoch" not in x])
    assert "merged positions: 40 rows, 25 positions, longest run 2" in r.stdout
