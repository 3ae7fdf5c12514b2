"""The replay window without a GPU: replay.append_reference (the kernel's statement in numpy) against the .history route bit for bit,
the ring's bookkeeping on the host backend, the ABI and the defaults, and the refusals that need no device."""
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from alphaquoridorgnn_amd import replay   # noqa: E402
from alphaquoridorgnn_amd.replay import ReplayWindow, append_reference   # noqa: E402


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def counts_rows(N, n, seed, top=32767):
    """A generation as the engine leaves it: records with legal bytes (positions on the board, walls 0..2, the ply counter in bytes
    68-69 set), counts up to `top` -- row 0 without a visit, row 1 with a single one, row 2 full of `top` -- and z in -1, 0, 1."""
    rng = np.random.RandomState(seed)
    A, nw = _A(N), (N - 1) ** 2
    S = np.zeros((n, 72), dtype=np.uint8)
    S[:, 0], S[:, 2] = rng.randint(0, N * N, n), rng.randint(0, N * N, n)
    S[:, 1], S[:, 3] = rng.randint(0, 11, n), rng.randint(0, 11, n)
    S[:, 4:4 + nw] = rng.randint(0, 3, (n, nw))
    S[:, 68], S[:, 69], S[:, 70] = rng.randint(0, 256, n), rng.randint(0, 2, n), N
    V = rng.randint(0, top + 1, (n, A)).astype(np.int64)
    V[rng.rand(n, A) < 0.5] = 0
    small = rng.rand(n) < 0.5
    V[small] = np.minimum(V[small], rng.randint(1, 40, (int(small.sum()), 1)))       # the sums a real search gives, too
    if n > 0:
        V[0] = 0
    if n > 1:
        V[1] = 0
        V[1, rng.randint(A)] = 1
    if n > 2:
        V[2] = top
    Z = rng.choice([-1, 0, 1], n).astype(np.int8)
    return S, V.astype(np.uint16), Z


def finished_rows(N, n, seed):
    rng = np.random.RandomState(seed)
    S = rng.randint(0, 256, (n, 72)).astype(np.uint8)
    P = rng.rand(n, _A(N)).astype(np.float32)
    Z = rng.choice([-1.0, 0.0, 1.0], n).astype(np.float32)
    return S, P, Z


def file_route(S, V, Z, N, tmp_path):
    """self_play._history_rows -> pickle -> the conversion of train_network._train_loop; numpy (s, p, v)."""
    from alphaquoridorgnn_amd.pv_network_gnn import pack_states
    from alphaquoridorgnn_amd.self_play import _history_rows
    path = tmp_path / f"rows{N}.history"
    with open(path, "wb") as f:
        pickle.dump(_history_rows(torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z), N), f)
    with open(path, "rb") as f:
        history = pickle.load(f)
    s, p, v = zip(*history)
    return (pack_states(s, N), torch.tensor(np.array(p), dtype=torch.float32).numpy(),
            torch.tensor(np.array(v), dtype=torch.float32).numpy())


# ------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize("N", (3, 5, 9))
def test_append_reference_equals_the_file_route(N, tmp_path):
    n, A = 23, _A(N)
    S, V, Z = counts_rows(N, n, seed=N)
    r72, rpi, rz = np.full((n, 72), 0xA5, np.uint8), np.full((n, A), -7.25, np.float32), np.full((n,), -7.25, np.float32)
    append_reference(N, S, V.view(np.int16), Z, None, None, 0, r72, rpi, rz)
    s, p, v = file_route(S, V, Z, N, tmp_path)
    assert np.array_equal(_bits(rpi), _bits(p)) and np.array_equal(_bits(rz), _bits(v))
    assert (rpi[0] == 0).all() and rpi[1].sum() == 1.0
    keep = np.ones(72, bool)
    keep[68:70] = False                                  # the ply counter: to_array() drops it, and it is no network input
    assert np.array_equal(r72[:, keep], s[:, keep])
    assert np.array_equal(r72, S)                        # the ring holds the record verbatim


def test_append_reference_reads_counts_as_unsigned():
    N, n = 9, 40
    A = _A(N)
    S, V, Z = counts_rows(N, n, seed=77, top=65535)
    assert V.max() == 65535 and V[2].astype(np.int64).sum() == A * 65535
    want = np.zeros((n, A), np.float32)
    for i in range(n):
        tot = int(V[i].astype(np.int64).sum())
        if tot:
            want[i] = (V[i].astype(np.float64) / np.float64(tot)).astype(np.float32)
    for form in (V, V.view(np.int16)):
        r72, rpi, rz = np.zeros((n, 72), np.uint8), np.ones((n, A), np.float32), np.ones((n,), np.float32)
        append_reference(N, S, form, Z, None, None, 0, r72, rpi, rz)
        assert np.array_equal(_bits(rpi), _bits(want)) and np.array_equal(rz, Z.astype(np.float32))


def test_append_reference_wraps_and_leaves_the_rest():
    N, n, cap = 5, 7, 10
    A = _A(N)
    S, P, Z = finished_rows(N, n, seed=1)
    r72, rpi, rz = np.full((cap, 72), 0xA5, np.uint8), np.full((cap, A), -7.25, np.float32), np.full((cap,), -7.25, np.float32)
    append_reference(N, S, None, None, P, Z, 6, r72, rpi, rz)
    slots = (6 + np.arange(n)) % cap
    assert np.array_equal(r72[slots], S) and np.array_equal(_bits(rpi[slots]), _bits(P)) and np.array_equal(rz[slots], Z)
    rest = np.setdiff1d(np.arange(cap), slots)
    assert (r72[rest] == 0xA5).all() and (rpi[rest] == -7.25).all() and (rz[rest] == -7.25).all()


# ------------------------------------------------------------------ bookkeeping on the host backend
def _generation(N, m, tag):
    S, P, Z = finished_rows(N, m, seed=1000 + tag)
    S[:, 71] = tag
    return tuple(torch.from_numpy(x) for x in (S, P, Z))


def _held(window):
    return [x.numpy() for x in window.rows()]


def _concat(gens):
    return [np.concatenate([g[j].numpy() for g in gens]) for j in range(3)]


def _same_rows(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_generations_wrap_the_ring_and_evict_by_count():
    N = 5
    w = ReplayWindow(N, max_generations=3, capacity_rows=20)
    assert len(w) == 0 and w.generations == [] and w.index().numel() == 0 and w.rows()[0].shape == (0, 72)
    gens = [_generation(N, m, tag) for tag, m in enumerate((6, 5, 7, 4, 6))]
    for i, g in enumerate(gens):
        w.append_rows(*g)
        held = gens[max(0, i - 2):i + 1]
        assert w.generations == [int(x[0].shape[0]) for x in held] and len(w) == sum(w.generations)
        assert _same_rows(_held(w), _concat(held))
    # 6 + 5 + 7 = 18 rows, then 4: the first is dropped by count and the fourth wraps (slots 18, 19, 0, 1)
    idx = w.index().numpy()
    assert idx.dtype == np.int64 and len(np.unique(idx)) == len(w) == 17
    assert np.array_equal(idx, (idx[0] + np.arange(17)) % 20)             # one circular interval, the oldest row first
    assert (np.diff(idx) < 0).sum() == 1                                   # ... that wraps
    s72 = w.tensors()[0].numpy()
    assert [int(t) for t in s72[idx][:, 71]] == [2] * 7 + [3] * 4 + [4] * 6
    assert all(x.shape[0] == 20 for x in w.tensors())
    w.clear()
    assert len(w) == 0 and w.generations == [] and w.index().numel() == 0 and w.tensors()[0].shape[0] == 20
    w.append_rows(*gens[0])
    assert _same_rows(_held(w), _concat(gens[:1])) and w.index()[0].item() == 0


def test_eviction_by_capacity():
    N = 3
    w = ReplayWindow(N, max_generations=10, capacity_rows=12)
    gens = [_generation(N, m, tag) for tag, m in enumerate((5, 5, 4, 12, 1))]
    w.append_rows(*gens[0])
    w.append_rows(*gens[1])
    assert w.generations == [5, 5]
    w.append_rows(*gens[2])                   # 14 > 12: the oldest goes, fewer than max_generations are held
    assert w.generations == [5, 4] and _same_rows(_held(w), _concat(gens[1:3]))
    w.append_rows(*gens[3])                   # fills the ring alone
    assert w.generations == [12] and _same_rows(_held(w), _concat(gens[3:4]))
    w.append_rows(*gens[4])
    assert w.generations == [1] and _same_rows(_held(w), _concat(gens[4:5]))


def test_a_generation_larger_than_the_ring_keeps_its_newest_rows():
    N = 3
    w = ReplayWindow(N, max_generations=2, capacity_rows=8)
    first, big = _generation(N, 3, 0), _generation(N, 13, 1)
    w.append_rows(*first)
    w.append_rows(*big)
    assert w.generations == [8] and len(w) == 8
    assert _same_rows(_held(w), [x.numpy()[5:] for x in big])


def test_lazy_capacity():
    N = 3
    w = ReplayWindow(N, max_generations=3)
    with pytest.raises(ValueError):
        w.tensors()
    with pytest.raises(ValueError):
        w.append_rows(*_generation(N, 0, 9))
    w.append_rows(*_generation(N, 7, 0))
    assert w.capacity == 3 * 11 and w.tensors()[1].shape == (33, _A(N))
    w.append_rows(*_generation(N, 14, 1))
    w.append_rows(*_generation(N, 14, 2))     # 35 > 33: games grew, so the window holds two generations, not three
    assert w.generations == [14, 14]


def test_counts_history_and_files_agree(tmp_path):
    """append_counts, append_history of the same generation's .history rows and extend_from_files of its file hold the same targets."""
    from alphaquoridorgnn_amd.self_play import _history_rows
    N = 5
    S, V, Z = counts_rows(N, 19, seed=4)
    a, b, c = (ReplayWindow(N, max_generations=2, capacity_rows=50) for _ in range(3))
    a.append_counts(torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
    history = _history_rows(torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z), N)
    b.append_history(history)
    paths = []
    for k in range(2):
        paths.append(tmp_path / f"2026010100000{k}.history")
        with open(paths[-1], "wb") as f:
            pickle.dump(history[:10] if k == 0 else history[10:], f)
    c.extend_from_files(paths)
    assert a.generations == b.generations == [19] and c.generations == [10, 9]
    keep = np.ones(72, bool)
    keep[68:70] = False
    for w in (b, c):
        assert _same_rows(_held(a)[1:], _held(w)[1:]) and np.array_equal(_held(a)[0][:, keep], _held(w)[0][:, keep])
    assert a.index().device.type == "cpu" and a.rows()[1].dtype == torch.float32


# ------------------------------------------------------------------ ABI and defaults
def test_abi_and_binding():
    from alphaquoridorgnn_amd import _lib
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    assert re.search(r"\bint\s+aqg_replay_append\s*\(", header)
    res, args = _lib.SIGNATURES["aqg_replay_append"]
    assert res is _lib._c.c_int and len(args) == 14
    assert re.search(r"\breplay\b", open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "build.sh")).read())


def test_defaults_and_train_cycle_options():
    from alphaquoridorgnn_amd import self_play as sp, train_cycle as tc, train_network as tn
    assert sp.SP_REPLAY is None and sp.SP_WRITE_HISTORY is True
    assert tn.TRAIN_WINDOW is None and tn.TRAIN_GENERATIONS == 1 and tn.TRAIN_EPOCH_ROWS is None
    args = tc._parser().parse_args([])
    assert (args.replay_generations, args.replay_rows, args.epoch_rows, args.no_history_file) == (0, None, None, False)
    assert tc._set_replay_options(args) is None
    assert sp.SP_REPLAY is None and tn.TRAIN_WINDOW is None and tn.TRAIN_GENERATIONS == 1 and sp.SP_WRITE_HISTORY is True
    args = tc._parser().parse_args(["--replay-generations", "4", "--replay-rows", "9000", "--epoch-rows", "4096", "--no-history-file"])
    assert (args.replay_generations, args.replay_rows, args.epoch_rows, args.no_history_file) == (4, 9000, 4096, True)
    with pytest.raises(ValueError):
        tc._set_replay_options(tc._parser().parse_args(["--no-history-file"]))
    assert sp.SP_WRITE_HISTORY is True


def test_epoch_order(monkeypatch):
    from alphaquoridorgnn_amd import train_network as tn
    perm, index = torch.tensor([3, 0, 2, 1]), torch.tensor([8, 9, 0, 1])
    assert tn._epoch_order(perm, None) is perm
    assert tn._epoch_order(perm, index).tolist() == [1, 8, 0, 9]
    monkeypatch.setattr(tn, "TRAIN_EPOCH_ROWS", 3)
    assert tn._epoch_order(perm, None).tolist() == [3, 0, 2] and tn._epoch_order(perm, index).tolist() == [1, 8, 0]
    monkeypatch.setattr(tn, "TRAIN_EPOCH_ROWS", 99)
    assert tn._epoch_order(perm, index).tolist() == [1, 8, 0, 9]


# ------------------------------------------------------------------ refusals that need no device
def test_refusals():
    N = 5
    A = _A(N)
    S, V, Z = (torch.from_numpy(x) for x in counts_rows(N, 6, seed=2))
    V = V.view(torch.int16)
    _, P, ZF = (torch.from_numpy(x) for x in finished_rows(N, 6, seed=2))
    w = ReplayWindow(N, max_generations=2, capacity_rows=16)
    bad = [lambda: w.append_counts(S, V.to(torch.int32), Z), lambda: w.append_counts(S, V, Z.to(torch.float32)),
           lambda: w.append_counts(S[:, :71], V, Z), lambda: w.append_counts(S, V[:, :A - 1], Z), lambda: w.append_counts(S, V[:5], Z),
           lambda: w.append_counts(S.to(torch.int8), V, Z), lambda: w.append_rows(S, P.double(), ZF), lambda: w.append_rows(S, P, Z),
           lambda: w.append_rows(S, P, ZF[:5]), lambda: w.append_rows(S, V, ZF),
           lambda: w.append_rows(S, torch.zeros((6, _A(9))), ZF),                                   # another board's policy
           lambda: w.append_history([[[[0, 3], [8, 3], [0] * 64], [0.0] * _A(9), 1]]),
           lambda: w.append_history([[[[0, 3], [8, 3], [0] * 16], [0.0] * (A - 1), 1]])]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert len(w) == 0 and w.generations == [] and not any(x.any() for x in w.tensors())          # nothing was written
    for kw in (dict(board_size=4), dict(max_generations=0), dict(capacity_rows=0)):
        with pytest.raises(ValueError):
            ReplayWindow(**kw)
    r72, rpi, rz = np.zeros((4, 72), np.uint8), np.zeros((4, A), np.float32), np.zeros((4,), np.float32)
    s, v, z, p, zf = S.numpy(), V.numpy(), Z.numpy(), P.numpy(), ZF.numpy()
    for args in ((s[:3], v[:3], z[:3], p[:3], zf[:3], 0), (s[:3], None, None, None, None, 0), (s[:3], v[:3], None, None, zf[:3], 0),
                 (s[:5], v[:5], z[:5], None, None, 0), (s[:3], v[:3], z[:3], None, None, 4), (s[:3], v[:3], z[:3], None, None, -1)):
        with pytest.raises(ValueError):
            append_reference(N, *args[:5], args[5], r72, rpi, rz)
    assert not r72.any() and not rpi.any()


def test_no_history_file_needs_a_window(monkeypatch):
    from alphaquoridorgnn_amd import self_play as sp
    monkeypatch.setattr(sp, "SP_WRITE_HISTORY", False)

    def played(*a, **k):
        raise AssertionError("a game was played")
    monkeypatch.setattr(sp, "MultiSetSelfPlay", played)
    monkeypatch.setattr(sp, "load_network", played)
    with pytest.raises(ValueError, match="SP_WRITE_HISTORY"):
        sp.self_play(games=2)


def test_a_window_of_another_board_is_refused(monkeypatch):
    from alphaquoridorgnn_amd import train_network as tn
    w = ReplayWindow(3, max_generations=1, capacity_rows=4)
    w.append_rows(*_generation(3, 2, 0))
    monkeypatch.setattr(tn, "TRAIN_WINDOW", w)
    with pytest.raises(ValueError, match="3x3"):
        tn._training_rows(torch.device("cpu"), 5)
    s, p, v, index = tn._training_rows(torch.device("cpu"), 3)
    assert s.shape == (4, 72) and index.tolist() == [0, 1]
