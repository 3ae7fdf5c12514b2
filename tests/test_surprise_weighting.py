"""Policy surprise weighting on the GPU (csrc/replay_surprise.hip): the rows kernel against replay.surprise_reference within the bar
of tests/_surprise.py, and everything behind k -- q, the counts, the index -- bit for bit against the numpy statements; surprise_index
end to end on the rows of a tiny self-play generation for every network kind; the C entries' refusals; train_network() /
train_cnn_network() byte for byte against the option off; one cycle of train_cycle --surprise-weighting."""
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

from tests._surprise import (BOARDS, EXACT, SIZES, SPECIAL, exact_rows, network_rows, policy_size, special_rows, target_rows,   # noqa: E402
                             within_bar)

pytestmark = pytest.mark.gpu

FILL_F32, FILL_I32, MARGIN = np.float32(-7.25), np.int32(-77), 3


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _t(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _at(t, items):
    return ctypes.c_void_p(t.data_ptr() + items * t.element_size())


# ------------------------------------------------------------------ the rows kernel
def _rows_launch(dev, N, pi, net, index=None, chunks=None):
    """aqg_replay_surprise_rows over device copies, one launch per (offset, n) of `chunks` (default: one launch of all m rows), each fed
    its own slice of net; k and q have MARGIN sentinel entries in front and behind, checked here.  Returns (k, q) of the m rows."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    A, m = policy_size(N), net.shape[0]
    d_pi, d_index = _t(dev, pi), _t(dev, index)
    k = torch.full((m + 2 * MARGIN,), float(FILL_F32), device=dev)
    q = torch.full((m + 2 * MARGIN,), int(FILL_I32), dtype=torch.int32, device=dev)
    for off, n in chunks or ((0, m),):
        d_net = _t(dev, net[off:off + n])
        rc = lib.aqg_replay_surprise_rows(N, A, _lib.ptr(d_net), _lib.ptr(d_pi), _lib.ptr(d_index), pi.shape[0], m, off, n,
                                          _at(k, MARGIN), _at(q, MARGIN), _lib.stream_ptr(dev))
        assert rc == 0, lib.aqg_last_error()
        torch.cuda.synchronize()
        assert d_net.cpu().numpy().tobytes() == np.ascontiguousarray(net[off:off + n]).tobytes()
    assert d_pi.cpu().numpy().tobytes() == pi.tobytes()
    hk, hq = k.cpu().numpy(), q.cpu().numpy()
    for h, fill in ((hk, FILL_F32), (hq, FILL_I32)):
        assert np.all(h[:MARGIN] == fill) and np.all(h[m + MARGIN:] == fill)
    return hk[MARGIN:m + MARGIN], hq[MARGIN:m + MARGIN]


def _targets(pi, m, index):
    """The target rows the bar is computed on: the rows index names (zeros for an entry outside pi), non-finite entries as zeros."""
    rows = np.arange(m) if index is None else np.asarray(index)
    inside = (rows >= 0) & (rows < pi.shape[0])
    t = np.zeros((m, pi.shape[1]), np.float32)
    t[inside] = pi[rows[inside]]
    return np.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)


def _check_rows(dev, N, pi, net, index=None, chunks=None):
    from alphaquoridorgnn_amd.replay import surprise_reference, surprise_weights
    k, q = _rows_launch(dev, N, pi, net, index, chunks)
    k_ref, _ = surprise_reference(pi, net, index)
    ok = within_bar(k, k_ref, _targets(pi, net.shape[0], index))
    print(f"rows kernel {N}x{N} m={net.shape[0]}: max |k - k_ref| = {np.abs(k.astype(np.float64) - k_ref).max():.3e}")
    assert np.all(ok), (np.flatnonzero(~ok), k[~ok], k_ref[~ok])
    assert np.array_equal(q, surprise_weights(k))                # behind k: bit for bit
    return k, q


@pytest.mark.parametrize("N", BOARDS)
def test_rows_kernel_against_the_reference(dev, N):
    """m = 1, and one below, at and one above a wavefront's four rows, a workgroup's sixteen and four workgroups' sixty-four: all rows
    in order, and an index in an order of its own that skips ring rows filled with NaN."""
    A = policy_size(N)
    for m in SIZES:
        rng = np.random.RandomState(100 * N + m)
        pi, net = target_rows(rng, m + 9, A), network_rows(rng, m, A)
        k, _ = _check_rows(dev, N, pi, net)
        if m >= 15:
            assert k.max() > 0.5 and len(set(k.tolist())) > m // 2
        index = rng.permutation(m + 9)[:m].astype(np.int64)
        pi[np.setdiff1d(np.arange(m + 9), index)] = np.nan
        _check_rows(dev, N, pi, net, index)


@pytest.mark.parametrize("N", BOARDS)
def test_rows_kernel_in_chunks(dev, N):
    """40 rows in chunks of 16 (two whole, one of 8), each launch with its own policy buffer: the bits of the single launch."""
    A, rng = policy_size(N), np.random.RandomState(200 + N)
    pi, net = target_rows(rng, 55, A), network_rows(rng, 40, A)
    index = rng.permutation(55)[:40].astype(np.int64)
    seams = ((0, 16), (16, 16), (32, 8))
    for idx in (None, index):
        whole = _check_rows(dev, N, pi, net, idx)
        parts = _check_rows(dev, N, pi, net, idx, chunks=seams)
        assert whole[0].tobytes() == parts[0].tobytes() and np.array_equal(whole[1], parts[1])
    # a launch of a middle chunk alone writes its own rows and no other
    k, q = _rows_launch(dev, N, pi, net, index, chunks=((16, 16),))
    assert np.all(k[:16] == FILL_F32) and np.all(k[32:] == FILL_F32) and np.all(q[:16] == FILL_I32) and np.all(q[32:] == FILL_I32)
    assert k[16:32].tobytes() == whole[0][16:32].tobytes()


@pytest.mark.parametrize("N", BOARDS)
def test_rows_kernel_special_and_exact_rows(dev, N):
    """Every special row reads k = 0 and q = 0 (bit for bit), alone in its wavefront's group and beside ordinary rows; an index entry
    outside the ring is one more; t == p and the one-hot target on p = 1 give +0.0 exactly; p = 0 under a positive target is the
    reference's value within the bar."""
    A, rng = policy_size(N), np.random.RandomState(300 + N)
    pi, net = special_rows(rng, A)
    k, q = _check_rows(dev, N, pi, net)
    assert k.tobytes() == np.zeros(len(SPECIAL), np.float32).tobytes() and not q.any(), dict(zip(SPECIAL, k))
    more_pi, more_net = target_rows(rng, 6, A), network_rows(rng, 6, A)
    order = rng.permutation(len(SPECIAL) + 6)
    mixed_pi, mixed_net = np.concatenate([pi, more_pi])[order], np.concatenate([net, more_net])[order]
    k, q = _check_rows(dev, N, mixed_pi, mixed_net)
    assert not k[order < len(SPECIAL)].any() and np.all(k[order >= len(SPECIAL)] > 0)
    k, q = _check_rows(dev, N, more_pi, more_net, index=np.array([0, 6, 2, -1, 4, 2 ** 40], np.int64))
    assert k[[1, 3, 5]].tobytes() == np.zeros(3, np.float32).tobytes() and not q[[1, 3, 5]].any() and np.all(k[[0, 2, 4]] > 0)
    pi, net, want = exact_rows(rng, A)
    k, q = _check_rows(dev, N, pi, net)
    assert len(want) == len(EXACT) and k[:2].tobytes() == np.zeros(2, np.float32).tobytes() and not q[:2].any()
    assert abs(float(k[2]) - 126 * np.log(2)) < 1e-5 and abs(float(k[3]) - 62.5 * np.log(2)) < 1e-5


# ------------------------------------------------------------------ the counts kernel
def _counts_launch(dev, q, slots, seed, update, E, U, C, total=None):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    m = q.shape[0]
    d_q, d_slots = _t(dev, q), _t(dev, slots)
    d_total = torch.tensor([int(q.astype(np.int64).sum()) if total is None else total], dtype=torch.int64, device=dev)
    count = torch.full((m + 2 * MARGIN,), int(FILL_I32), dtype=torch.int32, device=dev)
    rc = lib.aqg_replay_surprise_counts(_lib.ptr(d_q), _lib.ptr(d_slots), _lib.ptr(d_total), m, E, U, C, seed, update, _at(count, MARGIN),
                                        _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0, lib.aqg_last_error()
    h = count.cpu().numpy()
    assert np.all(h[:MARGIN] == FILL_I32) and np.all(h[m + MARGIN:] == FILL_I32) and np.array_equal(d_q.cpu().numpy(), q)
    return h[MARGIN:m + MARGIN]


def test_counts_kernel_equals_numpy_bit_for_bit(dev):
    """The sizes of the rows kernel, and one below, at and one above the counts launch's 256 rows a workgroup; with ring slots and
    without; E below, at and above m; U = 0, 0.5 and 1; C = 1, 8 and 255."""
    from alphaquoridorgnn_amd.replay import surprise_counts_reference
    for m in SIZES + (255, 256, 257, 1000):
        rng = np.random.RandomState(m)
        q = (rng.exponential(0.4, m) * 2 ** 20).astype(np.int32)
        q[rng.permutation(m)[:m // 3]] = 0
        slots = rng.permutation(5 * m + 7)[:m].astype(np.int64)
        for s, (E, U, C) in enumerate(((m, 0.5, 8), (max(m // 3, 1), 0.0, 1), (4 * m + 3, 0.25, 255), (2 * m, 1.0, 8), (m, 0.9, 2))):
            for rows in (slots, None):
                got = _counts_launch(dev, q, rows, 17 + s, m, E, U, C)
                assert np.array_equal(got, surprise_counts_reference(q, rows, 17 + s, m, E, U, C)), (m, E, U, C)


def test_counts_kernel_on_crafted_weights(dev):
    """All zero (uniform); one dominant row that hits C; f with a fraction of exactly 0 and of exactly 0.5; U = 1 at m = 49; a seed and
    an update of 64 bits."""
    from alphaquoridorgnn_amd.replay import surprise_counts_reference
    big = (1 << 64) - 3
    zero = np.zeros(49, np.int32)
    assert _counts_launch(dev, zero, None, 1, 2, 49, 0.5, 8).tolist() == [1] * 49
    assert _counts_launch(dev, zero, None, 1, 2, 3 * 49, 0.0, 8).tolist() == [3] * 49
    half = _counts_launch(dev, zero, None, big, big - 5, 98, 0.5, 8, total=0)
    assert np.array_equal(half, surprise_counts_reference(zero, None, big, big - 5, 98, 0.5, 8)) and half.tolist() == [2] * 49
    some = _counts_launch(dev, zero, None, big, big - 5, 24, 0.5, 8)
    assert np.array_equal(some, surprise_counts_reference(zero, None, big, big - 5, 24, 0.5, 8)) and set(some.tolist()) == {0, 1}
    q = np.random.RandomState(3).randint(0, 2 ** 26, 49).astype(np.int32)
    assert _counts_launch(dev, q, None, 5, 6, 49, 1.0, 8).tolist() == [1] * 49
    assert _counts_launch(dev, q, None, 5, 6, 98, 1.0, 8).tolist() == [2] * 49
    q = np.zeros(64, np.int32)
    q[5] = 80 * 2 ** 20
    got = _counts_launch(dev, q, None, 0, 0, 64, 0.5, 8)
    assert got[5] == 8 and np.array_equal(got, surprise_counts_reference(q, None, 0, 0, 64, 0.5, 8)) and set(np.delete(got, 5).tolist()) == {0, 1}
    assert _counts_launch(dev, np.array([1, 1, 2, 4], np.int32), None, 3, 9, 16, 0.5, 5).tolist() == [3, 3, 4, 5]
    q = np.array([1, 3], np.int32)
    assert np.array_equal(_counts_launch(dev, q, None, 3, 9, 4, 0.5, 8), surprise_counts_reference(q, None, 3, 9, 4, 0.5, 8))


# ------------------------------------------------------------------ end to end
def _played_window(dev, N, games=4, sims=8):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.replay import ReplayWindow
    w = ReplayWindow(N, max_generations=2, device=dev)
    for g in range(2):
        eng = BatchedSelfPlay(None, num_games=games, sims=sims, board_size=N, evaluator="fake", fake_bias=0, seed=70 + g)
        eng.play_generation()
        w.append_counts(*eng.history_tensors())
    return w


def _network(kind, N, dev):
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    torch.manual_seed(40 + N)
    if kind == "cnn":
        net = CNNNetwork(16, 2, board_size=N)
        with torch.no_grad():
            for mod in net.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.uniform_(-0.3, 0.3)
                    mod.running_var.uniform_(0.5, 2.0)
        return net.to(dev)
    return GraphPolicyValueNetwork(6, kind[0], kind[1], policy_size(N), board_size=N).to(dev)


def _check_index(result, h_pi, h_slots, net, seed, update, E, U, C):
    """(index, k, count) of surprise_index: k within the bar of the reference fed the network's policy; q, the counts and the index bit
    for bit from the numpy statements fed the device's k.  Returns the counts."""
    from alphaquoridorgnn_amd.replay import surprise_counts_reference, surprise_reference, surprise_weights
    index, k, count = result
    hk = k.cpu().numpy()
    k_ref, _ = surprise_reference(h_pi, net, h_slots)
    assert k.dtype == torch.float32 and np.all(within_bar(hk, k_ref, h_pi[h_slots])) and hk.max() > 0
    want = surprise_counts_reference(surprise_weights(hk), h_slots, seed, update, E, U, C)
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), want)
    assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), np.repeat(h_slots, want))
    return want


@pytest.mark.parametrize("kind,N", [((128, 3), 5), ((128, 3), 9), ((64, 2), 5), ("cnn", 5)])
def test_surprise_index_end_to_end(dev, kind, N):
    """On the generations of a tiny self-play: k within the bar, q, the counts and the index bit for bit (_check_index); the same in
    chunks of 16 rows; the module's mode, its parameters and its running statistics are as they were; the window's counter advances;
    the statistics are the counts'."""
    from alphaquoridorgnn_amd.replay import surprise_index
    w = _played_window(dev, N)
    model = _network(kind, N, dev).train()
    state = {name: x.detach().clone() for name, x in model.state_dict().items()}
    s72, pi, _ = w.tensors()
    slots, m = w.index(), len(w)
    assert m > 40
    stats = {}
    first = w.surprise_index(model, seed=5, stats=stats)
    assert model.training and w.surprise_updates == 1
    assert all(torch.equal(x, state[name]) for name, x in model.state_dict().items())
    model.eval()
    with torch.no_grad():
        net = model.forward_states(s72.index_select(0, slots).contiguous())[0].cpu().numpy()
    h_pi, h_slots = pi.cpu().numpy(), slots.cpu().numpy()
    want = _check_index(first, h_pi, h_slots, net, 5, 0, m, 0.5, 8)
    hk = first[1].cpu().numpy()
    assert stats == dict(rows=m, expanded=int(want.sum()), left_out=int((want == 0).sum()), most_copies=int(want.max()),
                         mean_kl=stats["mean_kl"]) and abs(stats["mean_kl"] - hk.astype(np.float64).mean()) < 1e-9
    assert 0 < stats["left_out"] < m and stats["most_copies"] > 1
    _check_index(w.surprise_index(model, seed=5, update=0, chunk_rows=16), h_pi, h_slots, net, 5, 0, m, 0.5, 8)
    assert w.surprise_updates == 1 and not model.training
    _check_index(w.surprise_index(model, seed=6, expected_rows=2 * m + 1, uniform_share=0.25, max_copies=3), h_pi, h_slots, net, 6, 1,
                 2 * m + 1, 0.25, 3)
    assert w.surprise_updates == 2
    rows = [x.contiguous() for x in w.rows()[:2]]
    index3, k3, count3 = surprise_index(model, *rows, seed=5, update=0, uniform_share=1.0)
    assert torch.equal(index3, torch.arange(m, device=dev)) and count3.tolist() == [1] * m
    assert np.all(within_bar(k3.cpu().numpy(), hk, h_pi[h_slots]))
    with pytest.raises(ValueError):
        surprise_index(model, *rows, seed=5, update=0, uniform_share=1.5)
    with pytest.raises(ValueError):
        surprise_index(model, *rows, seed=5, update=0, max_copies=0)
    with pytest.raises(ValueError):
        surprise_index(model, rows[0].cpu(), rows[1].cpu(), seed=5, update=0)
    empty = surprise_index(model, rows[0][:0], rows[1][:0], seed=5, update=0)
    assert [tuple(x.shape) for x in empty] == [(0,), (0,), (0,)]


# ------------------------------------------------------------------ refusals
def test_the_c_entries_refuse_on_the_host(dev):
    """Every refusal of the two entries, made before any launch: -1 with a message, outputs and sources as they were."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, A, rows, m = 5, policy_size(5), 30, 20
    rng = np.random.RandomState(0)
    host = [network_rows(rng, m, A), target_rows(rng, rows, A), rng.permutation(rows)[:m].astype(np.int64)]
    net, pi, index = [_t(dev, x) for x in host]
    k = torch.full((m,), float(FILL_F32), device=dev)
    q = torch.full((m,), int(FILL_I32), dtype=torch.int32, device=dev)
    count = torch.full((m,), int(FILL_I32), dtype=torch.int32, device=dev)
    total = torch.tensor([12345], dtype=torch.int64, device=dev)
    st, p = _lib.stream_ptr(dev), _lib.ptr

    def refused(rc, word):
        assert rc == -1 and word in lib.aqg_last_error().decode(), (rc, lib.aqg_last_error())

    def rows_call(board=N, policy=A, net_=p(net), pi_=p(pi), index_=p(index), ring=rows, total_rows=m, offset=0, n=m, k_=p(k), q_=p(q)):
        return lib.aqg_replay_surprise_rows(board, policy, net_, pi_, index_, ring, total_rows, offset, n, k_, q_, st)

    for board in (4, 11, 0):
        refused(rows_call(board=board), "board_size")
    refused(rows_call(policy=A + 1), "policy_size")
    refused(rows_call(total_rows=-1), "m out of range")
    refused(rows_call(total_rows=(1 << 24) + 1), "m out of range")
    refused(rows_call(index_=None, total_rows=rows + 1, n=1), "m out of range")
    refused(rows_call(ring=-1), "negative")
    refused(rows_call(offset=-1), "chunk")
    refused(rows_call(n=-1), "chunk")
    refused(rows_call(offset=1), "chunk")
    refused(rows_call(offset=m, n=1), "chunk")
    for name in ("net_", "pi_", "k_", "q_"):
        refused(rows_call(**{name: None}), "must be given")
    refused(rows_call(k_=_at(net, m * A - 1)), "overlaps a source")
    refused(rows_call(q_=_at(pi, A - 1)), "overlaps a source")                  # inside the one certain row of a gathered ring
    refused(rows_call(k_=ctypes.c_void_p(index.data_ptr() + 8 * m - 4)), "overlaps a source")
    refused(rows_call(q_=_at(k, m - 1)), "k overlaps q")
    assert rows_call(n=0, net_=None, pi_=None, index_=None, k_=None, q_=None) == 0
    assert rows_call(total_rows=0, n=0, net_=None, pi_=None, index_=None, k_=None, q_=None) == 0

    def counts_call(q_=p(q), index_=p(index), total_=p(total), n=m, E=m, U=0.5, C=8, count_=p(count)):
        return lib.aqg_replay_surprise_counts(q_, index_, total_, n, E, U, C, 1, 2, count_, st)

    refused(counts_call(n=-1), "m out of range")
    refused(counts_call(n=(1 << 24) + 1), "m out of range")
    for U in (-0.01, 1.01, float("nan"), float("inf")):
        refused(counts_call(U=U), "uniform_share")
    for C in (0, -1, 256):
        refused(counts_call(C=C), "max_copies")
    for E in (0, -5, (1 << 40) + 1):
        refused(counts_call(E=E), "expected_rows")
    for name in ("q_", "total_", "count_"):
        refused(counts_call(**{name: None}), "must be given")
    refused(counts_call(count_=_at(q, m - 1)), "overlaps a source")
    refused(counts_call(count_=ctypes.c_void_p(index.data_ptr() + 8 * m - 4)), "overlaps a source")
    refused(counts_call(count_=ctypes.c_void_p(total.data_ptr() + 4)), "overlaps a source")
    assert counts_call(n=0, q_=None, index_=None, total_=None, count_=None) == 0
    torch.cuda.synchronize()
    for x, hx in zip((net, pi, index), host):
        assert x.cpu().numpy().tobytes() == hx.tobytes()
    for x, fill in ((k, FILL_F32), (q, FILL_I32), (count, FILL_I32)):
        assert bool((x == (float(fill) if x.is_floating_point() else int(fill))).all())
    assert rows_call() == 0 and counts_call() == 0                  # and the calls they were variations of are good ones
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the loop end to end
_LOOP = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, train_network as tn
from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork, load_network as load_cnn
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, load_network, pack_states
from alphaquoridorgnn_amd.replay import (KEY_BYTES, ReplayWindow, merge_reference, surprise_counts_reference, surprise_index,
                                         surprise_weights)

g = np.load(os.path.join(os.environ["AQG_REPO"], "tests", "golden", "cnn_train_5x5.npz"))
rows = [[[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:20]]], p.tolist(), int(z)]
        for s, p, z in zip(g["states"], g["pi"], g["z"])]
_, first = np.unique(pack_states([r[0] for r in rows], 5)[:, KEY_BYTES], axis=0, return_index=True)
rows = [rows[i] for i in sorted(first)]                       # the golden rows repeat positions: each one once
assert len(rows) == 25 and constants.BOARD_SIZE == 5
older = [[s, [0.25 * x + 0.75 / 57 for x in p], -z] for s, p, z in rows[:15]]      # the first 15 positions again, other targets
os.makedirs("data")
with open("data/20260101000001.history", "wb") as f:
    pickle.dump(rows, f)
os.makedirs(constants.PV_NETWORK_PATH)
BEST = constants.PV_NETWORK_PATH + "best.pth"
tn.NUM_EPOCH = 2
dev = aqd.device()
train, load = tn.train_network, load_network


def run():
    torch.manual_seed(11)               # the epochs' shuffles
    train()
    with open(constants.PV_NETWORK_PATH + "latest.pth", "rb") as f:
        return f.read()


def window(histories, generations=2):
    w = ReplayWindow(5, max_generations=generations, device=dev)
    for h in histories:
        w.append_history(h)
    return w


def expansion(s, p, index, update, share=0.5):
    """The host-built index: the numpy statements fed the device's k of best.pth on these rows."""
    _, k, _ = surprise_index(load(BEST, dev), s, p, index, seed=tn.TRAIN_SURPRISE_SEED, update=update, uniform_share=share)
    slots = np.arange(len(k)) if index is None else index.cpu().numpy()
    count = surprise_counts_reference(surprise_weights(k.cpu().numpy()), slots, tn.TRAIN_SURPRISE_SEED, update, len(k), share, 8)
    return np.repeat(slots, count), count


def on_the_expansion(w, index):
    """The option off on a window whose index() is `index`."""
    keep, w._index = w._index, torch.from_numpy(index).to(dev)
    tn.TRAIN_WINDOW, tn.TRAIN_SURPRISE_WEIGHTING = w, False
    try:
        return run()
    finally:
        w._index = keep


def suite(tag):
    two = window([older, rows])
    tn.TRAIN_WINDOW, tn.TRAIN_SURPRISE_WEIGHTING = two, False
    off = run()
    tn.TRAIN_SURPRISE_WEIGHTING, tn.TRAIN_SURPRISE_UNIFORM_SHARE = True, 1.0
    print(tag, "SHARE_ONE_IS_OFF", run() == off, two.surprise_updates == 1)
    tn.TRAIN_SURPRISE_UNIFORM_SHARE = 0.5
    on = run()
    index, count = expansion(two.tensors()[0], two.tensors()[1], two.index(), 1)
    print(tag, "HALF_IS_THE_HOST_EXPANSION", on_the_expansion(two, index) == on, on != off, two.surprise_updates == 2,
          0 < int((count == 0).sum()) < 40, int(count.max()) > 1)
    tn.TRAIN_SURPRISE_WEIGHTING, tn.TRAIN_MIRROR, tn.TRAIN_EPOCH_ROWS, tn.TRAIN_WINDOW = True, True, 24, two
    mirrored = run()
    index, _ = expansion(two.tensors()[0], two.tensors()[1], two.index(), 2)
    print(tag, "MIRROR_AND_EPOCH_ROWS", on_the_expansion(two, index) == mirrored, mirrored != on)
    tn.TRAIN_MIRROR, tn.TRAIN_EPOCH_ROWS = False, None
    return two


# ---- the GNN (a 6/16/2 network: GeneralTrainer) and the default 6/128/3 (GNNTrainer)
torch.manual_seed(3)
torch.save(GraphPolicyValueNetwork(6, 16, 2, 57, board_size=5).state_dict(), BEST)
two = suite("GENERAL")
# with the merge in front: the merged rows are compact (index None), a row's draw is keyed by its merged row
tn.TRAIN_WINDOW, tn.TRAIN_SURPRISE_WEIGHTING, tn.TRAIN_MERGE_POSITIONS = two, True, True
merged_on = run()
s, p, z = (x.cpu().numpy() for x in two.rows())
merged = merge_reference(s, p, z)
host = ReplayWindow(5, max_generations=1, device=dev)
host.append_rows(*(torch.from_numpy(x) for x in merged[:3]))
tn.TRAIN_MERGE_POSITIONS = False
index, count = expansion(host.tensors()[0][:25].contiguous(), host.tensors()[1][:25].contiguous(), None, 3)
print("MERGE_THEN_SURPRISE", on_the_expansion(host, index) == merged_on, len(count) == 25, two.surprise_updates == 4)
# the file route: no window, the module's counter
tn.TRAIN_WINDOW, tn.TRAIN_SURPRISE_WEIGHTING = None, True
before = tn._surprise_updates
file_on = run()
one = window([rows], 1)
index, _ = expansion(one.tensors()[0], one.tensors()[1], one.index(), before)
print("FILE_ROUTE", on_the_expansion(one, index) == file_on, tn._surprise_updates == before + 1, one.surprise_updates == 0)
torch.manual_seed(4)
torch.save(GraphPolicyValueNetwork(6, 128, 3, 57, board_size=5).state_dict(), BEST)
suite("FUSED")
# ---- the residual CNN
torch.manual_seed(5)
torch.save(CNNNetwork(8, 1, board_size=5).state_dict(), BEST)
train, load = tn.train_cnn_network, load_cnn
suite("CNN")
'''


def test_the_loop_with_surprise_weighting(dev, tmp_path):
    """One child process on the 5x5 board, NUM_EPOCH = 2, a window of two generations (40 rows): with U = 1 latest.pth is the option
    off's, byte for byte under the same torch seed; with U = 0.5 it is, byte for byte, the option off on a window whose index() is the
    expansion built on the host from the numpy statements fed the device's k -- also with the mirror and TRAIN_EPOCH_ROWS on top, with
    the merge in front, on the file route, and for all three trainers."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    want = [f"{tag} {line}" for tag in ("GENERAL", "FUSED", "CNN")
            for line in ("SHARE_ONE_IS_OFF True True", "HALF_IS_THE_HOST_EXPANSION True True True True True", "MIRROR_AND_EPOCH_ROWS True True")]
    for line in want + ["MERGE_THEN_SURPRISE True True True", "FILE_ROUTE True True True"]:
        assert line in r.stdout, (line, [x for x in r.stdout.splitlines() if x[:1].isupper() and "Epoch" not in x])
    assert "surprise weighting: 40 rows -> 40 rows, 0 left out, most copies 1, mean KL " in r.stdout
    assert "merged positions: 40 rows, 25 positions, longest run 2\nsurprise weighting: 25 rows -> " in r.stdout


_CYCLE = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
from alphaquoridorgnn_amd import constants, train_cycle as tc, train_network as tn
tc.main(["--cycles", "1", "--games", "6", "--sims", "6", "--epochs", "2", "--eval-games", "2", "--hidden-dim", "32", "--num-gcn-layers", "2",
         "--replay-generations", "2", "--surprise-weighting", "--surprise-uniform-share", "0.25", "--surprise-max-copies", "4",
         "--surprise-seed", "21"])
print("SETTINGS", tn.TRAIN_SURPRISE_WEIGHTING, tn.TRAIN_SURPRISE_UNIFORM_SHARE, tn.TRAIN_SURPRISE_MAX_COPIES, tn.TRAIN_SURPRISE_SEED,
      tn.TRAIN_WINDOW.surprise_updates, os.path.exists(constants.PV_NETWORK_PATH + "latest.pth"))
'''


def test_one_cycle_with_surprise_weighting(dev, tmp_path):
    """train_cycle --surprise-weighting with its three coefficients on 5x5: the update prints the stage's line, the window's counter has
    advanced once, latest.pth is written."""
    import re
    (tmp_path / "cycle.py").write_text(_CYCLE)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "cycle.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "SETTINGS True 0.25 4 21 1 True" in r.stdout, r.stdout[-2000:]
    line = re.search(r"surprise weighting: (\d+) rows -> (\d+) rows, (\d+) left out, most copies (\d+), mean KL ([0-9.]+)", r.stdout)
    assert line, r.stdout[-2000:]
    n, M, left, most = (int(x) for x in line.groups()[:4])
    assert n > 0 and 0 < M <= 4 * n and left < n and 1 <= most <= 4 and "Epoch 2/2" in r.stdout
