"""The mirror-symmetry augmentation on the GPU: aqg_augment_gather (csrc/augment.hip) against its numpy statement bit for bit, the
seeded draw against train_network.draw_mirror_flips, the mirror as a symmetry of the device's rules, a mirrored epoch / step of each
trainer against the same epoch / step on host-mirrored data, the refusals, and train_network() with TRAIN_MIRROR on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _util as U   # noqa: E402
from tests.test_mirror_augment_cpu import augment_reference   # noqa: E402

pytestmark = pytest.mark.gpu

CANARY_ROWS = 3
CANARY_U8, CANARY_F32 = 0xA5, np.float32(-7.25)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _rows(N, rows, seed):
    """Source rows that leave nothing to luck: every record byte random (positions off the board, wall values above 2 and the bytes
    behind the wall slots included) except byte 70 = N; pi random bit patterns' worth of floats with -0.0 and NaNs of two payloads."""
    rng = np.random.RandomState(seed)
    S = rng.randint(0, 256, size=(rows, 72)).astype(np.uint8)
    on_board = rng.rand(rows, 2) < 0.8
    S[:, 0] = np.where(on_board[:, 0], rng.randint(0, N * N, rows), S[:, 0])
    S[:, 2] = np.where(on_board[:, 1], rng.randint(0, N * N, rows), S[:, 2])
    S[:, 70] = N
    P = rng.randn(rows, _A(N)).astype(np.float32)
    bits = P.view(np.int32)
    kind = rng.randint(0, 12, size=P.shape)
    P[kind == 0] = -0.0
    bits[kind == 1] = 0x7FC00001
    bits[kind == 2] = np.int32(-4194299)               # 0xFFC00005: a negative NaN with a payload
    Z = rng.choice([-1.0, 0.0, 1.0], rows).astype(np.float32)
    return S, P, Z


def _launch(dev, N, S, P, Z, order, flips, n, use_seed=0, seed=0, epoch=0):
    """aqg_augment_gather through the binding on outputs with CANARY_ROWS rows of a pattern behind row n; returns the n rows of each
    output as numpy after checking the canaries."""
    from alphaquoridorgnn_amd import _lib
    A = _A(N)
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    dS, dP, dZ, dO, dF = t(S), t(P), t(Z), t(order), t(flips)
    m = n + CANARY_ROWS
    oS = None if S is None else torch.full((m, 72), CANARY_U8, dtype=torch.uint8, device=dev)
    oP = None if P is None else torch.full((m, A), float(CANARY_F32), dtype=torch.float32, device=dev)
    oZ = None if Z is None else torch.full((m,), float(CANARY_F32), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().aqg_augment_gather(N, A, _lib.ptr(dS), _lib.ptr(dP), _lib.ptr(dZ), _lib.ptr(dO), _lib.ptr(dF), use_seed, seed,
                                              epoch, n, _lib.ptr(oS), _lib.ptr(oP), _lib.ptr(oZ), _lib.stream_ptr(dev)),
               "aqg_augment_gather")
    out = []
    for o, canary in ((oS, CANARY_U8), (oP, CANARY_F32), (oZ, CANARY_F32)):
        if o is None:
            out.append(None)
            continue
        h = o.cpu().numpy()
        assert (h[n:] == canary).all(), "a row behind n was written"
        out.append(h[:n])
    return out


def _same(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape
            assert np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g, w.view(np.int32) if w.dtype == np.float32 else w)


# ------------------------------------------------------------------ the kernel against numpy
@pytest.mark.parametrize("N", (3, 5, 7, 9))
def test_kernel_equals_numpy_bit_for_bit(dev, N):
    """One row; n on either side of 64 = four workgroups of 16 rows (63 ends inside a wavefront's group of 4 rows, 65 opens a
    workgroup with one row); a ragged tail behind 16 workgroups.  Every order form x every flip form; outputs compared as bit
    patterns, canary rows behind n intact."""
    rng = np.random.RandomState(100 + N)
    for n in (1, 63, 64, 65, 257):
        for order_kind in ("none", "permutation", "repeats"):
            rows = n + 5 if order_kind == "repeats" else n
            S, P, Z = _rows(N, rows, seed=1000 * N + n)
            order = {"none": None, "permutation": rng.permutation(rows).astype(np.int64),
                     "repeats": rng.randint(0, rows, size=n).astype(np.int64)}[order_kind]
            if order_kind == "repeats" and n > 1:
                order[1] = order[0]
                assert len(set(order.tolist())) < rows            # repeated and omitted rows
            for flips in (None, np.ones(rows, np.uint8), (np.arange(rows) % 2).astype(np.uint8),
                          rng.randint(0, 2, size=rows).astype(np.uint8) * rng.randint(1, 256, size=rows).astype(np.uint8)):
                _same(_launch(dev, N, S, P, Z, order, flips, n), augment_reference(N, S, P, Z, order, flips))
    n, rows = 65, 70
    S, P, Z = _rows(N, rows, seed=77 + N)
    order = rng.randint(0, rows, size=n).astype(np.int64)
    flips = rng.randint(0, 2, size=rows).astype(np.uint8)
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)):           # states-only, policy-only, ...
        s, p, z = (x if k else None for x, k in zip((S, P, Z), keep))
        _same(_launch(dev, N, s, p, z, order, flips, n), augment_reference(N, s, p, z, order, flips))
    # a flipped record's pawns: the formula of the header, the off-board bytes copied through
    got = _launch(dev, N, S, None, None, None, np.ones(rows, np.uint8), rows)[0]
    on = S[:, 0] < N * N
    assert np.array_equal(got[on, 0], (S[on, 0] // N) * N + (N - 1 - S[on, 0] % N)) and np.array_equal(got[~on, 0], S[~on, 0])
    assert (~on).any() and on.any()
    assert _launch(dev, N, S, P, Z, None, None, 0)[0].shape == (0, 72)               # n = 0: nothing is launched or written


def test_zero_rows_and_more_rows_than_the_source(dev):
    """An empty order over a non-empty source gives empty outputs (their pointers are NULL), in every entry point; an order longer
    than the source is gathered too, also into an output that starts right behind the shorter source."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd import train_network as tn
    N, rows = 5, 20
    S, P, Z = _rows(N, rows, seed=4)
    dS, dP, dZ = (torch.from_numpy(x).to(dev) for x in (S, P, Z))
    none = torch.zeros((0,), dtype=torch.int64, device=dev)
    table = torch.ones(rows, dtype=torch.uint8, device=dev)
    for out in (tn.augment_gather(dS, dP, dZ, order=none, board_size=N), tn.augment_gather(dS, dP, dZ, order=none, seed=3, board_size=N),
                tn._augment_launch(N, dS, dP, dZ, none, table), tn._augment_launch(N, dS, dP, dZ, none, (3, 1)),
                tn._augment_launch(N, dS, None, None, none, None)):
        assert [None if x is None else tuple(x.shape) for x in out][0] == (0, 72)
        assert all(x is None or x.shape[0] == 0 for x in out)
    # the library itself: NULL outputs beside a non-empty source are what an empty array hands it
    assert _lib.load().aqg_augment_gather(N, _A(N), _lib.ptr(dS), _lib.ptr(dP), _lib.ptr(dZ), _lib.ptr(none), _lib.ptr(table), 0, 0, 0, 0,
                                          None, None, None, _lib.stream_ptr(dev)) == 0
    e = tuple(x[:0] for x in (dS, dP, dZ))
    assert all(x.shape[0] == 0 for x in tn.augment_gather(*e, board_size=N))
    order = np.random.RandomState(6).randint(0, rows, size=3 * rows).astype(np.int64)
    flips = (np.arange(rows) % 3 == 0).astype(np.uint8)
    d_order, d_flips = torch.from_numpy(order).to(dev), torch.from_numpy(flips).to(dev)      # named: alive until the launch has run
    got = tn.augment_gather(dS, dP, dZ, order=d_order, flips=d_flips, board_size=N)
    _same([x.cpu().numpy() for x in got], augment_reference(N, S, P, Z, order, flips))
    buf = torch.full(((rows + 3 * rows + 1) * 72,), CANARY_U8, dtype=torch.uint8, device=dev)       # source | output | canary row
    buf[:rows * 72] = dS.reshape(-1)
    src, out = buf[:rows * 72], buf[rows * 72:]
    _lib.check(_lib.load().aqg_augment_gather(N, _A(N), _lib.ptr(src), None, None, _lib.ptr(d_order), _lib.ptr(d_flips), 0, 0, 0,
                                              3 * rows, _lib.ptr(out), None, None, _lib.stream_ptr(dev)), "aqg_augment_gather")
    h = buf.cpu().numpy()
    assert np.array_equal(h[:rows * 72].reshape(rows, 72), S) and (h[-72:] == CANARY_U8).all()
    assert np.array_equal(h[rows * 72:-72].reshape(3 * rows, 72), augment_reference(N, S, None, None, order, flips)[0])


def test_seeded_mode_equals_table_mode(dev):
    from alphaquoridorgnn_amd.train_network import augment_gather, draw_mirror_flips
    N, rows = 9, 300
    S, P, Z = _rows(N, rows, seed=5)
    dS, dP, dZ = (torch.from_numpy(x).to(dev) for x in (S, P, Z))
    order = torch.from_numpy(np.random.RandomState(8).permutation(rows)[:257]).to(dev)
    seen = []
    for seed, epoch in ((20261018, 0), (20261018, 1), (2 ** 64 - 1, 7)):
        table = draw_mirror_flips(seed, epoch, rows)
        a = augment_gather(dS, dP, dZ, order=order, seed=seed, epoch=epoch, board_size=N)
        b = augment_gather(dS, dP, dZ, order=order, flips=torch.from_numpy(table).to(dev), board_size=N)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
        _same([x.cpu().numpy() for x in a], augment_reference(N, S, P, Z, order.cpu().numpy(), table))
        # the raw entry point in seeded mode, for a shuffled order and for none
        _same(_launch(dev, N, S, P, Z, order.cpu().numpy(), None, 257, use_seed=1, seed=seed, epoch=epoch),
              augment_reference(N, S, P, Z, order.cpu().numpy(), table))
        _same(_launch(dev, N, S, P, Z, None, None, rows, use_seed=1, seed=seed, epoch=epoch), augment_reference(N, S, P, Z, None, table))
        seen.append(table)
    assert not np.array_equal(seen[0], seen[1])                 # the epoch changes the draw
    plain = augment_gather(dS, dP, dZ, order=order, board_size=N)                     # neither: a plain gather
    for x, src in zip(plain, (dS, dP, dZ)):
        y = src.index_select(0, order)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


# ------------------------------------------------------------------ the rules on the device
@pytest.mark.parametrize("N", (3, 5, 9))
def test_device_rules_commute_with_the_mirror(dev, N):
    from alphaquoridorgnn_amd.game_logic import legal_actions_batch, mirror_actions, mirror_batch, mirror_policy_batch, next_batch
    g = U.golden(f"walk_{N}x{N}.npz")
    pick = slice(None) if N < 9 else slice(0, 14000, 27)
    recs, actions = g["states"][pick], g["actions"][pick]
    if N == 9:
        recs, actions = recs[:512], actions[:512]
        assert recs.shape[0] == 512
    S = torch.from_numpy(np.ascontiguousarray(recs)).to(dev)
    M = mirror_batch(S, N)
    assert torch.equal(mirror_batch(M, N), S) and not torch.equal(M, S)
    mask, _, count = legal_actions_batch(S, N)
    mmask, _, mcount = legal_actions_batch(M, N)
    assert torch.equal(mcount, count)
    assert torch.equal(mmask, mirror_policy_batch(mask.float(), N).to(torch.uint8))
    assert int(count.sum()) > 0
    played = actions >= 0
    assert played.sum() >= recs.shape[0] // 2
    a = torch.from_numpy(actions[played].astype(np.int32)).to(dev)
    ma = torch.from_numpy(mirror_actions(actions[played], N).astype(np.int32)).to(dev)
    idx = torch.from_numpy(np.flatnonzero(played)).to(dev)
    assert torch.equal(mirror_batch(next_batch(S[idx].contiguous(), a, N), N), next_batch(M[idx].contiguous(), ma, N))


# ------------------------------------------------------------------ the trainers
def _make(kind, dev):
    """(trainer class, a fresh model of fixed weights on the device, board size) of one small model per trainer."""
    from alphaquoridorgnn_amd import train_network as tn
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    torch.manual_seed(31)
    if kind == "gnn":
        return tn.GNNTrainer, GraphPolicyValueNetwork(6, 128, 3, _A(9), board_size=9).to(dev).eval(), 9
    if kind == "general":
        return tn.GeneralTrainer, GraphPolicyValueNetwork(6, 16, 2, _A(5), board_size=5).to(dev).eval(), 5
    return tn.CNNTrainer, CNNNetwork(8, 1, board_size=5).to(dev).eval(), 5


def _training_rows(N, n, seed):
    states = U.golden(f"walk_{N}x{N}.npz")["states"]
    recs = np.ascontiguousarray(states[:: states.shape[0] // n][:n])
    rng = np.random.RandomState(seed)
    A = _A(N)
    pi = rng.rand(n, A) * (rng.rand(n, A) < 0.2)
    pi[:, 0] += 1e-3
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    z = rng.choice([-1.0, 0.0, 1.0], n).astype(np.float32)
    return recs, pi, z


def _snapshot(trainer, result):
    """Everything a run leaves behind: parameters, Adam moments, running statistics and counters (CNN), the returned losses."""
    out = [p.detach().clone() for p in trainer.params] + [x.clone() for x in trainer.adam_m + trainer.adam_v]
    out += [b.detach().clone() for b in trainer.model.buffers()]
    out += [torch.stack([x.reshape(()) for x in result]) if isinstance(result, tuple) else result.clone()]
    return out


def _identical(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                                       y.view(torch.int32) if y.dtype == torch.float32 else y)
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ("gnn", "general", "cnn"))
def test_mirrored_training_equals_training_on_host_mirrored_rows(dev, kind):
    """37 positions in batches of 16 (two full steps and a short one): run_epoch(mirror=table) and step(mirror=table) leave the
    trainer bit-identical to the same call without `mirror` on a host-mirrored copy of the rows; mirror=None is the call without it."""
    n, batch = 37, 16
    _, _, N = _make(kind, dev)
    recs, pi, z = _training_rows(N, n, seed=3)
    rng = np.random.RandomState(12)
    table = rng.randint(0, 2, size=n).astype(np.uint8)
    assert 0 < table.sum() < n
    order = torch.from_numpy(rng.permutation(n)).to(dev)
    mrecs, mpi, mz = augment_reference(N, recs, pi, z, None, table)
    assert not np.array_equal(mrecs, recs) and not np.array_equal(mpi, pi)
    d = lambda *xs: tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs)   # noqa: E731
    plain, mirrored, dtable = d(recs, pi, z), d(mrecs, mpi, mz), d(table)[0]

    def epoch(rows, **kw):
        cls, model, _ = _make(kind, dev)
        tr = cls(model, max_batch=batch)
        return _snapshot(tr, tr.run_epoch(*rows, order, lr=7e-4, batch=batch, **kw))

    def step(rows, **kw):
        cls, model, _ = _make(kind, dev)
        tr = cls(model, max_batch=batch)
        return _snapshot(tr, tr.step(*(x[:batch].contiguous() for x in rows), lr=7e-4, **kw))

    fused = epoch(plain, mirror=dtable)
    assert _identical(fused, epoch(mirrored))
    off = epoch(plain)
    assert _identical(off, epoch(plain, mirror=None))
    assert not _identical(fused, off)                               # the mirrored rows are other data
    assert _identical(epoch(plain, mirror=(9, 4)), epoch(plain, mirror=d(_flips(9, 4, n))[0]))      # the seeded form is the table's
    one = step(plain, mirror=dtable[:batch].contiguous())
    assert _identical(one, step(mirrored))
    assert _identical(step(plain), step(plain, mirror=None))
    assert not _identical(one, step(plain))


def _flips(seed, epoch, n):
    from alphaquoridorgnn_amd.train_network import draw_mirror_flips
    return draw_mirror_flips(seed, epoch, n)


def test_a_mirrored_epoch_reads_nothing_back(dev):
    from tests.test_gnn_graph_autograd import _sync_count
    cls, model, N = _make("general", dev)
    recs, pi, z = _training_rows(N, 37, seed=3)
    S, P, Z = (torch.from_numpy(x).to(dev) for x in (recs, pi, z))
    order = torch.randperm(37, device=dev)
    table = torch.from_numpy(_flips(1, 0, 37)).to(dev)
    tr = cls(model, max_batch=16)
    tr.run_epoch(S, P, Z, order, batch=16, mirror=table)
    torch.cuda.synchronize()
    assert _sync_count(lambda: torch.zeros(1, device=dev).item()) == 1       # the counter sees a read
    assert _sync_count(lambda: tr.run_epoch(S, P, Z, order, batch=16, mirror=table)) == 0
    assert _sync_count(lambda: tr.run_epoch(S, P, Z, order, batch=16, mirror=(3, 1))) == 0
    assert _sync_count(lambda: tr.step(S[:16].contiguous(), P[:16].contiguous(), Z[:16].contiguous(), mirror=(3, 1))) == 0


# ------------------------------------------------------------------ refusals
def test_refusals(dev):
    from alphaquoridorgnn_amd import _lib, train_network as tn
    from alphaquoridorgnn_amd.game_logic import mirror_batch, mirror_policy_batch
    lib = _lib.load()
    N, n = 5, 40
    S, P, Z = (torch.from_numpy(x).to(dev) for x in _rows(N, n, seed=2))
    out = torch.empty_like(S)
    st = _lib.stream_ptr(dev)
    call = lambda A, o72: lib.aqg_augment_gather(N, A, _lib.ptr(S), None, None, None, None, 0, 0, 0, n, _lib.ptr(o72), None, None, st)   # noqa: E731
    with pytest.raises(_lib.HipLibraryError, match="overlaps"):
        _lib.check(call(_A(N), S), "aqg_augment_gather")                        # in place
    with pytest.raises(_lib.HipLibraryError, match="overlaps"):
        _lib.check(call(_A(N), S[n // 2:]), "aqg_augment_gather")               # inside the source
    with pytest.raises(_lib.HipLibraryError, match="policy_size"):
        _lib.check(call(_A(N) + 1, out), "aqg_augment_gather")
    with pytest.raises(_lib.HipLibraryError, match="policy_size"):
        _lib.check(call(_A(9), out), "aqg_augment_gather")
    assert call(_A(N), out) == 0
    cls, model, _ = _make("general", dev)
    tr = cls(model, max_batch=16)
    order = torch.arange(n, device=dev)
    table = torch.ones(n, dtype=torch.uint8, device=dev)
    before = [p.detach().clone() for p in tr.params]
    with pytest.raises(ValueError, match="pre_shuffle"):
        tr.run_epoch(S, P, Z, order, batch=16, pre_shuffle=False, mirror=table)
    with pytest.raises(ValueError, match="mirror"):
        tr.run_epoch(S, P, Z, order, batch=16, mirror=table[:-1].contiguous())         # not one entry per source row
    with pytest.raises(ValueError, match="mirror"):
        tr.run_epoch(S, P, Z, order, batch=16, mirror=table.to(torch.int64))
    with pytest.raises(ValueError, match="mirror"):
        tr.step(S[:16].contiguous(), P[:16].contiguous(), Z[:16].contiguous(), mirror="yes")
    assert tr.step_count == 0 and all(torch.equal(a, b) for a, b in zip(before, tr.params))      # refused before anything ran
    for bad in (torch.tensor([0, n], device=dev), torch.tensor([-1, 0], device=dev)):
        with pytest.raises(ValueError, match="order"):
            tn.augment_gather(S, P, Z, order=bad, board_size=N)
    with pytest.raises(ValueError):
        tn.augment_gather(S, P, Z, flips=table, seed=1, board_size=N)
    with pytest.raises(ValueError):
        tn.augment_gather(S, P[:, :-1].contiguous(), Z, board_size=N)
    with pytest.raises(ValueError):
        mirror_batch(P, N)
    with pytest.raises(ValueError):
        mirror_policy_batch(P, 9)


# ------------------------------------------------------------------ train_network() end to end
_TRAIN = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, train_network as tn
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork

g = np.load(os.path.join(os.environ["AQG_REPO"], "tests", "golden", "cnn_train_5x5.npz"))
rows = [[[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:20]]], p.tolist(), int(z)]
        for s, p, z in zip(g["states"], g["pi"], g["z"])]
assert len(rows) == 40 and constants.BOARD_SIZE == 5
os.makedirs("data")
with open("data/20260101000000.history", "wb") as f:
    pickle.dump(rows, f)
os.makedirs(constants.PV_NETWORK_PATH)
torch.manual_seed(3)
torch.save(GraphPolicyValueNetwork(6, 16, 2, 57, board_size=5).state_dict(), constants.PV_NETWORK_PATH + "best.pth")
tn.NUM_EPOCH = 2


def run():
    torch.manual_seed(11)               # the epochs' shuffles
    tn.train_network()
    return torch.load(constants.PV_NETWORK_PATH + "latest.pth", map_location="cpu", weights_only=True)


def same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


defaults = run()                        # the constants as the module sets them
tn.TRAIN_MIRROR, tn.TRAIN_MIRROR_SEED = True, 5
on1, on2 = run(), run()
tn.TRAIN_MIRROR_SEED = 6
other = run()
tn.TRAIN_MIRROR = False
off = run()
print("REPEATS", same(on1, on2))
print("DIFFERS", not same(on1, off), not same(on1, other))
print("OFF_IS_DEFAULT", same(off, defaults))
'''


def test_train_network_with_the_mirror_on(dev, tmp_path):
    """A 5x5 best.pth, a 40-row history, NUM_EPOCH = 2: latest.pth is identical across two runs with TRAIN_MIRROR on and one seed,
    differs from the run with the feature off (and from another seed's), and the off run's equals the one with the constants at
    their defaults."""
    (tmp_path / "train.py").write_text(_TRAIN)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "train.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "REPEATS True" in r.stdout, r.stdout[-2000:]
    assert "DIFFERS True True" in r.stdout, r.stdout[-2000:]
    assert "OFF_IS_DEFAULT True" in r.stdout, r.stdout[-2000:]
