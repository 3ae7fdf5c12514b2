"""The replay window on the GPU: aqg_replay_append (csrc/replay.hip) against replay.append_reference bit for bit in both forms, with
every slot outside the written interval untouched; the C entry's refusals; an append that reads nothing back; and the loop end to end
on the 5x5 board -- train_network() from a window against the file route, self_play() into a window against the file it wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_replay_window_cpu import _A, _bits, counts_rows, finished_rows   # noqa: E402

pytestmark = pytest.mark.gpu

FILL_U8, FILL_F32 = 0xA5, np.float32(-7.25)
# csrc/replay.hip: RPL_GROUP = 4 rows per wavefront group, RPL_ROWS = 16 rows per workgroup
GROUP, ROWS = 4, 16
SIZES = (0, 1, GROUP - 1, GROUP, GROUP + 1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 5)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def test_the_sizes_are_the_kernels():
    src = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "replay.hip")).read()
    assert f"RPL_GROUP = {GROUP}" in src and f"RPL_WAVES = {ROWS // GROUP}" in src and "RPL_ROWS = RPL_WAVES * RPL_GROUP" in src


def _filled(capacity, A):
    return (np.full((capacity, 72), FILL_U8, np.uint8), np.full((capacity, A), FILL_F32, np.float32),
            np.full((capacity,), FILL_F32, np.float32))


def _call(dev, N, A, src, n, capacity, head, rings):
    """The C entry on device copies of `src` = (states72, visits, z_i8, pi, z_f32) and of the host rings; (rc, rings back on the host)."""
    from alphaquoridorgnn_amd import _lib
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d = [t(x.view(np.int16) if x is not None and x.dtype == np.uint16 else x) for x in src]
    r = [t(x) for x in rings]
    rc = _lib.load().aqg_replay_append(N, A, *(_lib.ptr(x) for x in d), n, capacity, head, *(_lib.ptr(x) for x in r), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in r]


@pytest.mark.parametrize("N", (3, 5, 7, 9))
def test_kernel_equals_the_reference_bit_for_bit(dev, N):
    """n = 0, 1, and one below, at and one above a wavefront's group (4 rows) and a workgroup (16 rows), and two workgroups plus five
    rows; written at head 0, at capacity - 5 (the write wraps once n > 5) and into a ring of exactly n rows from slot 3 (every slot
    written, wrapped).  Counts up to 65,535 with a row without a visit, one with a single visit and one full of 65,535.  The rings are
    pre-filled with a pattern: every slot outside the written interval must still hold it."""
    from alphaquoridorgnn_amd.replay import append_reference
    A = _A(N)
    for n in SIZES:
        S, V, Z = counts_rows(N, n, seed=100 * N + n, top=65535)
        S2, P, ZF = finished_rows(N, n, seed=200 * N + n)
        for capacity, head in ((n + 7, 0), (n + 7, n + 2), (max(n, 1), 3 % max(n, 1))):
            for src in ((S, V, Z, None, None), (S2, None, None, P, ZF)):
                want = _filled(capacity, A)
                append_reference(N, *src, head, *want)
                rc, got = _call(dev, N, A, src, n, capacity, head, _filled(capacity, A))
                assert rc == 0
                for g, w in zip(got, want):
                    assert np.array_equal(_bits(g), _bits(w)), (N, n, capacity, head, "counts" if src[1] is not None else "rows")
                written = (head + np.arange(n)) % capacity
                rest = np.setdiff1d(np.arange(capacity), written)
                assert (got[0][rest] == FILL_U8).all() and (got[1][rest] == FILL_F32).all() and (got[2][rest] == FILL_F32).all()


def test_c_entry_refusals(dev):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, n, capacity = 5, 20, 32
    A = _A(N)
    S, V, Z = counts_rows(N, n, seed=1)
    _, P, ZF = finished_rows(N, n, seed=1)
    counts, rows = (S, V, Z, None, None), (S, None, None, P, ZF)

    def refused(match, src, *, A_=A, n_=n, capacity_=capacity, head=0):
        rc, got = _call(dev, N, A_, src, n_, capacity_, head, _filled(capacity, A))
        assert rc != 0 and match in lib.aqg_last_error().decode(), (match, lib.aqg_last_error())
        assert (got[0] == FILL_U8).all() and (got[1] == FILL_F32).all() and (got[2] == FILL_F32).all()   # the rings are as they were

    refused("policy_size", counts, A_=_A(9))
    refused("policy_size", rows, A_=_A(3))
    refused("n > capacity", counts, capacity_=n - 1)
    refused("head", counts, head=capacity)
    refused("head", rows, head=-1)
    refused("capacity", rows, capacity_=0)
    refused("negative", rows, n_=-1)
    refused("form", (S, V, Z, P, ZF))                      # both
    refused("form", (S, None, None, None, None))           # neither
    refused("form", (S, V, None, None, ZF))                # half of each
    refused("must be given", (None, V, Z, None, None))
    rc, _ = _call(dev, N, A, (None, None, None, None, None), 0, capacity, 0, _filled(capacity, A))
    assert rc == 0                                          # n == 0: no pointer is looked at
    # a ring that overlaps a source: the pi ring IS the source, and a record ring that begins inside the source records
    st = _lib.stream_ptr(dev)
    dS, dP, dZ = (torch.from_numpy(x).to(dev) for x in (S, P, ZF))
    r72, rpi, rz = (torch.from_numpy(x).to(dev) for x in _filled(capacity, A))
    big72 = torch.full((n + capacity, 72), FILL_U8, dtype=torch.uint8, device=dev)
    for s_, p_, ring72_, ringpi_, n_, cap_ in ((dS, dP, r72, dP, n, n), (big72, dP, big72[n - 1:], rpi, n, capacity)):
        rc = lib.aqg_replay_append(N, A, _lib.ptr(s_), None, None, _lib.ptr(p_), _lib.ptr(dZ), n_, cap_, 0, _lib.ptr(ring72_),
                                   _lib.ptr(ringpi_), _lib.ptr(rz), st)
        assert rc != 0 and "overlaps" in lib.aqg_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(dP.cpu(), torch.from_numpy(P)) and (big72 == FILL_U8).all() and (rz == float(FILL_F32)).all()


def test_the_window_on_the_device_is_the_window_on_the_host(dev):
    """The same appends -- counts, rows, a wrap, an oversized generation -- into a GPU window and a host one: same bookkeeping, same
    rows bit for bit, same rings."""
    from alphaquoridorgnn_amd.replay import ReplayWindow
    N = 7
    g, h = ReplayWindow(N, max_generations=3, capacity_rows=40, device=dev), ReplayWindow(N, max_generations=3, capacity_rows=40)
    assert g.device.type == "cuda" and g.tensors()[0].device == g.device
    for k, m in enumerate((17, 9, 21, 45, 6)):
        if k % 2 == 0:
            S, V, Z = counts_rows(N, m, seed=k)
            args = (torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
            g.append_counts(*(x.to(dev) if k else x for x in args))          # inputs may live on any device
            h.append_counts(*args)
        else:
            args = tuple(torch.from_numpy(x) for x in finished_rows(N, m, seed=k))
            g.append_rows(*(x.to(dev) for x in args))
            h.append_rows(*args)
        assert g.generations == h.generations and len(g) == len(h)
        assert g.index().device == g.device and torch.equal(g.index().cpu(), h.index())
        for a, b in zip(g.rows(), h.rows()):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.numpy()))
    for a, b in zip(g.tensors(), h.tensors()):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.numpy()))


def test_an_append_reads_nothing_back(dev):
    from alphaquoridorgnn_amd.replay import ReplayWindow
    from tests.test_gnn_graph_autograd import _sync_count
    N = 5
    S, V, Z = (torch.from_numpy(x).to(dev) for x in (lambda s, v, z: (s, v.view(np.int16), z))(*counts_rows(N, 37, seed=5)))
    w = ReplayWindow(N, max_generations=2, capacity_rows=80, device=dev)
    w.append_counts(S, V, Z)
    torch.cuda.synchronize()
    assert _sync_count(lambda: torch.zeros(1, device=dev).item()) == 1       # the counter sees a read
    assert _sync_count(lambda: w.append_counts(S, V, Z)) == 0
    # the third drops the first and wraps
    assert _sync_count(lambda: w.append_rows(S, w.rows()[1][:37].contiguous(), w.rows()[2][:37].contiguous())) == 0
    assert _sync_count(lambda: (w.index(), w.tensors(), w.rows())) == 0
    assert w.generations == [37, 37]


# ------------------------------------------------------------------ the loop end to end
_LOOP = r'''
import os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, pv_mcts, self_play as sp, train_network as tn
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, pack_states
from alphaquoridorgnn_amd.replay import ReplayWindow

g = np.load(os.path.join(os.environ["AQG_REPO"], "tests", "golden", "cnn_train_5x5.npz"))
rows = [[[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:20]]], p.tolist(), int(z)]
        for s, p, z in zip(g["states"], g["pi"], g["z"])]
assert len(rows) == 40 and constants.BOARD_SIZE == 5
older = [[s, p, -z] for s, p, z in rows[:25]]                  # another generation: fewer rows, the outcomes reversed
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


def window(generations, histories=(), files=()):
    w = ReplayWindow(5, max_generations=generations, device=dev)
    for h in histories:
        w.append_history(h)
    w.extend_from_files(files)
    return w


defaults = run()                        # (c) the constants as the module sets them: the newest file
for mirror in (False, True):            # (a) a fresh one-generation window against the file route
    tn.TRAIN_MIRROR, tn.TRAIN_MIRROR_SEED = mirror, 5
    from_file = run()
    tn.TRAIN_WINDOW = window(1, [rows])
    print("ONE_GENERATION_IS_THE_FILE_ROUTE", mirror, run() == from_file, (from_file == defaults) == (not mirror))
    tn.TRAIN_WINDOW = ReplayWindow(5, max_generations=1, device=dev)          # an empty window is the file route
    print("EMPTY_WINDOW_IS_THE_FILE_ROUTE", mirror, run() == from_file)
    tn.TRAIN_WINDOW = None
tn.TRAIN_MIRROR, tn.TRAIN_MIRROR_SEED = False, 0
tn.TRAIN_WINDOW = window(2, [older, rows])         # (b) two generations
two1, two2 = run(), run()
print("TWO_GENERATIONS", two1 != defaults, two1 == two2, tn.TRAIN_WINDOW.generations == [25, 40])
tn.TRAIN_WINDOW = window(2, files=FILES)           # (e) TRAIN_GENERATIONS over two files against extend_from_files
from_files = run()
tn.TRAIN_WINDOW, tn.TRAIN_GENERATIONS = None, 2
print("TRAIN_GENERATIONS", run() == from_files, from_files == two1)
tn.TRAIN_GENERATIONS, tn.TRAIN_EPOCH_ROWS = 1, 16
short = run()
tn.TRAIN_EPOCH_ROWS = 4000
print("EPOCH_ROWS", short != defaults, run() == defaults)
tn.TRAIN_EPOCH_ROWS = None
print("OFF_IS_DEFAULT", run() == defaults)         # (c) every option back at its default

pv_mcts.PV_EVALUATE_COUNT = 8                      # (d) self-play into a window and into the file
sp.SP_REPLAY = ReplayWindow(5, max_generations=2, capacity_rows=8192, device=dev)
path = sp.self_play(games=6, seed=17)
with open(path, "rb") as f:
    s, p, v = zip(*pickle.load(f))
s = pack_states(s, 5)
p = torch.tensor(np.array(p), dtype=torch.float32).numpy()
v = torch.tensor(np.array(v), dtype=torch.float32).numpy()
ws, wp, wv = (x.cpu().numpy() for x in sp.SP_REPLAY.rows())
keep = np.ones(72, bool)
keep[68:70] = False
print("SELF_PLAY_ROWS", len(s) >= 6, ws.shape == s.shape and np.array_equal(ws[:, keep], s[:, keep]),
      wp.shape == p.shape and np.array_equal(wp.view(np.int32), p.view(np.int32)),
      wv.shape == v.shape and np.array_equal(wv.view(np.int32), v.view(np.int32)))
first = sp.SP_REPLAY.generations
sp.self_play(games=6, seed=18)
print("SELF_PLAY_GENERATIONS", first == [len(s)], len(sp.SP_REPLAY.generations) == 2, sp.SP_REPLAY.generations[0] == len(s))
sp.SP_WRITE_HISTORY = False
before = sorted(os.listdir("data"))
print("NO_FILE", sp.self_play(games=6, seed=19) is None, sorted(os.listdir("data")) == before, len(sp.SP_REPLAY.generations) == 2)
'''


def test_the_loop_with_a_window(dev, tmp_path):
    """One child process on the 5x5 board with a 6/16/2 best.pth, NUM_EPOCH = 2 and the 40 golden rows (see the issue's (a) - (e) in
    the script): a one-generation window trains to the file route's latest.pth byte for byte, mirror off and on; two generations
    train to another one, the same twice; TRAIN_GENERATIONS = 2 over two files equals extend_from_files; the defaults give the run
    from before anything was set; self_play() fills the window with the rows of the file it wrote, and a second call adds a
    generation."""
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for line in ("ONE_GENERATION_IS_THE_FILE_ROUTE False True True", "ONE_GENERATION_IS_THE_FILE_ROUTE True True True",
                 "EMPTY_WINDOW_IS_THE_FILE_ROUTE False True", "EMPTY_WINDOW_IS_THE_FILE_ROUTE True True",
                 "TWO_GENERATIONS True True True", "TRAIN_GENERATIONS True True", "EPOCH_ROWS True True", "OFF_IS_DEFAULT True",
                 "SELF_PLAY_ROWS True True True True", "SELF_PLAY_GENERATIONS True True True", "NO_FILE True True True"):
        assert line in r.stdout, (line, r.stdout[-3000:])
