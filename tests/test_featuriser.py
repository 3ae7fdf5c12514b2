"""The board featuriser alone (csrc/board_featuriser.hip: boards_prep_kernel through aqg_gcn_boards_graph; include/aqgnn.h): the six
planes per tile against the reference's own recorded planes, the ELL adjacency against oracle.gnn.board_edges, independence of
the batch around a board, guarded outputs and the argument checks.  The states, their coverage conditions and the expected values
come from tests/test_cnn_conv_edges_cpu.py, where they are checked without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_cnn_conv_edges_cpu import (ELL_REL_BOUND, FEAT_BATCHES, FEAT_N, expected_ell, expected_features,   # noqa: E402
                                           feat_coverage, feat_states)
from tests.test_graph_primitives import Guarded, last_error, to_dev                                            # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def lib():
    from alphaquoridorgnn_amd import _lib
    return _lib.load()


def run_graph(lib, dev, N, recs):
    """aqg_gcn_boards_graph into guarded x / ell_idx / ell_w -> (x [R,6] f32, idx [R,5] i32, w [R,5] f32) on the host."""
    from alphaquoridorgnn_amd import _lib
    B, R = recs.shape[0], recs.shape[0] * N * N
    gx, gi, gw = Guarded(dev, (R, 6)), Guarded(dev, (R, 5)), Guarded(dev, (R, 5))
    d72 = to_dev(dev, np.array(recs))                                     # (a copy: the shared states are read-only)
    rc = lib.aqg_gcn_boards_graph(N, _lib.ptr(d72), B, _lib.ptr(gx.view), _lib.ptr(gi.view), _lib.ptr(gw.view), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert gx.intact() and gi.intact() and gw.intact(), "aqg_gcn_boards_graph wrote outside x[B*V,6] / ell_idx[B*V,5] / ell_w[B*V,5]"
    return gx.host(), gi.view.view(torch.int32).cpu().numpy(), gw.host()


@pytest.fixture(scope="module")
def graphs(lib, dev):
    """The featuriser's output on feat_states(N), computed once per board size."""
    cache = {}

    def get(N):
        if N not in cache:
            cache[N] = run_graph(lib, dev, N, feat_states(N)[0])
        return cache[N]
    return get


@pytest.mark.parametrize("N", FEAT_N)
def test_planes_bit_for_bit(graphs, N):
    """x[b V + t][f] == planes[b, f, t // N, t % N] of the reference's recording (3x3, 5x5, 9x9: all 200 states), and
    oracle.gnn.node_features on every state (7x7 has no recording), as uint32."""
    recs, planes = feat_states(N)
    missing = [k for k, ok in feat_coverage(recs, N).items() if not ok]
    assert not missing, missing
    V = N * N
    x = graphs(N)[0].reshape(-1, V, 6)
    assert x.dtype == np.float32
    if planes is not None:
        want = np.ascontiguousarray(planes.reshape(planes.shape[0], 6, V).transpose(0, 2, 1))
        assert np.array_equal(x[:want.shape[0]].view(np.uint32), want.view(np.uint32))
    want = expected_features(recs)
    bad = np.argwhere(x.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} features differ, first at [board, tile, plane] {bad[0].tolist()}"


@pytest.mark.parametrize("N", FEAT_N)
def test_adjacency_vs_board_edges(graphs, N):
    """Slot 0 is the node itself, slots 1..4 up / down / left / right; a closed or off-board side is index -1 and weight exactly
    0.0f; indices exactly; weights against 1 / sqrt(d_i d_j) in float64 under ((1 + 2^-24)^3 - 1) w -- the kernel multiplies two
    correctly rounded f32 inverse roots, `di * dinv_of_bits(...)`: three f32 roundings; w(i -> j) == w(j -> i) bit for bit; a tile
    with all four sides closed has self weight exactly 1.0f."""
    recs, _ = feat_states(N)
    V = N * N
    _, idx, w = graphs(N)
    eidx, ew = expected_ell(recs)
    bad = np.argwhere(idx != eidx)
    assert bad.size == 0, f"{len(bad)} indices differ, first at [row, slot] {bad[0].tolist()}: {idx[tuple(bad[0])]} vs {eidx[tuple(bad[0])]}"
    closed = eidx < 0
    assert closed.any() and (w.view(np.uint32)[closed] == 0).all()                       # +0.0f, not -0.0f, not a small number
    err = np.abs(w.astype(np.float64) - ew)
    bound = ELL_REL_BOUND * ew
    ratio = float((err[~closed] / bound[~closed]).max())
    print(f"ELL weights {N}x{N}: worst {ratio:.3g} of the bound")
    assert (err <= bound).all(), f"worst error is {ratio:.3g} x the derived bound"
    rows, slots = np.nonzero(~closed & (np.arange(5)[None, :] > 0))
    back = {1: 2, 2: 1, 3: 4, 4: 3}
    j = idx[rows, slots]
    bslots = np.array([back[s] for s in slots])
    assert (idx[j, bslots] == rows).all()
    assert np.array_equal(w[rows, slots].view(np.uint32), w[j, bslots].view(np.uint32))
    lone = closed[:, 1:].all(1)
    if lone.any():
        assert (w[lone, 0].view(np.uint32) == np.float32(1.0).view(np.uint32)).all()
    inv = {d: np.float32(1.0 / np.sqrt(np.float64(d))) for d in range(1, 6)}           # dinv_of's constants: the f32 nearest d^-1/2
    deg = 1 + (~closed[:, 1:]).sum(1)
    self_w = np.array([inv[d] * inv[d] for d in deg], dtype=np.float32)
    assert np.array_equal(w[:, 0].view(np.uint32), self_w.view(np.uint32))             # the self loop: di * di, one product


@pytest.mark.parametrize("N", FEAT_N)
def test_batch_position_and_size(lib, dev, N):
    """A board's V feature rows and 5 V adjacency rows are the same, indices shifted by b V, whether it is computed alone, first,
    last or inside a batch: batches of 1, 2, 257 and 1025 boards (never a multiple of the 256-thread block)."""
    recs, _ = feat_states(N)
    V = N * N
    big_n = max(FEAT_BATCHES)
    pool = np.ascontiguousarray(recs[np.arange(big_n) * 7 % recs.shape[0]])
    x, idx, w = run_graph(lib, dev, N, pool)
    x, idx, w = x.reshape(big_n, V, 6), idx.reshape(big_n, V, 5), w.reshape(big_n, V, 5)

    def same(lo, hi):
        xs, ids, ws = run_graph(lib, dev, N, pool[lo:hi])
        shifted = np.where(ids >= 0, ids + lo * V, -1).reshape(hi - lo, V, 5)
        assert np.array_equal(xs.reshape(-1, V, 6).view(np.uint32), x[lo:hi].view(np.uint32)), (lo, hi)
        assert np.array_equal(shifted, idx[lo:hi]), (lo, hi)
        assert np.array_equal(ws.reshape(-1, V, 5).view(np.uint32), w[lo:hi].view(np.uint32)), (lo, hi)

    for B in FEAT_BATCHES[:-1]:
        same(0, B)                                  # first in a smaller batch
        same(big_n - B, big_n)                      # last in a smaller batch (B = 1: the last board alone)
    same(500, 501)                                  # a middle board alone


def test_argument_checks(lib, dev):
    """Board size 4 and a negative B return non-zero with a message; B = 0 returns 0 and writes nothing."""
    from alphaquoridorgnn_amd import _lib
    recs = feat_states(5)[0][:4]
    d72 = to_dev(dev, np.array(recs))
    gx, gi, gw = Guarded(dev, (100, 6)), Guarded(dev, (100, 5)), Guarded(dev, (100, 5))

    def call(N, B):
        return lib.aqg_gcn_boards_graph(N, _lib.ptr(d72), B, _lib.ptr(gx.view), _lib.ptr(gi.view), _lib.ptr(gw.view), _lib.stream_ptr(dev))

    assert call(4, 4) != 0 and "board_size" in last_error(lib)
    assert call(5, -1) != 0 and "negative" in last_error(lib)
    assert call(5, 0) == 0
    torch.cuda.synchronize()
    assert gx.untouched() and gi.untouched() and gw.untouched()
