"""GPU: aqg_legal_actions against the host oracle, bit for bit -- mask, ordered list and count -- over the task layouts of the wall
searches: one fill per lane (at most 32 candidates to search) and the interleaved form (33 and more, up to the 63 that a position
can leave).  Hand-built positions (tests/witness_cases.py), random-walk states at every board size, crowded positions.  No kernel
contains the witness-path filter: nothing here covers it."""
import numpy as np
import pytest
import torch

from tests import witness_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()          # raises if the HIP library is missing: no fallback
    return _lib.require_gpu()


def _check(dev, N, recs):
    from alphaquoridorgnn_amd import game_logic as gl
    from oracle import quoridor as oq
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 72)
    a, c, m = oq.legal_actions_batch(recs)
    mask, order, count = gl.legal_actions_batch(torch.from_numpy(recs).to(dev), N)
    A = N * N + 2 * (N - 1) ** 2
    assert np.array_equal(count.cpu().numpy(), c)
    assert np.array_equal(mask.cpu().numpy(), m[:, :A])
    o = order.cpu().numpy()
    for i in range(recs.shape[0]):
        assert np.array_equal(o[i, :c[i]], a[i, :c[i]]), i


@pytest.mark.parametrize("N", [5, 9])
def test_hand_built_positions_one_fill_per_lane(dev, N):
    pos = W.hand_positions(N)
    assert all(W.survivors(N, r)[0] <= 32 for r in pos.values())
    _check(dev, N, np.stack(list(pos.values())))


@pytest.mark.parametrize("N", [3, 5, 7, 9])
def test_random_walk_states(dev, N):
    _check(dev, N, W.random_walk_states(N, 2048, seed=200 + N))


def test_more_than_32_candidates_interleaved_layout(dev):
    batch = np.stack([W.crowded(9, 32, seed=s) for s in (1, 2, 3)])
    for r in batch:
        assert 32 < W.survivors(9, r)[0] <= 64
    _check(dev, 9, batch)


def test_most_crowded_position_fills_the_round(dev):
    """More than 63 candidates to search cannot be built (tests/test_witness_filter_cpu.py::test_most_crowded_position): the fullest
    round there is, 63 tasks in 63 lanes, among positions of the other layouts in one batch."""
    r = W.most_crowded()
    assert W.survivors(9, r)[0] == 63
    _check(dev, 9, np.stack([r, W.crowded(9, 32, seed=1), W.hand_positions(9)["last_gap"], r]))
