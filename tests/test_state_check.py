"""The record checker on the device (csrc/state_check.hip, aqg_states72_check) held byte for byte to the numpy statement
game_logic.check_state_reference: crafted records that set each flag bit alone and in pairs -- pawn cells of 255 and wall bytes of 255
among them -- and records of random bytes, on 3x3, 5x5 and 9x9, at B = 1, 63, 64, 65 and 257 (the edges of a 256-thread workgroup and
of a wavefront), the flag buffer between sentinels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _start_positions as SP   # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL, PAD = 0x5A, 64
BATCHES = (1, 63, 64, 65, 257)
_CASES = {}


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _cases(N):
    """257 records of one board and the statement's flags, computed once: the crafted ones, then garbage."""
    from alphaquoridorgnn_amd.game_logic import check_state_reference
    if N not in _CASES:
        crafted = np.stack([rec for _, rec, _ in SP.crafted_records(N)])
        recs = np.concatenate([crafted, SP.garbage_records(N, max(BATCHES) - len(crafted), seed=20 + N)])
        want = np.asarray([check_state_reference(r, N) for r in recs], dtype=np.uint8)
        want.setflags(write=False)
        _CASES[N] = (recs, want)
    return _CASES[N]


def _launch(dev, N, recs, num_walls, draw):
    from alphaquoridorgnn_amd import _lib
    B = recs.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(recs)).to(dev)
    before = d.clone()
    buf = torch.full((PAD + B + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    out = ctypes.c_void_p(buf.data_ptr() + PAD)
    _lib.check(_lib.load().aqg_states72_check(N, _lib.ptr(d), B, num_walls, draw, out, _lib.stream_ptr(dev)), "aqg_states72_check")
    got = buf.cpu().numpy()
    assert (got[:PAD] == SENTINEL).all() and (got[PAD + B:] == SENTINEL).all(), "the launch wrote outside its B flags"
    assert torch.equal(d, before), "the records were written to"
    return got[PAD:PAD + B]


@pytest.mark.parametrize("N", (3, 5, 9))
def test_crafted_records_by_name(dev, N):
    """Each crafted record against its hand-stated flags (which the statement gives too: tests/test_start_positions_cpu.py)."""
    cases = SP.crafted_records(N)
    got = _launch(dev, N, np.stack([rec for _, rec, _ in cases]), *SP.params(N))
    for (name, _, flags), g in zip(cases, got):
        assert int(g) == flags, (name, int(g), flags)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", (3, 5, 9))
def test_kernel_is_the_statement(dev, N, B):
    recs, want = _cases(N)
    got = _launch(dev, N, recs[:B], *SP.params(N))
    assert np.array_equal(got, want[:B]), np.flatnonzero(got != want[:B])[:8]


def test_python_entry_and_other_constants(dev):
    """game_logic.check_states_batch, with the board's own constants and with others; the entry point's refusals."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.game_logic import check_state_reference, check_states_batch
    recs, want = _cases(5)
    d = torch.from_numpy(recs[:40].copy()).to(dev)
    assert np.array_equal(check_states_batch(d, 5).cpu().numpy(), want[:40])
    got = check_states_batch(d, 5, num_walls=3, plies_for_draw=2).cpu().numpy()
    assert np.array_equal(got, [check_state_reference(r, 5, num_walls=3, plies_for_draw=2) for r in recs[:40]])
    assert check_states_batch(d[:0], 5).shape == (0,)
    with pytest.raises(ValueError, match="uint8"):
        check_states_batch(d.to(torch.int32), 5)
    lib = _lib.load()
    out = torch.zeros((40,), dtype=torch.uint8, device=dev)
    for args in ((4, _lib.ptr(d), 40, 2, 28, _lib.ptr(out)), (5, _lib.ptr(d), -1, 2, 28, _lib.ptr(out)), (5, None, 40, 2, 28, _lib.ptr(out)),
                 (5, _lib.ptr(d), 40, 2, 28, None), (5, _lib.ptr(d), 40, 128, 28, _lib.ptr(out)), (5, _lib.ptr(d), 40, 2, 65536, _lib.ptr(out))):
        assert lib.aqg_states72_check(*args, _lib.stream_ptr(dev)) != 0, args[0:1] + args[2:5]
    torch.cuda.synchronize()
    assert not out.any()
