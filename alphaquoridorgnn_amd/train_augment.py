"""Mirror-symmetry augmentation of training rows: the fused gather + flip launch (aqg_augment_gather, include/aqgnn.h), the seeded
draw it makes restated in numpy, and the checked stand-alone entry."""
import numpy as np
import torch

from . import _lib
from .constants import BOARD_SIZE, num_actions


def draw_mirror_flips(seed, epoch, n):
    """The flips of source rows 0 .. n-1 in epoch `epoch` under `seed`, uint8 [n] -- the seeded draw of aqg_augment_gather in numpy
    (include/aqgnn.h): row r is mirrored iff f(K(seed, epoch), r) < 0.5 with the counter-based generator of agents.draw_uniforms.
    A pure function of (seed, epoch, r): a prefix of a longer draw is the shorter draw."""
    from .agents import draw_uniforms
    return (draw_uniforms(seed, epoch, n) < 0.5).astype(np.uint8)


def _mirror_arguments(mirror, rows, dev):
    """(flips tensor or None, use_seed, seed, epoch) of a `mirror` argument: a uint8 [rows] device table indexed by source row, or
    (seed, epoch).  Shapes and types only -- nothing is read back from the device."""
    if isinstance(mirror, torch.Tensor):
        if mirror.dtype != torch.uint8 or mirror.dim() != 1 or mirror.shape[0] != rows or mirror.device != dev:
            raise ValueError(f"a mirror table is a uint8 [{rows}] tensor on {dev}, one entry per source row")
        return mirror.contiguous(), 0, 0, 0
    try:
        seed, epoch = mirror
        seed, epoch = int(seed), int(epoch)
    except (TypeError, ValueError):
        raise ValueError("mirror is None, a uint8 device table indexed by source row, or (seed, epoch)") from None
    if epoch < 0:
        raise ValueError("mirror: the epoch must be >= 0")
    return None, 1, seed & ((1 << 64) - 1), epoch


def _augment_launch(board_size, states72, pi, z, order, mirror):
    """The fused launch on contiguous device tensors of one device: (out72, out_pi, out_z), None where the input is None.  order:
    int64 source rows, NOT checked here (augment_gather checks them); mirror: as _mirror_arguments, or None for a plain gather."""
    src = next(x for x in (states72, pi, z) if x is not None)
    dev, rows = src.device, int(src.shape[0])
    n = rows if order is None else int(order.shape[0])
    flips, use_seed, seed, epoch = (None, 0, 0, 0) if mirror is None else _mirror_arguments(mirror, rows, dev)
    outs = [None if x is None else torch.empty((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev) for x in (states72, pi, z)]
    A = num_actions(board_size)
    _lib.check(_lib.load().aqg_augment_gather(board_size, A, _lib.ptr(states72), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(order),
                                              _lib.ptr(flips), use_seed, seed, epoch, n, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                              _lib.ptr(outs[2]), _lib.stream_ptr(dev)), "aqg_augment_gather")
    return tuple(outs)


def augment_gather(states72, pi, z, order=None, flips=None, seed=None, epoch=0, board_size=BOARD_SIZE):
    """Gather and mirror training rows in one launch (aqg_augment_gather): output row i is source row order[i] (None: row i),
    mirrored iff flips[that source row] is set -- or, with flips None and a seed, iff draw_mirror_flips(seed, epoch, rows) says so.
    With neither it is a plain gather.  states72 uint8 [rows,72], pi float32 [rows,A], z float32 [rows]: device tensors, each may be
    None (and so is its output).  Returns (out72, out_pi, out_z), freshly allocated, with len(order) rows (any number, none
    included).  order is checked against the row count with one host read."""
    given = [x for x in (states72, pi, z) if x is not None]
    if not given:
        raise ValueError("augment_gather: at least one of states72, pi, z is needed")
    dev = _lib.require_gpu(given[0].device)
    rows = int(given[0].shape[0])
    A = num_actions(board_size)
    for x, name, dtype, tail in ((states72, "states72", torch.uint8, (72,)), (pi, "pi", torch.float32, (A,)), (z, "z", torch.float32, ())):
        if x is not None and (x.device != dev or x.dtype != dtype or tuple(x.shape) != (rows,) + tail):
            raise ValueError(f"augment_gather: {name} must be a {dtype} {[rows, *tail]} tensor on {dev} ({board_size}x{board_size} board)")
    states72, pi, z = (None if x is None else x.contiguous() for x in (states72, pi, z))
    if order is not None:
        order = order.to(dev, torch.int64).contiguous()
        if order.dim() != 1:
            raise ValueError("augment_gather: order is a 1-D tensor of source rows")
        if order.numel():
            lo, hi = torch.stack((order.min(), order.max())).tolist()          # the one host read
            if lo < 0 or hi >= rows:
                raise ValueError(f"augment_gather: order holds a row outside 0..{rows - 1}")
    if flips is not None and seed is not None:
        raise ValueError("augment_gather: give flips or seed, not both")
    mirror = flips if flips is not None else None if seed is None else (seed, epoch)
    return _augment_launch(board_size, states72, pi, z, order, mirror)
