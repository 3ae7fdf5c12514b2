"""The position merge on the GPU (csrc/replay_merge.hip): rows that hold the same position become one row with the mean targets.
replay_reference.merge_reference is its statement in numpy; ReplayWindow.merged() calls it on the ring."""
import torch

from . import _lib
from .constants import BOARD_SIZE, check_board_size, num_actions


def check_gpu_rows(what, board_size, specs):
    """specs: (tensor, name, dtype, shape) each, the first being states72: every tensor must have its dtype and shape and lie on
    the GPU states72 is on.  Shared with replay_surprise.surprise_index."""
    dev = specs[0][0].device
    for x, name, dtype, shape in specs:
        if x.dtype != dtype or tuple(x.shape) != shape or not x.is_cuda or x.device != dev:
            raise ValueError(f"{what}: {name} must be a {dtype} {list(shape)} tensor on the GPU ({board_size}x{board_size} board)")


def merge_positions(states72, pi, z, index=None, board_size=BOARD_SIZE):
    """The position merge on the GPU: (out72 uint8 [u,72], out_pi float32 [u,A], out_z float32 [u], count int32 [u]) of the rows
    index[0..n) (int64, on the tensors' device; None: all rows) of the device tensors (states72, pi, z) -- merge_reference's result bit
    for bit.  aqg_replay_position_keys hashes the rows, torch sorts the keys (stable), aqg_replay_run_heads marks where the key BYTES
    change, torch turns that into runs in first-occurrence order, aqg_replay_merge_runs writes the rows.  Host reads: the bounds of
    index, and the run starts (whose number sizes the outputs)."""
    check_board_size(board_size, "merge_positions")
    A = num_actions(board_size)
    rows = int(states72.shape[0]) if states72.dim() == 2 else -1
    check_gpu_rows("merge_positions", board_size, ((states72, "states72", torch.uint8, (rows, 72)), (pi, "pi", torch.float32, (rows, A)),
                                                   (z, "z", torch.float32, (rows,))))
    dev = states72.device
    states72, pi, z = states72.contiguous(), pi.contiguous(), z.contiguous()
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1 or index.device != dev:
            raise ValueError("merge_positions: index must be an int64 [n] tensor on the rows' device")
        index = index.contiguous()
        if index.numel():
            lo, hi = torch.stack((index.min(), index.max())).tolist()
            if lo < 0 or hi >= rows:
                raise ValueError("merge_positions: index names a row the arrays do not have")
    n = rows if index is None else int(index.numel())
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        if n == 0:
            return (torch.zeros((0, 72), dtype=torch.uint8, device=dev), torch.zeros((0, A), dtype=torch.float32, device=dev),
                    torch.zeros((0,), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev))
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        _lib.check(lib.aqg_replay_position_keys(_lib.ptr(states72), _lib.ptr(index), n, _lib.ptr(keys), st), "aqg_replay_position_keys")
        perm = torch.sort(keys, stable=True).indices                    # places of the input; equal keys stay in input order
        src = perm if index is None else index[perm]                    # the same, as rows of the arrays
        heads = torch.empty((n,), dtype=torch.uint8, device=dev)
        _lib.check(lib.aqg_replay_run_heads(_lib.ptr(states72), _lib.ptr(src), n, _lib.ptr(heads), st), "aqg_replay_run_heads")
        starts = heads.nonzero().squeeze(1)                             # the one device-to-host read: u sizes the outputs
        u = int(starts.numel())
        if u == n:                                                      # no repeats: every run is its own row, in input order
            src = torch.arange(n, dtype=torch.int64, device=dev) if index is None else index
            starts = torch.arange(n, dtype=torch.int64, device=dev)
        else:
            # runs into first-occurrence order (a stable sort keeps a run's rows in input order, so its first place is perm[start])
            lengths = torch.diff(starts, append=torch.tensor([n], dtype=torch.int64, device=dev))
            rank = torch.sort(perm[starts]).indices                     # rank[o] = the run that becomes output row o
            lengths_out = lengths[rank]
            starts_out = torch.cumsum(lengths_out, 0) - lengths_out
            where = torch.empty_like(rank)
            where[rank] = starts_out                                    # where[r] = the first place of run r in the new order
            run_of = torch.cumsum(heads, 0, dtype=torch.int64) - 1
            place = where[run_of] + (torch.arange(n, dtype=torch.int64, device=dev) - starts[run_of])
            moved = torch.empty_like(src)
            moved[place] = src
            src, starts = moved, starts_out.contiguous()
        out = (torch.empty((u, 72), dtype=torch.uint8, device=dev), torch.empty((u, A), dtype=torch.float32, device=dev),
               torch.empty((u,), dtype=torch.float32, device=dev), torch.empty((u,), dtype=torch.int32, device=dev))
        floats = int(lib.aqg_replay_merge_workspace_floats(board_size, n, u))
        work = torch.empty((floats,), dtype=torch.float32, device=dev) if floats else None
        _lib.check(lib.aqg_replay_merge_runs(board_size, A, _lib.ptr(states72), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(src), _lib.ptr(starts),
                                             n, u, *(_lib.ptr(x) for x in out), _lib.ptr(work), floats, st), "aqg_replay_merge_runs")
    return out
