"""Policy surprise weighting on the GPU (csrc/replay_surprise.hip): the rows an update trains on, drawn by KL(target || network).
replay_reference.surprise_reference and surprise_counts_reference are the two launches in numpy; ReplayWindow.surprise_index calls
surprise_index on the ring."""
import torch

from . import _lib
from .constants import check_board_size, num_actions
from .replay_merge import check_gpu_rows
from .replay_reference import SURPRISE_MAX_ROWS, check_surprise_options


def expand_rows(base, count, total=None):
    """Step 5 on torch tensors of one device: base int64 [m] (the rows in input order) with row j repeated count[j] times.  total: the
    sum of count when the caller has it (it then costs no read of the device)."""
    return torch.repeat_interleave(base, count.to(torch.int64), output_size=None if total is None else int(total))


def surprise_index(model, states72, pi, index=None, *, seed, update, expected_rows=None, uniform_share=0.5, max_copies=8,
                   chunk_rows=16384, stats=None):
    """The rows an update trains on, drawn by policy surprise, on the GPU: (index int64 [M], k float32 [m], count int32 [m]) for the rows
    index[0..m) (int64, on the tensors' device; None: all rows) of the device tensors states72 uint8 [rows,72] and pi float32 [rows,A].
    The returned index names those rows in input order, row j count[j] times -- a valid `index` for every trainer's epoch.

    model.forward_states runs over the records in chunks of at most chunk_rows rows (the policy buffer stays at most chunk_rows * 4A
    bytes), in eval mode, without autograd, with its fp16-range guard, and the module's mode is left as it was; one
    aqg_replay_surprise_rows launch per chunk, the exact integer sum of q on the device, one aqg_replay_surprise_counts launch, and
    torch.cumsum / torch.repeat_interleave for the expansion.  expected_rows None: m.  One device-to-host read of its own (besides the
    forward's guard): M with the statistics, which a dict given as `stats` receives -- rows, expanded, left_out, most_copies, mean_kl.
    surprise_reference and surprise_counts_reference are the two launches in numpy."""
    E, U, C = check_surprise_options(expected_rows, uniform_share, max_copies)
    if int(chunk_rows) < 1:
        raise ValueError("surprise_index: chunk_rows must be >= 1")
    board_size, A = int(model.board_size), int(model.policy_output_size)
    check_board_size(board_size, "surprise_index")
    if A != num_actions(board_size):            # a policy head that is not the board's
        raise ValueError("surprise_index: unsupported board_size (odd 3..9)")
    rows = int(states72.shape[0]) if states72.dim() == 2 else -1
    check_gpu_rows("surprise_index", board_size, ((states72, "states72", torch.uint8, (rows, 72)), (pi, "pi", torch.float32, (rows, A))))
    dev = states72.device
    states72, pi = states72.contiguous(), pi.contiguous()
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1 or index.device != dev:
            raise ValueError("surprise_index: index must be an int64 [m] tensor on the rows' device")
        index = index.contiguous()
    m = rows if index is None else int(index.numel())
    if m > SURPRISE_MAX_ROWS:
        raise ValueError(f"surprise_index: {m} rows; 2^24 at most")
    if m == 0:
        if stats is not None:
            stats.update(rows=0, expanded=0, left_out=0, most_copies=0, mean_kl=0.0)
        return (torch.zeros((0,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.float32, device=dev),
                torch.zeros((0,), dtype=torch.int32, device=dev))
    E = m if E is None else E
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    chunk = int(chunk_rows)
    was_training = bool(getattr(model, "training", False))
    with torch.cuda.device(dev):
        k = torch.empty((m,), dtype=torch.float32, device=dev)
        q = torch.empty((m,), dtype=torch.int32, device=dev)
        count = torch.empty((m,), dtype=torch.int32, device=dev)
        model.eval()
        try:
            with torch.no_grad():
                for off in range(0, m, chunk):
                    n = min(chunk, m - off)
                    records = states72[off:off + n] if index is None else states72.index_select(0, index[off:off + n])
                    net_policy = model.forward_states(records.contiguous())[0].contiguous()
                    _lib.check(lib.aqg_replay_surprise_rows(board_size, A, _lib.ptr(net_policy), _lib.ptr(pi), _lib.ptr(index), rows, m, off, n,
                                                            _lib.ptr(k), _lib.ptr(q), st), "aqg_replay_surprise_rows")
        finally:
            model.train(was_training)
        total = q.sum(dtype=torch.int64).reshape(1)                    # exact, and it stays on the device
        _lib.check(lib.aqg_replay_surprise_counts(_lib.ptr(q), _lib.ptr(index), _lib.ptr(total), m, E, U, C, int(seed) & ((1 << 64) - 1),
                                                  int(update) & ((1 << 64) - 1), _lib.ptr(count), st), "aqg_replay_surprise_counts")
        ends = torch.cumsum(count, 0, dtype=torch.int64)
        M, left_out, most, kl_sum = torch.stack((ends[-1].double(), (count == 0).sum().double(), count.max().double(),
                                                 k.sum(dtype=torch.float64))).tolist()          # the one read
        base = torch.arange(m, dtype=torch.int64, device=dev) if index is None else index
        expanded = expand_rows(base, count, M)
    if stats is not None:
        stats.update(rows=m, expanded=int(M), left_out=int(left_out), most_copies=int(most), mean_kl=kl_sum / m)
    return expanded, k, count
